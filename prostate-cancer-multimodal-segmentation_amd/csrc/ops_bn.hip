// BatchNorm3d (train / eval) + ReLU of the U-Net step, forward and backward (NDHWC, gfx950).
//
// Reference op replaced (path relative to the reference repo):
//   BatchNorm3d + ReLU(inplace)   models/unet3d.py:31-39
// Every per-channel statistic is a two-level reduction: fp32 per-block partials written
// to a [rows][C][2] buffer, combined in fp64 in a fixed order (run-to-run reproducible).
// Every launch here is grid-stride with a capped grid; pcms_stream_grid_cap (a test switch,
// host side only, defined here for all the ops units) lowers every cap at once so that
// tests/test_stream_regimes.py reaches the many-trips-per-thread paths at small shapes.
#include "ops_units.h"
#include "pcms_hip.h"
#include <climits>

namespace {

// ---------------- BatchNorm statistics ----------------
// Stage 1: fp32 partial rows [rows][C][2] -> fp64 column sums [RB][C][2] (RB row groups).
// block = 256 threads = 4 row lanes x 64 channels; grid = (ceil(C / 64), RB).
// cnt != NULL: rows are (sum, M2 about the row mean) with per-row voxel counts cnt[rows];
// column 2 then accumulates M2 + sum^2 / count (= the row's sum of squares, formed in fp64).
constexpr int kRB = 64;
__global__ void __launch_bounds__(256) colsum2_kernel(const float* part, int rows, int C, const float* cnt,
                                                      double* out) {
  __shared__ double red[4][64][2];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s1 = 0.0, s2 = 0.0;
  auto add = [&](const float2 v, int r) {
    s1 += (double)v.x;
    if (cnt) {
      const double n = (double)cnt[r];
      s2 += (double)v.y + (n > 0.0 ? (double)v.x * (double)v.x / n : 0.0);
    } else {
      s2 += (double)v.y;
    }
  };
  if (c < C) {
    // rows r, r + 256, ... added in that order, four rows' loads in flight per trip
    constexpr int RS = kRB * 4;
    int r = blockIdx.y * 4 + rl;
    for (; r + 3 * RS < rows; r += 4 * RS) {
      float2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float2*>(part + ((long)(r + u * RS) * C + c) * 2);
#pragma unroll
      for (int u = 0; u < 4; ++u) add(v[u], r + u * RS);
    }
    for (; r < rows; r += RS) add(*reinterpret_cast<const float2*>(part + ((long)r * C + c) * 2), r);
  }
  red[rl][cl][0] = s1;
  red[rl][cl][1] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int g = 1; g < 4; ++g) { s1 += red[g][cl][0]; s2 += red[g][cl][1]; }
    out[((long)blockIdx.y * C + c) * 2] = s1;
    out[((long)blockIdx.y * C + c) * 2 + 1] = s2;
  }
}

// the kRB row sums of channel c, added in row order; 16 rows' loads in flight at a time (one
// thread per channel: a dependent load -> add chain made each finalize launch ~8 us)
__device__ __forceinline__ void colsum_final(const double* ws, int C, int c, double& s1, double& s2) {
  s1 = 0.0; s2 = 0.0;
  const double2* p = reinterpret_cast<const double2*>(ws) + c;
#pragma unroll
  for (int r0 = 0; r0 < kRB; r0 += 16) {
    double2 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[(long)(r0 + i) * C];
#pragma unroll
    for (int i = 0; i < 16; ++i) { s1 += v[i].x; s2 += v[i].y; }
  }
}

// Stage 2: -> mean/invstd/scale/shift (+ running stats when training)
__device__ __forceinline__ void bn_finalize_one(int c, double s1, double s2, double count, const float* gamma,
                                                const float* beta, float* rmean, float* rvar, float momentum,
                                                float eps, float* scale, float* shift, float* mean_out,
                                                float* invstd_out) {
  const double mean = s1 / count;
  double var = s2 / count - mean * mean;
  if (var < 0) var = 0;
  const double inv = 1.0 / sqrt(var + (double)eps);
  scale[c] = (float)((double)gamma[c] * inv);
  shift[c] = (float)((double)beta[c] - mean * (double)gamma[c] * inv);
  mean_out[c] = (float)mean;
  invstd_out[c] = (float)inv;
  if (rmean) {
    const double unb = count > 1 ? var * count / (count - 1) : var;
    rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
    rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * unb);
  }
}
__global__ void bn_finalize_kernel(const double* ws, int C, double count, const float* gamma, const float* beta,
                                   float* rmean, float* rvar, long long* nbt, float momentum, float eps,
                                   float* scale, float* shift, float* mean_out, float* invstd_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (nbt && c == 0) *nbt += 1;
  if (c >= C) return;
  double s1, s2;
  colsum_final(ws, C, c, s1, s2);
  bn_finalize_one(c, s1, s2, count, gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean_out, invstd_out);
}

// Eval-mode BatchNorm folded into the conv before it (UNet3D.predict / inference,
// models/unet3d.py:298-344: BN over the running statistics is an affine map per output
// channel): w' = w sc, b' = b sc + sh, sc / sh in fp64 as bn_eval_coeffs_kernel forms them.
// w: [Cout][K] fp32 (torch layout, K = Cin x 27).
__global__ void bn_fold_kernel(const float* w, const float* b, const float* gamma, const float* beta,
                               const float* rmean, const float* rvar, float eps, int Cout, long K, float* wo,
                               float* bo) {
  const int co = blockIdx.y;
  const double inv = 1.0 / sqrt((double)rvar[co] + (double)eps);
  const double sc = (double)gamma[co] * inv;
  const float scf = (float)sc;
  for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < K; k += (long)gridDim.x * blockDim.x)
    wo[(long)co * K + k] = w[(long)co * K + k] * scf;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double sh = (double)beta[co] - (double)rmean[co] * sc;
    bo[co] = (float)((b ? (double)b[co] : 0.0) * sc + sh);
  }
}

__global__ void bn_eval_coeffs_kernel(const float* gamma, const float* beta, const float* rmean,
                                      const float* rvar, float eps, int C, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double inv = 1.0 / sqrt((double)rvar[c] + (double)eps);
  scale[c] = (float)((double)gamma[c] * inv);
  shift[c] = (float)((double)beta[c] - (double)rmean[c] * (double)gamma[c] * inv);
}

// a = relu(y * scale[c] + shift[c]); 16-byte vectors.  Block = (256 / CG) voxel lanes x
// CG channel groups, so every thread keeps its VEC channels' coefficients in registers.
// NT: non-temporal loads and stores for tensors far larger than the Infinity Cache
// (measured: level-0 bn_relu 90 -> 87 us; walking the voxels in reverse to catch the
// producer's cached tail bought nothing)
template <typename T, bool NT>
__global__ void __launch_bounds__(TPB) bn_relu_kernel(const T* y, T* a, const float* scale, const float* shift,
                                                      int C, long nvox) {
  constexpr int VEC = Elem<T>::kVec;
  const int CG = C / VEC;
  const int cg = threadIdx.x % CG, vl = threadIdx.x / CG, VL = TPB / CG;
  const int c0 = cg * VEC;
  float sc[VEC], sh[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sc[j] = scale[c0 + j]; sh[j] = shift[c0 + j]; }
  for (long v = (long)blockIdx.x * VL + vl; v < nvox; v += (long)gridDim.x * VL) {
    float x[VEC];
    ld16<NT>(y + v * C + c0, x);
#pragma unroll
    for (int j = 0; j < VEC; ++j) x[j] = bn_relu1(x[j], sc[j], sh[j]);
    st16<NT>(a + v * C + c0, x);
  }
}

// BN+ReLU backward, pass 1: per-block partial sums of g and g*xhat, g = da * [a > 0].
// Block: 256 threads = (256 / C8) voxel lanes x C8 channel groups of VEC channels.
template <typename T, bool NT>
__global__ void __launch_bounds__(TPB) bn_relu_bwd_reduce_kernel(
    const T* da, const T* y, const float* scale, const float* shift, const float* mean,
    const float* invstd, float* part, int C, long nvox) {
  constexpr int VEC = Elem<T>::kVec;
  __shared__ float red[TPB * VEC * 2];
  const int CG = C / VEC;
  const int cg = threadIdx.x % CG, vl = threadIdx.x / CG, VL = TPB / CG;
  const int c0 = cg * VEC;
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], sg[VEC], sgx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sc[j] = scale[c0 + j]; sh[j] = shift[c0 + j]; mu[j] = mean[c0 + j]; is[j] = invstd[c0 + j];
    sg[j] = 0.f; sgx[j] = 0.f;
  }
  // four voxel rows' loads in flight per trip, accumulated in the same voxel order as one
  // at a time (identical sums)
  const long stride = (long)gridDim.x * VL;
  long v = (long)blockIdx.x * VL + vl;
  auto acc1 = [&](const float (&dv)[VEC], const float (&yv)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float g = (yv[j] * sc[j] + sh[j] > 0.f) ? dv[j] : 0.f;
      sg[j] += g;
      sgx[j] += g * ((yv[j] - mu[j]) * is[j]);
    }
  };
#ifndef BNR_U
#define BNR_U 2  // voxel rows in flight per thread and trip (A/B: 1 / 4 / 8 slower, profiles/r4_bnr_unroll_ab.txt)
#endif
  for (; v + (BNR_U - 1) * stride < nvox; v += BNR_U * stride) {
    float dv[BNR_U][VEC], yv[BNR_U][VEC];
#pragma unroll
    for (int u = 0; u < BNR_U; ++u) {
      ld16<NT>(da + (v + u * stride) * C + c0, dv[u]);
      ld16<NT>(y + (v + u * stride) * C + c0, yv[u]);
    }
#pragma unroll
    for (int u = 0; u < BNR_U; ++u) acc1(dv[u], yv[u]);
  }
  for (; v < nvox; v += stride) {
    float dv[VEC], yv[VEC];
    load16<T>(da + v * C + c0, dv);
    load16<T>(y + v * C + c0, yv);
    acc1(dv, yv);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    red[(vl * C + c0 + j) * 2] = sg[j];
    red[(vl * C + c0 + j) * 2 + 1] = sgx[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += TPB) {
    float a = 0.f, b = 0.f;
    for (int l = 0; l < VL; ++l) { a += red[(l * C + c) * 2]; b += red[(l * C + c) * 2 + 1]; }
    part[((long)blockIdx.x * C + c) * 2] = a;
    part[((long)blockIdx.x * C + c) * 2 + 1] = b;
  }
}

// pass 2: fp64 column sums -> dgamma/dbeta (+=) and the apply coefficients
//   dy = k1*g + k2*xhat + k3, k1 = gamma*invstd, k2 = -k1*sum(g xhat)/M, k3 = -k1*sum(g)/M
__device__ __forceinline__ void bn_bwd_finalize_one(int c, double s1, double s2, double count, const float* gamma,
                                                    const float* invstd, float* dgamma, float* dbeta, float* coef) {
  dbeta[c] += (float)s1;
  dgamma[c] += (float)s2;
  const double k1 = (double)gamma[c] * (double)invstd[c];
  coef[c * 3 + 0] = (float)k1;
  coef[c * 3 + 1] = (float)(-k1 * s2 / count);
  coef[c * 3 + 2] = (float)(-k1 * s1 / count);
}
__global__ void bn_bwd_finalize_kernel(const double* ws, int C, double count, const float* gamma,
                                       const float* invstd, float* dgamma, float* dbeta, float* coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1, s2;
  colsum_final(ws, C, c, s1, s2);
  bn_bwd_finalize_one(c, s1, s2, count, gamma, invstd, dgamma, dbeta, coef);
}

// Few partial rows (<= kSmallRows): the column sums and the finalize in ONE launch, one block
// per 64 channels (no cross-block dependency): 4 row lanes x 64 channels, lane rl adds rows
// rl, rl + 4, ... in order (8 rows' loads in flight), the 4 lanes summed in a fixed order
// (deterministic).  Saves the second launch of the two-stage path (~5 us each, 36 per step).
constexpr int kSmallRows = 512;
// 16 row lanes x 64 channels per block: a thread sums every 16th partial row, 8 rows' loads
// in flight per trip (the sums were latency-bound chains of ~rows / 32 dependent trips on 4
// row lanes); the 16 lane sums are added in lane order
constexpr int kCfRL = 16;
// rows in flight per thread per trip (16: one trip for <= 256 rows, two for 512; 8 took up to
// four dependent trips of memory latency); the row order of every sum is the same for any value
#ifndef PCMS_CF_U
#define PCMS_CF_U 16
#endif
constexpr int kCfU = PCMS_CF_U;
template <bool BWD>
__global__ void __launch_bounds__(64 * kCfRL) colsum_finalize_small_kernel(
    const float* part, int rows, int C, const float* cnt, double count, const float* gamma, const float* beta,
    float* rmean, float* rvar, long long* nbt, float momentum, float eps, float* scale, float* shift,
    float* mean_out, float* invstd, float* dgamma, float* dbeta, float* coef) {
  __shared__ double red[kCfRL][64][2];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  if (!BWD && nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    int r = rl;
    for (; r < rows; r += kCfU * kCfRL) {  // the last trip predicated, loads still batched
      float2 v[kCfU];
      float nv[kCfU];
#pragma unroll
      for (int u = 0; u < kCfU; ++u)
        if (r + kCfRL * u < rows) {
          v[u] = *reinterpret_cast<const float2*>(part + ((long)(r + kCfRL * u) * C + c) * 2);
          nv[u] = cnt ? cnt[r + kCfRL * u] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < kCfU; ++u) {
        if (r + kCfRL * u >= rows) break;
        s1 += (double)v[u].x;
        if (cnt) {
          const double n = (double)nv[u];
          s2 += (double)v[u].y + (n > 0.0 ? (double)v[u].x * (double)v[u].x / n : 0.0);
        } else {
          s2 += (double)v[u].y;
        }
      }
    }
  }
  red[rl][cl][0] = s1;
  red[rl][cl][1] = s2;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int g = 1; g < kCfRL; ++g) { s1 += red[g][cl][0]; s2 += red[g][cl][1]; }
    if constexpr (BWD) bn_bwd_finalize_one(c, s1, s2, count, gamma, invstd, dgamma, dbeta, coef);
    else bn_finalize_one(c, s1, s2, count, gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean_out, invstd);
  }
}

#ifndef BNA_REV
#define BNA_REV 0
#endif
// pass 3: dy of every element (bn_bwd_dy, ops_units.h: the pool apply rounds the same way)
// NT: as bn_relu_kernel (level-0 apply: 805 MB in 118 us = 6.8 TB/s)
template <typename T, bool NT>
__global__ void __launch_bounds__(TPB) bn_relu_bwd_apply_kernel(
    const T* da, const T* y, const float* scale, const float* shift, const float* mean, const float* invstd,
    const float* coef, T* dy, int C, long nvox) {
  constexpr int VEC = Elem<T>::kVec;
  const int CG = C / VEC;
  const int cg = threadIdx.x % CG, vl = threadIdx.x / CG, VL = TPB / CG;
  const int c0 = cg * VEC;
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], k1[VEC], k2[VEC], k3[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = c0 + j;
    sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; is[j] = invstd[c];
    k1[j] = coef[c * 3]; k2[j] = coef[c * 3 + 1]; k3[j] = coef[c * 3 + 2];
  }
  for (long v0 = (long)blockIdx.x * VL + vl; v0 < nvox; v0 += (long)gridDim.x * VL) {
    // BNA_REV: walk the voxels from the end -- the reduce pass before this one finishes at the
    // high voxels, so what it left in the Infinity Cache is read first (elementwise: any order
    // gives the same bits)
    const long v = BNA_REV ? nvox - 1 - v0 : v0;
    float dv[VEC], yv[VEC], o[VEC];
    ld16<NT>(da + v * C + c0, dv);
    ld16<NT>(y + v * C + c0, yv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_bwd_dy(dv[j], yv[j], sc[j], sh[j], mu[j], is[j], k1[j], k2[j], k3[j]);
    st16<NT>(dy + v * C + c0, o);
  }
}

// Eval-mode BatchNorm + ReLU backward (running statistics, so the coefficients are constants:
// a pure apply, no reduction): dy = da * scale where relu(y scale + shift) passed, else 0 -- the
// mask from the forward's own expression (bn_bwd_eval_dy).  The input-gradient backward of an
// eval forward (saliency): no parameter gradient is formed.
template <typename T, bool NT>
__global__ void __launch_bounds__(TPB) bn_relu_bwd_eval_kernel(const T* da, const T* y, const float* scale,
                                                               const float* shift, T* dy, int C, long nvox) {
  constexpr int VEC = Elem<T>::kVec;
  const int CG = C / VEC;
  const int cg = threadIdx.x % CG, vl = threadIdx.x / CG, VL = TPB / CG;
  const int c0 = cg * VEC;
  float sc[VEC], sh[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sc[j] = scale[c0 + j]; sh[j] = shift[c0 + j]; }
  for (long v = (long)blockIdx.x * VL + vl; v < nvox; v += (long)gridDim.x * VL) {
    float dv[VEC], yv[VEC], o[VEC];
    ld16<NT>(da + v * C + c0, dv);
    ld16<NT>(y + v * C + c0, yv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_bwd_eval_dy(dv[j], yv[j], sc[j], sh[j]);
    st16<NT>(dy + v * C + c0, o);
  }
}

}  // namespace

int g_stream_grid_cap = INT_MAX;

// the BN-backward reduce passes' block cap (their partial-row count): kSmallRows (512, the
// product: the finalize is one launch; round 6 kernel trace -15 us per step vs 2048,
// profiles/r6_bn_rows_cap_ab.txt) or more (two-stage finalize)
#ifndef PCMS_BN_ROWS_CAP
#define PCMS_BN_ROWS_CAP 512
#endif
int g_bn_rows_cap = PCMS_BN_ROWS_CAP;

int bn_bwd_finalize2_launch(const float* part, int rows, int C, double count, const float* gamma,
                            const float* invstd, float* dgamma, float* dbeta, float* coef, double* ws, hipStream_t s) {
  PCMS_LAUNCH(colsum2_kernel, dim3(cdiv(C, 64), kRB), dim3(256), 0, s, part, rows, C, (const float*)nullptr, ws);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, (const double*)ws, C, count, gamma,
                     invstd, dgamma, dbeta, coef);
  PCMS_CHECK_LAUNCH();
}

// the elementwise passes: their grid (four voxel rows per thread), and whether the tensor is
// large enough to stream past the caches
static int ew_grid(int dtype, int C, long nvox) {
  const int VL = TPB / (C / vec_of(dtype));
  return stream_grid(nvox, VL * 4, 8192);
}
static bool bn_nt(int dtype, int C, long nvox) { return nvox * C * bytes_of(dtype) >= kNtBytesBn; }

extern "C" {

// A/B switch: v <= 0 queries, returns the old value; set before the workspace queries
int pcms_bn_bwd_rows_cap(int v) {
  const int old = g_bn_rows_cap;
  if (v > 0) g_bn_rows_cap = v;
  return old;
}

// test switch: an extra cap on every grid and row count of the ops units (stream_grid), so
// that the capped-grid regimes of the streaming kernels are reachable at a small shape;
// v <= 0 queries, returns the old value; default INT_MAX (no extra cap); set before the
// workspace queries
int pcms_stream_grid_cap(int v) {
  const int old = g_stream_grid_cap;
  if (v > 0) g_stream_grid_cap = v;
  return old;
}

int pcms_bn_finalize(const float* part, int rows, int C, double count, const float* gamma, const float* beta,
                     float* rmean, float* rvar, long long* nbt, float momentum, float eps,
                     float* scale, float* shift, float* mean, float* invstd, double* ws, hipStream_t s) {
  const float* cnt = part + (long)rows * C * 2;
  if (rows <= kSmallRows) {
    hipLaunchKernelGGL(colsum_finalize_small_kernel<false>, dim3(cdiv(C, 64)), dim3(64 * kCfRL), 0, s, part, rows, C,
                       cnt, count, gamma, beta, rmean, rvar, nbt, momentum, eps, scale, shift, mean, invstd, nullptr,
                       nullptr, nullptr);
    PCMS_CHECK_LAUNCH();
  }
  PCMS_LAUNCH(colsum2_kernel, dim3(cdiv(C, 64), kRB), dim3(256), 0, s, part, rows, C, cnt, ws);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, (const double*)ws, C, count, gamma,
                     beta, rmean, rvar, nbt, momentum, eps, scale, shift, mean, invstd);
  PCMS_CHECK_LAUNCH();
}

int pcms_bn_ws_doubles(int C) { return kRB * C * 2; }

int pcms_bn_fold(const float* w, const float* b, const float* gamma, const float* beta, const float* rmean,
                 const float* rvar, float eps, int Cout, long K, float* wo, float* bo, hipStream_t s) {
  if (Cout <= 0 || K <= 0) return -1;
  hipLaunchKernelGGL(bn_fold_kernel, dim3(stream_grid(K, 256, 64), Cout), dim3(256), 0, s, w, b, gamma, beta, rmean, rvar,
                     eps, Cout, K, wo, bo);
  PCMS_CHECK_LAUNCH();
}

int pcms_bn_eval_coeffs(const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                        int C, float* scale, float* shift, hipStream_t s) {
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, gamma, beta, rmean, rvar, eps, C, scale, shift);
  PCMS_CHECK_LAUNCH();
}

int pcms_bn_relu(int dtype, const void* y, void* a, const float* scale, const float* shift, int C, long nvox,
                 hipStream_t s) {
  const int VEC = vec_of(dtype);
  if (C % VEC || TPB % (C / VEC)) return -1;
  const int grid = ew_grid(dtype, C, nvox);
  return for_stream(dtype, bn_nt(dtype, C, nvox), [&](auto t, auto p) {
    using T = decltype(t);
    hipLaunchKernelGGL((bn_relu_kernel<T, decltype(p)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)y, (T*)a, scale,
                       shift, C, nvox);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_bn_relu_bwd_eval(int dtype, const void* da, const void* y, const float* scale, const float* shift, void* dy,
                          int C, long nvox, hipStream_t s) {
  const int VEC = vec_of(dtype);
  if ((dtype != PCMS_BF16 && dtype != PCMS_F32) || C <= 0 || C % VEC || TPB % (C / VEC) || nvox < 1) return -1;
  if (!da || !y || !scale || !shift || !dy) return -2;
  const int grid = ew_grid(dtype, C, nvox);
  return for_stream(dtype, bn_nt(dtype, C, nvox), [&](auto t, auto p) {
    using T = decltype(t);
    hipLaunchKernelGGL((bn_relu_bwd_eval_kernel<T, decltype(p)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)da,
                       (const T*)y, scale, shift, (T*)dy, C, nvox);
    PCMS_CHECK_LAUNCH();
  });
}

// number of partial rows pcms_bn_relu_bwd_reduce writes (caller sizes `part`)
int pcms_bn_bwd_rows(int dtype, int C, long nvox) {
  const int VL = TPB / (C / vec_of(dtype));
  // small (deep) grids: one trip of 4 rows per thread and 4x the blocks (a block's reduction
  // is a chain of memory latencies), as long as the rows stay on the one-launch finalize
  const int small = stream_grid(nvox, VL * 4, 2048);
  return small <= kSmallRows ? small : stream_grid(nvox, VL * 16, g_bn_rows_cap);
}

int pcms_bn_relu_bwd(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                     const float* mean, const float* invstd, const float* gamma, float* part, float* coef,
                     float* dgamma, float* dbeta, void* dy, int C, long nvox, double* ws, hipStream_t s) {
  const int VEC = vec_of(dtype);
  if (C % VEC || (TPB % (C / VEC)) != 0) return -1;
  const int rows = pcms_bn_bwd_rows(dtype, C, nvox);
  // the reduce keeps the default cache policy: what it leaves in the Infinity Cache the apply
  // pass below re-reads (measured: nt here 99 us but the apply 118 -> 135 us at level 0)
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    PCMS_LAUNCH((bn_relu_bwd_reduce_kernel<T, false>), dim3(rows), dim3(TPB), 0, s, (const T*)da, (const T*)y, scale,
                shift, mean, invstd, part, C, nvox);
    return pcms_bn_relu_bwd_finish(dtype, da, y, scale, shift, mean, invstd, gamma, part, rows, coef, dgamma, dbeta,
                                   dy, C, nvox, ws, s);
  });
}

int pcms_bn_relu_bwd_finish(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                            const float* mean, const float* invstd, const float* gamma, const float* part, int rows,
                            float* coef, float* dgamma, float* dbeta, void* dy, int C, long nvox, double* ws,
                            hipStream_t s) {
  const int VEC = vec_of(dtype);
  if (C % VEC || (TPB % (C / VEC)) != 0) return -1;
  if (rows <= kSmallRows) {
    PCMS_LAUNCH(colsum_finalize_small_kernel<true>, dim3(cdiv(C, 64)), dim3(64 * kCfRL), 0, s, part, rows, C,
                (const float*)nullptr, (double)nvox, gamma, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, nullptr,
                nullptr, nullptr, const_cast<float*>(invstd), dgamma, dbeta, coef);
  } else {
    const int rc = bn_bwd_finalize2_launch(part, rows, C, (double)nvox, gamma, invstd, dgamma, dbeta, coef, ws, s);
    if (rc != 0) return rc;
  }
  if (dy == nullptr) return 0;  // dy NULL: the consumer applies (coef)
  const int grid = ew_grid(dtype, C, nvox);
  return for_stream(dtype, bn_nt(dtype, C, nvox), [&](auto t, auto p) {
    using T = decltype(t);
    hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<T, decltype(p)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)da,
                       (const T*)y, scale, shift, mean, invstd, (const float*)coef, (T*)dy, C, nvox);
    PCMS_CHECK_LAUNCH();
  });
}

}  // extern "C"
