// The 1x1x1 output conv of the U-Net step (NDHWC in, NCDHW fp32 logits out; gfx950), forward
// and backward, alone and fused with the decoder's last BatchNorm + ReLU.
//
// Reference op replaced (path relative to the reference repo):
//   outc Conv3d(64, ncls, 1)      models/unet3d.py:222
// Every launch here is grid-stride with a capped grid (stream_grid, ops_units.h).
#include "ops_units.h"
#include "pcms_hip.h"

namespace {

// ---------------- output head: logits (NCDHW fp32) = b + a . w ----------------
// 8 lanes per voxel, 8 channels each (Cin = 64); NC = n_classes (<= 4, a template argument
// so per-class registers exist only for real classes).  Every kernel walks kHU voxels per
// trip with all of their loads (activations and, backward, dlogits) issued before the first
// use: these are pure streams, bound by bytes in flight per CU.
constexpr int kHU = 4;

template <typename T, bool NT>
__device__ __forceinline__ void head_ld(const T* p, float (&x)[8]) {
  ld16<NT>(p, x);
  if constexpr (sizeof(T) == 4) ld16<NT>(p + 4, x + 4);
}
template <typename T, bool NT>
__device__ __forceinline__ void head_st(T* p, const float (&x)[8]) {
  st16<NT>(p, x);
  if constexpr (sizeof(T) == 4) st16<NT>(p + 4, x + 4);
}

// act 0: logits; 1: sigmoid(logits) (UNet3D.predict, models/unet3d.py:298-318); 2:
// (sigmoid(logits) > thr) as 0 / 1 (UNet3D.inference, :320-344) -- the eval outputs leave the
// head kernel finished.
// BN: ``a`` is the decoder's last pre-BN conv output y2 and the head applies that block's
// BatchNorm + ReLU itself (models/unet3d.py:37-39 fused into :222): a = round_T(relu(y sc +
// sh)), the value the bn_relu pass would have stored, so the logits are bit-identical and
// the a2 tensor (the largest activation of the step) is never written or read.
// voxel v of an (N, nvox) grid as (sample q, voxel-in-sample r), stepped without a division
// per voxel (the heads index the NCDHW logit gradient by both; a runtime 32-bit division per
// lane and voxel was a large share of their VALU)
struct VoxQR {
  uint32_t q, r, nv;
  __device__ VoxQR(long v, long nvox) : q((uint32_t)(v / nvox)), r((uint32_t)(v % nvox)), nv((uint32_t)nvox) {}
  __device__ void advance(uint32_t k) {
    r += k;
    while (r >= nv) { r -= nv; ++q; }
  }
  __device__ VoxQR plus(uint32_t k) const {
    VoxQR o = *this;
    o.advance(k);
    return o;
  }
};

template <typename T, bool NT, bool BN, int NC>
__global__ void __launch_bounds__(TPB, 3) head_fwd_kernel(const T* a, const float* w, const float* b, float* logits,
                                                       long nvox_per_n, int N, int act, float thr,
                                                       const float* bn_scale, const float* bn_shift) {
  const long total = (long)N * nvox_per_n;
  const int sub = threadIdx.x & 7;
  float sc[8], sh[8], wk[NC][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (BN) { sc[j] = bn_scale[sub * 8 + j]; sh[j] = bn_shift[sub * 8 + j]; }
#pragma unroll
    for (int k = 0; k < NC; ++k) wk[k][j] = w[k * 64 + sub * 8 + j];
  }
  auto one = [&](const VoxQR& p, float (&x)[8]) {
    if constexpr (BN) {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = round_st<T>(bn_relu1(x[j], sc[j], sh[j]));
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += x[j] * wk[k][j];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (sub == 0) {
        float o = s + b[k];
        if (act != 0) {
          const float pr = 1.f / (1.f + expf(-o));
          o = act == 1 ? pr : (pr > thr ? 1.f : 0.f);
        }
        logits[((long)p.q * NC + k) * nvox_per_n + p.r] = o;
      }
    }
  };
  const long stride = ((long)gridDim.x * blockDim.x) >> 3;
  long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 3;
  VoxQR pv(v, nvox_per_n);
  for (; v + (kHU - 1) * stride < total; v += kHU * stride) {
    float x[kHU][8];
#pragma unroll
    for (int u = 0; u < kHU; ++u) head_ld<T, NT>(a + (v + u * stride) * 64 + sub * 8, x[u]);
#pragma unroll
    for (int u = 0; u < kHU; ++u) one(u ? pv.plus((uint32_t)(u * stride)) : pv, x[u]);
    pv.advance((uint32_t)(kHU * stride));
  }
  for (; v < total; v += stride) {
    float x[8];
    head_ld<T, NT>(a + v * 64 + sub * 8, x);
    one(pv, x);
    pv.advance((uint32_t)stride);
  }
}

// da[v, c] = sum_k dl[k, v] w[k, c]  (written);  per-block partials of dw[k, c] = sum_v dl a,
// db[k] = sum_v dl.  NT: non-temporal a / da streams (level-0 sized).
// BN (the decoder's last BatchNorm + ReLU fused, see head_fwd_kernel): ``a`` is y2; the head
// input a2 = round_T(relu(y sc + sh)) is recomputed, da is NOT written: its round_T value
// feeds the BatchNorm-backward partial sums directly -- per block one row [64][2] of
// (sum g, sum g xhat), g = da [y sc + sh > 0], xhat = (y - mean) invstd -- and
// head_bn_apply_kernel recomputes da from dlogits (rank NC) instead of re-reading it.
struct HeadBN {
  const float *scale, *shift, *mean, *invstd;
  float* part;  // [blocks][64][2]
};
template <typename T, bool NT, bool BN, int NC>
__global__ void __launch_bounds__(TPB, (BN && NC > 2) ? 2 : 3) head_bwd_kernel(const T* a, const float* dlogits, const float* w,
                                                       T* da, float* part, long nvox_per_n, int N, HeadBN bn) {
  __shared__ float red[TPB / 64][NC][65];
  __shared__ float bred[TPB / 64][64][2];
  const long total = (long)N * nvox_per_n;
  const int sub = threadIdx.x & 7, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float accw[NC][8], accb[NC], wk[NC][8];
  float sc[8], sh[8], mu[8], is[8], sg[8], sgx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int k = 0; k < NC; ++k) { accw[k][j] = 0.f; wk[k][j] = w[k * 64 + sub * 8 + j]; }
    if constexpr (BN) {
      const int c = sub * 8 + j;
      sc[j] = bn.scale[c]; sh[j] = bn.shift[c]; mu[j] = bn.mean[c]; is[j] = bn.invstd[c];
      sg[j] = 0.f; sgx[j] = 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) accb[k] = 0.f;
  auto ld_dl = [&](const VoxQR& p, float (&dl)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k) dl[k] = dlogits[((long)p.q * NC + k) * nvox_per_n + p.r];
  };
  // channel pairs in packed fp32 (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: the same IEEE
  // operation per element as the scalar forms, half the VALU issue; the kernel was VALU-bound)
  // and one v_cvt_pk_bf16_f32 per pair for the T rounding
  auto round2 = [](f32x2_t v) -> f32x2_t {
    if constexpr (sizeof(T) == 2) {
      const uint32_t u = pack_bf16x2(v[0], v[1]);
      return (f32x2_t){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
    } else {
      return v;
    }
  };
  auto one = [&](long v, const float (&x)[8], const float (&dl)[NC]) {
    float o[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x2_t x2 = {x[2 * q], x[2 * q + 1]};
      f32x2_t z2 = {0.f, 0.f}, av2 = x2;
      if constexpr (BN) {
        z2 = __builtin_elementwise_fma(x2, (f32x2_t){sc[2 * q], sc[2 * q + 1]}, (f32x2_t){sh[2 * q], sh[2 * q + 1]});
        av2 = round2((f32x2_t){fmaxf(z2[0], 0.f), fmaxf(z2[1], 0.f)});
      }
      f32x2_t o2 = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const f32x2_t d2 = {dl[k], dl[k]};
        o2 = __builtin_elementwise_fma(d2, (f32x2_t){wk[k][2 * q], wk[k][2 * q + 1]}, o2);
        const f32x2_t a2 = __builtin_elementwise_fma(d2, av2, (f32x2_t){accw[k][2 * q], accw[k][2 * q + 1]});
        accw[k][2 * q] = a2[0];
        accw[k][2 * q + 1] = a2[1];
      }
      if constexpr (BN) {
        const f32x2_t r2 = round2(o2);
        const f32x2_t g2 = {z2[0] > 0.f ? r2[0] : 0.f, z2[1] > 0.f ? r2[1] : 0.f};
        const f32x2_t t2 = (x2 - (f32x2_t){mu[2 * q], mu[2 * q + 1]}) * (f32x2_t){is[2 * q], is[2 * q + 1]};
        // sum g xhat as a product then a sum (not fused), as the separate reduce pass forms it
        f32x2_t sgx2 = {sgx[2 * q], sgx[2 * q + 1]}, sg2 = {sg[2 * q], sg[2 * q + 1]};
        {
#pragma clang fp contract(off)
          sgx2 = sgx2 + g2 * t2;
          sg2 = sg2 + g2;
        }
        sg[2 * q] = sg2[0]; sg[2 * q + 1] = sg2[1];
        sgx[2 * q] = sgx2[0]; sgx[2 * q + 1] = sgx2[1];
      }
      o[2 * q] = o2[0];
      o[2 * q + 1] = o2[1];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (sub == 0) accb[k] += dl[k];
    if constexpr (!BN) head_st<T, NT>(da + v * 64 + sub * 8, o);
  };
  const long stride = ((long)gridDim.x * blockDim.x) >> 3;
  long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 3;
  VoxQR pv(v, nvox_per_n);
#ifndef HEADB_U
#define HEADB_U 2
#endif
  constexpr int U = NC > 2 ? 1 : (BN || NC > 1) ? HEADB_U : kHU;  // (registers: the BN form holds 6 x 8 per-channel values)
#pragma unroll 1
  for (; v + (U - 1) * stride < total; v += U * stride) {
    float x[U][8], dl[U][NC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      head_ld<T, NT>(a + (v + u * stride) * 64 + sub * 8, x[u]);
      ld_dl(u ? pv.plus((uint32_t)(u * stride)) : pv, dl[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(v + u * stride, x[u], dl[u]);
    pv.advance((uint32_t)(U * stride));
  }
  for (; v < total; v += stride) {
    float x[8], dl[NC];
    head_ld<T, NT>(a + v * 64 + sub * 8, x);
    ld_dl(pv, dl);
    one(v, x, dl);
    pv.advance((uint32_t)stride);
  }
  // reduce accw over the 8 voxel-lanes of each wave that share `sub`
#pragma unroll
  for (int k = 0; k < NC; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = accw[k][j];
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 8) red[wave][k][sub * 8 + j] = s;
    }
    float sb = wave_sum(accb[k]);
    if (lane == 0) red[wave][k][64] = sb;
  }
  if constexpr (BN) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s1 = sg[j], s2 = sgx[j];
      s1 += __shfl_xor(s1, 8, 64); s2 += __shfl_xor(s2, 8, 64);
      s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
      s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
      if (lane < 8) { bred[wave][sub * 8 + j][0] = s1; bred[wave][sub * 8 + j][1] = s2; }
    }
  }
  __syncthreads();
  // this block's partial row [NC][65] (dw row k, then db[k]); rows_sum_kernel adds the rows
  // in block order
  for (int idx = threadIdx.x; idx < NC * 65; idx += TPB) {
    const int k = idx / 65, c = idx % 65;
    float s = 0.f;
    for (int wv = 0; wv < TPB / 64; ++wv) s += red[wv][k][c];
    part[(long)blockIdx.x * NC * 65 + idx] = s;
  }
  if constexpr (BN) {
    if (threadIdx.x < 128) {
      const int c = threadIdx.x >> 1, q = threadIdx.x & 1;
      float s = 0.f;
      for (int wv = 0; wv < TPB / 64; ++wv) s += bred[wv][c][q];
      bn.part[((long)blockIdx.x * 64 + c) * 2 + q] = s;
    }
  }
}

// BN-backward apply of the decoder's last BatchNorm + ReLU from the head's gradient, which is
// recomputed per voxel from dlogits (da[v, c] = sum_k dl[k, v] w[k, c], rounded to T exactly as
// head_bwd_kernel would have stored it) instead of being written and read back:
// dy = k1 g + k2 xhat + k3, g = da [y sc + sh > 0] (bn_relu_bwd_apply_kernel's arithmetic).
template <typename T, bool NT, int NC>
__global__ void __launch_bounds__(TPB, 2) head_bn_apply_kernel(const T* y, const float* dlogits, const float* w,
                                                            const float* scale, const float* shift,
                                                            const float* mean, const float* invstd,
                                                            const float* coef, T* dy, long nvox_per_n, int N) {
  const long total = (long)N * nvox_per_n;
  const int sub = threadIdx.x & 7;
  // dy = k1 g + A (y - mean) + k3 with A = k2 invstd: the centred form (A y + (k3 - A mean)
  // loses ~eps |mean| / std to cancellation when |mean| >> std); six per-channel values held
  float sc[8], sh[8], k1[8], A[8], mu[8], k3[8], wk[NC][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = sub * 8 + j;
    sc[j] = scale[c]; sh[j] = shift[c];
    k1[j] = coef[c * 3];
    A[j] = coef[c * 3 + 1] * invstd[c];
    mu[j] = mean[c];
    k3[j] = coef[c * 3 + 2];
#pragma unroll
    for (int k = 0; k < NC; ++k) wk[k][j] = w[k * 64 + c];
  }
  auto ld_dl = [&](const VoxQR& p, float (&dl)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k) dl[k] = dlogits[((long)p.q * NC + k) * nvox_per_n + p.r];
  };
  auto one = [&](long v, const float (&x)[8], const float (&dl)[NC]) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += dl[k] * wk[k][j];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float g = (x[j] * sc[j] + sh[j] > 0.f) ? round_st<T>(o[j]) : 0.f;
      o[j] = k1[j] * g + (A[j] * (x[j] - mu[j]) + k3[j]);
    }
    head_st<T, NT>(dy + v * 64 + sub * 8, o);
  };
  const long stride = ((long)gridDim.x * blockDim.x) >> 3;
  long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 3;
  VoxQR pv(v, nvox_per_n);
#ifndef HEADA_U
#define HEADA_U 2
#endif
  constexpr int U = NC > 1 ? 1 : HEADA_U;  // (registers: 5 x 8 per-channel values + NC x 8 weights held)
#pragma unroll 1
  for (; v + (U - 1) * stride < total; v += U * stride) {
    float x[U][8], dl[U][NC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      head_ld<T, NT>(y + (v + u * stride) * 64 + sub * 8, x[u]);
      ld_dl(u ? pv.plus((uint32_t)(u * stride)) : pv, dl[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(v + u * stride, x[u], dl[u]);
    pv.advance((uint32_t)(U * stride));
  }
  for (; v < total; v += stride) {
    float x[8], dl[NC];
    head_ld<T, NT>(y + v * 64 + sub * 8, x);
    ld_dl(pv, dl);
    one(v, x, dl);
    pv.advance((uint32_t)stride);
  }
}

// Eval-mode backward of the fused head (head_fwd_kernel<BN>) down to the last decoder block's
// pre-BN conv output y: dy[v, c] = (sum_k dl[k, v] w[k, c]) * scale[c] where relu(y scale +
// shift) passed, else 0 (bn_bwd_eval_dy).  One pass over y and dlogits; the block's ReLU output
// was never stored and no parameter gradient is written.
template <typename T, bool NT, int NC>
__global__ void __launch_bounds__(TPB, 2) head_bn_bwd_eval_kernel(const T* y, const float* dlogits, const float* w,
                                                               const float* scale, const float* shift, T* dy,
                                                               long nvox_per_n, int N) {
  const long total = (long)N * nvox_per_n;
  const int sub = threadIdx.x & 7;
  float sc[8], sh[8], wk[NC][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = sub * 8 + j;
    sc[j] = scale[c]; sh[j] = shift[c];
#pragma unroll
    for (int k = 0; k < NC; ++k) wk[k][j] = w[k * 64 + c];
  }
  const long stride = ((long)gridDim.x * blockDim.x) >> 3;
  long v = (blockIdx.x * (long)blockDim.x + threadIdx.x) >> 3;
  VoxQR pv(v, nvox_per_n);
  for (; v < total; v += stride) {
    float x[8], dl[NC], o[8];
    head_ld<T, NT>(y + v * 64 + sub * 8, x);
#pragma unroll
    for (int k = 0; k < NC; ++k) dl[k] = dlogits[((long)pv.q * NC + k) * nvox_per_n + pv.r];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += dl[k] * wk[k][j];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bn_bwd_eval_dy(o[j], x[j], sc[j], sh[j]);
    head_st<T, NT>(dy + v * 64 + sub * 8, o);
    pv.advance((uint32_t)stride);
  }
}

// dw[k][c] += col (k, c), db[k] += col (k, 64) of the summed head partial rows
__global__ void head_bwd_finish_kernel(const float* sums, int ncls, float* dw, float* db) {
  const int idx = threadIdx.x;
  if (idx >= ncls * 65) return;
  const int k = idx / 65, c = idx % 65;
  if (c < 64) dw[k * 64 + c] += sums[idx];
  else db[k] += sums[idx];
}

// f(std::integral_constant<int, NC>{}) for NC = n_classes, a template argument of the head
// kernels (1..4); -1 for any other ncls
template <int NC = 1, typename F>
int with_ncls(int ncls, F&& f) {
  if constexpr (NC > 4) return -1;
  else return ncls == NC ? f(std::integral_constant<int, NC>{}) : with_ncls<NC + 1>(ncls, f);
}
// a head launch site: f(T{}, NT{}, NC{}) for the storage, the cache policy and n_classes
template <typename F>
int for_head(int dtype, bool nt, int ncls, F&& f) {
  return for_stream(dtype, nt, [&](auto t, auto p) { return with_ncls(ncls, [&](auto nc) { return f(t, p, nc); }); });
}
// the head's streams (64 channels per voxel) bypass the caches from kNtBytes on
bool head_nt(int dtype, long nvox) { return nvox * 64 * bytes_of(dtype) >= kNtBytes; }

// BN: the fused form (sc / sh: the decoder's last BatchNorm coefficients)
template <bool BN>
int head_fwd_any(int dtype, const void* a, const float* w, const float* b, float* out, long nvox_per_n, int N, int ncls,
                 int act, float thr, const float* sc, const float* sh, hipStream_t s) {
  if ((long)N * nvox_per_n >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  if (act < 0 || act > 2) return -1;
  const int grid = stream_grid((long)N * nvox_per_n * 8, TPB);
  return for_head(dtype, head_nt(dtype, (long)N * nvox_per_n), ncls, [&](auto t, auto p, auto nc) {
    using T = decltype(t);
    hipLaunchKernelGGL((head_fwd_kernel<T, decltype(p)::value, BN, decltype(nc)::value>), dim3(grid), dim3(TPB), 0, s,
                       (const T*)a, w, b, out, nvox_per_n, N, act, thr, sc, sh);
    PCMS_CHECK_LAUNCH();
  });
}

int head_bwd_rows(long nvox) { return stream_grid(nvox * 8, TPB, 2048); }

// the head partial rows [grid][ncls][65] -> dw[k][c] += (k, c), db[k] += (k, 64)
int head_finish(int grid, float* ws, int ncls, float* dw, float* db, hipStream_t s) {
  float* sums = ws + (long)grid * ncls * 65;
  if (const int rc = rows_sum_launch(false, ws, grid, ncls * 65, sums, s)) return rc;
  hipLaunchKernelGGL(head_bwd_finish_kernel, dim3(1), dim3(320), 0, s, (const float*)sums, ncls, dw, db);
  PCMS_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int pcms_head_fwd(int dtype, const void* a, const float* w, const float* b, float* out, long nvox_per_n, int N,
                  int ncls, int act, float thr, hipStream_t s) {
  return head_fwd_any<false>(dtype, a, w, b, out, nvox_per_n, N, ncls, act, thr, nullptr, nullptr, s);
}

int pcms_head_bn_fwd(int dtype, const void* y, const float* scale, const float* shift, const float* w,
                     const float* b, float* out, long nvox_per_n, int N, int ncls, int act, float thr,
                     hipStream_t s) {
  if (scale == nullptr || shift == nullptr) return -2;
  return head_fwd_any<true>(dtype, y, w, b, out, nvox_per_n, N, ncls, act, thr, scale, shift, s);
}

// workspace: the per-block partial rows + one summed row
int pcms_head_bwd_ws_floats(long nvox_per_n, int N, int ncls) {
  return (head_bwd_rows((long)N * nvox_per_n) + 1) * ncls * 65;
}

int pcms_head_bwd(int dtype, const void* a, const float* dlogits, const float* w, void* da, float* dw, float* db,
                  float* ws, long nvox_per_n, int N, int ncls, hipStream_t s) {
  if ((long)N * nvox_per_n >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  if (ncls > 4 || ncls < 1) return -1;
  if (ws == nullptr) return -2;
  const long nvox = (long)N * nvox_per_n;
  const int grid = head_bwd_rows(nvox);
  return for_head(dtype, head_nt(dtype, nvox), ncls, [&](auto t, auto p, auto nc) {
    using T = decltype(t);
    PCMS_LAUNCH((head_bwd_kernel<T, decltype(p)::value, false, decltype(nc)::value>), dim3(grid), dim3(TPB), 0, s,
                (const T*)a, dlogits, w, (T*)da, ws, nvox_per_n, N, HeadBN{});
    return head_finish(grid, ws, ncls, dw, db, s);
  });
}

int pcms_head_bn_bwd_rows(long nvox_per_n, int N) { return head_bwd_rows((long)N * nvox_per_n); }

int pcms_head_bn_bwd(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                     const float* invstd, const float* gamma, const float* dlogits, const float* w, float* dw,
                     float* db, float* ws, float* bnpart, float* coef, float* dgamma, float* dbeta, void* dy,
                     long nvox_per_n, int N, int ncls, double* bnws, hipStream_t s) {
  if ((long)N * nvox_per_n >= (1L << 31)) return -7;  // 32-bit index math in the kernels
  if (ncls > 4 || ncls < 1) return -1;
  if (ws == nullptr || bnpart == nullptr || bnws == nullptr || coef == nullptr) return -2;
  const long nvox = (long)N * nvox_per_n;
  const int grid = head_bwd_rows(nvox);
  const HeadBN bn{scale, shift, mean, invstd, bnpart};
  // pass 1: head weight / bias partials + BatchNorm-backward partial sums (reads y2, dlogits;
  // always the cached form), their row sums, then the BatchNorm coefficients
  int rc = for_head(dtype, false, ncls, [&](auto t, auto p, auto nc) {
    using T = decltype(t);
    PCMS_LAUNCH((head_bwd_kernel<T, decltype(p)::value, true, decltype(nc)::value>), dim3(grid), dim3(TPB), 0, s,
                (const T*)y, dlogits, w, (T*)nullptr, ws, nvox_per_n, N, bn);
    return head_finish(grid, ws, ncls, dw, db, s);
  });
  if (rc != 0) return rc;
  rc = bn_bwd_finalize2_launch(bnpart, grid, 64, (double)nvox, gamma, invstd, dgamma, dbeta, coef, bnws, s);
  if (rc != 0) return rc;
  // pass 2: dy of the BatchNorm input (reads y2, dlogits)
  const int agrid = stream_grid(nvox * 8, TPB);
  return for_head(dtype, head_nt(dtype, nvox), ncls, [&](auto t, auto p, auto nc) {
    using T = decltype(t);
    hipLaunchKernelGGL((head_bn_apply_kernel<T, decltype(p)::value, decltype(nc)::value>), dim3(agrid), dim3(TPB), 0, s,
                       (const T*)y, dlogits, w, scale, shift, mean, invstd, (const float*)coef, (T*)dy, nvox_per_n, N);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_head_bn_bwd_eval(int dtype, const void* y, const float* scale, const float* shift, const float* dlogits,
                          const float* w, void* dy, long nvox_per_n, int N, int ncls, hipStream_t s) {
  if ((long)N * nvox_per_n >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  if (ncls > 4 || ncls < 1 || N < 1 || nvox_per_n < 1 || (dtype != PCMS_BF16 && dtype != PCMS_F32)) return -1;
  if (!y || !scale || !shift || !dlogits || !w || !dy) return -2;
  const long nvox = (long)N * nvox_per_n;
  const int grid = stream_grid(nvox * 8, TPB);
  return for_head(dtype, head_nt(dtype, nvox), ncls, [&](auto t, auto p, auto nc) {
    using T = decltype(t);
    hipLaunchKernelGGL((head_bn_bwd_eval_kernel<T, decltype(p)::value, decltype(nc)::value>), dim3(grid), dim3(TPB), 0,
                       s, (const T*)y, dlogits, w, scale, shift, (T*)dy, nvox_per_n, N);
    PCMS_CHECK_LAUNCH();
  });
}

}  // extern "C"
