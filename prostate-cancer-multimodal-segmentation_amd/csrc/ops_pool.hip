// MaxPool3d(2) of the U-Net step (NDHWC, gfx950), forward and backward, and its fusions with the
// BatchNorm + ReLU of the block whose output is pooled: the forward apply, the backward
// reduction and the backward apply per 2x2x2 cell.
//
// Reference op replaced (path relative to the reference repo):
//   MaxPool3d(2)                  models/unet3d.py:80
// Every launch here is grid-stride with a capped grid (stream_grid, ops_units.h).
#include "ops_units.h"
#include "pcms_hip.h"

namespace {

// ---------------- MaxPool3d(2), floor mode; first max wins (PyTorch scan order) -------
template <typename T>
__global__ void maxpool_fwd_kernel(const T* a, T* p, int N, int D, int H, int W, int C) {
  constexpr int VEC = Elem<T>::kVec;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2, CV = C / VEC;
  const long total = (long)N * Do * Ho * Wo * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // 32-bit index decomposition (host: total < 2^31): 64-bit division is a long sequence
    const uint32_t ii = (uint32_t)i;
    const int cv = ii % CV; uint32_t r = ii / CV;
    const int wo = r % Wo; r /= Wo;
    const int ho = r % Ho; r /= Ho;
    const int d_o = r % Do; const long n = r / Do;
    float m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
    for (int k = 0; k < 8; ++k) {
      const long vin = ((n * D + 2 * d_o + (k >> 2)) * H + 2 * ho + ((k >> 1) & 1)) * W + 2 * wo + (k & 1);
      float v[VEC];
      load16<T>(a + vin * C + cv * VEC, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (v[j] > m[j] || v[j] != v[j]) m[j] = v[j];
    }
    store16<T>(p + i * VEC, m);
  }
}

// da[argmax] += dp (da already holds the skip-path gradient)
template <typename T>
__global__ void maxpool_bwd_kernel(const T* a, const T* dp, T* da, int N, int D, int H, int W, int C) {
  constexpr int VEC = Elem<T>::kVec;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2, CV = C / VEC;
  const long total = (long)N * Do * Ho * Wo * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const uint32_t ii = (uint32_t)i;  // 32-bit index decomposition (host: total < 2^31)
    const int cv = ii % CV; uint32_t r = ii / CV;
    const int wo = r % Wo; r /= Wo;
    const int ho = r % Ho; r /= Ho;
    const int d_o = r % Do; const long n = r / Do;
    float m[VEC];
    int arg[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { m[j] = -INFINITY; arg[j] = 0; }
    long vin[8];
    for (int k = 0; k < 8; ++k) {
      vin[k] = ((n * D + 2 * d_o + (k >> 2)) * H + 2 * ho + ((k >> 1) & 1)) * W + 2 * wo + (k & 1);
      float v[VEC];
      load16<T>(a + vin[k] * C + cv * VEC, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (v[j] > m[j] || (v[j] != v[j] && m[j] == m[j])) { m[j] = v[j]; arg[j] = k; }
    }
    float g[VEC];
    load16<T>(dp + i * VEC, g);
    for (int k = 0; k < 8; ++k) {
      float o[VEC];
      load16<T>(da + vin[k] * C + cv * VEC, o);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] += (arg[j] == k) ? g[j] : 0.f;
      store16<T>(da + vin[k] * C + cv * VEC, o);
    }
  }
}

// ---------------- encoder block output: BN + ReLU fused with the MaxPool3d of Down3D --------
// (models/unet3d.py:37-39 of a DoubleConv, then :80 of the next Down3D.)  One thread per
// (2x2x2 cell of the ceil-sized grid, VEC channels): a = round_T(relu(y sc + sh)) for the cell's
// children is stored (the block output, read by the skip connection), and for whole cells the
// max of those stored values (maxpool_fwd_kernel's scan order and NaN rule) -- the output is
// pooled while it is in registers instead of being read back by a separate pass.
template <typename T, bool NT>
__global__ void __launch_bounds__(TPB) bn_relu_pool_kernel(const T* y, T* a, T* p, const float* scale,
                                                           const float* shift, int N, int D, int H, int W,
                                                           int C) {
  constexpr int VEC = Elem<T>::kVec;
  const int Dc = (D + 1) / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2, CV = C / VEC;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const long total = (long)N * Dc * Hc * Wc * CV;
  const long stride = (long)gridDim.x * blockDim.x;  // multiple of CV (host): cv is per thread
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int cv = (int)(i % CV);
  float sc[VEC], sh[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sc[j] = scale[cv * VEC + j]; sh[j] = shift[cv * VEC + j]; }
  for (; i < total; i += stride) {
    uint32_t r = (uint32_t)(i / CV);  // 32-bit decomposition (host: cells < 2^31)
    const int wc = r % Wc; r /= Wc;
    const int hc = r % Hc; r /= Hc;
    const int dc = r % Dc; const long n = r / Dc;
    float m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
    float v[8][VEC];
    long vin[8];
    bool in[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int d = 2 * dc + (k >> 2), h = 2 * hc + ((k >> 1) & 1), w = 2 * wc + (k & 1);
      in[k] = d < D && h < H && w < W;
      vin[k] = ((n * D + d) * H + h) * W + w;
#ifndef BRP_NTLOAD
#define BRP_NTLOAD 1  // A/B: y loads non-temporal with the stores (1) or cached (0)
#endif
      if (in[k]) ld16<NT && BRP_NTLOAD>(y + vin[k] * C + cv * VEC, v[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!in[k]) continue;
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[k][j] = round_st<T>(bn_relu1(v[k][j], sc[j], sh[j]));
      st16<NT>(a + vin[k] * C + cv * VEC, v[k]);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (v[k][j] > m[j] || v[k][j] != v[k][j]) m[j] = v[k][j];
    }
    if (dc < Do && hc < Ho && wc < Wo) store16<T>(p + (((n * Do + dc) * Ho + hc) * Wo + wc) * C + cv * VEC, m);
  }
}

// MaxPool3d backward fused with the BatchNorm + ReLU backward reduction of the block whose
// output was pooled: da (the block output's gradient, already holding the skip-path part) +=
// dp at the argmax of a = round_T(relu(y sc + sh)) -- a recomputed from y exactly as
// bn_relu_pool_kernel stored it, maxpool_bwd_kernel's first-max / NaN rule -- and, over every
// voxel (the floor-mode leftovers too), the partial sums of g = da [y sc + sh > 0] and g xhat
// per channel: one [C][2] row per block (bn_relu_bwd_reduce_kernel's quantities), so the
// BatchNorm backward needs no reduction pass over da and y of its own.
// STORE false (pcms_maxpool_bwd_bn_sums): the same sums, da left as it was (the skip-path part
// only) -- maxpool_bn_apply_kernel forms the pooled-path sum again where it applies the BN.
template <typename T, bool STORE = true>
__global__ void __launch_bounds__(TPB, 3) maxpool_bwd_bn_kernel(const T* y, const float* scale, const float* shift,
                                                             const float* mean, const float* invstd, const T* dp,
                                                             T* da, float* part, int N, int D, int H, int W,
                                                             int C) {
  constexpr int VEC = Elem<T>::kVec;
  __shared__ float red[TPB][VEC][2];
  const int Dc = (D + 1) / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2, CV = C / VEC;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const long total = (long)N * Dc * Hc * Wc * CV;
  const long stride = (long)gridDim.x * blockDim.x;  // multiple of CV (host)
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int cv = (int)(i % CV);
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], sg[VEC], sgx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = cv * VEC + j;
    sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; is[j] = invstd[c];
    sg[j] = 0.f; sgx[j] = 0.f;
  }
  // a cell's 8 y chunks, 8 da chunks and its dp chunk are all loaded (raw 16-B vectors) before
  // the first use: one memory round trip per cell instead of one per child
  auto unpack = [](const u32x4_t r, float (&o)[VEC]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { o[2 * q] = __uint_as_float(r[q] << 16); o[2 * q + 1] = __uint_as_float(r[q] & 0xffff0000u); }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = __uint_as_float(r[q]);
    }
  };
  for (; i < total; i += stride) {
    uint32_t r = (uint32_t)(i / CV);
    const int wc = r % Wc; r /= Wc;
    const int hc = r % Hc; r /= Hc;
    const int dc = r % Dc; const long n = r / Dc;
    const bool whole = dc < Do && hc < Ho && wc < Wo;
    u32x4_t yr[8], dr[8], gr = {0u, 0u, 0u, 0u};
    // child k: voxel v0 + (k >> 2) H W + ((k >> 1) & 1) W + (k & 1) (recomputed where used)
    const long v0 = ((n * D + 2 * dc) * H + 2 * hc) * W + 2 * wc;
    const bool ind = 2 * dc + 1 < D, inh = 2 * hc + 1 < H, inw = 2 * wc + 1 < W;
    auto vk = [&](int k) { return v0 + (long)(k >> 2) * H * W + ((k >> 1) & 1) * W + (k & 1); };
    auto ink = [&](int k) { return (!(k & 4) || ind) && (!(k & 2) || inh) && (!(k & 1) || inw); };
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      yr[k] = (u32x4_t){0u, 0u, 0u, 0u};
      dr[k] = yr[k];
      if (ink(k)) {
        yr[k] = *reinterpret_cast<const u32x4_t*>(y + vk(k) * C + cv * VEC);
        dr[k] = *reinterpret_cast<const u32x4_t*>(da + vk(k) * C + cv * VEC);
      }
    }
    if (whole) gr = *reinterpret_cast<const u32x4_t*>(dp + (((n * Do + dc) * Ho + hc) * Wo + wc) * C + cv * VEC);
    float g[VEC], m[VEC];
    int arg[VEC];
    unpack(gr, g);
#pragma unroll
    for (int j = 0; j < VEC; ++j) { m[j] = -INFINITY; arg[j] = 0; }
    // channel pairs in packed fp32 (the same IEEE operation per element as the scalar forms,
    // half the VALU issue: the kernel was VALU-bound) and one v_cvt_pk_bf16_f32 per pair
    auto round2 = [](f32x2_t v) -> f32x2_t {
      if constexpr (sizeof(T) == 2) {
        const uint32_t u = pack_bf16x2(v[0], v[1]);
        return (f32x2_t){__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
      } else {
        return v;
      }
    };
    auto z2of = [&](const float (&yv)[VEC], int q) {
      return __builtin_elementwise_fma((f32x2_t){yv[2 * q], yv[2 * q + 1]}, (f32x2_t){sc[2 * q], sc[2 * q + 1]},
                                       (f32x2_t){sh[2 * q], sh[2 * q + 1]});
    };
    if (whole) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float yv[VEC];
        unpack(yr[k], yv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float av = round_st<T>(bn_relu1(yv[j], sc[j], sh[j]));
          if (av > m[j] || (av != av && m[j] == m[j])) { m[j] = av; arg[j] = k; }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!ink(k)) continue;
      float yv[VEC], o[VEC];
      // (an opaque copy: the compiler would otherwise keep the argmax pass's 64 BN values live
      // for this pass, past the register budget)
      u32x4_t yk = yr[k];
      asm volatile("" : "+v"(yk));
      unpack(yk, yv);
      unpack(dr[k], o);
      if (whole) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] += (arg[j] == k) ? g[j] : 0.f;
        if constexpr (STORE) store16<T>(da + vk(k) * C + cv * VEC, o);
      }
#pragma unroll
      for (int q = 0; q < VEC / 2; ++q) {
        const f32x2_t z2 = z2of(yv, q);
        const f32x2_t r2 = round2((f32x2_t){o[2 * q], o[2 * q + 1]});
        const f32x2_t g2 = {z2[0] > 0.f ? r2[0] : 0.f, z2[1] > 0.f ? r2[1] : 0.f};
        const f32x2_t t2 = ((f32x2_t){yv[2 * q], yv[2 * q + 1]} - (f32x2_t){mu[2 * q], mu[2 * q + 1]}) *
                           (f32x2_t){is[2 * q], is[2 * q + 1]};
        f32x2_t sg2 = {sg[2 * q], sg[2 * q + 1]}, sgx2 = {sgx[2 * q], sgx[2 * q + 1]};
        {
#pragma clang fp contract(off)  // a product then a sum, as the separate reduce pass forms it
          sgx2 = sgx2 + g2 * t2;
          sg2 = sg2 + g2;
        }
        sg[2 * q] = sg2[0]; sg[2 * q + 1] = sg2[1];
        sgx[2 * q] = sgx2[0]; sgx[2 * q + 1] = sgx2[1];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) { red[threadIdx.x][j][0] = sg[j]; red[threadIdx.x][j][1] = sgx[j]; }
  __syncthreads();
  // this block's row: channel c = cv' VEC + j sums threads t = cv' + CV k in t order
  const int c0 = (int)(((long)blockIdx.x * blockDim.x) % CV);  // the cv of thread 0
  for (int e = threadIdx.x; e < C * 2; e += TPB) {
    const int c = e >> 1, q = e & 1, cvc = c / VEC, j = c % VEC;
    const int t0 = (cvc - c0 + CV) % CV;
    float acc = 0.f;
    for (int t = t0; t < TPB; t += CV) acc += red[t][j][q];
    part[((long)blockIdx.x * C + c) * 2 + q] = acc;
  }
}

// The consumer half of the pair above (pcms_maxpool_bn_apply): per 2x2x2 cell, the block
// output's gradient da = gx + dp at the argmax -- recomputed from y exactly as
// maxpool_bwd_bn_kernel forms it, rounded to T as that kernel stores it -- and then
// bn_relu_bwd_apply_kernel's dy = k1 g + k2 xhat + k3 (its arithmetic, expression for
// expression).  With pcms_maxpool_bwd_bn_sums before it, da is never written to HBM: this
// pass reads gx + dp (+ 1/8 of a tensor) where the stored form wrote da and read it back.
template <typename T, bool NT>
// (two blocks per CU: its 7 x VEC per-channel coefficients do not fit the three-block budget)
__global__ void __launch_bounds__(TPB, 2) maxpool_bn_apply_kernel(const T* y, const float* scale, const float* shift,
                                                               const float* mean, const float* invstd,
                                                               const float* coef, const T* dp, const T* gx, T* dy,
                                                               int N, int D, int H, int W, int C) {
  constexpr int VEC = Elem<T>::kVec;
  const int Dc = (D + 1) / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2, CV = C / VEC;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const long total = (long)N * Dc * Hc * Wc * CV;
  const long stride = (long)gridDim.x * blockDim.x;  // multiple of CV (host)
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int cv = (int)(i % CV);
  float sc[VEC], sh[VEC], mu[VEC], is[VEC], k1[VEC], k2[VEC], k3[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = cv * VEC + j;
    sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; is[j] = invstd[c];
    k1[j] = coef[c * 3]; k2[j] = coef[c * 3 + 1]; k3[j] = coef[c * 3 + 2];
  }
  for (; i < total; i += stride) {
    uint32_t r = (uint32_t)(i / CV);
    const int wc = r % Wc; r /= Wc;
    const int hc = r % Hc; r /= Hc;
    const int dc = r % Dc; const long n = r / Dc;
    const bool whole = dc < Do && hc < Ho && wc < Wo;
    const long v0 = ((n * D + 2 * dc) * H + 2 * hc) * W + 2 * wc;
    const bool ind = 2 * dc + 1 < D, inh = 2 * hc + 1 < H, inw = 2 * wc + 1 < W;
    auto vk = [&](int k) { return v0 + (long)(k >> 2) * H * W + ((k >> 1) & 1) * W + (k & 1); };
    auto ink = [&](int k) { return (!(k & 4) || ind) && (!(k & 2) || inh) && (!(k & 1) || inw); };
    // raw 16-B vectors (4 registers each), unpacked where used: the cell's 16 loads and its
    // dp load all in flight before the first use, in maxpool_bwd_bn_kernel's register budget
    auto unpack = [](const u32x4_t r, float (&o)[VEC]) {
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { o[2 * q] = __uint_as_float(r[q] << 16); o[2 * q + 1] = __uint_as_float(r[q] & 0xffff0000u); }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __uint_as_float(r[q]);
      }
    };
    auto ldraw = [](const T* p) -> u32x4_t {
      if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
      else return *reinterpret_cast<const u32x4_t*>(p);
    };
    u32x4_t yr[8], dr[8], gr = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      yr[k] = (u32x4_t){0u, 0u, 0u, 0u};
      dr[k] = yr[k];
      if (ink(k)) {
        yr[k] = ldraw(y + vk(k) * C + cv * VEC);
        dr[k] = ldraw(gx + vk(k) * C + cv * VEC);
      }
    }
    if (whole) gr = *reinterpret_cast<const u32x4_t*>(dp + (((n * Do + dc) * Ho + hc) * Wo + wc) * C + cv * VEC);
    float g[VEC], m[VEC];
    int arg[VEC];
    unpack(gr, g);
#pragma unroll
    for (int j = 0; j < VEC; ++j) { m[j] = -INFINITY; arg[j] = 0; }
    if (whole) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float yv[VEC];
        unpack(yr[k], yv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float av = round_st<T>(bn_relu1(yv[j], sc[j], sh[j]));
          if (av > m[j] || (av != av && m[j] == m[j])) { m[j] = av; arg[j] = k; }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!ink(k)) continue;
      float yv[VEC], o[VEC], out[VEC];
      u32x4_t yk = yr[k];
      asm volatile("" : "+v"(yk));  // (as maxpool_bwd_bn_kernel: keep the argmax pass's values dead)
      unpack(yk, yv);
      unpack(dr[k], o);
      if (whole) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = round_st<T>(o[j] + ((arg[j] == k) ? g[j] : 0.f));
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) out[j] = bn_bwd_dy(o[j], yv[j], sc[j], sh[j], mu[j], is[j], k1[j], k2[j], k3[j]);
      st16<NT>(dy + vk(k) * C + cv * VEC, out);
    }
  }
}

}  // namespace

// grid of the cell kernels: a multiple of CV / gcd so every thread keeps one channel group
static int cell_grid(long total, int CV, int cap) {
  int g = stream_grid(total, TPB, cap);
  const int per = CV / std::__gcd(CV, TPB);  // blocks per period of cv
  return std::max(per, g / per * per);
}
// *cells: the 2x2x2 cells of the ceil-sized grid; -7 when the cell kernels' 32-bit index math
// cannot hold their children
static int pool_cells(int N, int D, int H, int W, long* cells) {
  *cells = (long)N * ((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);
  return *cells * 8 >= (1L << 31) ? -7 : 0;
}
static bool pool_nt(int dtype, int N, int D, int H, int W, int C) {
  return (long)N * D * H * W * C * bytes_of(dtype) >= kNtBytesBn;
}

extern "C" {

int pcms_maxpool_fwd(int dtype, const void* a, void* p, int N, int D, int H, int W, int C, hipStream_t s) {
  if ((long)N * D * H * W * C >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  const long total = (long)N * (D / 2) * (H / 2) * (W / 2) * (C / vec_of(dtype));
  const int grid = stream_grid(total, TPB);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)a, (T*)p, N, D, H, W, C);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_maxpool_bwd(int dtype, const void* a, const void* dp, void* da, int N, int D, int H, int W, int C,
                     hipStream_t s) {
  if ((long)N * D * H * W * C >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  const long total = (long)N * (D / 2) * (H / 2) * (W / 2) * (C / vec_of(dtype));
  const int grid = stream_grid(total, TPB);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)a, (const T*)dp, (T*)da, N, D, H,
                       W, C);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_bn_relu_pool(int dtype, const void* y, void* a, void* p, const float* scale, const float* shift, int N,
                      int D, int H, int W, int C, hipStream_t s) {
  const int VEC = vec_of(dtype), CV = C / VEC;
  if (C % VEC) return -1;
  long cells;
  if (const int rc = pool_cells(N, D, H, W, &cells)) return rc;
  const int grid = cell_grid(cells * CV, CV, 8192);
  return for_stream(dtype, pool_nt(dtype, N, D, H, W, C), [&](auto t, auto nt) {
    using T = decltype(t);
    hipLaunchKernelGGL((bn_relu_pool_kernel<T, decltype(nt)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)y, (T*)a,
                       (T*)p, scale, shift, N, D, H, W, C);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_maxpool_bwd_bn_rows(int dtype, int N, int D, int H, int W, int C) {
  const int CV = C / vec_of(dtype);
  long cells;
  pool_cells(N, D, H, W, &cells);  // (a size query: the launches return the -7)
  return cell_grid(cells * CV, CV, g_bn_rows_cap);
}

// store: da += dp at the argmax (pcms_maxpool_bwd_bn); else da is read only (..._bn_sums)
static int maxpool_bwd_bn_any(bool store, int dtype, const void* y, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const void* dp, void* da, float* part, int N,
                              int D, int H, int W, int C, hipStream_t s) {
  const int VEC = vec_of(dtype);
  if (C % VEC || TPB % (C / VEC)) return -1;
  long cells;
  if (const int rc = pool_cells(N, D, H, W, &cells)) return rc;
  const int grid = pcms_maxpool_bwd_bn_rows(dtype, N, D, H, W, C);
  return for_stream(dtype, store, [&](auto t, auto st) {
    using T = decltype(t);
    hipLaunchKernelGGL((maxpool_bwd_bn_kernel<T, decltype(st)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)y, scale,
                       shift, mean, invstd, (const T*)dp, (T*)da, part, N, D, H, W, C);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_maxpool_bwd_bn(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const void* dp, void* da, float* part, int N, int D, int H, int W,
                        int C, hipStream_t s) {
  return maxpool_bwd_bn_any(true, dtype, y, scale, shift, mean, invstd, dp, da, part, N, D, H, W, C, s);
}

int pcms_maxpool_bwd_bn_sums(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const void* dp, const void* da, float* part, int N, int D, int H,
                             int W, int C, hipStream_t s) {
  return maxpool_bwd_bn_any(false, dtype, y, scale, shift, mean, invstd, dp, const_cast<void*>(da), part, N, D, H, W,
                            C, s);
}

int pcms_maxpool_bn_apply(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* coef, const void* dp, const void* da, void* dy, int N,
                          int D, int H, int W, int C, hipStream_t s) {
  const int VEC = vec_of(dtype), CV = C / VEC;
  if (C % VEC || TPB % CV) return -1;
  long cells;
  if (const int rc = pool_cells(N, D, H, W, &cells)) return rc;
  const int grid = cell_grid(cells * CV, CV, 8192);
  return for_stream(dtype, pool_nt(dtype, N, D, H, W, C), [&](auto t, auto nt) {
    using T = decltype(t);
    hipLaunchKernelGGL((maxpool_bn_apply_kernel<T, decltype(nt)::value>), dim3(grid), dim3(TPB), 0, s, (const T*)y,
                       scale, shift, mean, invstd, coef, (const T*)dp, (const T*)da, (T*)dy, N, D, H, W, C);
    PCMS_CHECK_LAUNCH();
  });
}

}  // extern "C"
