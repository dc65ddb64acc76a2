// Case prediction on the device (gfx950): predict.py's host forms normalise / prepare_case /
// tta_mean / mask_on_grid evaluated per voxel, bit for bit.
//
//   pcms_volume_minmax         lo, hi of a raw volume's decoded fp32 values (normalise's v.min(),
//                              v.max()): per-workgroup partials, then a one-workgroup finish
//   pcms_resample_linear_norm  pcms_resample_linear's gather with every corner (v - lo) / den
//   pcms_flip_mean             the mean of k probability volumes, volume j un-flipped on the way
//   pcms_prob_to_mask          the gather on an fp32 volume, thresholded into a byte mask
//
// The host forms are numpy expressions in which every product, sum and quotient rounds on its
// own; so must they here: no contraction into FMAs anywhere in this file (the fp32 quotient is
// the compiler's correctly rounded division).
#include "resample_common.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

// ---- minimum and maximum of the decoded values -------------------------------------------
constexpr int MM_MAX_WGS = 1024;           // partials the finish kernel folds
constexpr int MM_PER_WG = TPB * 16;        // elements per workgroup before the grid stops growing
inline int minmax_grid(long n) { return grid_for(n, MM_PER_WG, MM_MAX_WGS); }

// numpy's min / max: a NaN operand wins (the comparisons alone would drop it)
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : b != b ? b : b < a ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : b != b ? b : b > a ? b : a; }

// the workgroup's (lo, hi) in thread 0: waves by shuffles, then the four wave results in order
__device__ __forceinline__ void block_minmax(float& lo, float& hi) {
  __shared__ float part[2][WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = nan_min(lo, __shfl_xor(lo, o, 64));
    hi = nan_max(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = lo;
    part[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      lo = nan_min(lo, part[0][w]);
      hi = nan_max(hi, part[1][w]);
    }
  }
}

// work[2 b], work[2 b + 1]: workgroup b's (lo, hi).  The source needs only its element's
// alignment: the elements before the first 16-byte boundary and after the last whole vector are
// read one by one, the body as 16-byte vectors.  Every thread starts from element 0 (a member
// of the set), so no identity value is needed and a NaN there is kept.
template <typename T>
__global__ void __launch_bounds__(TPB) minmax_partial_kernel(const T* __restrict__ src, long n, Scale sc,
                                                             float* __restrict__ work) {
  constexpr int V = 16 / (int)sizeof(T);
  const long to_boundary = (long)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T));
  const long head = to_boundary < n ? to_boundary : n;
  const long nvec = (n - head) / V;
  const long tail0 = head + nvec * V;
  const long tid = blockIdx.x * (long)TPB + threadIdx.x, nthr = (long)gridDim.x * TPB;
  float lo = image_value(src[0], sc), hi = lo;
  const u32x4_t* body = reinterpret_cast<const u32x4_t*>(src + head);
  for (long i = tid; i < nvec; i += nthr) {
    const u32x4_t raw = body[i];
    T e[V];
    __builtin_memcpy(e, &raw, 16);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float v = image_value(e[j], sc);
      lo = nan_min(lo, v);
      hi = nan_max(hi, v);
    }
  }
  const long nedge = head + (n - tail0);  // < 2 V
  for (long i = tid; i < nedge; i += nthr) {
    const float v = image_value(src[i < head ? i : tail0 + (i - head)], sc);
    lo = nan_min(lo, v);
    hi = nan_max(hi, v);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    work[2 * blockIdx.x] = lo;
    work[2 * blockIdx.x + 1] = hi;
  }
}

// one workgroup: the partials in a fixed order -> lohi
__global__ void __launch_bounds__(TPB) minmax_finish_kernel(const float* __restrict__ work, int nparts,
                                                            float* __restrict__ lohi) {
  float lo = work[0], hi = work[1];
  for (int i = threadIdx.x; i < nparts; i += TPB) {
    lo = nan_min(lo, work[2 * i]);
    hi = nan_max(hi, work[2 * i + 1]);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    lohi[0] = lo;
    lohi[1] = hi;
  }
}

// ---- the normalised resample and the mask ----------------------------------------------------
// (a corner is resample_common.h's normalised(): patch.hip forms the same one)
template <typename T>
__global__ void __launch_bounds__(TPB) resample_linear_norm_kernel(const T* __restrict__ src,
                                                                   const float* __restrict__ lohi,
                                                                   float* __restrict__ out, Axis ad, Axis ah, Axis aw,
                                                                   Scale sc) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  const float lo = lohi[0], hi = lohi[1];
  const float den = (float)((double)hi - (double)lo);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const Tap td = linear_tap(ad, d), th = linear_tap(ah, h), tw = linear_tap(aw, w);
    float res = 0.f;
    if (!(td.outside || th.outside || tw.outside))
      res = gather_linear(ad, ah, aw, td, th, tw,
                          [&](long x) { return (double)normalised(image_value(src[x], sc), lo, den); });
    out[i] = res;
  }
}

// mask_on_grid: the gather on the probabilities, `>` against the threshold; the fp32 value is
// kept only when the caller asks for it
__global__ void __launch_bounds__(TPB) prob_to_mask_kernel(const float* __restrict__ prob, float threshold,
                                                           uint8_t* __restrict__ mask, float* __restrict__ native,
                                                           Axis ad, Axis ah, Axis aw) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const Tap td = linear_tap(ad, d), th = linear_tap(ah, h), tw = linear_tap(aw, w);
    float res = 0.f;
    if (!(td.outside || th.outside || tw.outside))
      res = gather_linear(ad, ah, aw, td, th, tw, [&](long x) { return (double)prob[x]; });
    mask[i] = res > threshold ? 1 : 0;
    if (native != nullptr) native[i] = res;
  }
}

// ---- tta_mean ------------------------------------------------------------------------------
constexpr int MAX_FLIPS = 8;  // the distinct flip sets of three axes
struct Flips {
  int k;
  int mask[MAX_FLIPS];  // bit a: volume j is flipped along axis a (0 D, 1 H, 2 W)
};

// acc = probs[0]; acc = acc + flip(probs[j]) for j = 1 .. k - 1 in order; out = acc / (float)k
__global__ void __launch_bounds__(TPB) flip_mean_kernel(const float* __restrict__ probs, float* __restrict__ out,
                                                        Flips f, int D, int H, int W) {
  const long HW = (long)H * W;
  const long total = (long)D * HW;
  const float fk = (float)f.k;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / W), w = (int)(r - (long)h * W);
    float acc = probs[i];
    for (int j = 1; j < f.k; ++j) {
      const int m = f.mask[j];
      const long dd = (m & 1) ? D - 1 - d : d, hh = (m & 2) ? H - 1 - h : h, ww = (m & 4) ? W - 1 - w : w;
      acc = acc + probs[j * total + (dd * H + hh) * W + ww];
    }
    out[i] = acc / fk;
  }
}

}  // namespace

extern "C" {

int pcms_volume_minmax_work_floats(long n) { return n < 1 ? -1 : 2 * minmax_grid(n); }

int pcms_volume_minmax(const void* src, int datatype, long n, double scl_slope, double scl_inter, float* lohi,
                       float* work, hipStream_t s) {
  if (src == nullptr || lohi == nullptr || work == nullptr || n < 1) return -1;
  if (misaligned(lohi, alignof(float)) || misaligned(work, alignof(float))) return -1;
  const Scale sc = make_scale(scl_slope, scl_inter);
  const int grid = minmax_grid(n);
  const int rc = for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    hipLaunchKernelGGL(minmax_partial_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, n, sc, work);
    PCMS_CHECK_LAUNCH();
  });
  if (rc != 0) return rc;
  hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(TPB), 0, s, (const float*)work, grid, lohi);
  PCMS_CHECK_LAUNCH();
}

int pcms_resample_linear_norm(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                              double scl_inter, const float* lohi, float* out, int D, int H, int W, hipStream_t s) {
  if (src == nullptr || lohi == nullptr || out == nullptr) return -1;
  if (Di < 1 || Hi < 1 || Wi < 1 || D < 1 || H < 1 || W < 1) return -1;
  if (misaligned(lohi, alignof(float)) || misaligned(out, alignof(float))) return -1;
  const Axis ad = make_axis(Di, D), ah = make_axis(Hi, H), aw = make_axis(Wi, W);
  const Scale sc = make_scale(scl_slope, scl_inter);
  const int grid = grid_for((long)D * H * W, TPB);
  return for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    hipLaunchKernelGGL(resample_linear_norm_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, lohi, out, ad, ah,
                       aw, sc);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_flip_mean(const float* probs, int k, const int* flipmask, float* out, int D, int H, int W, hipStream_t s) {
  if (probs == nullptr || flipmask == nullptr || out == nullptr) return -1;
  if (k < 1 || k > MAX_FLIPS || D < 1 || H < 1 || W < 1) return -1;
  if (misaligned(probs, alignof(float)) || misaligned(out, alignof(float))) return -1;
  Flips f{};
  f.k = k;
  for (int j = 0; j < k; ++j) {
    if (flipmask[j] < 0 || flipmask[j] > 7 || (j == 0 && flipmask[j] != 0)) return -1;
    f.mask[j] = flipmask[j];
  }
  hipLaunchKernelGGL(flip_mean_kernel, dim3(grid_for((long)D * H * W, TPB)), dim3(TPB), 0, s, probs, out, f, D, H, W);
  PCMS_CHECK_LAUNCH();
}

int pcms_prob_to_mask(const float* prob, int Dt, int Ht, int Wt, float threshold, unsigned char* mask,
                      float* prob_native, int D, int H, int W, hipStream_t s) {
  if (prob == nullptr || mask == nullptr) return -1;
  if (Dt < 1 || Ht < 1 || Wt < 1 || D < 1 || H < 1 || W < 1) return -1;
  if (misaligned(prob, alignof(float)) || misaligned(prob_native, alignof(float))) return -1;
  const Axis ad = make_axis(Dt, D), ah = make_axis(Ht, H), aw = make_axis(Wt, W);
  hipLaunchKernelGGL(prob_to_mask_kernel, dim3(grid_for((long)D * H * W, TPB)), dim3(TPB), 0, s, prob, threshold, mask,
                     prob_native, ad, ah, aw);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
