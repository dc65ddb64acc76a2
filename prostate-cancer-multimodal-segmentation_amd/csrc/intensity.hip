// Percentile intensity normalisation on the device (gfx950): intensity.py's host forms
// intensity_window / normalise_window evaluated on a raw NIfTI volume, bit for bit.
//
//   pcms_volume_window           lohi = the values at two ranks of the selected voxels' sorted
//                                order: an exact most-significant-digit radix select of both
//                                ranks at once, 8 bits per pass, 4 passes over the volume
//   pcms_resample_linear_window  pcms_resample_linear_norm's gather with every corner clipped to
//                                [lo, hi] first
//   pcms_patch_resample_window   pcms_patch_resample_linear's gather with that corner
//
// The select is nine launches: one that zeroes the workspace, then per pass a histogram of one
// digit of the keys that match the digits fixed so far and a one-workgroup scan that fixes the
// next digit of both ranks.  Counts are integers, summed by integer atomics (LDS, then one global
// add per non-empty bin and workgroup into one of eight copies of the rows), so the result is a
// function of the input alone.  The consumers' arithmetic is numpy's: every difference and
// quotient rounds on its own, no contraction into FMAs anywhere in this file.
#include "resample_common.h"

#include "ops_units.h"
#include "wave_hist.h"
#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVES = TPB / 64;
constexpr int BINS = 256;              // one 8-bit digit per pass
constexpr int PASSES = 4;
// Workgroup b adds its non-empty bins once to copy b % COPIES of the global rows; the scan sums
// the copies.  The adds to one hot bin queue up behind each other: with one copy 512 workgroups
// took 82 us for the 24x512x512 int16 select and 1536 took 107 us; with 8 copies 1536 take 58 us
// (16 copies 71 us, 32 copies 99 us: the one-workgroup scan then reads too many rows;
// profiles/intensity_ab.txt)
constexpr int SEL_MAX_WGS = 2048;      // 256 CUs x 8 workgroups
constexpr int COPIES = 8;
constexpr int SEL_PER_WG = TPB * 16;   // elements per workgroup before the grid stops growing
static_assert(BINS == TPB, "the scan kernel holds one bin per thread");

// The workspace.  prefix[r]: the key digits fixed so far for rank r (0: lo, 1: hi), in place, the
// digits still open zero; rank[r]: the rank among the keys that share that prefix; m: the size of
// the selected set; hist[p][c][r]: copy c of pass p's digit counts of the keys matching prefix[r]
// (row 1 is left empty while both prefixes are equal).
struct Work {
  uint32_t prefix[2];
  long long rank[2];
  long long m;
  long long pad[4];
  uint32_t hist[PASSES][COPIES][2][BINS];
};
static_assert(sizeof(Work) == 64 + PASSES * COPIES * 2 * BINS * 4, "Work is a 64-byte state block and the rows");

// the order-preserving u32 image of v + 0.f (-0 folded into +0); every NaN is the top key
__device__ __forceinline__ uint32_t key_of(float v) {
  const float f = v + 0.f;
  if (f != f) return 0xffffffffu;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) {
  if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(TPB) window_init_kernel(uint32_t* __restrict__ work, int words) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < words; i += gridDim.x * TPB) work[i] = 0u;
}

// Pass `pass` (0: the top digit): of the selected voxels whose key matches prefix[r] in the digits
// above this one, count digit (key >> (24 - 8 pass)) & 255 into row r of the workgroup's LDS
// histogram, which then goes to hist[pass][blockIdx.x % COPIES].  Loads as in
// minmax_partial_kernel (predict.hip): the elements before the first 16-byte boundary and after
// the last whole vector one by one, the body as 16-byte vectors, grid-stride.  Every loop bound
// is the wave's, not the lane's, so that all 64 lanes reach each ballot; a lane past the end
// counts nothing.
template <typename T>
__global__ void __launch_bounds__(TPB) window_hist_kernel(const T* __restrict__ src, long n, Scale sc, int pass,
                                                          int use_above, float above, Work* __restrict__ work) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ uint32_t hist[2 * BINS];
  for (int b = threadIdx.x; b < 2 * BINS; b += TPB) hist[b] = 0u;
  __syncthreads();
  const uint32_t plo = work->prefix[0], phi = work->prefix[1];
  const bool same = plo == phi;  // both ranks still follow one prefix: one row serves both
  const int dshift = 24 - 8 * pass;
  const uint32_t pmask = pass == 0 ? 0u : 0xffffffffu << (dshift + 8);
  const int lane = threadIdx.x & 63;
  auto count = [&](float v, bool in) {
    const bool sel = in && (!use_above || v > above);  // false for NaN
    const uint32_t key = key_of(v);
    const uint32_t digit = (key >> dshift) & (BINS - 1);
    const uint32_t top = key & pmask;
    // the prefixes differ when two rows are kept, so a key matches one of them at the most
    const bool mlo = top == plo, mhi = !same && top == phi;
    bin_add(hist, digit + (mhi ? BINS : 0), sel && (mlo || mhi), lane);
  };

  const long to_boundary = (long)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T));
  const long head = to_boundary < n ? to_boundary : n;
  const long nvec = (n - head) / V;
  const long tail0 = head + nvec * V;
  const long wave0 = blockIdx.x * (long)TPB + (threadIdx.x - lane), nthr = (long)gridDim.x * TPB;
  const u32x4_t* body = reinterpret_cast<const u32x4_t*>(src + head);
  for (long base = wave0; base < nvec; base += nthr) {
    const long i = base + lane;
    const bool in = i < nvec;
    u32x4_t raw = {0u, 0u, 0u, 0u};
    if (in) raw = body[i];
    T e[V];
    __builtin_memcpy(e, &raw, 16);
#pragma unroll
    for (int j = 0; j < V; ++j) count(image_value(e[j], sc), in);
  }
  const long nedge = head + (n - tail0);  // < 2 V
  for (long base = wave0; base < nedge; base += nthr) {
    const long i = base + lane;
    const bool in = i < nedge;
    T raw = T{};
    if (in) raw = src[i < head ? i : tail0 + (i - head)];
    count(image_value(raw, sc), in);
  }
  __syncthreads();
  uint32_t* rows = work->hist[pass][blockIdx.x % COPIES][0];
  for (int b = threadIdx.x; b < (same ? BINS : 2 * BINS); b += TPB) {
    const uint32_t c = hist[b];
    if (c != 0u) __hip_atomic_fetch_add(rows + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup, one bin per thread: the exclusive scan of pass `pass`'s row for each rank (a
// scan inside each wave by shuffles, the four wave totals through LDS); the thread whose bin
// holds the rank appends its digit to the prefix and leaves the rank inside the bin.  Pass 0 also
// has m, the row's total, and forms both ranks from it in integers:
// r_lo = floor(q_lo (m - 1) / 10^6), r_hi = ceil(q_hi (m - 1) / 10^6); m == 0: lohi = (0, 0) and
// the later passes leave it.  The last pass turns the two complete keys into lohi.
__global__ void __launch_bounds__(TPB) window_scan_kernel(Work* __restrict__ work, int pass, int ppm_lo, int ppm_hi,
                                                          float* __restrict__ lohi) {
  __shared__ uint32_t wtot[2][WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t p[2] = {work->prefix[0], work->prefix[1]};
  const bool same = p[0] == p[1];
  long long m = pass == 0 ? 0 : work->m;
  long long r[2] = {work->rank[0], work->rank[1]};
  uint32_t h[2], x[2];
  h[0] = h[1] = 0u;
  for (int c = 0; c < COPIES; ++c) {
    h[0] += work->hist[pass][c][0][t];
    if (!same) h[1] += work->hist[pass][c][1][t];
  }
  if (same) h[1] = h[0];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    x[k] = h[k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x[k], o, 64);
      if (lane >= o) x[k] += y;
    }
    if (lane == 63) wtot[k][wv] = x[k];
  }
  __syncthreads();  // also: every thread has read the state before any thread writes it
  long long excl[2], total = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t below = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t tw = wtot[k][w];
      below += w < wv ? tw : 0u;
      if (k == 0) total += tw;
    }
    excl[k] = (long long)below + (x[k] - h[k]);
  }
  if (pass == 0) {
    m = total;
    if (t == 0) work->m = m;
    if (m == 0) {
      if (t < 2) lohi[t] = 0.f;
      return;
    }
    r[0] = ((long long)ppm_lo * (m - 1)) / 1000000;
    r[1] = ((long long)ppm_hi * (m - 1) + 999999) / 1000000;
  } else if (m == 0) {
    return;
  }
  const int dshift = 24 - 8 * pass;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (h[k] != 0u && excl[k] <= r[k] && r[k] < excl[k] + (long long)h[k]) {  // exactly one thread
      const uint32_t key = p[k] | ((uint32_t)t << dshift);
      work->prefix[k] = key;
      work->rank[k] = r[k] - excl[k];
      if (pass == PASSES - 1) lohi[k] = value_of(key);
    }
  }
}

// resample_linear_norm_kernel (predict.hip) with the clipped corner
template <typename T>
__global__ void __launch_bounds__(TPB) resample_linear_window_kernel(const T* __restrict__ src,
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
                          [&](long x) { return (double)windowed(image_value(src[x], sc), lo, hi, den); });
    out[i] = res;
  }
}

// patch_resample_kernel (patch.hip) with the clipped corner: the same indexing, inside rules,
// rolled element loop and store rule; lo, hi and den are wave-uniform and kept in SGPRs
constexpr int MAX_WGS = 2048;
constexpr int MAX_PATCHES = 64;
struct Grid {
  int Gd, Gh, Gw;
};
__device__ __forceinline__ float uniform(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

template <typename T>
__global__ void __launch_bounds__(TPB) patch_resample_window_kernel(const T* __restrict__ src,
                                                                    const float* __restrict__ lohi,
                                                                    const int* __restrict__ origins,
                                                                    float* __restrict__ out, long stride, int P,
                                                                    Affine m, Dims g, Grid gr, Scale sc, float gain,
                                                                    float bias, int intensity, int vec) {
  const int qw = (g.W + 3) >> 2;
  const int plane = g.D * g.H;
  const long total = (long)P * plane * qw;
  const float lo = uniform(lohi[0]), hi = uniform(lohi[1]);
  const float den = uniform((float)((double)hi - (double)lo));
  for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
    const long row = i / qw;
    const int c0 = (int)(i - row * qw) * 4;
    const int p = (int)(row / plane);
    const int rem = (int)(row - (long)p * plane);
    const int a = rem / g.H, b = rem - a * g.H;
    const long qd = (long)origins[3 * p] + a, qh = (long)origins[3 * p + 1] + b;
    const long qw0 = (long)origins[3 * p + 2] + c0;
    const bool row_in = qd >= 0 && qd < gr.Gd && qh >= 0 && qh < gr.Gh;
    const int id = (int)qd, ih = (int)qh;  // read only where row_in: then inside the grid
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
      const long q = qw0 + e;
      if (row_in && c0 + e < g.W && q >= 0 && q < gr.Gw) {
        int jd = id, jh = ih;
        asm volatile("" : "+v"(jd), "+v"(jh));
        const double fd = (double)jd, fh = (double)jh, fw = (double)q;
        const double cd = affine_coord(m.d, fd, fh, fw), ch = affine_coord(m.h, fd, fh, fw),
                     cw = affine_coord(m.w, fd, fh, fw);
        v[e] = affine_linear_gather(g, cd, ch, cw, gain, bias, intensity,
                                    [&](long x) { return (double)windowed(image_value(src[x], sc), lo, hi, den); });
      }
    }
    float* dst = out + p * stride + (long)rem * g.W + c0;
    if (vec) {
      *reinterpret_cast<f32x4_t*>(dst) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < g.W) dst[e] = v[e];
    }
  }
}

}  // namespace

extern "C" {

int pcms_volume_window_work_bytes(long n) { return (n < 1 || n > 0x7fffffffL) ? -1 : (int)sizeof(Work); }

int pcms_volume_window(const void* src, int datatype, long n, double scl_slope, double scl_inter, int ppm_lo,
                       int ppm_hi, int use_above, float above, float* lohi, void* work, hipStream_t s) {
  if (src == nullptr || lohi == nullptr || work == nullptr || n < 1 || n > 0x7fffffffL) return -1;
  if (misaligned(lohi, alignof(float)) || misaligned(work, alignof(Work))) return -1;
  if (ppm_lo < 0 || ppm_hi > 1000000 || ppm_lo >= ppm_hi) return -1;
  if (use_above && !std::isfinite(above)) return -1;
  const Scale sc = make_scale(scl_slope, scl_inter);
  const int grid = stream_grid(n, SEL_PER_WG, SEL_MAX_WGS);
  Work* w = static_cast<Work*>(work);
  return for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    PCMS_LAUNCH(window_init_kernel, dim3(cdiv(sizeof(Work) / 4, TPB * 8)), dim3(TPB), 0, s, (uint32_t*)work,
                (int)(sizeof(Work) / 4));
    for (int pass = 0; pass < PASSES; ++pass) {
      PCMS_LAUNCH(window_hist_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, n, sc, pass, use_above ? 1 : 0,
                  above, w);
      PCMS_LAUNCH(window_scan_kernel, dim3(1), dim3(TPB), 0, s, w, pass, ppm_lo, ppm_hi, lohi);
    }
    return 0;
  });
}

int pcms_resample_linear_window(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
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
    hipLaunchKernelGGL(resample_linear_window_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, lohi, out, ad, ah,
                       aw, sc);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_patch_resample_window(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                               double scl_inter, const double* affine12, const float* lohi, float gain, float bias,
                               int Gd, int Gh, int Gw, const int* origins, int P, float* out, long patch_stride, int D,
                               int H, int W, hipStream_t s) {
  if (!affine_args_ok(src, out, affine12, Di, Hi, Wi, D, H, W, gain, bias)) return -1;
  if (lohi == nullptr || origins == nullptr || Gd < 1 || Gh < 1 || Gw < 1 || P < 1 || P > MAX_PATCHES) return -1;
  if (misaligned(origins, alignof(int)) || misaligned(lohi, alignof(float))) return -1;
  if (patch_stride < (long)D * H * W || (long)D * H > 0x7fffffffL) return -1;  // a patch's rows are counted in an int
  const Affine m = make_affine(affine12);  // copied into the kernel arguments
  const Dims g{Di, Hi, Wi, D, H, W};
  const Grid gr{Gd, Gh, Gw};
  const Scale sc = make_scale(scl_slope, scl_inter);
  const long quads = (long)P * D * H * ((W + 3) / 4);
  const int grid = grid_for(quads, TPB, MAX_WGS);
  const int intensity = (gain == 1.f && bias == 0.f) ? 0 : 1;
  const int vec = (W % 4 == 0 && patch_stride % 4 == 0 && !misaligned(out, 16)) ? 1 : 0;
  return for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    hipLaunchKernelGGL(patch_resample_window_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, lohi, origins, out,
                       patch_stride, P, m, g, gr, sc, gain, bias, intensity, vec);
    PCMS_CHECK_LAUNCH();
  });
}

}  // extern "C"
