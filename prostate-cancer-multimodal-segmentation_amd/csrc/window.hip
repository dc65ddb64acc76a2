// Sliding-window prediction on the device (gfx950): window.py's host forms gather_windows /
// blend_windows evaluated per voxel, bit for bit.
//
//   pcms_window_gather   a batch of B windows (and their flipped copies) cut out of a (C, D, H, W)
//                        volume, zero outside it: the network's input batch
//   pcms_window_blend    acc += wgt * tta_mean(window), wsum += wgt for a batch of windows, one
//                        thread per volume voxel, the windows in ascending index: no atomics
//   pcms_window_finish   prob = acc / wsum
//
// The host forms are numpy expressions in which every product, sum and quotient rounds on its
// own; so must they here: no contraction into FMAs anywhere in this file (the fp32 quotient is
// the compiler's correctly rounded division).
#include "common.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int MAX_WGS = 2048;   // 256 CUs x 8 workgroups; the grid-stride loops take the rest
constexpr int MAX_FLIPS = 8;    // the distinct flip sets of three axes
constexpr int MAX_AXIS = 512;   // the longest window axis: three weight tables of it in LDS

// flip set j in bits 3 j .. 3 j + 2 (bit 0: D, bit 1: H, bit 2: W): one kernel argument, indexed
// by shifts, so a per-thread j reads no array
__device__ __forceinline__ int flip_of(unsigned packed, int j) { return (int)(packed >> (3 * j)) & 7; }

// ---- gather_windows ------------------------------------------------------------------------
// out is (B k, C, wd, wh, ww); one thread forms four consecutive w positions of one output row.
// Entry (win, j) at window index (a, b, c) holds the window's voxel (a', b', c'), the primed
// index mirrored (n - 1 - i) along the axes of flip set j, which is volume voxel start + primed
// index, or 0 outside the volume.  A thread's reads are four neighbours of one source row, in
// reverse order for a W flip.  VEC: ww % 4 == 0 and out 16-byte aligned, one 16-byte store.
template <bool VEC>
__global__ void __launch_bounds__(TPB) window_gather_kernel(const float* __restrict__ x, const int* __restrict__ starts,
                                                            unsigned flips, int k, int C, int D, int H, int W, int B,
                                                            int wd, int wh, int ww, float* __restrict__ out) {
  const int qw = (ww + 3) >> 2;
  const int plane = wd * wh;
  const long total = (long)B * k * C * plane * qw;
  for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
    const long row = i / qw;
    const int c0 = (int)(i - row * qw) * 4;
    const int vol = (int)(row / plane);  // (win k + j) C + ch: below 2^31, checked on the host
    const int p = (int)(row - (long)vol * plane);
    const int a = p / wh, b = p - a * wh;
    const int entry = vol / C, ch = vol - entry * C;
    const int win = entry / k, j = entry - win * k;
    const int m = flip_of(flips, j);
    const long d = (long)starts[3 * win] + ((m & 1) ? wd - 1 - a : a);
    const long h = (long)starts[3 * win + 1] + ((m & 2) ? wh - 1 - b : b);
    const long sw = starts[3 * win + 2];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (d >= 0 && d < D && h >= 0 && h < H) {
      const float* __restrict__ src = x + (((long)ch * D + d) * H + h) * W;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + e;
        const long w = sw + ((m & 4) ? ww - 1 - c : c);
        if (c < ww && w >= 0 && w < W) v[e] = src[w];
      }
    }
    float* dst = out + row * ww + c0;
    if constexpr (VEC) {
      f32x4_t r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = v[e];
      *reinterpret_cast<f32x4_t*>(dst) = r;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < ww) dst[e] = v[e];
    }
  }
}

// [lo, hi) grown by the part of [start, start + w) inside [0, n)
__device__ __forceinline__ void box_axis(int start, int w, int n, int& lo, int& hi) {
  const long a = start < 0 ? 0L : (long)start;
  const long e = (long)start + w;
  const long b = e > n ? (long)n : e;
  if (a < b) {
    lo = a < lo ? (int)a : lo;
    hi = b > hi ? (int)b : hi;
  }
}

// ---- blend_windows --------------------------------------------------------------------------
// Windows first .. first + B - 1 of the table `starts`; probs holds their B k probability windows.
// Every thread folds the batch's bounding box (clipped to the volume) out of the B starts
// (uniform reads), then takes the box's voxels in a grid-stride loop: acc and wsum read once, the
// covering windows visited in ascending index, m = tta_mean's value at the voxel (entry 0 as it
// is, entry j read at the mirrored index, summed in order, / (float)k), acc = acc + wgt m,
// wsum = wsum + wgt with wgt = (wtd[a] wth[b]) wtw[c] from the tables in LDS, and one write of
// each when a window covered the voxel.  Voxels are disjoint between threads: no atomics.
__global__ void __launch_bounds__(TPB) window_blend_kernel(const float* __restrict__ probs,
                                                           const int* __restrict__ starts, int first, int B,
                                                           unsigned flips, int k, const float* __restrict__ wts, int wd,
                                                           int wh, int ww, float* __restrict__ acc,
                                                           float* __restrict__ wsum, int D, int H, int W) {
  __shared__ float tab[3 * MAX_AXIS];
  for (int t = threadIdx.x; t < wd + wh + ww; t += TPB) tab[t] = wts[t];
  const int* __restrict__ st = starts + 3 * (long)first;
  int d0 = D, d1 = 0, h0 = H, h1 = 0, w0 = W, w1 = 0;
  for (int b = 0; b < B; ++b) {
    box_axis(st[3 * b], wd, D, d0, d1);
    box_axis(st[3 * b + 1], wh, H, h0, h1);
    box_axis(st[3 * b + 2], ww, W, w0, w1);
  }
  __syncthreads();
  if (d1 <= d0 || h1 <= h0 || w1 <= w0) return;
  const int bh = h1 - h0, bw = w1 - w0;
  const long total = (long)(d1 - d0) * bh * bw;
  const long win = (long)wd * wh * ww;
  const float fk = (float)k;
  for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
    const long line = i / bw;
    const int w = w0 + (int)(i - line * bw);
    const int dd = (int)(line / bh);
    const int h = h0 + (int)(line - (long)dd * bh), d = d0 + dd;
    const long vox = ((long)d * H + h) * W + w;
    float a = acc[vox], s = wsum[vox];
    bool covered = false;
    for (int b = 0; b < B; ++b) {
      const long la = (long)d - st[3 * b], lb = (long)h - st[3 * b + 1], lc = (long)w - st[3 * b + 2];
      if (la < 0 || la >= wd || lb < 0 || lb >= wh || lc < 0 || lc >= ww) continue;
      const int ia = (int)la, ib = (int)lb, ic = (int)lc;
      const float wgt = (tab[ia] * tab[wd + ib]) * tab[wd + wh + ic];
      const float* __restrict__ p = probs + (long)b * k * win;
      float m = p[((long)ia * wh + ib) * ww + ic];
      for (int j = 1; j < k; ++j) {
        const int f = flip_of(flips, j);
        const int ja = (f & 1) ? wd - 1 - ia : ia, jb = (f & 2) ? wh - 1 - ib : ib, jc = (f & 4) ? ww - 1 - ic : ic;
        m = m + p[j * win + ((long)ja * wh + jb) * ww + jc];
      }
      if (k > 1) m = m / fk;  // tta_mean divides by float32(k); x / 1 is x
      a = a + wgt * m;
      s = s + wgt;
      covered = true;
    }
    if (covered) {
      acc[vox] = a;
      wsum[vox] = s;
    }
  }
}

// ---- prob = acc / wsum ---------------------------------------------------------------------
// [head, head + 4 nvec): the part all three pointers see 16-byte aligned, as vectors; the
// elements before and after it one by one (nvec == 0 when the pointers' offsets differ)
__global__ void __launch_bounds__(TPB) window_finish_kernel(const float* __restrict__ acc,
                                                            const float* __restrict__ wsum, float* __restrict__ prob,
                                                            long n, long head, long nvec) {
  const long tid = blockIdx.x * (long)TPB + threadIdx.x, nthr = (long)gridDim.x * TPB;
  const f32x4_t* __restrict__ va = reinterpret_cast<const f32x4_t*>(acc + head);
  const f32x4_t* __restrict__ vs = reinterpret_cast<const f32x4_t*>(wsum + head);
  f32x4_t* __restrict__ vp = reinterpret_cast<f32x4_t*>(prob + head);
  for (long i = tid; i < nvec; i += nthr) {
    const f32x4_t a = va[i], s = vs[i];
    f32x4_t r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = a[e] / s[e];
    vp[i] = r;
  }
  const long tail0 = head + 4 * nvec;
  const long nedge = head + (n - tail0);
  for (long i = tid; i < nedge; i += nthr) {
    const long at = i < head ? i : tail0 + (i - head);
    prob[at] = acc[at] / wsum[at];
  }
}

// the k host flip sets as one word; false for a set outside 0..7 or a first set that is not 0
inline bool pack_flips(const int* flipmask, int k, unsigned* packed) {
  *packed = 0;
  for (int j = 0; j < k; ++j) {
    if (flipmask[j] < 0 || flipmask[j] > 7 || (j == 0 && flipmask[j] != 0)) return false;
    *packed |= (unsigned)flipmask[j] << (3 * j);
  }
  return true;
}

inline bool bad_window(int wd, int wh, int ww) {
  return wd < 1 || wh < 1 || ww < 1 || wd > MAX_AXIS || wh > MAX_AXIS || ww > MAX_AXIS;
}

}  // namespace

extern "C" {

int pcms_window_gather(const float* x, int C, int D, int H, int W, const int* starts, int B, const int* flipmask, int k,
                       int wd, int wh, int ww, float* out, hipStream_t s) {
  if (x == nullptr || starts == nullptr || flipmask == nullptr || out == nullptr) return -1;
  if (C < 1 || D < 1 || H < 1 || W < 1 || B < 1 || k < 1 || k > MAX_FLIPS || bad_window(wd, wh, ww)) return -1;
  if (misaligned(x, alignof(float)) || misaligned(out, alignof(float)) || misaligned(starts, alignof(int))) return -1;
  if ((long)B * k * C > 0x7fffffffL) return -1;
  unsigned flips;
  if (!pack_flips(flipmask, k, &flips)) return -1;
  const long quads = (long)B * k * C * wd * wh * ((ww + 3) / 4);
  const int grid = grid_for(quads, TPB, MAX_WGS);
  if (ww % 4 == 0 && !misaligned(out, 16))
    hipLaunchKernelGGL(window_gather_kernel<true>, dim3(grid), dim3(TPB), 0, s, x, starts, flips, k, C, D, H, W, B, wd,
                       wh, ww, out);
  else
    hipLaunchKernelGGL(window_gather_kernel<false>, dim3(grid), dim3(TPB), 0, s, x, starts, flips, k, C, D, H, W, B, wd,
                       wh, ww, out);
  PCMS_CHECK_LAUNCH();
}

int pcms_window_blend(const float* probs, const int* starts, int first_window, int B, const int* flipmask, int k,
                      const float* wts, int wd, int wh, int ww, float* acc, float* wsum, int D, int H, int W,
                      hipStream_t s) {
  if (probs == nullptr || starts == nullptr || flipmask == nullptr || wts == nullptr || acc == nullptr ||
      wsum == nullptr)
    return -1;
  if (first_window < 0 || B < 1 || k < 1 || k > MAX_FLIPS || D < 1 || H < 1 || W < 1 || bad_window(wd, wh, ww))
    return -1;
  if (misaligned(probs, alignof(float)) || misaligned(wts, alignof(float)) || misaligned(acc, alignof(float)) ||
      misaligned(wsum, alignof(float)) || misaligned(starts, alignof(int)))
    return -1;
  if ((long)first_window + B > 0x7fffffffL / 3) return -1;
  unsigned flips;
  if (!pack_flips(flipmask, k, &flips)) return -1;
  // the bounding box is known on the device only: sized for the whole volume, capped
  const int grid = grid_for((long)D * H * W, TPB, MAX_WGS);
  hipLaunchKernelGGL(window_blend_kernel, dim3(grid), dim3(TPB), 0, s, probs, starts, first_window, B, flips, k, wts,
                     wd, wh, ww, acc, wsum, D, H, W);
  PCMS_CHECK_LAUNCH();
}

int pcms_window_finish(const float* acc, const float* wsum, float* prob, long n, hipStream_t s) {
  if (acc == nullptr || wsum == nullptr || prob == nullptr || n < 1) return -1;
  if (misaligned(acc, alignof(float)) || misaligned(wsum, alignof(float)) || misaligned(prob, alignof(float)))
    return -1;
  const uintptr_t off = (uintptr_t)prob & 15;
  long head = n, nvec = 0;
  if (((uintptr_t)acc & 15) == off && ((uintptr_t)wsum & 15) == off) {
    const long to_boundary = (long)(((16 - off) & 15) / sizeof(float));
    head = to_boundary < n ? to_boundary : n;
    nvec = (n - head) / 4;
  }
  const int grid = grid_for(nvec > 0 ? nvec : n, TPB, MAX_WGS);
  hipLaunchKernelGGL(window_finish_kernel, dim3(grid), dim3(TPB), 0, s, acc, wsum, prob, n, head, nvec);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
