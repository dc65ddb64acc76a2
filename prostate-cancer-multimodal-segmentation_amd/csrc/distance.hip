// Surface distances on the device (gfx950): distance.py's host forms surface / edt_sq and the
// per-direction statistics of surface_metrics, the transform bit for bit.
//
//   pcms_mask_surface            surface(mask): foreground with a face neighbour that is
//                                background or outside the volume
//   pcms_edt_sq                  the exact squared Euclidean distance to the nearest feature
//                                voxel under per-axis spacing, fp64
//   pcms_surface_distance_stats  the squared distances at the voxels of surface(a), their count,
//                                maximum and the sum of their square roots
//
// The transform is three passes over lines (distance_lines.h has the arithmetic, why the
// separable form has the bits of the definition, and the loop bounds):
//   W  one wave per row: the row's features as ballot words in LDS, every voxel the distance
//      to the nearest set bit; stored as a byte (W <= 255) or 16 bits, a sentinel for a row
//      without a feature
//   H  one workgroup per (d, slab of SLAB adjacent w, chunk of 64 h): the slab's H x SLAB
//      integers staged in LDS, every thread minimises over its own line for the chunk's
//      positions, walking outward from its own position (the chunks restage the slab, a 2-byte
//      read per voxel from L2, and give 24 x 384 x 384 1728 workgroups, four resident per CU,
//      where one per slab left the machine at one wave per SIMD)
//   D  one workgroup per (h, slab) on the H pass's fp64 values, in place: a workgroup reads only
//      the D x SLAB values it then overwrites, after a barrier
// A slab is SLAB = 32 columns: 64 to 256-byte contiguous segments per line position in global
// memory, consecutive lanes on consecutive LDS words.  LINE_BYTES is the line buffer of one
// workgroup (its LDS is that plus 256 bytes for the workgroup-wide OR): 32 KiB where the slab fits
// it (H = 384 as 16-bit integers: 24 KiB; four workgroups per 160 KiB CU), else 64 KiB (two per
// CU) with the slab halved until the line fits; 2048 positions of fp64 fit at 4 columns.  Longer
// axes cannot be staged: MAX_AXIS.
//
// Workspace bytes: the W pass's integers (n or 2 n), or the statistics' partials (24 bytes per
// workgroup, at most ST_MAX_WGS of them), whichever is larger.
#include "common.h"

#include "distance_lines.h"
#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

using namespace pcms_edt;

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int SLAB_LOG2 = 5;  // SLAB = 32 columns
constexpr int CHUNK = 64;      // line positions one workgroup of the H pass computes (8 per thread at 32 columns)
constexpr int LDS_SMALL = 32 << 10, LDS_LARGE = 64 << 10;
constexpr long MAX_VOXELS = (1l << 30) - 4096;  // 2 n bytes of workspace fit an int
constexpr int ST_MAX_WGS = 1024;                // partials the finish kernel folds
constexpr int ST_PER_WG = TPB * 16;             // voxels per workgroup before the grid stops growing
constexpr int ST_WORDS = 3;                     // count, max, sum

// a line in LDS, `step` elements between consecutive positions
template <typename T>
struct LdsLine {
  const T* p;
  int step;
  __device__ __forceinline__ T load(int i) const { return p[i * step]; }
};
struct LdsWords {
  const uint64_t* p;
  __device__ __forceinline__ uint64_t load(int i) const { return p[i]; }
};
struct GlobalBytes {
  const uint8_t* p;
  __device__ __forceinline__ uint8_t load(long i) const { return p[i]; }
};

__global__ void __launch_bounds__(TPB) surface_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                      int D, int H, int W) {
  const long HW = (long)H * W;
  const long n = (long)D * HW;
  const GlobalBytes m{mask};
  for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / W), w = (int)(r - (long)h * W);
    out[i] = on_surface(m, d, h, w, D, H, W) ? 1 : 0;
  }
}

// ---- W pass --------------------------------------------------------------------------------
template <typename G>
__global__ void __launch_bounds__(TPB) edt_w_kernel(const uint8_t* __restrict__ feat, G* __restrict__ g1, long rows,
                                                    int W, int nwords) {
  __shared__ uint64_t bits[WAVES][MAX_WORDS];
  constexpr int NONE = sizeof(G) == 1 ? NONE8 : NONE16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = blockIdx.x * (long)WAVES + wave;
  const bool valid = row < rows;
  for (int c = 0; c < nwords; ++c) {  // nwords is uniform: every wave reaches the barrier
    const int pos = c * 64 + lane;
    const bool f = valid && pos < W && feat[row * W + pos] != 0;
    const uint64_t word = __ballot(f);
    if (lane == 0) bits[wave][c] = word;
  }
  __syncthreads();
  if (!valid) return;
  const LdsWords m{bits[wave]};
  for (int c = 0; c < nwords; ++c) {
    const int pos = c * 64 + lane;
    if (pos >= W) break;
    const int dist = w_line_dist(m, nwords, pos);
    g1[row * W + pos] = (G)(dist < 0 ? NONE : dist);
  }
}

// ---- H and D passes ------------------------------------------------------------------------
// Workgroup b takes slab b % nslab and chunk (b / nslab) % nchunk of outer index
// b / (nslab nchunk): it stages the slab's whole lines and computes `chunk` positions of them.
// Element (p, w) of its lines sits at base + p * stride + w in src and dst; base =
// outer * outer_stride + slab * sw.  More than one chunk only where src and dst are different
// arrays (the H pass): in place, another workgroup would overwrite what this one still stages.
struct Lines {
  int L;              // positions per line
  long stride;        // elements between consecutive positions
  long outer_stride;  // elements between consecutive outer indices
  int W, nslab, lg;   // row length, slabs per row, log2 of the slab's columns
  int nchunk, chunk;  // chunks per line, positions per chunk
};

template <typename T, int LINE_BYTES>
__global__ void __launch_bounds__(TPB) edt_line_kernel(const T* src, double* dst, Lines ln, double s_axis, double s_w) {
  __shared__ T line[LINE_BYTES / sizeof(T)];
  constexpr bool H_PASS = !std::is_same<T, double>::value;
  constexpr int NONE = sizeof(T) == 1 ? NONE8 : NONE16;
  const int sw = 1 << ln.lg;
  const int slab = blockIdx.x % ln.nslab;
  const int rest = blockIdx.x / ln.nslab;
  const int p0 = (rest % ln.nchunk) * ln.chunk;
  const long outer = rest / ln.nchunk;
  const int w0 = slab * sw;
  const long base = outer * ln.outer_stride + w0;
  const int total = ln.L * sw;  // <= LINE_BYTES / sizeof(T): the launcher chose lg so
  bool any = false;             // a candidate that is not "no feature"
  for (int idx = threadIdx.x; idx < total; idx += TPB) {
    const int p = idx >> ln.lg, w = idx & (sw - 1);
    T v;
    if constexpr (H_PASS) v = (T)NONE; else v = infinity();  // columns past the row: never read back
    if (w0 + w < ln.W) {
      v = src[base + p * ln.stride + w];
      if constexpr (H_PASS) any = any || v != (T)NONE; else any = any || v < infinity();
    }
    line[idx] = v;
  }
  // the barrier; without any candidate in the slab every minimum is +inf and nothing walks
  const bool some = __syncthreads_or(any) != 0;
  const int p1 = p0 + ln.chunk < ln.L ? p0 + ln.chunk : ln.L;
  const int count = (p1 - p0) * sw;
  for (int idx = threadIdx.x; idx < count; idx += TPB) {
    const int p = p0 + (idx >> ln.lg), w = idx & (sw - 1);
    if (w0 + w >= ln.W) continue;
    const LdsLine<T> m{line + w, sw};
    double best = infinity();
    if (some) {
      if constexpr (H_PASS) best = h_line_min(m, ln.L, p, s_axis, s_w, NONE);
      else best = d_line_min(m, ln.L, p, s_axis);
    }
    dst[base + p * ln.stride + w] = best;
  }
}

// ---- statistics ------------------------------------------------------------------------------
struct Stats {
  long long count;
  double mx, sum;
};

// the workgroup's statistics in thread 0: waves by shuffles, then the wave results in order
__device__ __forceinline__ void block_stats(Stats& st) {
  __shared__ Stats part[WAVES];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    st.count += __shfl_xor(st.count, o, 64);
    const double other = __shfl_xor(st.mx, o, 64);
    st.mx = other > st.mx ? other : st.mx;
    st.sum = st.sum + __shfl_xor(st.sum, o, 64);
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = st;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      st.count += part[w].count;
      st.mx = part[w].mx > st.mx ? part[w].mx : st.mx;
      st.sum = st.sum + part[w].sum;
    }
  }
}

__device__ __forceinline__ void store_stats(const Stats& st, double* dst) {
  dst[0] = __longlong_as_double(st.count);
  dst[1] = st.mx;
  dst[2] = st.sum;
}

__global__ void __launch_bounds__(TPB) sd_partial_kernel(const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ sq, double* __restrict__ sd_sq,
                                                         double* __restrict__ part, int D, int H, int W) {
  const long HW = (long)H * W;
  const long n = (long)D * HW;
  const GlobalBytes m{mask};
  Stats st{0, -1.0, 0.0};
  for (long i = blockIdx.x * (long)TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / W), w = (int)(r - (long)h * W);
    double v = -1.0;
    if (on_surface(m, d, h, w, D, H, W)) {
      v = sq[i];
      st.count += 1;
      st.mx = v > st.mx ? v : st.mx;
      st.sum = st.sum + sqrt(v);
    }
    sd_sq[i] = v;
  }
  block_stats(st);
  if (threadIdx.x == 0) store_stats(st, part + ST_WORDS * blockIdx.x);
}

// one workgroup: the partials in a fixed order -> stats
__global__ void __launch_bounds__(TPB) sd_finish_kernel(const double* __restrict__ part, int nparts,
                                                        double* __restrict__ stats) {
  Stats st{0, -1.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += TPB) {
    st.count += __double_as_longlong(part[ST_WORDS * i]);
    const double mx = part[ST_WORDS * i + 1];
    st.mx = mx > st.mx ? mx : st.mx;
    st.sum = st.sum + part[ST_WORDS * i + 2];
  }
  block_stats(st);
  if (threadIdx.x == 0) store_stats(st, stats);
}

// ---- host side -------------------------------------------------------------------------------
inline long voxels(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1 || D > MAX_AXIS || H > MAX_AXIS || W > MAX_AXIS) return -1;
  const long n = (long)D * H * W;
  return n > MAX_VOXELS ? -1 : n;
}
inline int stats_grid(long n) { return grid_for(n, ST_PER_WG, ST_MAX_WGS); }
inline long work_bytes(long n, int W) {
  const long g1 = (n * (W <= NONE8 ? 1 : 2) + 7) & ~7l;
  const long st = (long)ST_MAX_WGS * ST_WORDS * 8;
  return g1 > st ? g1 : st;
}
inline bool good_spacing(double s) { return s > 0.0 && s < infinity(); }  // false for a NaN

// the slab's columns (as log2) for lines of L elements of `elem` bytes: 32, halved until the
// slab fits LDS_LARGE (MAX_AXIS positions of fp64 at 4 columns)
inline int slab_log2(int L, int elem) {
  int lg = SLAB_LOG2;
  while (((long)L << lg) * elem > LDS_LARGE) --lg;
  return lg;
}

template <typename T>
int launch_lines(const T* src, double* dst, int L, long stride, long outer_stride, long nouter, int W, double s_axis,
                 double s_w, hipStream_t s) {
  const bool in_place = (const void*)src == (const void*)dst;
  Lines ln;
  ln.L = L;
  ln.stride = stride;
  ln.outer_stride = outer_stride;
  ln.W = W;
  ln.lg = slab_log2(L, (int)sizeof(T));
  ln.nslab = cdiv(W, 1 << ln.lg);
  ln.chunk = in_place ? L : CHUNK;
  ln.nchunk = cdiv(L, ln.chunk);
  const long grid = nouter * ln.nslab * ln.nchunk;
  if (((long)L << ln.lg) * (long)sizeof(T) <= LDS_SMALL)
    hipLaunchKernelGGL((edt_line_kernel<T, LDS_SMALL>), dim3((unsigned)grid), dim3(TPB), 0, s, src, dst, ln, s_axis,
                       s_w);
  else
    hipLaunchKernelGGL((edt_line_kernel<T, LDS_LARGE>), dim3((unsigned)grid), dim3(TPB), 0, s, src, dst, ln, s_axis,
                       s_w);
  PCMS_CHECK_LAUNCH();
}

template <typename G>
int launch_edt(const uint8_t* feat, const double* sp, double* out, G* g1, int D, int H, int W, hipStream_t s) {
  const long rows = (long)D * H;
  hipLaunchKernelGGL(edt_w_kernel<G>, dim3((unsigned)cdiv(rows, WAVES)), dim3(TPB), 0, s, feat, g1, rows, W,
                     cdiv(W, 64));
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  rc = launch_lines<G>(g1, out, H, W, (long)H * W, D, W, sp[1], sp[2], s);
  if (rc != 0) return rc;
  return launch_lines<double>(out, out, D, (long)H * W, W, H, W, sp[0], 0.0, s);
}

}  // namespace

extern "C" {

int pcms_mask_surface(const unsigned char* mask, unsigned char* out, int D, int H, int W, hipStream_t s) {
  const long n = voxels(D, H, W);
  if (mask == nullptr || out == nullptr || n < 0 || overlap(mask, n, out, n)) return -1;
  hipLaunchKernelGGL(surface_kernel, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, mask, out, D, H, W);
  PCMS_CHECK_LAUNCH();
}

int pcms_edt_work_bytes(int D, int H, int W) {
  const long n = voxels(D, H, W);
  return n < 0 ? -1 : (int)work_bytes(n, W);
}

int pcms_edt_sq(const unsigned char* feat, const double* spacing, double* out, void* work, int D, int H, int W,
                hipStream_t s) {
  const long n = voxels(D, H, W);
  if (feat == nullptr || spacing == nullptr || out == nullptr || work == nullptr || n < 0) return -1;
  if (misaligned(out, alignof(double)) || misaligned(work, 8)) return -1;
  if (!good_spacing(spacing[0]) || !good_spacing(spacing[1]) || !good_spacing(spacing[2])) return -1;
  const long wb = work_bytes(n, W);
  if (overlap(feat, n, out, 8 * n) || overlap(feat, n, work, wb) || overlap(out, 8 * n, work, wb)) return -1;
  if (W <= NONE8) return launch_edt<uint8_t>(feat, spacing, out, (uint8_t*)work, D, H, W, s);
  return launch_edt<uint16_t>(feat, spacing, out, (uint16_t*)work, D, H, W, s);
}

int pcms_surface_distance_stats(const unsigned char* mask_a, const double* sq_b, double* sd_sq_out, void* stats,
                                void* work, int D, int H, int W, hipStream_t s) {
  const long n = voxels(D, H, W);
  if (mask_a == nullptr || sq_b == nullptr || sd_sq_out == nullptr || stats == nullptr || work == nullptr || n < 0)
    return -1;
  if (misaligned(sq_b, alignof(double)) || misaligned(sd_sq_out, alignof(double)) || misaligned(stats, 8) ||
      misaligned(work, 8))
    return -1;
  const long wb = work_bytes(n, W), sb = ST_WORDS * 8;
  const void* ins[2] = {mask_a, sq_b};
  const long in_bytes[2] = {n, 8 * n};
  for (int i = 0; i < 2; ++i)
    if (overlap(ins[i], in_bytes[i], sd_sq_out, 8 * n) || overlap(ins[i], in_bytes[i], stats, sb) ||
        overlap(ins[i], in_bytes[i], work, wb))
      return -1;
  if (overlap(sd_sq_out, 8 * n, stats, sb) || overlap(sd_sq_out, 8 * n, work, wb) || overlap(stats, sb, work, wb))
    return -1;
  const int grid = stats_grid(n);
  hipLaunchKernelGGL(sd_partial_kernel, dim3(grid), dim3(TPB), 0, s, mask_a, sq_b, sd_sq_out, (double*)work, D, H, W);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(sd_finish_kernel, dim3(1), dim3(TPB), 0, s, (const double*)work, grid, (double*)stats);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
