// Patch training on the device (gfx950): data.py's host forms pick_origins / resample_patch
// evaluated per voxel, bit for bit.
//
//   pcms_foreground_pick        the origins of P patches of a label grid: a patch with a rank takes
//                               the box around the r-th foreground voxel in flat order, every other
//                               one its fallback origin; chosen on the device, consumed there
//   pcms_patch_resample_linear  pcms_resample_affine_linear evaluated only at the voxels of P
//                               patches whose origins are device memory, zero outside the grid
//
// The pick is three launches and no atomics: per-chunk foreground counts, one workgroup's
// exclusive scan of them, one workgroup per patch that finds its chunk by binary search and its
// voxel by ballots.  The resample's coordinate arithmetic is resample_common.h's: every product
// and sum rounds on its own, no contraction into FMAs anywhere in this file.
#include "resample_common.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_WGS = 2048;          // 256 CUs x 8 workgroups; the grid-stride loops take the rest
constexpr int MAX_PATCHES = 64;
constexpr int CHUNK = TPB * 16;        // voxels per counting chunk: four 16-byte loads per thread
constexpr int WAVE_SPAN = CHUNK / WAVES;  // consecutive voxels one wave of the pick re-reads
constexpr int STEPS = WAVE_SPAN / 64;     // ... in this many 64-lane steps

inline long chunks_of(long n) { return (n + CHUNK - 1) / CHUNK; }

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- counts[k] = the number of voxels > 0 in [k CHUNK, min((k + 1) CHUNK, n)) -----------------
// A workgroup takes chunks blockIdx.x, blockIdx.x + gridDim.x, ...  VEC (label 16-byte aligned):
// a chunk starts at a multiple of CHUNK floats, so its whole quads are 16-byte loads and only the
// last chunk has up to three single voxels after them; else every voxel is a load of its own.
template <bool VEC>
__global__ void __launch_bounds__(TPB) foreground_count_kernel(const float* __restrict__ label, long n, int nchunks,
                                                               int* __restrict__ counts) {
  __shared__ int part[WAVES];
  for (int k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const long c0 = (long)k * CHUNK;
    const int len = (int)(n - c0 < CHUNK ? n - c0 : CHUNK);
    int cnt = 0;
    if constexpr (VEC) {
      const int quads = len >> 2;
      const f32x4_t* __restrict__ v = reinterpret_cast<const f32x4_t*>(label + c0);
      for (int q = threadIdx.x; q < quads; q += TPB) {
        const f32x4_t x = v[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt += x[e] > 0.f ? 1 : 0;
      }
      const int e = 4 * quads + threadIdx.x;
      if (e < len) cnt += label[c0 + e] > 0.f ? 1 : 0;
    } else {
      for (int e = threadIdx.x; e < len; e += TPB) cnt += label[c0 + e] > 0.f ? 1 : 0;
    }
    cnt = wave_sum_int(cnt);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = part[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) sum += part[w];
      counts[k] = sum;
    }
    __syncthreads();  // part is reused by the next chunk
  }
}

// ---- one workgroup: work[k] = sum of counts below k, work[nchunks] = *total = T -----------------
// TPB counts per pass: an inclusive scan inside each wave by shuffles, the four wave totals
// through LDS, the running sum of the passes so far carried in a register of every thread.
__global__ void __launch_bounds__(TPB) foreground_scan_kernel(int* __restrict__ work, int nchunks,
                                                              int* __restrict__ total) {
  __shared__ int wtot[WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nchunks; base += TPB) {
    const int i = base + threadIdx.x;
    const int v = i < nchunks ? work[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wv] = x;
    __syncthreads();
    int below = 0, pass = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int t = wtot[w];
      below += w < wv ? t : 0;
      pass += t;
    }
    if (i < nchunks) work[i] = carry + below + (x - v);
    carry += pass;
    __syncthreads();  // wtot is reused by the next pass
  }
  if (threadIdx.x == 0) {
    work[nchunks] = carry;
    *total = carry;
  }
}

struct Box {
  int Gd, Gh, Gw, wd, wh, ww;
};
__device__ __forceinline__ int clamp_origin(long o, int G, int w) {
  const long top = G > w ? G - w : 0;
  return (int)(o < 0 ? 0 : o > top ? top : o);
}

// ---- one workgroup per patch ------------------------------------------------------------------
// rank_u and fallback are device memory and are not trusted.  A patch takes its fallback row
// (clamped into [0, max(G - w, 0)]) when its rank is below 0 or the grid has no foreground; else
// r = floor(rank T) capped at T - 1 (a NaN compares false and so lands there too), the chunk is
// the last one whose prefix is <= r, and wave v re-reads voxels [v, v + 1) WAVE_SPAN of it in
// STEPS steps of 64: the ballots give the wave's total and, after the four totals met in LDS, the
// lane whose voxel has exactly r - prefix foreground voxels before it in the chunk writes the
// clamped origin.  Exactly one lane does: prefix[k] <= r < prefix[k] + counts[k].
__global__ void __launch_bounds__(TPB) foreground_pick_kernel(const float* __restrict__ label, long n, int nchunks,
                                                              const int* __restrict__ prefix, Box g,
                                                              const double* __restrict__ rank_u,
                                                              const int* __restrict__ fallback,
                                                              int* __restrict__ picks) {
  __shared__ int wtot[WAVES];
  const int p = blockIdx.x;
  const int T = prefix[nchunks];
  const double u = rank_u[p];
  if (u < 0.0 || T < 1) {
    if (threadIdx.x < 3) {
      const int a = threadIdx.x;
      picks[3 * p + a] = clamp_origin(fallback[3 * p + a], a == 0 ? g.Gd : a == 1 ? g.Gh : g.Gw,
                                      a == 0 ? g.wd : a == 1 ? g.wh : g.ww);
    }
    return;
  }
  const double x = floor(u * (double)T);
  const int r = x < (double)(T - 1) ? (int)x : T - 1;  // 0 <= x here, or NaN / too large: T - 1
  int lo = 0, hi = nchunks - 1;  // the last k with prefix[k] <= r; prefix[0] = 0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int local = r - prefix[lo];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long first = (long)lo * CHUNK + (long)wv * WAVE_SPAN + lane;
  unsigned mine = 0;
  int total = 0;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const long at = first + s * 64;
    const bool fg = at < n && label[at] > 0.f;
    total += __popcll(__ballot(fg));
    mine |= (fg ? 1u : 0u) << s;
  }
  if (lane == 0) wtot[wv] = total;
  __syncthreads();
  int target = local;
  for (int w = 0; w < wv; ++w) target -= wtot[w];
  if (target < 0 || target >= total) return;  // wave-uniform: another wave holds the voxel
  const unsigned long long below = (1ull << lane) - 1ull;
  int seen = 0;
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const bool fg = (mine >> s) & 1u;
    const unsigned long long m = __ballot(fg);
    if (fg && seen + __popcll(m & below) == target) {
      const long v = first + s * 64;
      const long hw = (long)g.Gh * g.Gw;
      const int vd = (int)(v / hw);
      const int rem = (int)(v - vd * hw);
      const int vh = rem / g.Gw, vw = rem - vh * g.Gw;
      picks[3 * p] = clamp_origin((long)vd - g.wd / 2, g.Gd, g.wd);
      picks[3 * p + 1] = clamp_origin((long)vh - g.wh / 2, g.Gh, g.wh);
      picks[3 * p + 2] = clamp_origin((long)vw - g.ww / 2, g.Gw, g.ww);
    }
    seen += __popcll(m);
  }
}

// ---- resample_patch ---------------------------------------------------------------------------
// out + p stride is patch p, (D, H, W); one thread forms four consecutive w of one patch row.
// Patch index (a, b, c) stands for grid index q = (a, b, c) + origin_p, formed in 64-bit integers
// (an origin is device memory and is not trusted) and exact as a double; the voxel is 0 where q
// leaves the grid, else resample_affine's value at q: the coordinate, the inside rule on the
// doubles -- so nothing outside src is read wherever q lies -- the lerps and the intensity step.
// NORM: every corner is intensity.normalise's value, as in pcms_resample_linear_norm.  vec (W % 4
// == 0, out and stride 16-byte aligned): one 16-byte store, else up to four scalars.
// Registers: the four elements are a rolled loop whose row indices pass through an empty asm, so
// that the row's three partial coordinate sums are formed per element instead of staying live
// across the loop, and den is wave-uniform and kept in an SGPR; unrolled, the normalising
// instances needed 67..69 VGPRs, one wave per SIMD fewer.
struct Grid {
  int Gd, Gh, Gw;
};

template <typename T, bool NORM>
__global__ void __launch_bounds__(TPB) patch_resample_kernel(const T* __restrict__ src, const float* __restrict__ lohi,
                                                             const int* __restrict__ origins, float* __restrict__ out,
                                                             long stride, int P, Affine m, Dims g, Grid gr, Scale sc,
                                                             float gain, float bias, int intensity, int vec) {
  const int qw = (g.W + 3) >> 2;
  const int plane = g.D * g.H;
  const long total = (long)P * plane * qw;
  float lo = 0.f, den = 1.f;
  if constexpr (NORM) {
    lo = lohi[0];
    const float d = (float)((double)lohi[1] - (double)lo);
    den = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d)));
  }
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
        if constexpr (NORM)
          v[e] = affine_linear_gather(g, cd, ch, cw, gain, bias, intensity,
                                      [&](long x) { return (double)normalised(image_value(src[x], sc), lo, den); });
        else
          v[e] = affine_linear_value(src, g, sc, cd, ch, cw, gain, bias, intensity);
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

template <typename T>
int launch_patches(const void* src, const float* lohi, const int* origins, float* out, long stride, int P,
                   const Affine& m, const Dims& g, const Grid& gr, const Scale& sc, float gain, float bias,
                   hipStream_t s) {
  if (misaligned(src, alignof(T))) return -1;
  const long quads = (long)P * g.D * g.H * ((g.W + 3) / 4);
  const int grid = grid_for(quads, TPB, MAX_WGS);
  const int intensity = (gain == 1.f && bias == 0.f) ? 0 : 1;
  const int vec = (g.W % 4 == 0 && stride % 4 == 0 && !misaligned(out, 16)) ? 1 : 0;
  if (lohi != nullptr)
    hipLaunchKernelGGL((patch_resample_kernel<T, true>), dim3(grid), dim3(TPB), 0, s, (const T*)src, lohi, origins, out,
                       stride, P, m, g, gr, sc, gain, bias, intensity, vec);
  else
    hipLaunchKernelGGL((patch_resample_kernel<T, false>), dim3(grid), dim3(TPB), 0, s, (const T*)src, lohi, origins,
                       out, stride, P, m, g, gr, sc, gain, bias, intensity, vec);
  PCMS_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

int pcms_foreground_pick_chunk(void) { return CHUNK; }

int pcms_foreground_pick_work_ints(long n) { return (n < 1 || n > 0x7fffffffL) ? -1 : (int)chunks_of(n) + 1; }

int pcms_foreground_pick(const float* label, long n, int Gd, int Gh, int Gw, int wd, int wh, int ww,
                         const double* rank_u, const int* fallback, int P, int* picks, int* work, hipStream_t s) {
  if (label == nullptr || rank_u == nullptr || fallback == nullptr || picks == nullptr || work == nullptr) return -1;
  if (P < 1 || P > MAX_PATCHES || Gd < 1 || Gh < 1 || Gw < 1 || wd < 1 || wh < 1 || ww < 1) return -1;
  if (n > 0x7fffffffL || n != (long)Gd * Gh * Gw) return -1;
  if (misaligned(label, alignof(float)) || misaligned(rank_u, alignof(double)) || misaligned(fallback, alignof(int)) ||
      misaligned(picks, alignof(int)) || misaligned(work, alignof(int)))
    return -1;
  const int nchunks = (int)chunks_of(n);
  const int grid = nchunks < MAX_WGS ? nchunks : MAX_WGS;
  if (!misaligned(label, 16))
    hipLaunchKernelGGL(foreground_count_kernel<true>, dim3(grid), dim3(TPB), 0, s, label, n, nchunks, work);
  else
    hipLaunchKernelGGL(foreground_count_kernel<false>, dim3(grid), dim3(TPB), 0, s, label, n, nchunks, work);
  hipLaunchKernelGGL(foreground_scan_kernel, dim3(1), dim3(TPB), 0, s, work, nchunks, picks + 3 * P);
  hipLaunchKernelGGL(foreground_pick_kernel, dim3(P), dim3(TPB), 0, s, label, n, nchunks, (const int*)work,
                     Box{Gd, Gh, Gw, wd, wh, ww}, rank_u, fallback, picks);
  PCMS_CHECK_LAUNCH();
}

int pcms_patch_resample_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                               double scl_inter, const double* affine12, const float* lohi, float gain, float bias,
                               int Gd, int Gh, int Gw, const int* origins, int P, float* out, long patch_stride, int D,
                               int H, int W, hipStream_t s) {
  if (!affine_args_ok(src, out, affine12, Di, Hi, Wi, D, H, W, gain, bias)) return -1;
  if (origins == nullptr || Gd < 1 || Gh < 1 || Gw < 1 || P < 1 || P > MAX_PATCHES) return -1;
  if (misaligned(origins, alignof(int)) || misaligned(lohi, alignof(float))) return -1;
  if (patch_stride < (long)D * H * W || (long)D * H > 0x7fffffffL) return -1;  // a patch's rows are counted in an int
  const Affine m = make_affine(affine12);  // copied into the kernel arguments
  const Dims g{Di, Hi, Wi, D, H, W};
  const Grid gr{Gd, Gh, Gw};
  const Scale sc = make_scale(scl_slope, scl_inter);
  return for_datatype(datatype, [&](auto t) {
    return launch_patches<decltype(t)>(src, lohi, origins, out, patch_stride, P, m, g, gr, sc, gain, bias, s);
  });
}

}  // extern "C"
