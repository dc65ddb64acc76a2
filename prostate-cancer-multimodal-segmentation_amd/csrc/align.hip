// The similarity of rigid registration on the device (gfx950): align.py's host form
// joint_histogram evaluated on two raw NIfTI volumes, on the counts exactly.
//
//   pcms_joint_histogram  hist[bf][bm] = the number of lattice voxels q of the fixed volume whose
//                         window-normalised value falls in bin bf while the linear sample of the
//                         window-normalised moving volume at A q + t falls in bin bm
//
// Three launches: one zeroes the workspace, one gathers and counts, one sums the copies of the
// table.  Counts are integers, summed by integer atomics (LDS, then one global add per non-empty
// bin and workgroup into one of eight copies of the table), so the table is a function of the
// inputs alone.  The arithmetic is numpy's: every product, sum, difference and quotient rounds on
// its own, no contraction into FMAs anywhere in this file.
#include "resample_common.h"

#include "ops_units.h"
#include "pcms_hip.h"
#include "wave_hist.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_BINS = 64;           // the LDS table: 64 x 64 counts of 32 bits, 16 KB
// Workgroup b adds its non-empty bins once to copy b % COPIES of the table in work.  One
// evaluation of 24x384x384 against 20x128x128 at stride (1, 1, 1) / (1, 2, 2): 1 copy 59.0 / 28.1
// us, 8 copies 57.2 / 27.1 us, 32 copies 57.9 / 27.5 us (at 2048 voxels per workgroup).  The
// kernel waits on its gathers, so it wants many workgroups in flight, not fat ones: 16384 voxels
// per workgroup 178 / 158 us, 8192: 99 / 82, 4096: 69 / 45, 2048: 57 / 27, 1024: 49.4 / 21.0,
// 512: 49.4 / 20.6, 256: 49.1 / 21.1 (profiles/align_ab.txt)
constexpr int COPIES = 8;
constexpr int JH_MAX_WGS = 4096;       // 256 CUs x 16 workgroups
constexpr int JH_PER_WG = TPB * 4;     // lattice voxels per workgroup before the grid stops growing

// the fixed volume and the lattice on it: index (a, b, e) of (Ld, Lh, Lw) is voxel (a sd, b sh, e sw)
struct Lattice {
  int Hf, Wf, Lh, Lw, sd, sh, sw;
};

__global__ void __launch_bounds__(TPB) joint_zero_kernel(uint32_t* __restrict__ work, int words) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < words; i += gridDim.x * TPB) work[i] = 0u;
}

__global__ void __launch_bounds__(TPB) joint_sum_kernel(const uint32_t* __restrict__ work, int nb,
                                                        uint32_t* __restrict__ hist) {
  const int b = blockIdx.x * TPB + threadIdx.x;
  if (b >= nb) return;
  uint32_t c = 0u;
#pragma unroll
  for (int k = 0; k < COPIES; ++k) c += work[k * nb + b];
  hist[b] = c;
}

// the fixed voxel x as image_value decodes it; the datatype code is uniform over the grid, so the
// switch is a scalar branch
__device__ __forceinline__ float fixed_value(const void* p, int code, long x, const Scale& sc) {
  switch (code) {
    case 2: return image_value(static_cast<const uint8_t*>(p)[x], sc);
    case 4: return image_value(static_cast<const int16_t*>(p)[x], sc);
    case 8: return image_value(static_cast<const int32_t*>(p)[x], sc);
    case 16: return image_value(static_cast<const float*>(p)[x], sc);
    case 64: return image_value(static_cast<const double*>(p)[x], sc);
    case 256: return image_value(static_cast<const int8_t*>(p)[x], sc);
    case 512: return image_value(static_cast<const uint16_t*>(p)[x], sc);
    case 768: return image_value(static_cast<const uint32_t*>(p)[x], sc);
    case 1024: return image_value(static_cast<const int64_t*>(p)[x], sc);
    default: return image_value(static_cast<const uint64_t*>(p)[x], sc);
  }
}

// align._bin_index: fl32(v * (float)bins) clamped to [0, bins - 1] as a float, then truncated
// (for v in [0, 1] that is min((int)fl32(v bins), bins - 1)); v is not a NaN
__device__ __forceinline__ uint32_t bin_of(float v, float fbins, float top) {
  const float b = v * fbins;
  return (uint32_t)(int)(b < 0.f ? 0.f : b > top ? top : b);
}

// One thread per lattice voxel, grid-stride.  The loop bound is the wave's, not the lane's, so
// that all 64 lanes reach the ballots of bin_add; a lane past the end counts nothing.  The moving
// sample is affine_linear_gather's (resample_common.h) of the windowed corners; the kernel hides
// the latency of its nine dependent loads by occupancy alone.
template <typename TM>
__global__ void __launch_bounds__(TPB) joint_hist_kernel(const void* __restrict__ fix, int fcode,
                                                         const float* __restrict__ flohi, const TM* __restrict__ mov,
                                                         const float* __restrict__ mlohi, Affine m, Dims g, Lattice lt,
                                                         Scale fsc, Scale msc, int bins, uint32_t* __restrict__ work) {
  __shared__ uint32_t hist[MAX_BINS * MAX_BINS];
  const int nb = bins * bins;
  for (int b = threadIdx.x; b < nb; b += TPB) hist[b] = 0u;
  __syncthreads();
  const float flo = flohi[0], fhi = flohi[1], mlo = mlohi[0], mhi = mlohi[1];
  const float fden = (float)((double)fhi - (double)flo), mden = (float)((double)mhi - (double)mlo);
  const float fbins = (float)bins, top = (float)(bins - 1);
  const int lane = threadIdx.x & 63;
  const long plane = (long)lt.Lh * lt.Lw;
  const long total = (long)g.D * plane;  // g.D, g.H, g.W: the lattice (Ld, Lh, Lw)
  const long wave0 = blockIdx.x * (long)TPB + (threadIdx.x - lane), nthr = (long)gridDim.x * TPB;
  for (long base = wave0; base < total; base += nthr) {
    const long i = base + lane;
    bool on = false;
    uint32_t bin = 0u;
    if (i < total) {
      const int a = (int)(i / plane);
      const int r = (int)(i - a * plane);
      const int b = r / lt.Lw, e = r - b * lt.Lw;
      const int qd = a * lt.sd, qh = b * lt.sh, qw = e * lt.sw;
      const double fd = (double)qd, fh = (double)qh, fw = (double)qw;
      const double cd = affine_coord(m.d, fd, fh, fw), ch = affine_coord(m.h, fd, fh, fw),
                   cw = affine_coord(m.w, fd, fh, fw);
      if (linear_inside(cd, g.Di) && linear_inside(ch, g.Hi) && linear_inside(cw, g.Wi)) {
        const float f = windowed(fixed_value(fix, fcode, ((long)qd * lt.Hf + qh) * lt.Wf + qw, fsc), flo, fhi, fden);
        const float v = affine_linear_gather(g, cd, ch, cw, 1.f, 0.f, 0, [&](long x) {
          return (double)windowed(image_value(mov[x], msc), mlo, mhi, mden);
        });
        on = f == f && v == v;  // neither is a NaN
        bin = on ? bin_of(f, fbins, top) * (uint32_t)bins + bin_of(v, fbins, top) : 0u;
      }
    }
    bin_add(hist, bin, on, lane);
  }
  __syncthreads();
  uint32_t* copy = work + (long)(blockIdx.x % COPIES) * nb;
  for (int b = threadIdx.x; b < nb; b += TPB) {
    const uint32_t c = hist[b];
    if (c != 0u) __hip_atomic_fetch_add(copy + b, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

inline bool bins_ok(int bins) { return bins >= 2 && bins <= MAX_BINS; }

}  // namespace

extern "C" {

int pcms_joint_histogram_work_bytes(int bins) { return bins_ok(bins) ? COPIES * bins * bins * 4 : -1; }

int pcms_joint_histogram(const void* fix, int fdatatype, int Df, int Hf, int Wf, double fslope, double finter,
                         const float* flohi, const void* mov, int mdatatype, int Dm, int Hm, int Wm, double mslope,
                         double minter, const float* mlohi, const double* affine12, int sd, int sh, int sw, int bins,
                         unsigned* hist, void* work, hipStream_t s) {
  if (fix == nullptr || mov == nullptr || flohi == nullptr || mlohi == nullptr || affine12 == nullptr ||
      hist == nullptr || work == nullptr)
    return -1;
  if (Df < 1 || Hf < 1 || Wf < 1 || Dm < 1 || Hm < 1 || Wm < 1 || sd < 1 || sh < 1 || sw < 1 || !bins_ok(bins))
    return -1;
  if (misaligned(flohi, alignof(float)) || misaligned(mlohi, alignof(float)) || misaligned(hist, alignof(uint32_t)) ||
      misaligned(work, alignof(uint32_t)))
    return -1;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(affine12[i])) return -1;
  const int Ld = (Df - 1) / sd + 1, Lh = (Hf - 1) / sh + 1, Lw = (Wf - 1) / sw + 1;
  if ((long)Ld * Lh > 0x7fffffffL || (long)Ld * Lh * Lw > 0x7fffffffL) return -1;
  const long total = (long)Ld * Lh * Lw;
  // the fixed element's alignment (the moving one's is checked where its type is known)
  const int fsize = for_datatype(fdatatype, [&](auto t) { return (int)sizeof(t); });
  if (fsize < 0 || misaligned(fix, (size_t)fsize)) return -1;
  const Affine m = make_affine(affine12);  // copied into the kernel arguments
  const Dims g{Dm, Hm, Wm, Ld, Lh, Lw};
  const Lattice lt{Hf, Wf, Lh, Lw, sd, sh, sw};
  const Scale fsc = make_scale(fslope, finter), msc = make_scale(mslope, minter);
  const int nb = bins * bins;
  const int grid = stream_grid(total, JH_PER_WG, JH_MAX_WGS);
  uint32_t* w = static_cast<uint32_t*>(work);
  return for_datatype(mdatatype, [&](auto t) {
    using TM = decltype(t);
    if (misaligned(mov, alignof(TM))) return -1;
    PCMS_LAUNCH(joint_zero_kernel, dim3(cdiv(COPIES * nb, TPB * 8)), dim3(TPB), 0, s, w, COPIES * nb);
    PCMS_LAUNCH(joint_hist_kernel<TM>, dim3(grid), dim3(TPB), 0, s, fix, fdatatype, flohi, (const TM*)mov, mlohi, m, g,
                lt, fsc, msc, bins, w);
    PCMS_LAUNCH(joint_sum_kernel, dim3(cdiv(nb, TPB)), dim3(TPB), 0, s, (const uint32_t*)w, nb, (uint32_t*)hist);
    return 0;
  });
}

}  // extern "C"
