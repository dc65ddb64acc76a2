// What the resampling kernels of resample.hip (loader, augmentation) and predict.hip (case
// prediction) share: the per-axis geometry and the 8-corner gather of data.resample, read_nifti's
// decoding of a voxel and the dispatch over the NIfTI datatype codes.  Every product and sum must
// round on its own, as numpy's do: no contraction into FMAs from here to the end of the
// including file.
#pragma once
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace {

// One axis of the output grid, formed on the host: ratio = (double)n_in / (double)n_out (numpy's
// n_in / n_out), edge = n_in - 0.5 (zero from there on), ident: n_in == n_out (the pass is skipped)
struct Axis {
  double ratio, edge;
  int n_in, n_out, ident;
};
struct Scale {
  double slope, inter;
  int on;  // read_nifti: slope not in (0, 1) or inter != 0, with slope 0 meaning 1
};

inline Axis make_axis(int n_in, int n_out) {
  return Axis{(double)n_in / (double)n_out, (double)n_in - 0.5, n_in, n_out, n_in == n_out ? 1 : 0};
}
inline Scale make_scale(double slope, double inter) {
  const int on = (!(slope == 0.0 || slope == 1.0) || inter != 0.0) ? 1 : 0;
  return Scale{slope == 0.0 ? 1.0 : slope, inter, on};
}

// a voxel as read_nifti hands it on: fp64 raw * slope + inter when scaling applies (product
// and sum rounded separately), else the raw value itself
template <typename T> __device__ __forceinline__ double scaled(T raw, const Scale& sc) {
  return (double)raw * sc.slope + sc.inter;
}
// the image sample ProstateDataset.__getitem__ resamples: that value as fp32
template <typename T> __device__ __forceinline__ float image_value(T raw, const Scale& sc) {
  return sc.on ? (float)scaled(raw, sc) : (float)raw;
}

struct Tap {
  long lo, hi;  // clamped neighbours
  double w;
  bool outside;
};
__device__ __forceinline__ Tap linear_tap(const Axis& a, int i) {
  Tap t;
  if (a.ident) {
    t.lo = t.hi = i;
    t.w = 0.0;
    t.outside = false;
    return t;
  }
  const double c = (double)i * a.ratio;
  const double f = floor(c);
  const long i0 = (int)f;  // c < n_in <= INT_MAX
  t.w = c - f;
  t.lo = i0 < a.n_in - 1 ? i0 : a.n_in - 1;  // c >= 0: no lower clamp can bind
  t.hi = i0 + 1 < a.n_in - 1 ? i0 + 1 : a.n_in - 1;
  t.outside = !(c < a.edge);
  return t;
}
__device__ __forceinline__ double lerp(double a, double b, double w) { return a * (1.0 - w) + b * w; }

// The 8-corner gather of data.resample at one output voxel whose taps are all inside:
// corner(index) is a source voxel as the fp64 value the host's first pass reads; the lerps run
// over D, then H, then W, an identity axis copied, one rounding to fp32
template <typename Corner>
__device__ __forceinline__ float gather_linear(const Axis& ad, const Axis& ah, const Axis& aw, const Tap& td,
                                               const Tap& th, const Tap& tw, Corner corner) {
  const long sH = aw.n_in, sD = (long)ah.n_in * aw.n_in;
  double vh[2];
#pragma unroll
  for (int jw = 0; jw < 2; ++jw) {
    const long xw = jw ? tw.hi : tw.lo;
    double vd[2];
#pragma unroll
    for (int jh = 0; jh < 2; ++jh) {
      const long xh = (jh ? th.hi : th.lo) * sH + xw;
      const double a = corner(td.lo * sD + xh);
      vd[jh] = ad.ident ? a : lerp(a, corner(td.hi * sD + xh), td.w);
    }
    vh[jw] = ah.ident ? vd[0] : lerp(vd[0], vd[1], th.w);
  }
  return (float)(aw.ident ? vh[0] : lerp(vh[0], vh[1], tw.w));
}

// f(T{}) for the element type of a NIfTI-1 datatype code (data._NIFTI_DTYPES); -1: no such code
template <typename F> int for_datatype(int code, F&& f) {
  switch (code) {
    case 2: return f(uint8_t{});
    case 4: return f(int16_t{});
    case 8: return f(int32_t{});
    case 16: return f(float{});
    case 64: return f(double{});
    case 256: return f(int8_t{});
    case 512: return f(uint16_t{});
    case 768: return f(uint32_t{});
    case 1024: return f(int64_t{});
    case 1280: return f(uint64_t{});
    default: return -1;
  }
}

}  // namespace
