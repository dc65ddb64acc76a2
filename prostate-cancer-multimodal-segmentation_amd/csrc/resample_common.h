// What the resampling kernels of resample.hip (loader, augmentation), deform.hip (elastic
// augmentation), predict.hip (case prediction), patch.hip (patch training), intensity.hip
// (percentile intensity window) and align.hip (joint histogram) share: the per-axis geometry and
// the 8-corner gather of resample.resample, the coordinate, inside rules and gather of resample.resample_affine,
// read_nifti's decoding of a voxel and the dispatch over the NIfTI datatype codes.  Every product and sum must
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

// The 8-corner gather of resample.resample at one output voxel whose taps are all inside:
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

// ---- the gather under a full 3x4 affine (resample.resample_affine; resample.hip and deform.hip) ----
// Output position (d, h, w) samples the source at c_a = ((A[a][0] d + A[a][1] h) + A[a][2] w) + t[a]
// (fp64, every product and sum rounded on its own, in this order); with A = diag(n_in / n_out)
// and t = 0 that is the plain kernels' coordinate.  A coordinate may lie anywhere (or be
// inf / NaN after an overflow), so inside / outside is decided on the doubles and an index is
// formed only from a coordinate known to be inside.
struct Row {
  double x, y, z, t;
};
struct Affine {
  Row d, h, w;
};
struct Dims {
  int Di, Hi, Wi, D, H, W;
};

// affine12 (row-major A[3][3], then t[3]) as the kernel argument
inline Affine make_affine(const double* a) {
  return Affine{Row{a[0], a[1], a[2], a[9]}, Row{a[3], a[4], a[5], a[10]}, Row{a[6], a[7], a[8], a[11]}};
}

__device__ __forceinline__ double affine_coord(const Row& r, double d, double h, double w) {
  return ((r.x * d + r.y * h) + r.z * w) + r.t;
}
// ITK's buffer rule (resample._axis_linear): inside iff -0.5 <= c < n - 0.5; false for NaN
__device__ __forceinline__ bool linear_inside(double c, int n) { return c >= -0.5 && c < (double)n - 0.5; }
// neighbours floor(c), floor(c) + 1 of an inside coordinate, each clamped to [0, n - 1] (c may be
// below 0 here: the lower clamp binds)
__device__ __forceinline__ Tap affine_tap(double c, int n) {
  Tap t;
  const double f = floor(c);
  const long i0 = (int)f;  // -1 <= f <= n - 1
  t.w = c - f;
  t.lo = i0 < 0 ? 0 : i0 > n - 1 ? n - 1 : i0;
  t.hi = i0 + 1 < 0 ? 0 : i0 + 1 > n - 1 ? n - 1 : i0 + 1;
  t.outside = false;
  return t;
}
// nearest index floor(c + 0.5) of one axis; -1: outside [0, n) (also for NaN), the output is 0
__device__ __forceinline__ long affine_nearest(double c, int n) {
  const double k = floor(c + 0.5);
  return (k >= 0.0 && k < (double)n) ? (long)(int)k : -1;
}

// the linear sample at source coordinates (cd, ch, cw): 0 outside, else the 8 corners lerped
// over D, then H, then W, one rounding to fp32, then the intensity step; corner(index) is a
// source voxel as the fp64 value the lerps read
template <typename Corner>
__device__ __forceinline__ float affine_linear_gather(const Dims& g, double cd, double ch, double cw, float gain,
                                                      float bias, int intensity, Corner corner) {
  const long sH = g.Wi, sD = (long)g.Hi * g.Wi;
  float res = 0.f;
  if (linear_inside(cd, g.Di) && linear_inside(ch, g.Hi) && linear_inside(cw, g.Wi)) {
    const Tap td = affine_tap(cd, g.Di), th = affine_tap(ch, g.Hi), tw = affine_tap(cw, g.Wi);
    double vh[2];
#pragma unroll
    for (int jw = 0; jw < 2; ++jw) {
      const long xw = jw ? tw.hi : tw.lo;
      double vd[2];
#pragma unroll
      for (int jh = 0; jh < 2; ++jh) {
        const long xh = (jh ? th.hi : th.lo) * sH + xw;
        vd[jh] = lerp(corner(td.lo * sD + xh), corner(td.hi * sD + xh), td.w);
      }
      vh[jw] = lerp(vd[0], vd[1], th.w);
    }
    res = (float)lerp(vh[0], vh[1], tw.w);
    if (intensity) res = res * gain + bias;  // two fp32 roundings (contraction is off)
  }
  return res;
}
// ... of a raw volume: the corners as ProstateDataset.__getitem__ decodes them
template <typename T>
__device__ __forceinline__ float affine_linear_value(const T* __restrict__ src, const Dims& g, const Scale& sc, double cd,
                                                     double ch, double cw, float gain, float bias, int intensity) {
  return affine_linear_gather(g, cd, ch, cw, gain, bias, intensity,
                              [&](long x) { return (double)image_value(src[x], sc); });
}

// intensity.normalise of one decoded value: den = fl32((double)hi - (double)lo), formed per thread
__device__ __forceinline__ float normalised(float v, float lo, float den) {
  return den == 0.f ? 0.f : (v - lo) / den;
}

// intensity.normalise_window of one decoded value: the clip written with comparisons (a NaN passes
// through), then intensity.normalise's difference and quotient
__device__ __forceinline__ float windowed(float v, float lo, float hi, float den) {
  if (den == 0.f) return 0.f;
  const float c = v < lo ? lo : v > hi ? hi : v;
  return (c - lo) / den;
}

// the label at source coordinates (cd, ch, cw): (float)value > 0 of the nearest voxel, the decoded
// value rounded to fp32 first; 0 outside
template <typename T>
__device__ __forceinline__ float affine_label_value(const T* __restrict__ src, const Dims& g, const Scale& sc, double cd,
                                                    double ch, double cw) {
  const long kd = affine_nearest(cd, g.Di), kh = affine_nearest(ch, g.Hi), kw = affine_nearest(cw, g.Wi);
  float res = 0.f;
  if (kd >= 0 && kh >= 0 && kw >= 0) {
    const T raw = src[(kd * g.Hi + kh) * g.Wi + kw];
    bool fg;
    if (sc.on) {
      fg = (float)scaled(raw, sc) > 0.f;
    } else if constexpr (sizeof(T) == 8 && std::is_floating_point<T>::value) {
      fg = (float)raw > 0.f;
    } else {
      fg = raw > (T)0;  // every other type keeps its sign through the fp32 rounding
    }
    res = fg ? 1.f : 0.f;
  }
  return res;
}

// what every affine entry point checks before a launch (the plain entry points' list, then the
// matrix and the intensity step)
inline bool affine_args_ok(const void* src, const float* out, const double* a, int Di, int Hi, int Wi, int D, int H,
                           int W, float gain, float bias) {
  if (src == nullptr || out == nullptr || a == nullptr) return false;
  if (Di < 1 || Hi < 1 || Wi < 1 || D < 1 || H < 1 || W < 1) return false;
  if (((uintptr_t)out) % alignof(float) != 0) return false;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(a[i])) return false;
  return std::isfinite(gain) && std::isfinite(bias);
}

// f(T{}) for the element type of a NIfTI-1 datatype code (nifti._NIFTI_DTYPES); -1: no such code
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
