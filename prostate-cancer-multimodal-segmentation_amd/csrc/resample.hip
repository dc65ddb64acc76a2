// Device-side resampling of one NIfTI volume to the training grid (gfx950): the loader's
// resample.resample (the reference's ResampleImageFilter geometry, script/data_loader.py:258-281
// linear for images, :383-406 nearest for labels) evaluated per output voxel, bit for bit.
//
// The source is the file's voxel bytes in their native type (NIfTI datatype code, little
// endian, (Di, Hi, Wi) with W fastest); the header's scl_slope / scl_inter are applied on the
// fly by read_nifti's rule.  Output index i of an axis samples the continuous input index
// c = (double)i * (n_in / n_out), the fp64 expression numpy forms (exact rational indices
// disagree with it for many size pairs).  resample.resample runs three separable fp64 passes
// (D, then H, then W); an 8-corner gather lerped in that order gives every intermediate the
// same two operands and so the same roundings.  Every product and sum below must round on its
// own, as numpy's do: no contraction into FMAs anywhere in this file.
#include "resample_common.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;

template <typename T>
__global__ void __launch_bounds__(TPB) resample_linear_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                              Axis ad, Axis ah, Axis aw, Scale sc) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const Tap td = linear_tap(ad, d), th = linear_tap(ah, h), tw = linear_tap(aw, w);
    float res = 0.f;
    if (!(td.outside || th.outside || tw.outside))
      res = gather_linear(ad, ah, aw, td, th, tw, [&](long x) { return (double)image_value(src[x], sc); });
    out[i] = res;
  }
}

// nearest index of one axis (rounded half up); -1: past the input (the output is 0 there)
__device__ __forceinline__ long nearest_index(const Axis& a, int i) {
  if (a.ident) return i;
  const long k = (int)floor((double)i * a.ratio + 0.5);  // <= n_in <= INT_MAX
  return k < a.n_in ? k : -1;
}

// round32: resample.resample's result is fp32 before the loader's `> 0`; a volume already of the
// target shape is not resampled and is compared as read (ProstateDataset.__getitem__)
template <typename T>
__global__ void __launch_bounds__(TPB) resample_label_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                             Axis ad, Axis ah, Axis aw, Scale sc, int round32) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const long kd = nearest_index(ad, d), kh = nearest_index(ah, h), kw = nearest_index(aw, w);
    float res = 0.f;
    if (kd >= 0 && kh >= 0 && kw >= 0) {
      const T raw = src[(kd * ah.n_in + kh) * aw.n_in + kw];
      bool fg;
      if (sc.on) {
        const double v = scaled(raw, sc);
        fg = round32 ? (float)v > 0.f : v > 0.0;
      } else if constexpr (sizeof(T) == 8 && std::is_floating_point<T>::value) {
        fg = round32 ? (float)raw > 0.f : raw > 0.0;
      } else {
        fg = raw > (T)0;  // every other type keeps its sign through the fp32 rounding
      }
      res = fg ? 1.f : 0.f;
    }
    out[i] = res;
  }
}

template <typename T>
int launch(bool label, const void* src, float* out, const Axis& ad, const Axis& ah, const Axis& aw, const Scale& sc,
           hipStream_t s) {
  if (((uintptr_t)src) % alignof(T) != 0) return -1;
  const long total = (long)ad.n_out * ah.n_out * aw.n_out;
  const int grid = grid_for(total, TPB);
  if (label)
    hipLaunchKernelGGL(resample_label_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, ad, ah, aw, sc,
                       (ad.ident && ah.ident && aw.ident) ? 0 : 1);
  else
    hipLaunchKernelGGL(resample_linear_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, ad, ah, aw, sc);
  PCMS_CHECK_LAUNCH();
}

int resample(bool label, const void* src, int code, int Di, int Hi, int Wi, double slope, double inter, float* out,
             int D, int H, int W, hipStream_t s) {
  if (src == nullptr || out == nullptr) return -1;
  if (Di < 1 || Hi < 1 || Wi < 1 || D < 1 || H < 1 || W < 1) return -1;
  if (((uintptr_t)out) % alignof(float) != 0) return -1;
  const Axis ad = make_axis(Di, D), ah = make_axis(Hi, H), aw = make_axis(Wi, W);
  const Scale sc = make_scale(slope, inter);
  return for_datatype(code, [&](auto t) { return launch<decltype(t)>(label, src, out, ad, ah, aw, sc, s); });
}

// ---- training-time augmentation: the same gather under a full 3x4 affine (resample.resample_affine) ----
// The coordinate, the inside rules and the gather are resample_common.h's (deform.hip shares them).
template <typename T>
__global__ void __launch_bounds__(TPB) resample_affine_linear_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                                     Affine m, Dims g, Scale sc, float gain, float bias,
                                                                     int intensity) {
  const long HW = (long)g.H * g.W;
  const long total = (long)g.D * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / g.W), w = (int)(r - (long)h * g.W);
    const double fd = (double)d, fh = (double)h, fw = (double)w;
    const double cd = affine_coord(m.d, fd, fh, fw), ch = affine_coord(m.h, fd, fh, fw),
                 cw = affine_coord(m.w, fd, fh, fw);
    out[i] = affine_linear_value(src, g, sc, cd, ch, cw, gain, bias, intensity);
  }
}

// the label: (float)value > 0 of the nearest voxel, the decoded value rounded to fp32 first
template <typename T>
__global__ void __launch_bounds__(TPB) resample_affine_label_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                                    Affine m, Dims g, Scale sc) {
  const long HW = (long)g.H * g.W;
  const long total = (long)g.D * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / g.W), w = (int)(r - (long)h * g.W);
    const double fd = (double)d, fh = (double)h, fw = (double)w;
    out[i] = affine_label_value(src, g, sc, affine_coord(m.d, fd, fh, fw), affine_coord(m.h, fd, fh, fw),
                                affine_coord(m.w, fd, fh, fw));
  }
}

template <typename T>
int launch_affine(bool label, const void* src, float* out, const Affine& m, const Dims& g, const Scale& sc, float gain,
                  float bias, hipStream_t s) {
  if (((uintptr_t)src) % alignof(T) != 0) return -1;
  const long total = (long)g.D * g.H * g.W;
  const int grid = grid_for(total, TPB);
  if (label)
    hipLaunchKernelGGL(resample_affine_label_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, m, g, sc);
  else
    hipLaunchKernelGGL(resample_affine_linear_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, m, g, sc,
                       gain, bias, (gain == 1.f && bias == 0.f) ? 0 : 1);
  PCMS_CHECK_LAUNCH();
}

int resample_affine(bool label, const void* src, int code, int Di, int Hi, int Wi, double slope, double inter,
                    const double* a, float gain, float bias, float* out, int D, int H, int W, hipStream_t s) {
  if (!affine_args_ok(src, out, a, Di, Hi, Wi, D, H, W, gain, bias)) return -1;
  const Affine m = make_affine(a);  // copied into the kernel arguments
  const Dims g{Di, Hi, Wi, D, H, W};
  const Scale sc = make_scale(slope, inter);
  return for_datatype(
      code, [&](auto t) { return launch_affine<decltype(t)>(label, src, out, m, g, sc, gain, bias, s); });
}

}  // namespace

extern "C" {

int pcms_resample_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                         float* out, int D, int H, int W, hipStream_t s) {
  return resample(false, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, out, D, H, W, s);
}

int pcms_resample_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                        float* out, int D, int H, int W, hipStream_t s) {
  return resample(true, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, out, D, H, W, s);
}

int pcms_resample_affine_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                double scl_inter, const double* affine12, float gain, float bias, float* out, int D, int H,
                                int W, hipStream_t s) {
  return resample_affine(false, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, affine12, gain, bias, out, D, H, W, s);
}

int pcms_resample_affine_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                               const double* affine12, float* out, int D, int H, int W, hipStream_t s) {
  return resample_affine(true, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, affine12, 1.f, 0.f, out, D, H, W, s);
}

}  // extern "C"
