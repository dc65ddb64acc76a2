// Elastic deformation in the augmenting resample launch (gfx950): resample.resample_deform per output
// voxel, bit for bit.  A smooth displacement u(d, h, w) -- a uniform cubic B-spline of one fp64
// control grid P[gd][gh][gw][3] per case, evaluated in the output grid's index space -- is added
// to the output index before the affine of resample.hip's augmenting kernels: p'_a = (double)
// index_a + u_a, c_a = ((A[a][0] p'_d + A[a][1] p'_h) + A[a][2] p'_w) + t[a], and from there the
// inside rules, clamps, lerp tree, gain / bias and nearest rule of resample_common.h unchanged.
//
// Per axis (extent N, g control points, ratio = (double)(g - 3) / (double)N formed on the host):
// x = (double)i * ratio, k = floor(x) (0 <= k <= g - 4), s = x - k, r = 1 - s, and
//   b0 = ((r r) r) / 6            b1 = ((3 s3 - 6 s2) + 4) / 6
//   b2 = ((((-3 s3) + 3 s2) + 3 s) + 1) / 6      b3 = s3 / 6          (s2 = s s, s3 = s2 s)
// u_c = sum_jd bd[jd] (sum_jh bh[jh] (sum_jw bw[jw] P[kd + jd][kh + jh][kw + jw][c])), every sum
// left to right from j = 0.  Every product, sum and (IEEE) division rounds on its own, as
// numpy's do: no contraction into FMAs anywhere in this file, no fast-math flags.
//
// The control grid (at most 512 points, 12 KB) is copied into LDS once per workgroup, in the
// [point][3] order it has in global memory: the three components of a point and the four points
// along W of one (jd, jh) row are 96 contiguous bytes behind one address, read as 8-byte words.
// Lanes run along W, so the lanes of a wave share kd, kh (when W >= 64) and hold only a few
// distinct kw, 24 B apart: distinct banks, identical addresses broadcast.  The grid is capped at
// four workgroups per CU's worth of blocks so that the copy is amortised over several voxels per
// thread.
#include "resample_common.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int MAX_POINTS = 512;  // gd * gh * gw: 12 KB of doubles, four workgroups per CU beside it
constexpr int MAX_BLOCKS = 1024;

struct Spline {
  double rd, rh, rw;  // (double)(g - 3) / (double)N per output axis
  int gd, gh, gw;
};

struct Basis {
  double b[4];
  int k;
};
__device__ __forceinline__ Basis spline_basis(int i, double ratio, int g) {
  Basis o;
  const double x = (double)i * ratio;
  const double f = floor(x);
  const int k = (int)f;  // 0 <= f <= g - 4: x <= (N - 1) (g - 3) / N, a whole (g - 3) / N below g - 3
  o.k = k < 0 ? 0 : k > g - 4 ? g - 4 : k;  // never binds; keeps the LDS index in range whatever x is
  const double s = x - f;
  const double r = 1.0 - s, s2 = s * s, s3 = s2 * s;
  o.b[0] = ((r * r) * r) / 6.0;
  o.b[1] = ((3.0 * s3 - 6.0 * s2) + 4.0) / 6.0;
  o.b[2] = ((((-3.0 * s3) + 3.0 * s2) + 3.0 * s) + 1.0) / 6.0;
  o.b[3] = s3 / 6.0;
  return o;
}

// the workgroup's copy of the control grid: every thread calls this once, before its first voxel
__device__ __forceinline__ void load_control(double* ctrl, const double* __restrict__ field, const Spline& sp) {
  const int n = sp.gd * sp.gh * sp.gw * 3;  // <= 3 * MAX_POINTS (checked on the host)
  for (int i = threadIdx.x; i < n; i += TPB) ctrl[i] = field[i];
  __syncthreads();
}

// p'_a = (double)index_a + u_a at output voxel (d, h, w)
__device__ __forceinline__ void deformed_index(const double* ctrl, const Spline& sp, int d, int h, int w, double& pd,
                                               double& ph, double& pw) {
  const Basis bd = spline_basis(d, sp.rd, sp.gd), bh = spline_basis(h, sp.rh, sp.gh), bw = spline_basis(w, sp.rw, sp.gw);
  const int rowh = sp.gw * 3, rowd = sp.gh * rowh;
  const double* base = ctrl + (bd.k * rowd + bh.k * rowh + bw.k * 3);
  double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int jd = 0; jd < 4; ++jd) {
    double uh[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int jh = 0; jh < 4; ++jh) {
      const double* p = base + (jd * rowd + jh * rowh);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double sw = ((bw.b[0] * p[c] + bw.b[1] * p[3 + c]) + bw.b[2] * p[6 + c]) + bw.b[3] * p[9 + c];
        const double t = bh.b[jh] * sw;
        uh[c] = jh == 0 ? t : uh[c] + t;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = bd.b[jd] * uh[c];
      u[c] = jd == 0 ? t : u[c] + t;
    }
  }
  pd = (double)d + u[0];
  ph = (double)h + u[1];
  pw = (double)w + u[2];
}

template <typename T>
__global__ void __launch_bounds__(TPB) resample_deform_linear_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                                     const double* __restrict__ field, Spline sp,
                                                                     Affine m, Dims g, Scale sc, float gain, float bias,
                                                                     int intensity) {
  __shared__ double ctrl[MAX_POINTS * 3];
  load_control(ctrl, field, sp);
  const long HW = (long)g.H * g.W;
  const long total = (long)g.D * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / g.W), w = (int)(r - (long)h * g.W);
    double pd, ph, pw;
    deformed_index(ctrl, sp, d, h, w, pd, ph, pw);
    const double cd = affine_coord(m.d, pd, ph, pw), ch = affine_coord(m.h, pd, ph, pw),
                 cw = affine_coord(m.w, pd, ph, pw);
    out[i] = affine_linear_value(src, g, sc, cd, ch, cw, gain, bias, intensity);
  }
}

template <typename T>
__global__ void __launch_bounds__(TPB) resample_deform_label_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                                    const double* __restrict__ field, Spline sp,
                                                                    Affine m, Dims g, Scale sc) {
  __shared__ double ctrl[MAX_POINTS * 3];
  load_control(ctrl, field, sp);
  const long HW = (long)g.H * g.W;
  const long total = (long)g.D * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / g.W), w = (int)(r - (long)h * g.W);
    double pd, ph, pw;
    deformed_index(ctrl, sp, d, h, w, pd, ph, pw);
    out[i] = affine_label_value(src, g, sc, affine_coord(m.d, pd, ph, pw), affine_coord(m.h, pd, ph, pw),
                                affine_coord(m.w, pd, ph, pw));
  }
}

template <typename T>
int launch_deform(bool label, const void* src, float* out, const double* field, const Spline& sp, const Affine& m,
                  const Dims& g, const Scale& sc, float gain, float bias, hipStream_t s) {
  if (((uintptr_t)src) % alignof(T) != 0) return -1;
  const long total = (long)g.D * g.H * g.W;
  const int grid = grid_for(total, TPB, MAX_BLOCKS);
  if (label)
    hipLaunchKernelGGL(resample_deform_label_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, field, sp, m, g,
                       sc);
  else
    hipLaunchKernelGGL(resample_deform_linear_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, field, sp, m,
                       g, sc, gain, bias, (gain == 1.f && bias == 0.f) ? 0 : 1);
  PCMS_CHECK_LAUNCH();
}

int resample_deform(bool label, const void* src, int code, int Di, int Hi, int Wi, double slope, double inter,
                    const double* a, const double* field, int gd, int gh, int gw, float gain, float bias, float* out,
                    int D, int H, int W, hipStream_t s) {
  if (!affine_args_ok(src, out, a, Di, Hi, Wi, D, H, W, gain, bias)) return -1;
  if (field == nullptr || ((uintptr_t)field) % alignof(double) != 0) return -1;
  if (gd < 4 || gh < 4 || gw < 4 || gd > MAX_POINTS || gh > MAX_POINTS || gw > MAX_POINTS) return -1;
  if ((long)gd * gh * gw > MAX_POINTS) return -1;
  const Spline sp{(double)(gd - 3) / (double)D, (double)(gh - 3) / (double)H, (double)(gw - 3) / (double)W, gd, gh, gw};
  const Affine m = make_affine(a);  // copied into the kernel arguments
  const Dims g{Di, Hi, Wi, D, H, W};
  const Scale sc = make_scale(slope, inter);
  return for_datatype(code, [&](auto t) {
    return launch_deform<decltype(t)>(label, src, out, field, sp, m, g, sc, gain, bias, s);
  });
}

}  // namespace

extern "C" {

int pcms_resample_deform_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                double scl_inter, const double* affine12, const double* field, int gd, int gh, int gw,
                                float gain, float bias, float* out, int D, int H, int W, hipStream_t s) {
  return resample_deform(false, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, affine12, field, gd, gh, gw, gain, bias,
                         out, D, H, W, s);
}

int pcms_resample_deform_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                               const double* affine12, const double* field, int gd, int gh, int gw, float* out, int D,
                               int H, int W, hipStream_t s) {
  return resample_deform(true, src, datatype, Di, Hi, Wi, scl_slope, scl_inter, affine12, field, gd, gh, gw, 1.f, 0.f,
                         out, D, H, W, s);
}

}  // extern "C"
