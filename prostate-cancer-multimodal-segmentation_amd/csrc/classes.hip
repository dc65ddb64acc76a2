// Mutually exclusive classes (gfx950): the softmax cross-entropy + Dice loss on class
// maps, class-map labels from raw NIfTI bytes, softmax planes and their argmax on the native grid,
// and per-class overlap counts.  classes.py holds the host forms.
//
//   pcms_softmax_loss_rows / _fwd / _bwd   SoftmaxDiceCELoss on (N, C, nvox) fp32 logits and an
//                                          (N, nvox) class map (fp32 or uint8), 2 <= C <= 8
//   pcms_resample_classes                  pcms_resample_label's nearest gather, a value table
//   pcms_resample_affine_classes           instead of `> 0`: class_values[j] -> j + 1, else 0
//   pcms_softmax_planes                    (B, C, n) logits -> class-major (C, B, n) probabilities
//   pcms_probs_to_labels                   pcms_prob_to_mask's gather per class plane, first maximum
//   pcms_class_overlap                     (|pred == c|, |ref == c|, |both|) per class, int64
//
// The loss, per voxel p = softmax_c(x) (the maximum subtracted, the sum in class order), y the
// one-hot label; a voxel whose label is not an integer in [0, C) enters no sum and gets no
// gradient.  A group g is the batch or one sample:
//   I_c = sum p_c y_c, P_c = sum p_c, T_c = sum y_c over the group's valid voxels
//   dice_c = (2 I_c + s) / (P_c + T_c + s)  (1 where the denominator is not positive)
//   region_g = mean_{c in K} (1 - dice_c),  K = {1..C-1}, or {0..C-1} with include_background
//   CE = sum_i w[y_i] (-log p_{y_i}) / sum_i w[y_i] over the batch's valid voxels (0 without one)
//   loss = ce_weight CE + dice_weight mean_g region_g
// Forward: softmax_partial_kernel<C> (grid = rows x N: one fp32 row of 3C + 2 sums per block --
// I, P, T per class, then the CE numerator and sum w) and softmax_finalize_kernel (one block: a
// group's rows summed in fp64 in a fixed order, the loss, and per group the 2C coefficients of
// dL/dp_c = A_c y_c + B_c, after them one float ce_weight / sum w).  Backward: softmax_bwd_kernel<C>,
//   dx_k = gout [ p_k (g_k - sum_j p_j g_j) + (ce_weight / sum w) w[y] (p_k - y_k) ],  g_c = A_c y_c + B_c.
// Every sum has a fixed order: the same bits on every run.  x - max <= 0, so no exponential
// overflows and the sum is at least 1: finite results for any finite logits.
//
// The gathers restate numpy expressions in which every product and sum rounds on its own
// (resample_common.h switches contraction off for the whole file).
#include "ops_units.h"
#include "resample_common.h"
#include "wave_hist.h"

#include "pcms_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_CLASSES = 8;

// ---- the loss -------------------------------------------------------------------------------
struct ClassWeights {
  float w[MAX_CLASSES];
};

// the class of a label, -1 for a voxel to ignore (not an integer in [0, C); NaN too)
template <int C> __device__ __forceinline__ int class_of_label(float t) {
  if (!(t >= 0.f && t < (float)C)) return -1;
  const int y = (int)t;
  return (float)y == t ? y : -1;
}
template <int C> __device__ __forceinline__ int class_of_label(uint8_t t) { return t < C ? (int)t : -1; }

// p = softmax(x) in place; returns -log p_y (y >= 0)
template <int C> __device__ __forceinline__ float softmax_nll(float (&x)[C], int y) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f, xy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float d = x[c] - m;
    xy = c == y ? d : xy;
    x[c] = expf(d);
    s += x[c];
  }
  const float r = 1.f / s;
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] *= r;
  return logf(s) - xy;
}

template <int C> struct Sums {
  float I[C], P[C], T[C], ce, sw;
};

template <int C, typename L>
__device__ __forceinline__ void add_voxel(Sums<C>& a, float (&x)[C], L t, const ClassWeights& cw) {
  const int y = class_of_label<C>(t);
  if (y < 0) return;
  const float nll = softmax_nll<C>(x, y);
  float wy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool on = c == y;
    a.I[c] += on ? x[c] : 0.f;
    a.P[c] += x[c];
    a.T[c] += on ? 1.f : 0.f;
    wy = on ? cw.w[c] : wy;
  }
  a.ce += wy * nll;
  a.sw += wy;
}

// four labels as one access (fp32: 16 bytes, uint8: 4 bytes)
__device__ __forceinline__ void load_labels4(const float* t, float* out) { load16<float>(t, out); }
__device__ __forceinline__ void load_labels4(const uint8_t* t, uint8_t* out) {
  const uint32_t v = *reinterpret_cast<const uint32_t*>(t);
#pragma unroll
  for (int u = 0; u < 4; ++u) out[u] = (uint8_t)(v >> (8 * u));
}

// a sample's C logit planes and its labels all allow the four-voxel accesses
template <typename L> __device__ __forceinline__ bool planes_vec_ok(const float* xs, long nvox, const L* ts) {
  return (((uintptr_t)xs) & 15) == 0 && (nvox & 3) == 0 && (((uintptr_t)ts) & (4 * sizeof(L) - 1)) == 0;
}

template <int C, typename L>
__device__ __forceinline__ void partial_sums(Sums<C>& a, const float* xs, const L* ts, unsigned n,
                                             const ClassWeights& cw) {
  const unsigned stride = gridDim.x * blockDim.x;
  unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (planes_vec_ok(xs, n, ts)) {
    // (nvox is a multiple of 4 here: no remainder)
    for (const unsigned n4 = n / 4; i < n4; i += stride) {
      float xv[C][4];
      L tv[4];
#pragma unroll
      for (int c = 0; c < C; ++c) load16<float>(xs + (size_t)c * n + 4 * (size_t)i, xv[c]);
      load_labels4(ts + 4 * (size_t)i, tv);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = xv[c][u];
        add_voxel<C>(a, x, tv[u], cw);
      }
    }
  } else {
    for (; i < n; i += stride) {
      float x[C];
#pragma unroll
      for (int c = 0; c < C; ++c) x[c] = xs[(size_t)c * n + i];
      add_voxel<C>(a, x, ts[i], cw);
    }
  }
}

// part[(sample * rows + block)][3C + 2]; grid = (rows, N)
template <int C>
__global__ void __launch_bounds__(TPB) softmax_partial_kernel(const float* x, const void* t, int t_u8, long nvox,
                                                              ClassWeights cw, float* part) {
  constexpr int K = 3 * C + 2;
  __shared__ float red[K][TPB / 64];
  const float* xs = x + (long)blockIdx.y * C * nvox;
  Sums<C> a{};
  // (nvox < 2^31 and the grid is at most 2^18 threads wide: every index fits 32 bits)
  if (t_u8)
    partial_sums<C>(a, xs, (const uint8_t*)t + (long)blockIdx.y * nvox, (unsigned)nvox, cw);
  else
    partial_sums<C>(a, xs, (const float*)t + (long)blockIdx.y * nvox, (unsigned)nvox, cw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float vi = wave_sum(a.I[c]), vp = wave_sum(a.P[c]), vt = wave_sum(a.T[c]);
    if (lane == 0) { red[c][wave] = vi; red[C + c][wave] = vp; red[2 * C + c][wave] = vt; }
  }
  const float vce = wave_sum(a.ce), vsw = wave_sum(a.sw);
  if (lane == 0) { red[3 * C][wave] = vce; red[3 * C + 1][wave] = vsw; }
  __syncthreads();
  if (threadIdx.x < K) {
    float r = 0.f;
    for (int w = 0; w < TPB / 64; ++w) r += red[threadIdx.x][w];
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * K + threadIdx.x] = r;
  }
}

struct SoftCfg {
  float smooth, ce_weight, dice_weight;
  int C, include_background, per_sample;
};

// One block of 256 threads.  Wave k sums columns k, k + 4, ... of each group's rows (lane l: rows
// l, l + 64, ... in fp64, the 64 lane sums by a fixed xor tree) into sums[g][3C + 2]; then thread
// j takes groups j, j + 256, ...: region_g and the backward's coefficients, all fp64, rounded once,
//   kk = dice_weight / (groups |K|),  Den = P_c + T_c + s
//   coef[g][c] = A_c = -2 kk / Den,  coef[g][C + c] = B_c = kk (2 I_c + s) / Den^2   (0 outside K, or Den <= 0);
// thread 0 adds the threads' region sums in thread order and the groups' CE sums in group order,
// writes the loss and coef[groups 2C] = ce_weight / sum w (0 without a valid voxel).
__global__ void __launch_bounds__(256) softmax_finalize_kernel(const float* part, int rows, int N, SoftCfg c,
                                                               double* sums, float* coef, float* loss) {
  __shared__ double red[256];
  const int C = c.C, K = 3 * C + 2;
  const int groups = c.per_sample ? N : 1;
  const long rpg = c.per_sample ? rows : (long)N * rows;
  const int l = threadIdx.x & 63;
  for (int g = 0; g < groups; ++g) {
    const float* pg = part + (long)g * rpg * K;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
      // eight rows' loads in flight per trip (one load -> add chain per row was latency-bound), added in row order
      double s = 0.0;
      long r = l;
      for (; r + 7 * 64 < rpg; r += 8 * 64) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = pg[(r + u * 64) * K + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
      }
      for (; r < rpg; r += 64) s += (double)pg[r * K + k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (l == 0) sums[g * K + k] = s;
    }
  }
  __syncthreads();
  const int c0 = c.include_background ? 0 : 1;
  const double kk = (double)c.dice_weight / ((double)groups * (double)(C - c0)), sm = c.smooth;
  double racc = 0.0;
  for (int g = threadIdx.x; g < groups; g += 256) {
    const double* sv = sums + g * K;
    double region = 0.0;
    for (int k = 0; k < C; ++k) {
      const double I = sv[k], den = sv[C + k] + sv[2 * C + k] + sm;
      const bool on = k >= c0 && den > 0.0;
      coef[g * 2 * C + k] = on ? (float)(-2.0 * kk / den) : 0.f;
      coef[g * 2 * C + C + k] = on ? (float)(kk * (2.0 * I + sm) / (den * den)) : 0.f;
      if (on) region += 1.0 - (2.0 * I + sm) / den;
    }
    racc += region / (double)(C - c0);
  }
  red[threadIdx.x] = racc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0, ce = 0.0, sw = 0.0;
    const int n = groups < 256 ? groups : 256;
    for (int i = 0; i < n; ++i) r += red[i];
    for (int g = 0; g < groups; ++g) { ce += sums[g * K + 3 * C]; sw += sums[g * K + 3 * C + 1]; }
    const bool any = sw > 0.0;
    loss[0] = (float)((double)c.ce_weight * (any ? ce / sw : 0.0) + (double)c.dice_weight * (r / (double)groups));
    coef[groups * 2 * C] = any ? (float)((double)c.ce_weight / sw) : 0.f;
  }
}

template <int C> struct BwdCoef {
  float A[C], B[C], ce, g;
};

template <int C, typename L>
__device__ __forceinline__ void dx_voxel(float (&x)[C], L t, const BwdCoef<C>& b, const ClassWeights& cw) {
  const int y = class_of_label<C>(t);
  if (y < 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.f;
    return;
  }
  softmax_nll<C>(x, y);
  float g[C], dot = 0.f, wy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool on = c == y;
    g[c] = on ? b.A[c] + b.B[c] : b.B[c];
    dot += x[c] * g[c];
    wy = on ? cw.w[c] : wy;
  }
  const float k = b.ce * wy;
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] = b.g * (x[c] * (g[c] - dot) + k * (x[c] - (c == y ? 1.f : 0.f)));
}

template <int C, typename L>
__device__ __forceinline__ void bwd_planes(const float* xs, const L* ts, float* ds, long nvox, const BwdCoef<C>& b,
                                           const ClassWeights& cw) {
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (planes_vec_ok(xs, nvox, ts) && (((uintptr_t)ds) & 15) == 0) {
    for (const long n4 = nvox / 4; i < n4; i += stride) {
      float xv[C][4];
      L tv[4];
#pragma unroll
      for (int c = 0; c < C; ++c) load16<float>(xs + c * nvox + 4 * i, xv[c]);
      load_labels4(ts + 4 * i, tv);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = xv[c][u];
        dx_voxel<C>(x, tv[u], b, cw);
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c][u] = x[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) store16<float>(ds + c * nvox + 4 * i, xv[c]);
    }
  } else {
    for (; i < nvox; i += stride) {
      float x[C];
#pragma unroll
      for (int c = 0; c < C; ++c) x[c] = xs[c * nvox + i];
      dx_voxel<C>(x, ts[i], b, cw);
#pragma unroll
      for (int c = 0; c < C; ++c) ds[c * nvox + i] = x[c];
    }
  }
}

// grid = (blocks per sample, N); a group's coefficients are read once per block
template <int C>
__global__ void __launch_bounds__(TPB) softmax_bwd_kernel(const float* x, const void* t, int t_u8, long nvox,
                                                          int per_sample, int groups, ClassWeights cw,
                                                          const float* coef, const float* gout, float* dx) {
  const float* cg = coef + (per_sample ? (long)blockIdx.y * 2 * C : 0);
  BwdCoef<C> b;
#pragma unroll
  for (int c = 0; c < C; ++c) { b.A[c] = cg[c]; b.B[c] = cg[C + c]; }
  b.ce = coef[(long)groups * 2 * C];
  b.g = gout ? gout[0] : 1.f;
  const float* xs = x + (long)blockIdx.y * C * nvox;
  float* ds = dx + (long)blockIdx.y * C * nvox;
  if (t_u8)
    bwd_planes<C>(xs, (const uint8_t*)t + (long)blockIdx.y * nvox, ds, nvox, b, cw);
  else
    bwd_planes<C>(xs, (const float*)t + (long)blockIdx.y * nvox, ds, nvox, b, cw);
}

// f(std::integral_constant<int, C>{}) for 2 <= C <= MAX_CLASSES; -1 otherwise
template <typename F> int for_classes(int C, F&& f) {
  switch (C) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return -1;
  }
}

// the checks both loss entry points share; the class weights (ones without a table) on success
int loss_args(const float* x, const void* t, int t_u8, long nvox, int N, int C, const float* class_weights,
              ClassWeights* cw) {
  if (x == nullptr || t == nullptr) return -1;
  if (misaligned(x, alignof(float)) || (!t_u8 && misaligned(t, alignof(float)))) return -1;
  if (C < 2 || C > MAX_CLASSES || N < 1 || N > 65535 || nvox < 1 || nvox >= (1L << 31)) return -1;
  for (int c = 0; c < MAX_CLASSES; ++c) {
    const float w = (class_weights != nullptr && c < C) ? class_weights[c] : 1.f;
    if (!(w >= 0.f) || !std::isfinite(w)) return -1;
    cw->w[c] = w;
  }
  return 0;
}

// ---- class-map labels ---------------------------------------------------------------------------
constexpr int MAX_CLASS_VALUES = MAX_CLASSES - 1;
struct ClassTable {
  int n;
  float v[MAX_CLASS_VALUES];
};

// classes.classes_of of one decoded fp32 value: j + 1 for the first j with v == class_values[j], else 0
__device__ __forceinline__ float class_of_value(float v, const ClassTable& t) {
  float r = 0.f;
#pragma unroll
  for (int j = MAX_CLASS_VALUES - 1; j >= 0; --j) r = (j < t.n && v == t.v[j]) ? (float)(j + 1) : r;
  return r;
}

// resample.resample(nearest=True)'s index of one axis (rounded half up); -1: past the input
__device__ __forceinline__ long nearest_axis(const Axis& a, int i) {
  if (a.ident) return i;
  const long k = (int)floor((double)i * a.ratio + 0.5);  // <= n_in <= INT_MAX
  return k < a.n_in ? k : -1;
}

template <typename T>
__global__ void __launch_bounds__(TPB) resample_classes_kernel(const T* __restrict__ src, float* __restrict__ out,
                                                               Axis ad, Axis ah, Axis aw, Scale sc, ClassTable tab) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const long kd = nearest_axis(ad, d), kh = nearest_axis(ah, h), kw = nearest_axis(aw, w);
    float res = 0.f;
    if (kd >= 0 && kh >= 0 && kw >= 0)
      res = class_of_value(image_value(src[(kd * ah.n_in + kh) * aw.n_in + kw], sc), tab);
    out[i] = res;
  }
}

template <typename T>
__global__ void __launch_bounds__(TPB) resample_affine_classes_kernel(const T* __restrict__ src,
                                                                      float* __restrict__ out, Affine m, Dims g,
                                                                      Scale sc, ClassTable tab) {
  const long HW = (long)g.H * g.W;
  const long total = (long)g.D * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / g.W), w = (int)(r - (long)h * g.W);
    const double fd = (double)d, fh = (double)h, fw = (double)w;
    const long kd = affine_nearest(affine_coord(m.d, fd, fh, fw), g.Di),
               kh = affine_nearest(affine_coord(m.h, fd, fh, fw), g.Hi),
               kw = affine_nearest(affine_coord(m.w, fd, fh, fw), g.Wi);
    float res = 0.f;
    if (kd >= 0 && kh >= 0 && kw >= 0) res = class_of_value(image_value(src[(kd * g.Hi + kh) * g.Wi + kw], sc), tab);
    out[i] = res;
  }
}

// the table of an entry point: 1 <= n <= 7 finite host floats
int make_table(const float* class_values, int n, ClassTable* tab) {
  if (class_values == nullptr || n < 1 || n > MAX_CLASS_VALUES) return -1;
  tab->n = n;
  for (int j = 0; j < MAX_CLASS_VALUES; ++j) {
    tab->v[j] = j < n ? class_values[j] : 0.f;
    if (!std::isfinite(tab->v[j])) return -1;
  }
  return 0;
}

// ---- softmax planes and their argmax on the native grid -------------------------------------------
// out[(c * B + b) * n + i] = softmax_c(x[(b * C + c) * n + i]): m = max_c x_c, e_c = expf(x_c - m),
// s summed in class order, p_c = e_c / s
template <int C> __device__ __forceinline__ void softmax_div(float (&x)[C]) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    x[c] = expf(x[c] - m);
    s += x[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] = x[c] / s;
}

template <int C>
__global__ void __launch_bounds__(TPB) softmax_planes_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                             int B, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if ((n & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0) {
    const long n4 = n / 4;
    for (const long total = (long)B * n4; i < total; i += stride) {
      const long b = i / n4, v = 4 * (i - b * n4);
      float xv[C][4];
#pragma unroll
      for (int c = 0; c < C; ++c) load16<float>(x + (b * C + c) * n + v, xv[c]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float p[C];
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = xv[c][u];
        softmax_div<C>(p);
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c][u] = p[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) store16<float>(out + ((long)c * B + b) * n + v, xv[c]);
    }
  } else {
    for (const long total = (long)B * n; i < total; i += stride) {
      const long b = i / n, v = i - b * n;
      float p[C];
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = x[(b * C + c) * n + v];
      softmax_div<C>(p);
#pragma unroll
      for (int c = 0; c < C; ++c) out[((long)c * B + b) * n + v] = p[c];
    }
  }
}

// classes.labels_on_grid: predict.hip's prob_to_mask gather on each of the C planes, the class of
// the largest value (the first one: strict >); outside the volume every plane is 0 and the class 0
__global__ void __launch_bounds__(TPB) probs_to_labels_kernel(const float* __restrict__ probs, int C,
                                                              uint8_t* __restrict__ labels,
                                                              float* __restrict__ native, Axis ad, Axis ah, Axis aw) {
  const long HW = (long)ah.n_out * aw.n_out;
  const long total = (long)ad.n_out * HW;
  const long plane = (long)ad.n_in * ah.n_in * aw.n_in;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i / HW);
    const long r = i - d * HW;
    const int h = (int)(r / aw.n_out), w = (int)(r - (long)h * aw.n_out);
    const Tap td = linear_tap(ad, d), th = linear_tap(ah, h), tw = linear_tap(aw, w);
    const bool inside = !(td.outside || th.outside || tw.outside);
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float* pc = probs + c * plane;
      float res = 0.f;
      if (inside) res = gather_linear(ad, ah, aw, td, th, tw, [&](long x) { return (double)pc[x]; });
      if (c == 0 || res > best) {
        best = res;
        arg = c;
      }
      if (native != nullptr) native[c * total + i] = res;
    }
    labels[i] = (uint8_t)arg;
  }
}

// ---- per-class overlap counts -----------------------------------------------------------------
// counts[3 c + (0, 1, 2)] += |pred == c|, |ref == c|, |pred == c and ref == c| of the block's
// share, c < C: an LDS table of 3 x 8 counters filled by wave_hist.h's wave-aggregated adds, then
// one 64-bit integer atomic per non-zero counter.  Integer sums: exact, the same on every run.
__device__ __forceinline__ void count_voxel(uint32_t* hist, uint32_t p, uint32_t r, bool on, uint32_t C, int lane) {
  bin_add(hist, p, on && p < C, lane);
  bin_add(hist + MAX_CLASSES, r, on && r < C, lane);
  bin_add(hist + 2 * MAX_CLASSES, p, on && p == r && p < C, lane);
}

__global__ void __launch_bounds__(TPB) class_overlap_kernel(const uint8_t* __restrict__ pred,
                                                            const uint8_t* __restrict__ ref, long n, int C,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ uint32_t hist[3 * MAX_CLASSES];
  if (threadIdx.x < 3 * MAX_CLASSES) hist[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * TPB;
  // four voxels per access where both maps allow it; every lane of a wave takes every trip
  const long n4 = ((((uintptr_t)pred) | ((uintptr_t)ref)) & 3) == 0 ? n / 4 : 0;
  for (long base = blockIdx.x * (long)TPB; base < n4; base += stride) {
    const long i = base + threadIdx.x;
    const bool on = i < n4;
    const uint32_t pw = on ? reinterpret_cast<const uint32_t*>(pred)[i] : 0u;
    const uint32_t rw = on ? reinterpret_cast<const uint32_t*>(ref)[i] : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) count_voxel(hist, (pw >> (8 * u)) & 255u, (rw >> (8 * u)) & 255u, on, (uint32_t)C, lane);
  }
  for (long base = 4 * n4 + blockIdx.x * (long)TPB; base < n; base += stride) {
    const long i = base + threadIdx.x;
    const bool on = i < n;
    count_voxel(hist, on ? pred[i] : 0u, on ? ref[i] : 0u, on, (uint32_t)C, lane);
  }
  __syncthreads();
  if (threadIdx.x < 3 * MAX_CLASSES) {
    const int k = threadIdx.x / MAX_CLASSES, c = threadIdx.x - k * MAX_CLASSES;
    const uint32_t v = hist[threadIdx.x];
    if (c < C && v != 0) atomicAdd(counts + 3 * c + k, (unsigned long long)v);
  }
}

}  // namespace

extern "C" {

int pcms_softmax_loss_rows(long nvox, int N) {
  if (nvox < 1 || N < 1) return -1;
  return stream_grid(nvox, TPB * 8, std::max(1, 1024 / N));
}

int pcms_softmax_loss_fwd(const float* x, const void* target, int target_u8, long nvox, int N, int C, int per_sample,
                          int include_background, float smooth, float ce_weight, float dice_weight,
                          const float* class_weights, float* part, double* sums, float* coef, float* loss,
                          hipStream_t s) {
  ClassWeights cw;
  if (loss_args(x, target, target_u8, nvox, N, C, class_weights, &cw) != 0) return -1;
  if (part == nullptr || sums == nullptr || coef == nullptr || loss == nullptr) return -1;
  if (misaligned(part, alignof(float)) || misaligned(sums, alignof(double)) || misaligned(coef, alignof(float)) ||
      misaligned(loss, alignof(float)))
    return -1;
  if (!(smooth >= 0.f) || !std::isfinite(smooth) || !std::isfinite(ce_weight) || !std::isfinite(dice_weight)) return -1;
  const int rows = pcms_softmax_loss_rows(nvox, N);
  const int rc = for_classes(C, [&](auto c) {
    PCMS_LAUNCH((softmax_partial_kernel<decltype(c)::value>), dim3(rows, N), dim3(TPB), 0, s, x, target, target_u8,
                nvox, cw, part);
    return 0;
  });
  if (rc != 0) return rc;
  const SoftCfg cfg{smooth, ce_weight, dice_weight, C, include_background ? 1 : 0, per_sample ? 1 : 0};
  hipLaunchKernelGGL(softmax_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)part, rows, N, cfg, sums, coef,
                     loss);
  PCMS_CHECK_LAUNCH();
}

int pcms_softmax_loss_bwd(const float* x, const void* target, int target_u8, long nvox, int N, int C, int per_sample,
                          const float* class_weights, const float* coef, const float* gout, float* dx,
                          hipStream_t s) {
  ClassWeights cw;
  if (loss_args(x, target, target_u8, nvox, N, C, class_weights, &cw) != 0) return -1;
  if (coef == nullptr || dx == nullptr || misaligned(coef, alignof(float)) || misaligned(dx, alignof(float)) ||
      misaligned(gout, alignof(float)))
    return -1;
  const int blocks = stream_grid(cdiv(nvox, 4), TPB, std::max(1, 8192 / N));
  const int groups = per_sample ? N : 1;
  return for_classes(C, [&](auto c) {
    hipLaunchKernelGGL((softmax_bwd_kernel<decltype(c)::value>), dim3(blocks, N), dim3(TPB), 0, s, x, target,
                       target_u8, nvox, per_sample ? 1 : 0, groups, cw, coef, gout, dx);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_resample_classes(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                          const float* class_values, int n_values, float* out, int D, int H, int W, hipStream_t s) {
  ClassTable tab;
  if (src == nullptr || out == nullptr || make_table(class_values, n_values, &tab) != 0) return -1;
  if (Di < 1 || Hi < 1 || Wi < 1 || D < 1 || H < 1 || W < 1 || misaligned(out, alignof(float))) return -1;
  const Axis ad = make_axis(Di, D), ah = make_axis(Hi, H), aw = make_axis(Wi, W);
  const Scale sc = make_scale(scl_slope, scl_inter);
  const int grid = grid_for((long)D * H * W, TPB);
  return for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    hipLaunchKernelGGL(resample_classes_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, ad, ah, aw, sc, tab);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_resample_affine_classes(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                 double scl_inter, const double* affine12, const float* class_values, int n_values,
                                 float* out, int D, int H, int W, hipStream_t s) {
  ClassTable tab;
  if (!affine_args_ok(src, out, affine12, Di, Hi, Wi, D, H, W, 1.f, 0.f)) return -1;
  if (make_table(class_values, n_values, &tab) != 0) return -1;
  const Affine m = make_affine(affine12);  // copied into the kernel arguments
  const Dims g{Di, Hi, Wi, D, H, W};
  const Scale sc = make_scale(scl_slope, scl_inter);
  const int grid = grid_for((long)D * H * W, TPB);
  return for_datatype(datatype, [&](auto t) {
    using T = decltype(t);
    if (misaligned(src, alignof(T))) return -1;
    hipLaunchKernelGGL(resample_affine_classes_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)src, out, m, g, sc,
                       tab);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_softmax_planes(const float* logits, int B, int C, long n, float* probs, hipStream_t s) {
  if (logits == nullptr || probs == nullptr || misaligned(logits, alignof(float)) || misaligned(probs, alignof(float)))
    return -1;
  if (B < 1 || n < 1 || C < 2 || C > MAX_CLASSES) return -1;
  if (overlap(logits, (long)B * C * n * 4, probs, (long)B * C * n * 4)) return -1;  // the layouts differ
  const int grid = stream_grid(cdiv((long)B * n, 4), TPB);
  return for_classes(C, [&](auto c) {
    hipLaunchKernelGGL((softmax_planes_kernel<decltype(c)::value>), dim3(grid), dim3(TPB), 0, s, logits, probs, B, n);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_probs_to_labels(const float* probs, int C, int Dt, int Ht, int Wt, unsigned char* labels, float* probs_native,
                         int D, int H, int W, hipStream_t s) {
  if (probs == nullptr || labels == nullptr) return -1;
  if (C < 1 || C > MAX_CLASSES || Dt < 1 || Ht < 1 || Wt < 1 || D < 1 || H < 1 || W < 1) return -1;
  if (misaligned(probs, alignof(float)) || misaligned(probs_native, alignof(float))) return -1;
  const Axis ad = make_axis(Dt, D), ah = make_axis(Ht, H), aw = make_axis(Wt, W);
  hipLaunchKernelGGL(probs_to_labels_kernel, dim3(grid_for((long)D * H * W, TPB)), dim3(TPB), 0, s, probs, C, labels,
                     probs_native, ad, ah, aw);
  PCMS_CHECK_LAUNCH();
}

int pcms_class_overlap(const unsigned char* pred, const unsigned char* ref, long n, int C, long* counts,
                       hipStream_t s) {
  if (pred == nullptr || ref == nullptr || counts == nullptr || misaligned(counts, alignof(long))) return -1;
  if (n < 1 || C < 1 || C > MAX_CLASSES) return -1;
  const int rc = (int)hipMemsetAsync(counts, 0, sizeof(long) * 3 * C, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(class_overlap_kernel, dim3(stream_grid(cdiv(n, 4), TPB, 1024)), dim3(TPB), 0, s, pred, ref, n, C,
                     (unsigned long long*)counts);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
