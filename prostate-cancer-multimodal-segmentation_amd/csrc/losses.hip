// Imbalance-aware losses on the fp32 logits (gfx950): a Tversky / focal-Tversky region term per
// group plus a focal voxel term.  A group is a contiguous run of nvox elements of the
// NCDHW tensors: groups = 1, nvox = M for sums over the batch (the reference's Dice convention),
// groups = N*C, nvox = D*H*W for sums per sample and channel.
//
//   per group g, p = sigmoid(x):   I = sum p t, P = sum p, T = sum t
//     D = (1-a-b) I + a P + b T + s,  TI = (I + s) / D,  region_g = max(1 - TI, 0)^gr
//   per voxel, ce = max(x,0) - x t + log1p(exp(-|x|)),  m = 1 - p_t = t (1-p) + (1-t) p:
//     v_i = a_i m^gv ce,  a_i = av t + (1-av)(1-t) (1 when av is off; gv = 0: v_i = a_i ce)
//   loss = w_region mean_g region_g + w_voxel (1/M) sum_i v_i
//
// Forward: region_partial_kernel (grid = rows x groups, one fp32 row [4] = (sum p t, sum p, sum t,
// sum v) per block) and region_finalize_kernel (one block: the rows of each group summed in fp64
// in row order, the loss, and the backward's two fp32 coefficients per group).  Backward: one
// elementwise launch that reads a group's coefficients once per block.  Every sum has a fixed
// order: the same bits on every run.  Every launch is grid-stride under stream_grid (ops_units.h).
//
// One expf serves the sigmoid, 1 - sigmoid and the softplus: e = exp(-|x|), p = 1/(1+e) or
// e/(1+e), so nothing overflows and 1 - p has no cancellation at any |x|.  m^gv is
// exp(gv log m): m = 0 gives exp(-inf) = 0, never 0 * inf (gv >= 1).
#include "ops_units.h"
#include "pcms_hip.h"

namespace {

struct VoxCfg {
  float gv;      // focal exponent (0 with POW off)
  float a0, a1;  // a_i = a0 + a1 t: (1-av, 2av-1), or (1, 0) when av is off
};

struct Vox {
  float p, q, ce;  // sigmoid(x), 1 - sigmoid(x), BCE-with-logits (VOX only)
};
template <bool VOX> __device__ __forceinline__ Vox vox_of(float x, float t) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  Vox v;
  v.p = x >= 0.f ? inv : e * inv;
  v.q = x >= 0.f ? e * inv : inv;
  v.ce = 0.f;
  if constexpr (VOX) v.ce = fmaxf(x, 0.f) - x * t + log1pf(e);
  return v;
}

struct Acc {
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
};
template <bool VOX, bool POW> __device__ __forceinline__ void add_one(Acc& s, float x, float t, const VoxCfg& c) {
  const Vox v = vox_of<VOX>(x, t);
  s.a += v.p * t;
  s.b += v.p;
  s.c += t;
  if constexpr (VOX) {
    float w = (c.a0 + c.a1 * t) * v.ce;
    if constexpr (POW) w *= expf(c.gv * logf(t * v.q + (1.f - t) * v.p));
    s.d += w;
  }
}

// a group's base is 16-byte aligned in both tensors: its first nvox / 4 * 4 elements go as vectors
__device__ __forceinline__ bool vec_ok(const float* x, const float* t) {
  return (((uintptr_t)x | (uintptr_t)t) & 15) == 0;
}

// partial rows: part[(g * rows + block)][4] = (sum p t, sum p, sum t, sum v) of the block's share
// of group g; grid = (rows, groups)
// four voxels, two at a time: all four chains (and a second vector's) interleaved hold more
// temporaries than the 64-VGPR budget leaves beside the loads in flight
template <bool VOX, bool POW>
__device__ __forceinline__ void add_four(Acc& s, const float* x, const float* t, const VoxCfg& c) {
  add_one<VOX, POW>(s, x[0], t[0], c);
  add_one<VOX, POW>(s, x[1], t[1], c);
  __builtin_amdgcn_sched_barrier(0);
  add_one<VOX, POW>(s, x[2], t[2], c);
  add_one<VOX, POW>(s, x[3], t[3], c);
  __builtin_amdgcn_sched_barrier(0);
}

template <bool VOX, bool POW>
__global__ void __launch_bounds__(TPB, 8) region_partial_kernel(const float* x, const float* t, long nvox, VoxCfg cfg,
                                                                float* part) {
  __shared__ float red[4][TPB / 64];
  const float* xg = x + (long)blockIdx.y * nvox;
  const float* tg = t + (long)blockIdx.y * nvox;
  // (groups * nvox < 2^31 and the grid is at most 2^18 threads wide: every index fits 32 bits)
  const unsigned n = (unsigned)nvox, stride = gridDim.x * blockDim.x;
  unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  Acc s;
  if (vec_ok(xg, tg)) {
    // two 16-byte loads of each tensor in flight per trip, then a one-vector tail, then the
    // group's last nvox % 4 elements
    const unsigned n4 = n / 4;
    for (; i + stride < n4; i += 2 * stride) {
      float xa[4], xb[4], ta[4], tb[4];
      load16<float>(xg + 4 * (size_t)i, xa);
      load16<float>(xg + 4 * (size_t)(i + stride), xb);
      load16<float>(tg + 4 * (size_t)i, ta);
      load16<float>(tg + 4 * (size_t)(i + stride), tb);
      add_four<VOX, POW>(s, xa, ta, cfg);
      add_four<VOX, POW>(s, xb, tb, cfg);
    }
    for (; i < n4; i += stride) {
      float xa[4], ta[4];
      load16<float>(xg + 4 * (size_t)i, xa);
      load16<float>(tg + 4 * (size_t)i, ta);
      add_four<VOX, POW>(s, xa, ta, cfg);
    }
    const unsigned j = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && j < n) add_one<VOX, POW>(s, xg[j], tg[j], cfg);
  } else {
    // a misaligned group (nvox % 4 != 0, odd groups): scalar loads, four in flight per trip
    for (; i + 3 * stride < n; i += 4 * stride) {
      float xv[4], tv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { xv[u] = xg[i + u * stride]; tv[u] = tg[i + u * stride]; }
      add_four<VOX, POW>(s, xv, tv, cfg);
    }
    for (; i < n; i += stride) add_one<VOX, POW>(s, xg[i], tg[i], cfg);
  }
  s.a = wave_sum(s.a); s.b = wave_sum(s.b); s.c = wave_sum(s.c); s.d = wave_sum(s.d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = s.a; red[1][wave] = s.b; red[2][wave] = s.c; red[3][wave] = s.d; }
  __syncthreads();
  if (threadIdx.x < 4) {
    float r = 0.f;
    for (int w = 0; w < TPB / 64; ++w) r += red[threadIdx.x][w];
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = r;
  }
}

// u^y, u > 0 (on its own so that its registers are allotted apart from the caller's)
__device__ __noinline__ double pow_pos(double u, double y) { return exp(y * log(u)); }

struct RegionCfg {
  float alpha, beta, gr, smooth, w_region, w_voxel;
};

// One block of 256 threads.  Wave k sums column k of each group's rows (lane l: rows l, l + 64,
// ... in fp64, the 64 lane sums by a fixed xor tree) into sums[g][k]; then thread j takes groups
// j, j + 256, ...: region_g and the backward's coefficients, all fp64, rounded once
//   dR = -gr (1-TI)^(gr-1) w_region / groups   (0 where 1 - TI <= 0 or D <= 0)
//   coef[g] = (cI, cP) = (dR (D - (I+s)(1-a-b)) / D^2,  -dR a (I+s) / D^2);
// thread 0 adds the threads' (sum region_g, sum v) in thread order and writes the loss.
template <bool GR1>
__global__ void __launch_bounds__(256, 8) region_finalize_kernel(const float* part, int rows, int groups, long nvox,
                                                              RegionCfg c, double* sums, float* coef, float* loss) {
  __shared__ double red[2][256];
  const int k = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int g = 0; g < groups; ++g) {
    const float* pg = part + (long)g * rows * 4;
    double s = 0.0;
    for (int r = l; r < rows; r += 64) s += (double)pg[r * 4 + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) sums[g * 4 + k] = s;
  }
  __syncthreads();
  red[0][threadIdx.x] = 0.0;
  red[1][threadIdx.x] = 0.0;
  const double ab = 1.0 - (double)c.alpha - (double)c.beta, sm = c.smooth;
  for (int g = threadIdx.x; g < groups; g += 256) {
    // the sums are read twice (volatile: no value stays in a register across the fp64 exp / log,
    // whose own registers fill most of the 64-VGPR budget), and the running sums live in LDS
    const volatile double* sv = sums + g * 4;
    double um1 = 1.0;  // (1-TI)^(gr-1)
    if constexpr (!GR1) {
      const double I = sv[0], D = ab * I + (double)c.alpha * sv[1] + (double)c.beta * sv[2] + sm;
      const double u = D > 0.0 ? 1.0 - (I + sm) / D : 0.0;
      um1 = u > 0.0 ? pow_pos(u, (double)c.gr - 1.0) : 0.0;
    }
    const double I = sv[0], P = sv[1], T = sv[2];
    const double D = ab * I + (double)c.alpha * P + (double)c.beta * T + sm;
    const double u = D > 0.0 ? 1.0 - (I + sm) / D : 0.0;
    const bool pos = u > 0.0;
    const double dR = pos ? -(double)c.gr * (double)c.w_region / (double)groups * um1 : 0.0;
    const double inv2 = D > 0.0 ? 1.0 / (D * D) : 0.0;
    coef[g * 2] = (float)(dR * (D - (I + sm) * ab) * inv2);
    coef[g * 2 + 1] = (float)(-dR * (double)c.alpha * (I + sm) * inv2);
    red[0][threadIdx.x] += pos ? um1 * u : 0.0;
    red[1][threadIdx.x] += sv[3];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0, v = 0.0;
    const int n = groups < 256 ? groups : 256;
    for (int i = 0; i < n; ++i) { r += red[0][i]; v += red[1][i]; }
    loss[0] = (float)((double)c.w_region * (r / (double)groups) + (double)c.w_voxel * (v / ((double)groups * (double)nvox)));
  }
}

// dx_i = gout [ (cI t + cP) p (1-p) + wm a_i dv_i ],  wm = w_voxel / M,
// dv_i = m^gv (p - t) - gv m^(gv-1) (2t - 1) p (1-p) ce   (gv = 0: p - t)
struct BwdCfg {
  float cI, cP, g, wm;
};
template <bool VOX, bool POW> __device__ __forceinline__ float dx_one(float x, float t, const BwdCfg& b, const VoxCfg& c) {
  const Vox v = vox_of<VOX>(x, t);
  const float pq = v.p * v.q;
  float r = (b.cI * t + b.cP) * pq;
  if constexpr (VOX) {
    float dv = v.p - t;
    if constexpr (POW) {
      const float m = t * v.q + (1.f - t) * v.p;
      // m^(gv-1): 1 at gv = 1 (also at m = 0, where the second term's p (1-p) is 0)
      const float mm1 = c.gv == 1.f ? 1.f : expf((c.gv - 1.f) * logf(m));
      dv = mm1 * (m * dv - c.gv * (2.f * t - 1.f) * pq * v.ce);
    }
    r += b.wm * (c.a0 + c.a1 * t) * dv;
  }
  return b.g * r;
}

// grid = (blocks per group, groups); a group's two coefficients are read once per block
template <bool VOX, bool POW>
__global__ void __launch_bounds__(TPB, 8) region_bwd_kernel(const float* x, const float* t, long nvox, VoxCfg cfg,
                                                         float wm, const float* coef, const float* gout, float* dx) {
  const float* xg = x + (long)blockIdx.y * nvox;
  const float* tg = t + (long)blockIdx.y * nvox;
  float* dg = dx + (long)blockIdx.y * nvox;
  const BwdCfg b{coef[2 * blockIdx.y], coef[2 * blockIdx.y + 1], gout ? gout[0] : 1.f, wm};
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (vec_ok(xg, tg) && ((uintptr_t)dg & 15) == 0) {
    const long n4 = nvox / 4;
    const f32x4_t* x4 = reinterpret_cast<const f32x4_t*>(xg);
    const f32x4_t* t4 = reinterpret_cast<const f32x4_t*>(tg);
    f32x4_t* d4 = reinterpret_cast<f32x4_t*>(dg);
    for (; i < n4; i += stride) {
      const f32x4_t xa = x4[i], ta = t4[i];
      f32x4_t o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = dx_one<VOX, POW>(xa[u], ta[u], b, cfg);
      d4[i] = o;
    }
    const long j = n4 * 4 + threadIdx.x;
    if (blockIdx.x == 0 && j < nvox) dg[j] = dx_one<VOX, POW>(xg[j], tg[j], b, cfg);
  } else {
    for (; i < nvox; i += stride) dg[i] = dx_one<VOX, POW>(xg[i], tg[i], b, cfg);
  }
}

// the checks both entry points share; the voxel-term constants on success
int check_args(const void* x, const void* t, long nvox, int groups, float focal_gamma, int use_focal_alpha,
               float focal_alpha, VoxCfg* v) {
  if (x == nullptr || t == nullptr) return -1;
  if (misaligned(x, alignof(float)) || misaligned(t, alignof(float))) return -1;
  if (groups < 1 || groups > 65535 || nvox < 1 || (long)groups * nvox >= (1L << 31)) return -1;
  if (!(focal_gamma == 0.f || focal_gamma >= 1.f) || !std::isfinite(focal_gamma)) return -1;
  if (use_focal_alpha && !(focal_alpha >= 0.f && focal_alpha <= 1.f)) return -1;
  *v = use_focal_alpha ? VoxCfg{focal_gamma, 1.f - focal_alpha, 2.f * focal_alpha - 1.f} : VoxCfg{focal_gamma, 1.f, 0.f};
  return 0;
}

// f(VOX, POW): the voxel term on (w_voxel != 0) and its focal power on (focal_gamma != 0)
template <typename F> int for_voxel(float w_voxel, float focal_gamma, F&& f) {
  if (w_voxel == 0.f) return f(std::false_type{}, std::false_type{});
  return focal_gamma == 0.f ? f(std::true_type{}, std::false_type{}) : f(std::true_type{}, std::true_type{});
}

}  // namespace

extern "C" {

int pcms_region_loss_rows(long nvox, int groups) {
  if (nvox < 1 || groups < 1) return -1;
  return stream_grid(nvox, TPB * 8, std::max(1, 1024 / groups));
}

int pcms_region_loss_fwd(const float* x, const float* t, long nvox, int groups, float alpha, float beta, float gamma,
                         float smooth, float focal_gamma, int use_focal_alpha, float focal_alpha, float w_region,
                         float w_voxel, float* part, double* sums, float* coef, float* loss, hipStream_t s) {
  VoxCfg v;
  if (check_args(x, t, nvox, groups, focal_gamma, use_focal_alpha, focal_alpha, &v) != 0) return -1;
  if (part == nullptr || sums == nullptr || coef == nullptr || loss == nullptr) return -1;
  if (misaligned(part, alignof(float)) || misaligned(sums, alignof(double)) || misaligned(coef, alignof(float)) ||
      misaligned(loss, alignof(float)))
    return -1;
  if (!(alpha >= 0.f) || !(beta >= 0.f) || !(smooth >= 0.f) || !(gamma > 0.f)) return -1;
  if (!std::isfinite(alpha) || !std::isfinite(beta) || !std::isfinite(smooth) || !std::isfinite(gamma) ||
      !std::isfinite(w_region) || !std::isfinite(w_voxel))
    return -1;
  const int rows = pcms_region_loss_rows(nvox, groups);
  const int rc = for_voxel(w_voxel, focal_gamma, [&](auto vox, auto pw) {
    PCMS_LAUNCH((region_partial_kernel<decltype(vox)::value, decltype(pw)::value>), dim3(rows, groups), dim3(TPB), 0, s,
                x, t, nvox, v, part);
    return 0;
  });
  if (rc != 0) return rc;
  const RegionCfg c{alpha, beta, gamma, smooth, w_region, w_voxel};
  if (gamma == 1.f)
    hipLaunchKernelGGL(region_finalize_kernel<true>, dim3(1), dim3(256), 0, s, (const float*)part, rows, groups, nvox, c,
                       sums, coef, loss);
  else
    hipLaunchKernelGGL(region_finalize_kernel<false>, dim3(1), dim3(256), 0, s, (const float*)part, rows, groups, nvox, c,
                       sums, coef, loss);
  PCMS_CHECK_LAUNCH();
}

int pcms_region_loss_bwd(const float* x, const float* t, long nvox, int groups, float focal_gamma, int use_focal_alpha,
                         float focal_alpha, float w_voxel, const float* coef, const float* gout, float* dx,
                         hipStream_t s) {
  VoxCfg v;
  if (check_args(x, t, nvox, groups, focal_gamma, use_focal_alpha, focal_alpha, &v) != 0) return -1;
  if (coef == nullptr || dx == nullptr || misaligned(coef, alignof(float)) || misaligned(dx, alignof(float)) ||
      misaligned(gout, alignof(float)) || !std::isfinite(w_voxel))
    return -1;
  const float wm = (float)((double)w_voxel / ((double)groups * (double)nvox));
  const int blocks = stream_grid(cdiv(nvox, 4), TPB, std::max(1, 8192 / groups));
  return for_voxel(w_voxel, focal_gamma, [&](auto vox, auto pw) {
    hipLaunchKernelGGL((region_bwd_kernel<decltype(vox)::value, decltype(pw)::value>), dim3(blocks, groups), dim3(TPB), 0,
                       s, x, t, nvox, v, wm, coef, gout, dx);
    PCMS_CHECK_LAUNCH();
  });
}

}  // extern "C"
