// The tail of the U-Net step (gfx950): DiceLoss / BCEDiceLoss forward / backward on the fp32
// logits, flat Adam over the parameter buffers, and the global gradient norm / clip.
//
// Reference ops replaced (paths relative to the reference repo):
//   DiceLoss / BCEDiceLoss        utils/losses.py:44-92, 124-152
//   optim.Adam(wd=1e-5, coupled)  utils/trainer.py:113-117
// Sums are two-level: per-block partial rows, combined in fp64 in a fixed order (run-to-run
// reproducible).  Every launch here is grid-stride with a capped grid (stream_grid,
// ops_units.h).
#include "ops_units.h"
#include "pcms_hip.h"

namespace {

// ---------------- losses ----------------
// partial rows: [block][4] = (sum p*t, sum p, sum t, sum bce)
__global__ void __launch_bounds__(TPB) loss_partial_kernel(const float* x, const float* t, long M, float* part) {
  __shared__ float red[4][TPB / 64];
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
  auto one = [&](float xv, float tv) {
    const float p = 1.f / (1.f + expf(-xv));
    a += p * tv; b += p; c += tv;
    d += fmaxf(xv, 0.f) - xv * tv + log1pf(expf(-fabsf(xv)));
  };
  // 8 elements' loads in flight per trip, accumulated in the same element order as one at a
  // time (identical sums; one element per trip was a chain of 8 memory latencies per thread)
  const long stride = (long)gridDim.x * blockDim.x;
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (; i + 7 * stride < M; i += 8 * stride) {
    float xv[8], tv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { xv[u] = x[i + u * stride]; tv[u] = t[i + u * stride]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) one(xv[u], tv[u]);
  }
  for (; i < M; i += stride) one(x[i], t[i]);
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); d = wave_sum(d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; red[3][wave] = d; }
  __syncthreads();
  if (threadIdx.x < 4) {
    float s = 0.f;
    for (int w = 0; w < TPB / 64; ++w) s += red[threadIdx.x][w];
    part[blockIdx.x * 4 + threadIdx.x] = s;
  }
}

// sums[0..3] (double) from partials; loss = wb*bce/M + wd*(1 - dice)
__global__ void loss_finalize_kernel(const float* part, int rows, long M, float smooth, float wb, float wd,
                                     double* sums, float* loss) {
  __shared__ double red[4][64];
  const int t = threadIdx.x;  // 256 threads: 4 sums x 64 lanes
  const int k = t >> 6, l = t & 63;
  double s = 0.0;
  for (int r = l; r < rows; r += 64) s += (double)part[r * 4 + k];
  red[k][l] = s;
  __syncthreads();
  if (t < 4) {
    double acc = 0.0;
    for (int i = 0; i < 64; ++i) acc += red[t][i];
    sums[t] = acc;
  }
  __syncthreads();
  if (t == 0) {
    const double I = sums[0], P = sums[1], Tt = sums[2], B = sums[3];
    const double dice = (2.0 * I + smooth) / (P + Tt + smooth);
    loss[0] = (float)(wb * (B / (double)M) + wd * (1.0 - dice));
  }
}

// dL/dx_i = gout * (wb*(p - t)/M + wd * -(2 t (P+T+s) - (2I+s)) / (P+T+s)^2 * p(1-p))
__global__ void loss_bwd_kernel(const float* x, const float* t, long M, const double* sums, float smooth,
                                float wb, float wd, const float* gout, float* dx) {
  const double I = sums[0], P = sums[1], Tt = sums[2];
  const double den = P + Tt + smooth, num = 2.0 * I + smooth;
  const float inv_den2 = (float)(1.0 / (den * den));
  const float fden = (float)den, fnum = (float)num;
  const float g = gout ? gout[0] : 1.f;
  const float invM = (float)(1.0 / (double)M);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < M; i += (long)gridDim.x * blockDim.x) {
    const float xv = x[i], tv = t[i];
    const float p = 1.f / (1.f + expf(-xv));
    const float ddice_dp = -(2.f * tv * fden - fnum) * inv_den2;
    dx[i] = g * (wb * (p - tv) * invM + wd * ddice_dp * p * (1.f - p));
  }
}

// ---------------- Adam (torch.optim.Adam, foreach, coupled weight decay) ----------
// g_eff = g * s, s = gscale * (*gmul if gmul) (the data-parallel 1/world mean, the gradient-
// clip coefficient, the AMP unscale); when s != 1 the scaled gradient is also written back,
// so param.grad afterwards holds what torch's clip_grad_norm_ / DDP mean would leave there.
__global__ void adam_kernel(float* p, float* g, float* m, float* v, long n, AdamCoef c, const float* gmul) {
  const float s = gmul ? c.gscale * gmul[0] : c.gscale;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], gi = g[i], mi = m[i], vi = v[i];
    adam_update(pi, gi, mi, vi, c, s);
    if (s != 1.f) g[i] = gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// The same over a list of [begin, end) element ranges of the flat buffers (the parameters the
// fused Adam + weight-pack kernels do not cover): blockIdx.y = range.
// p[b, e) = v for every [b, e) row of ranges (int64 pairs); grid.y = range
__global__ void fill_ranges_kernel(float* p, const long long* ranges, float v) {
  const long b = ranges[2 * blockIdx.y], e = ranges[2 * blockIdx.y + 1];
  for (long i = b + blockIdx.x * (long)blockDim.x + threadIdx.x; i < e; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void adam_ranges_kernel(float* p, float* g, float* m, float* v, const long long* ranges, AdamCoef c,
                                   const float* gmul) {
  const float s = gmul ? c.gscale * gmul[0] : c.gscale;
  const long b = ranges[2 * blockIdx.y], e = ranges[2 * blockIdx.y + 1];
  for (long i = b + blockIdx.x * (long)blockDim.x + threadIdx.x; i < e; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], gi = g[i], mi = m[i], vi = v[i];
    adam_update(pi, gi, mi, vi, c, s);
    if (s != 1.f) g[i] = gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// ---------------- global gradient norm / clip (torch.nn.utils.clip_grad_norm_) ----------
// pass 1: per-block fp64 partial sums of g^2 (fp32 squares), one row per block
constexpr int kNormBlocks = 1024;
__global__ void __launch_bounds__(TPB) sumsq_kernel(const float* g, long n, double* part) {
  __shared__ double red[TPB / 64];
  double s = 0.0;
  const long n4 = n / 4;
  const f32x4_t* g4 = reinterpret_cast<const f32x4_t*>(g);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4_t v = g4[i];
    s += (double)(v[0] * v[0]) + (double)(v[1] * v[1]) + (double)(v[2] * v[2]) + (double)(v[3] * v[3]);
  }
  if (blockIdx.x == 0)
    for (long i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) s += (double)(g[i] * g[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < TPB / 64; ++w) t += red[w];
    part[blockIdx.x] = t;
  }
}
// pass 2 (one block): norm = gscale * sqrt(sum of rows, in row order); mul = gscale *
// min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_'s clamped coefficient; max_norm <= 0:
// no clipping, mul = gscale)
__global__ void clip_finalize_kernel(const double* part, int rows, float gscale, float max_norm, float* norm_out,
                                     float* mul_out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += part[r];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];
    const float norm = (float)sqrt(t) * gscale;
    float coef = 1.f;
    if (max_norm > 0.f) coef = fminf(1.f, max_norm / (norm + 1e-6f));
    if (norm_out) norm_out[0] = norm;
    if (mul_out) mul_out[0] = gscale * coef;
  }
}
// g *= *mul (in place)
__global__ void scale_kernel(float* g, long n, const float* mul) {
  const float s = mul[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) g[i] *= s;
}

}  // namespace

extern "C" {

int pcms_loss_rows(long M) { return stream_grid(M, TPB * 8, 1024); }

// loss (device fp32 scalar) and sums (device fp64[4]); part: rows*4 floats
int pcms_loss_fwd(const float* x, const float* t, long M, float smooth, float wb, float wd, float* part,
                  double* sums, float* loss, hipStream_t s) {
  const int rows = pcms_loss_rows(M);
  PCMS_LAUNCH(loss_partial_kernel, dim3(rows), dim3(TPB), 0, s, x, t, M, part);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)part, rows, M, smooth, wb, wd, sums, loss);
  PCMS_CHECK_LAUNCH();
}

int pcms_loss_bwd(const float* x, const float* t, long M, const double* sums, float smooth, float wb, float wd,
                  const float* gout, float* dx, hipStream_t s) {
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(stream_grid(M, TPB)), dim3(TPB), 0, s, x, t, M, sums, smooth, wb, wd, gout, dx);
  PCMS_CHECK_LAUNCH();
}

// step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)  (host fp64 -> fp32)
int pcms_adam(float* p, float* g, float* m, float* v, long n, float step_size, float b1, float b2, float eps,
              float wd, float bc2_sqrt, float gscale, const float* gmul, hipStream_t s) {
  const AdamCoef c{step_size, b1, b2, eps, wd, bc2_sqrt, gscale};
  hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n, TPB, 16384)), dim3(TPB), 0, s, p, g, m, v, n, c, gmul);
  PCMS_CHECK_LAUNCH();
}

int pcms_adam_ranges(float* p, float* g, float* m, float* v, const long long* ranges, int nranges, long max_len,
                     float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                     const float* gmul, hipStream_t s) {
  if (nranges <= 0) return 0;
  const AdamCoef c{step_size, b1, b2, eps, wd, bc2_sqrt, gscale};
  hipLaunchKernelGGL(adam_ranges_kernel, dim3(stream_grid(max_len, TPB, 2048), nranges), dim3(TPB), 0, s, p, g, m, v,
                     ranges, c, gmul);
  PCMS_CHECK_LAUNCH();
}

int pcms_fill_ranges(float* p, const long long* ranges, int nranges, long max_len, float v, hipStream_t s) {
  if (nranges <= 0) return 0;
  hipLaunchKernelGGL(fill_ranges_kernel, dim3(stream_grid(max_len, TPB, 1024), nranges), dim3(TPB), 0, s, p, ranges, v);
  PCMS_CHECK_LAUNCH();
}

int pcms_grad_clip_ws_doubles(void) { return kNormBlocks; }

int pcms_grad_clip(float* g, long n, float gscale, float max_norm, int apply, double* ws, float* norm_out,
                   float* mul_out, hipStream_t s) {
  if (ws == nullptr || mul_out == nullptr || misaligned(g, 16)) return -1;
  const int rows = stream_grid(n / 4 + 1, TPB, kNormBlocks);
  PCMS_LAUNCH(sumsq_kernel, dim3(rows), dim3(TPB), 0, s, (const float*)g, n, ws);
  PCMS_LAUNCH(clip_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, rows, gscale, max_norm, norm_out,
              mul_out);
  if (!apply) return 0;
  hipLaunchKernelGGL(scale_kernel, dim3(stream_grid(n, TPB, 16384)), dim3(TPB), 0, s, g, n, (const float*)mul_out);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
