// Layout and glue kernels of the U-Net step (NDHWC, gfx950): the input layout pack and the
// output unpack, the elementwise add, the split-K conv epilogue, and the sub-box channel sum with
// the fixed-order row sum behind it.  Bandwidth-bound; every launch here is grid-stride with a
// capped grid (stream_grid, ops_units.h).  No reference op of its own: these replace the
// layout conversions and reductions that the reference leaves to torch around its modules.
#include "ops_units.h"
#include "pcms_hip.h"

namespace {

// ---------------- input: NCDHW fp32 (N, Cin, V) -> NDHWC T (N, V, Cp) ----------------
template <typename T>
__global__ void pack_input_kernel(const float* in, T* out, int N, int Cin, long V, int Cp) {
  const long total = (long)N * V;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / V, v = i % V;
    for (int c = 0; c < Cp; ++c) {
      const float x = c < Cin ? in[(n * Cin + c) * V + v] : 0.f;
      Elem<T>::st(out + i * Cp + c, x);
    }
  }
}

// the same with 4 voxels per thread (V % 4 == 0, Cin <= Cp == 8): one 16-B load per input
// channel, one 16-B (bf16) / two 16-B (fp32) stores per voxel
template <typename T>
__global__ void __launch_bounds__(256) pack_input4_kernel(const float* in, T* out, int N, int Cin, long V) {
  const long quads = (long)N * V / 4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < quads; i += (long)gridDim.x * blockDim.x) {
    const long n = (4 * i) / V, v = (4 * i) % V;
    f32x4_t x[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
      x[c] = c < Cin ? __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(in + (n * Cin + c) * V + v))
                     : (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (sizeof(T) == 2) {
        const u32x4_t o = {pack_bf16x2(x[0][k], x[1][k]), pack_bf16x2(x[2][k], x[3][k]),
                           pack_bf16x2(x[4][k], x[5][k]), pack_bf16x2(x[6][k], x[7][k])};
        *reinterpret_cast<u32x4_t*>(out + (4 * i + k) * 8) = o;
      } else {
        *reinterpret_cast<f32x4_t*>(out + (4 * i + k) * 8) = (f32x4_t){x[0][k], x[1][k], x[2][k], x[3][k]};
        *reinterpret_cast<f32x4_t*>(out + (4 * i + k) * 8 + 4) = (f32x4_t){x[4][k], x[5][k], x[6][k], x[7][k]};
      }
    }
  }
}

// ---------------- NDHWC (T, Cs stored channels) -> NCDHW fp32, first C channels ----------
template <typename T>
__global__ void unpack_output_kernel(const T* in, float* out, int N, int C, int Cs, long V) {
  const long total = (long)N * C * V;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long v = i % V, nc = i / V;
    const int c = (int)(nc % C);
    const long n = nc / C;
    out[i] = Elem<T>::ld(in + (n * V + v) * Cs + c);
  }
}

template <typename T>
__global__ void add_kernel(T* dst, const T* src, long nvec) {
  constexpr int VEC = Elem<T>::kVec;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
    float a[VEC], b[VEC];
    load16<T>(dst + i * VEC, a);
    load16<T>(src + i * VEC, b);
#pragma unroll
    for (int j = 0; j < VEC; ++j) a[j] += b[j];
    store16<T>(dst + i * VEC, a);
  }
}

// fp32 split-K slabs [splits][nvox][C] -> sum in split order + bias, store T, BN partial
// sums; 64 voxels per block row
constexpr int kMaxSplitSlabs = 16;  // slabs loaded together (more: summed one by one after)
// 16 voxel lanes x 64 channels per block: a thread owns 4 of the row's 64 voxels, so a voxel
// row is 4 rounds of slab loads instead of 16 (deep levels have few rows: level 4 is 8 rows x
// 16 channel blocks, and each round is a full memory latency)
constexpr int kSeThreads = 1024;
#ifndef SE_BATCH
#define SE_BATCH 0
#endif
template <typename T>
__global__ void __launch_bounds__(kSeThreads) split_epilogue_kernel(const float* acc, int splits, const float* bias,
                                                                    T* y0, T* y1, int cy0, float* stats, int C,
                                                                    long nvox, int relu) {
  // stats row = (sum, M2 about the row mean), count row after the [rows][C][2] block
  constexpr int NV = kSeThreads / 64, KPT = 64 / NV;
  __shared__ float red[NV][64][3];
  const int cl = threadIdx.x & 63, vl = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const long v0 = (long)blockIdx.x * 64;
  const float bc = bias ? bias[c] : 0.f;
  float xs[KPT];
  float s1 = 0.f, s2 = 0.f;
  int cntv = 0;
#if SE_BATCH
  // every slab load of the thread's KPT voxels issued before the first add: the store of a
  // voxel may alias the next voxel's slabs for the compiler, so the per-voxel loop below ran
  // KPT rounds of memory latency (same summation order either way)
  float part[KPT][kMaxSplitSlabs];
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const long v = v0 + vl + i * NV;
#pragma unroll
    for (int sp = 0; sp < kMaxSplitSlabs; ++sp)
      if (sp < splits && v < nvox) part[i][sp] = acc[((long)sp * nvox + v) * C + c];
  }
#endif
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const long v = v0 + vl + i * NV;
    xs[i] = 0.f;
    if (v >= nvox) continue;
#if SE_BATCH
    float x = part[i][0];
#pragma unroll
    for (int sp = 1; sp < kMaxSplitSlabs; ++sp)
      if (sp < splits) x += part[i][sp];
#else
    // the split slabs in split order (a fixed summation order); all of a voxel's slab loads
    // are issued before the first add (a load -> add chain per slab was latency-bound)
    float part[kMaxSplitSlabs];
#pragma unroll
    for (int sp = 0; sp < kMaxSplitSlabs; ++sp)
      if (sp < splits) part[sp] = acc[((long)sp * nvox + v) * C + c];
    float x = part[0];
#pragma unroll
    for (int sp = 1; sp < kMaxSplitSlabs; ++sp)
      if (sp < splits) x += part[sp];
#endif
    for (int sp = kMaxSplitSlabs; sp < splits; ++sp) x += acc[((long)sp * nvox + v) * C + c];
    x += bc;
    if (relu) x = fmaxf(x, 0.f);
    T* dst = c < cy0 ? y0 + v * cy0 + c : y1 + v * (C - cy0) + (c - cy0);
    Elem<T>::st(dst, x);
    xs[i] = x;
    s1 += x;
    ++cntv;
  }
  if (!stats) return;
  const float m = cntv ? s1 / cntv : 0.f;
  float sd = 0.f;
#pragma unroll
  for (int i = 0; i < KPT; ++i)
    if (v0 + vl + i * NV < nvox) { s2 += (xs[i] - m) * (xs[i] - m); sd += xs[i] - m; }
  if (cntv) s2 -= sd * sd / cntv;  // deviations about the rounded mean
  red[vl][cl][0] = s1;
  red[vl][cl][1] = s2;
  red[vl][cl][2] = (float)cntv;
  __syncthreads();
  if (vl == 0) {
    float S = 0.f, Nn = 0.f;
    for (int k = 0; k < NV; ++k) { S += red[k][cl][0]; Nn += red[k][cl][2]; }
    const float mb = Nn > 0.f ? S / Nn : 0.f;
    float M2 = 0.f, sdd = 0.f;
    for (int k = 0; k < NV; ++k) {
      const float n = red[k][cl][2];
      if (n > 0.f) {
        const float d = red[k][cl][0] / n - mb;
        M2 += red[k][cl][1] + n * d * d;
        sdd += n * d;
      }
    }
    if (Nn > 0.f) M2 -= sdd * sdd / Nn;
    stats[((long)blockIdx.x * C + c) * 2] = S;
    stats[((long)blockIdx.x * C + c) * 2 + 1] = M2;
    if (cl == 0 && blockIdx.y == 0) stats[(long)gridDim.x * C * 2 + blockIdx.x] = Nn;
  }
}

// ---------------- sum over a sub-box of an NDHWC tensor (ConvT bias grad) ----------
// Block: 256 threads = (256 / CG) voxel lanes x CG groups of VEC channels; 16-byte loads,
// LDS reduce over voxel lanes, one partial row [C] per block (summed in block order by
// rows_sum_kernel: no atomics, run-to-run reproducible).
template <typename T>
__global__ void __launch_bounds__(TPB) box_channel_sum_kernel(const T* x, float* part, int N, int D, int H, int W,
                                                              int C, int z0, int y0, int x0, int bd, int bh, int bw) {
  constexpr int VEC = Elem<T>::kVec;
  __shared__ float red[TPB * VEC];
  const int CG = C / VEC;
  const int cg = threadIdx.x % CG, vl = threadIdx.x / CG, VL = TPB / CG;
  const long nv = (long)N * bd * bh * bw;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  const long stride = (long)gridDim.x * VL;
  long i = (long)blockIdx.x * VL + vl;
  if (bd == D && bh == H && bw == W) {
    // the box is the whole grid (no pad): voxel i is row i; four rows' loads in flight per
    // trip, added in the same order as one at a time
    for (; i + 3 * stride < nv; i += 4 * stride) {
      float v[4][VEC];
#pragma unroll
      for (int u = 0; u < 4; ++u) load16<T>(x + (i + u * stride) * C + cg * VEC, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += v[u][j];
    }
  }
  for (; i < nv; i += stride) {
    const uint32_t ii = (uint32_t)i;  // 32-bit index decomposition (host: nv < 2^31)
    const int w = ii % bw; uint32_t r = ii / bw;
    const int h = r % bh; r /= bh;
    const int d = r % bd; const long n = r / bd;
    float v[VEC];
    load16<T>(x + (((n * D + z0 + d) * H + y0 + h) * W + x0 + w) * C + cg * VEC, v);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[vl * C + cg * VEC + j] = acc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += TPB) {
    float s = 0.f;
    for (int l = 0; l < VL; ++l) s += red[l * C + c];
    part[(long)blockIdx.x * C + c] = s;
  }
}

// out[c] += sum_r part[r][c] in a fixed order (deterministic).  Block = 8 columns x 32 row
// lanes: lane l sums rows l, l + 32, ... (4 independent chains); the 32 lane sums are
// added by a fixed LDS tree.
// ACC: out[c] += the column sum (false: out[c] = it -- no zero fill of out first)
template <bool ACC>
__global__ void __launch_bounds__(256) rows_sum_kernel(const float* part, int rows, int C, float* out) {
  __shared__ float red[32][9];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    int r = rl;
    for (; r + 96 < rows; r += 128) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += part[(long)(r + 32 * j) * C + c];
    }
    for (int j = 0; r < rows; r += 32, ++j) s[j & 3] += part[(long)r * C + c];
  }
  red[rl][cl] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (rl < w) red[rl][cl] += red[rl + w][cl];
    __syncthreads();
  }
  if (rl == 0 && c < C) out[c] = ACC ? out[c] + red[0][cl] : red[0][cl];
}

}  // namespace

int rows_sum_launch(bool acc, const float* part, int rows, int C, float* out, hipStream_t s) {
  return for_policy(acc, [&](auto a) {
    hipLaunchKernelGGL(rows_sum_kernel<decltype(a)::value>, dim3(cdiv(C, 8)), dim3(256), 0, s, part, rows, C, out);
    PCMS_CHECK_LAUNCH();
  });
}

extern "C" {

int pcms_pack_input(int dtype, const float* in, void* out, int N, int Cin, long V, int Cp, hipStream_t s) {
  const bool quads = Cp == 8 && Cin <= 8 && V % 4 == 0 && !misaligned(in, 16) && !misaligned(out, 16);
  // quads: ~one quad per thread, every load in flight at once
  const int grid = quads ? stream_grid((long)N * V / 4, TPB, 16 * 256) : stream_grid((long)N * V, TPB);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    if (quads) hipLaunchKernelGGL(pack_input4_kernel<T>, dim3(grid), dim3(TPB), 0, s, in, (T*)out, N, Cin, V);
    else hipLaunchKernelGGL(pack_input_kernel<T>, dim3(grid), dim3(TPB), 0, s, in, (T*)out, N, Cin, V, Cp);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_unpack_output(int dtype, const void* in, float* out, int N, int C, int Cs, long V, hipStream_t s) {
  if (C > Cs) return -1;
  const int grid = stream_grid((long)N * C * V, TPB);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(unpack_output_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)in, out, N, C, Cs, V);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_add(int dtype, void* dst, const void* src, long n, hipStream_t s) {
  if (n % vec_of(dtype)) return -1;
  const long nvec = n / vec_of(dtype);
  const int grid = stream_grid(nvec, TPB);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(add_kernel<T>, dim3(grid), dim3(TPB), 0, s, (T*)dst, (const T*)src, nvec);
    PCMS_CHECK_LAUNCH();
  });
}

int pcms_split_epilogue_rows(long nvox) { return cdiv(nvox, 64); }

int pcms_split_epilogue(int dtype, const float* acc, int splits, const float* bias, void* y0, void* y1, int cy0,
                        float* stats, int C, long nvox, int flags, hipStream_t s) {
  if (C % 64 || splits < 1) return -1;
  if (flags & ~PCMS_CONV_RELU || (stats && flags)) return -8;
  const int relu = flags & PCMS_CONV_RELU;
  if (y1 == nullptr) cy0 = C;
  const dim3 grid(cdiv(nvox, 64), C / 64);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(split_epilogue_kernel<T>, grid, dim3(kSeThreads), 0, s, acc, splits, bias, (T*)y0, (T*)y1, cy0,
                       stats, C, nvox, relu);
    PCMS_CHECK_LAUNCH();
  });
}

static int box_sum_rows(int dtype, int N, int C, int bd, int bh, int bw) {
  const int VL = TPB / (C / vec_of(dtype));
  return stream_grid((long)N * bd * bh * bw, VL * 8, 1024);
}
int pcms_box_channel_sum_ws_floats(int dtype, int N, int C, int bd, int bh, int bw) {
  return box_sum_rows(dtype, N, C, bd, bh, bw) * C;
}

int pcms_box_channel_sum(int dtype, const void* x, float* out, float* ws, int N, int D, int H, int W, int C,
                         int z0, int y0, int x0, int bd, int bh, int bw, hipStream_t s) {
  if ((long)N * D * H * W >= (1L << 31)) return -7;  // 32-bit index math in the kernel
  const int VEC = vec_of(dtype);
  if (C % VEC || TPB % (C / VEC)) return -1;
  if (ws == nullptr) return -2;
  const int grid = box_sum_rows(dtype, N, C, bd, bh, bw);
  return for_storage(dtype, [&](auto t) {
    using T = decltype(t);
    PCMS_LAUNCH(box_channel_sum_kernel<T>, dim3(grid), dim3(TPB), 0, s, (const T*)x, ws, N, D, H, W, C, z0, y0, x0, bd,
                bh, bw);
    return rows_sum_launch(true, ws, grid, C, out, s);
  });
}

}  // extern "C"
