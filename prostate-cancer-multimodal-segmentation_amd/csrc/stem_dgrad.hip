// Input gradient of the stem conv (inc.conv.0: Conv3d(n_modalities, 64, k=3, padding=1),
// models/unet3d.py:29; aten convolution_backward's grad_input in the reference):
//   dx[n][ci][d][h][w] = sum_{co < 64, kd, kh, kw} dy[n][d+1-kd][h+1-kh][w+1-kw][co] W[co][ci][kd][kh][kw]
// dy NDHWC (64 channels, storage type), dx fp32 NCDHW [N][cin_w][D][H][W], written once per
// element with plain stores (no zero fill, no atomics: two runs give the same bits).
//
// bf16: the gather formulation on v_mfma_f32_16x16x32_bf16 with the weights as the A operand
// (M = 8 input channels padded to 16 rows, K = 27 taps x 64 co) and 16 consecutive w voxels as
// the B columns, so the accumulator tile is [ci][w] and every ci row is one 64-byte run of the
// NCDHW output.  A 256-thread workgroup walks 4 x 4 x 16 boxes (persistent grid), one wave per
// d-plane, four h-rows (accumulator tiles) per wave: the 6 x 6 x 18 dy halo sits in LDS
// (144-byte voxel pitch: the 16 lanes of a B read hit 16 different 4-bank groups), the next
// box's halo is fetched into registers while the MFMAs of this one run, and each lane keeps
// its 54 weight fragments in registers for the whole grid.  The kernel is bound by its LDS
// reads, so a B fragment -- one halo row at one kw shift -- is read once and feeds the up to
// three (kh, h-row) pairs that use it (108 reads for 216 MFMAs per wave and box), and the reads
// run one group of three ahead of their MFMAs (one wave per SIMD: nothing else hides the LDS
// latency).  Every load
// and store is predicated on the volume, so any N, D, H, W >= 1 runs here.
// fp32: one thread per voxel, plain fmaf in a fixed tap / channel order (the parity build).
#include "conv_common.h"
#include "pcms_hip.h"

namespace {

constexpr int kDGPackElems = 27 * 64 * 8;  // both forms: 27 taps x 64 co x 8 ci

// bf16 form: [tap][ks 2][kg 4][ci 8][j 8] = W[co = 32 ks + 8 kg + j][ci][tap] -- lane (ci, kg)
// of the A operand of k-step (tap, ks) reads its 8 values as one 16-byte row.
// fp32 form: [tap][co][ci 8].  Input channels past cin_w are zero.
template <typename T>
__global__ void stem_dgrad_pack_kernel(const float* w, T* out, int cin_w) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= kDGPackElems) return;
  int tap, co, ci;
  if constexpr (sizeof(T) == 2) {
    const int j = e & 7, kg = (e >> 6) & 3, ks = (e >> 8) & 1;
    ci = (e >> 3) & 7;
    tap = e >> 9;
    co = ks * 32 + kg * 8 + j;
  } else {
    ci = e & 7;
    co = (e >> 3) & 63;
    tap = e >> 9;
  }
  const float v = ci < cin_w ? w[((long)co * cin_w + ci) * 27 + tap] : 0.f;
  out[e] = Elem<T>::cvt(v);
}

// ---------------------------------------------------------------- bf16: MFMA gather
constexpr int kDGBD = 4, kDGBH = 4, kDGBW = 16;                // output box
constexpr int kDGHH = kDGBH + 2, kDGHW = kDGBW + 2;            // halo plane
constexpr int kDGHVox = (kDGBD + 2) * kDGHH * kDGHW;           // 648 halo voxels
constexpr int kDGPitch = 144;                                  // bytes per halo voxel (128 + 16)
constexpr int kDGHaloBytes = kDGHVox * kDGPitch;               // 93312
constexpr int kDGLds = kDGHaloBytes;                           // one workgroup per CU
constexpr int kDGThr = 256;                                    // one wave per box d-plane
constexpr int kDGChunks = kDGHVox * 8;                         // 16-byte pieces of one halo
constexpr int kDGPer = (kDGChunks + kDGThr - 1) / kDGThr;      // 21 per thread
static_assert(kDGLds <= 160 * 1024, "LDS");

__device__ __forceinline__ f32x4_t dg_mfma(u32x4_t a, u32x4_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                 0, 0, 0);
}

struct DGBox {
  int n, d0, h0, w0;
};
// Boxes are numbered d fastest, then w, h, n, and a workgroup walks one contiguous range of
// them: a column of d-adjacent boxes, whose two shared halo planes it staged itself one box
// earlier, then the next column.  Dispatch is round-robin over the 8 XCDs (workgroup i on XCD
// i % 8, each with its own L2), so the workgroups of one XCD take neighbouring ranges: the halo
// rows shared with the w / h neighbour column are fetched by the same XCD at about the same time.
__device__ __forceinline__ DGBox dg_box(int box, int nbd, int nbh, int nbw) {
  DGBox b;
  b.d0 = (box % nbd) * kDGBD;
  box /= nbd;
  b.w0 = (box % nbw) * kDGBW;
  box /= nbw;
  b.h0 = (box % nbh) * kDGBH;
  b.n = box / nbh;
  return b;
}

// the thread's 21 pieces of the halo of box ``bx`` into registers (zeros outside the volume)
__device__ __forceinline__ void dg_fetch(const bf16_t* dy, const DGBox& bx, int D, int H, int W, u32x4_t (&r)[kDGPer]) {
#pragma unroll
  for (int i = 0; i < kDGPer; ++i) {
    const int c = threadIdx.x + i * kDGThr;
    const int hv = c >> 3, part = c & 7;
    const int hd = hv / (kDGHH * kDGHW), rem = hv % (kDGHH * kDGHW);
    const int d = bx.d0 - 1 + hd, h = bx.h0 - 1 + rem / kDGHW, w = bx.w0 - 1 + rem % kDGHW;
    const bool ok = c < kDGChunks && (unsigned)d < (unsigned)D && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const u32x4_t*>(dy + ((((long)bx.n * D + d) * H + h) * W + w) * 64 + part * 8);
    r[i] = v;
  }
}

__global__ void __launch_bounds__(kDGThr, 1) stem_dgrad_mfma_kernel(const bf16_t* dy, const bf16_t* wpack, float* dx,
                                                                    int N, int D, int H, int W, int cin_w, int nbd,
                                                                    int nbh, int nbw, int nbox) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* halo = smem;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = lane & 15, kg = lane >> 4;
  // the lane's A fragments, k-step (tap, ks): rows 8-15 of the A tile have no input channel
  u32x4_t afr[54];
#pragma unroll
  for (int k = 0; k < 54; ++k) {
    afr[k] = u32x4_t{0u, 0u, 0u, 0u};
    if (col < 8) afr[k] = reinterpret_cast<const u32x4_t*>(wpack)[(k * 4 + kg) * 8 + col];
  }
  u32x4_t r[kDGPer];
  const int G = gridDim.x;
  const int lg = (G & 7) == 0 ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  int box = (int)((long)lg * nbox / G);
  const int end = (int)((long)(lg + 1) * nbox / G);
  if (box < end) dg_fetch(dy, dg_box(box, nbd, nbh, nbw), D, H, W, r);
  for (; box < end; ++box) {
    const DGBox bx = dg_box(box, nbd, nbh, nbw);
    __syncthreads();  // the previous box's MFMAs have read the halo
#pragma unroll
    for (int i = 0; i < kDGPer; ++i) {
      const int c = threadIdx.x + i * kDGThr;
      if (c < kDGChunks) *reinterpret_cast<u32x4_t*>(halo + (c >> 3) * kDGPitch + (c & 7) * 16) = r[i];
    }
    __syncthreads();
    if (box + 1 < end) dg_fetch(dy, dg_box(box + 1, nbd, nbh, nbw), D, H, W, r);  // in flight beside the MFMAs
    const int d = bx.d0 + wv;
    if (d >= D) continue;  // (wave-uniform; the barriers are at the loop head)
    f32x4_t acc[kDGBH];
#pragma unroll
    for (int t = 0; t < kDGBH; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // dy at (d + 1 - kd, h + 1 - kh, w + 1 - kw); the halo starts at (d0 - 1, h0 - 1, w0 - 1):
    // halo row (wv + 2 - kd, hh) at shift kw serves h-row t = hh - 2 + kh of tap (kd, kh, kw).
    // Group g = (kd, hh, ks): its three kw fragments are read one group ahead of the MFMAs that
    // use them (one wave per SIMD: nothing else hides the LDS latency)
    const unsigned char* hb = halo + ((wv + 2) * kDGHH * kDGHW + col + 2) * kDGPitch + kg * 16;
    auto ldb = [&](int g, u32x4_t (&b)[3]) {
      const int kd = g / 12, hh = (g / 2) % kDGHH, ks = g & 1;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        b[kw] = *reinterpret_cast<const u32x4_t*>(hb + ((hh - kd * kDGHH) * kDGHW - kw) * kDGPitch + ks * 64);
    };
    u32x4_t bq[2][3];
    ldb(0, bq[0]);
#pragma unroll
    for (int g = 0; g < 36; ++g) {
      if (g + 1 < 36) ldb(g + 1, bq[(g + 1) & 1]);
      const int kd = g / 12, hh = (g / 2) % kDGHH, ks = g & 1;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int t = hh - 2 + kh;
          if (t >= 0 && t < kDGBH) acc[t] = dg_mfma(afr[(((kd * 3 + kh) * 3 + kw) << 1) + ks], bq[g & 1][kw], acc[t]);
        }
    }
    // accumulator (lane, i) = dx[ci = 4 (lane >> 4) + i][w = w0 + (lane & 15)]
    const int w = bx.w0 + col;
    const long V = (long)D * H * W;
#pragma unroll
    for (int t = 0; t < kDGBH; ++t) {
      const int h = bx.h0 + t;
      if (h >= H || w >= W) continue;
      float* o = dx + (long)bx.n * cin_w * V + ((long)d * H + h) * W + w;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ci = kg * 4 + i;
        if (ci < cin_w) o[ci * V] = acc[t][i];
      }
    }
  }
}

// ---------------------------------------------------------------- fp32 (and any T): plain fmaf
constexpr int kDPThr = 256;
constexpr int kDPLds = kDGPackElems * 4;  // 55296: the fp32 weights [tap][co][8]

template <typename T>
__global__ void __launch_bounds__(kDPThr) stem_dgrad_plain_kernel(const T* dy, const float* wpack, float* dx, int N,
                                                                  int D, int H, int W, int cin_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wl = reinterpret_cast<float*>(smem);
  for (int i = threadIdx.x; i < kDGPackElems / 4; i += kDPThr)
    reinterpret_cast<f32x4_t*>(wl)[i] = reinterpret_cast<const f32x4_t*>(wpack)[i];
  __syncthreads();
  constexpr int VEC = Elem<T>::kVec;
  const long V = (long)D * H * W, total = (long)N * V;
  for (long v = (long)blockIdx.x * kDPThr + threadIdx.x; v < total; v += (long)gridDim.x * kDPThr) {
    const int n = (int)(v / V);
    const long r = v % V;
    const int w = (int)(r % W), h = (int)((r / W) % H), d = (int)(r / ((long)W * H));
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int tap = 0; tap < 27; ++tap) {
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      const int dd = d + 1 - kd, hh = h + 1 - kh, ww = w + 1 - kw;
      if ((unsigned)dd >= (unsigned)D || (unsigned)hh >= (unsigned)H || (unsigned)ww >= (unsigned)W) continue;
      const T* g = dy + ((((long)n * D + dd) * H + hh) * W + ww) * 64;
      const float* wt = wl + tap * 64 * 8;
      for (int c0 = 0; c0 < 64; c0 += VEC) {
        float gv[VEC];
        load16<T>(g + c0, gv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const f32x4_t w0 = *reinterpret_cast<const f32x4_t*>(wt + (c0 + k) * 8);
          const f32x4_t w1 = *reinterpret_cast<const f32x4_t*>(wt + (c0 + k) * 8 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] = __builtin_fmaf(gv[k], w0[j], acc[j]);
            acc[4 + j] = __builtin_fmaf(gv[k], w1[j], acc[4 + j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < cin_w) dx[((long)n * cin_w + j) * V + r] = acc[j];
  }
}

}  // namespace

extern "C" {

int pcms_stem_dgrad_pack_elems(int dtype) { return dtype == PCMS_BF16 || dtype == PCMS_F32 ? kDGPackElems : -1; }

int pcms_stem_dgrad_pack(int dtype, const float* w, void* out, int cin_w, hipStream_t s) {
  if (cin_w < 1 || cin_w > 8 || (dtype != PCMS_BF16 && dtype != PCMS_F32)) return -1;
  if (w == nullptr || out == nullptr) return -2;
  const int grid = cdiv(kDGPackElems, 256);
  if (dtype == PCMS_BF16) hipLaunchKernelGGL(stem_dgrad_pack_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, w, (bf16_t*)out, cin_w);
  else hipLaunchKernelGGL(stem_dgrad_pack_kernel<float>, dim3(grid), dim3(256), 0, s, w, (float*)out, cin_w);
  PCMS_CHECK_LAUNCH();
}

int pcms_stem_dgrad(int dtype, const void* dy, const void* wpack, float* dx, int N, int D, int H, int W, int cin_w,
                    hipStream_t s) {
  if (cin_w < 1 || cin_w > 8 || N < 1 || D < 1 || H < 1 || W < 1 || (dtype != PCMS_BF16 && dtype != PCMS_F32)) return -1;
  if (dy == nullptr || wpack == nullptr || dx == nullptr) return -2;
  const long nvox = (long)N * D * H * W;
  if (nvox * 64 * (dtype == PCMS_BF16 ? 2 : 4) >= (1L << 31)) return -7;  // the kernels' 2 GiB buffer bound
  if (dtype == PCMS_BF16) {
    const int nbd = cdiv(D, kDGBD), nbh = cdiv(H, kDGBH), nbw = cdiv(W, kDGBW);
    const long nbox = (long)N * nbd * nbh * nbw;
    const int grid = (int)std::min<long>(nbox, device_cus());
    (void)hipFuncSetAttribute((const void*)stem_dgrad_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDGLds);
    hipLaunchKernelGGL(stem_dgrad_mfma_kernel, dim3(grid), dim3(kDGThr), kDGLds, s, (const bf16_t*)dy,
                       (const bf16_t*)wpack, dx, N, D, H, W, cin_w, nbd, nbh, nbw, (int)nbox);
  } else {
    const int grid = (int)std::max<long>(1, std::min<long>(cdiv(nvox, kDPThr), 8L * device_cus()));
    (void)hipFuncSetAttribute((const void*)stem_dgrad_plain_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kDPLds);
    hipLaunchKernelGGL(stem_dgrad_plain_kernel<float>, dim3(grid), dim3(kDPThr), kDPLds, s, (const float*)dy,
                       (const float*)wpack, dx, N, D, H, W, cin_w);
  }
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
