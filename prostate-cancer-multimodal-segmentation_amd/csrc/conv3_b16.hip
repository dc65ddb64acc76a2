// 3x3x3 convolution, the persistent big-box forward / dgrad kernel on 16x16x32 MFMAs
// (pcms_conv3_fwd16 and its split-K form), NDHWC, gfx950.
#include "common.h"
#include "pcms_hip.h"
#include <algorithm>
#include <type_traits>
#include <utility>

#include "conv_common.h"
#include "conv3_bigbox.h"
#include "conv3_units.h"

namespace {

// ------------------------------------------------------------------------------------
// Big-box forward / dgrad on v_mfma_f32_16x16x32_bf16 (round 5; pcms_conv3_fwd16).  The same
// persistent 8-wave workgroup, 8 x 8 x 16 boxes, 16-channel chunks and LDS-DMA halo pipeline
// as conv3_fwd_big_kernel, with the MFMA shape changed: K = 32 = a PAIR of taps x 16 channels
// (lanes 0-31 of a fragment hold tap 2 s, lanes 32-63 tap 2 s + 1; 14 k-steps per chunk, the
// 28th tap a zero weight), wave w = box d-plane w: 8 M-tiles (its 8 h-rows of 16 voxels) x 4
// N-tiles (all 64 output channels), so per k-step 8 A reads + 4 B loads feed 32 MFMAs -- half
// the A bytes per FLOP of the 32x32x16 kernel.  Why: the big-box convs run power-capped
// (1.4-1.9 GHz in step, profiles/r5_layer_times_clock.json), and this inner loop does the same
// FLOPs for ~11 % less time on every CU at once (tests/kexp/mfma_shape.hip:
// profiles/r5_mfma_shape_probe.txt: 1505-1529 vs 1358-1370 TFLOP/s, at 2.00-2.06 vs 1.90-1.94
// GHz).  Halo rows stay 32 B (16 channels) without a swizzle: a 16-lane ds_read_b128 group reads
// rows {0-3, 12-15} of one half and {4-11} of the other, all 64 banks once.  B fragments come
// from the pack16 layout (pack16_off: one contiguous 1 KiB per (chunk, tap pair, 16-channel
// tile)).  Epilogue: each wave stages one M-tile at a time (16 voxels x 64 channels, 144-B rows)
// in its own LDS slice -- no cross-wave barrier -- and writes whole 128-B channel rows.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4_t mfma16(s16x8_t a, s16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                 0, 0, 0);
}
// A/B builds: bit 1 s_setprio 1 for the 8-deep kernel (bit 0: the weight gradient, conv3_wgrad.hip;
// MI355X_MICROARCH.md, two waves per SIMD item 4); 0 in the product
#ifndef PCMS_SETPRIO
#define PCMS_SETPRIO 0
#endif
// (kB6Steps, the tap pairs per chunk, and pack16_off: conv3_bigbox.h)
// B prefetch distance (k-steps; (Dist + 1) | 14 so the ring index continues across chunks): 1
// with two waves per SIMD (8-deep boxes), 6 with one (4-deep: the other wave no longer covers
// a weight fetch that misses L2)
#ifndef B6_DIST4
#define B6_DIST4 6  // (A/B builds: -DB6_DIST4=1)
#endif
// NT = 8 (128 output channels per wave, 256 accumulators: one wave per SIMD only) keeps two
// register sets, Dist 1
template <int BD, int NT = 4> constexpr int b6_dist() { return BD == 8 || NT == 8 ? 1 : B6_DIST4; }
// geometry of a box of BD d-planes (one wave each): 8 (levels 0-1) or 4 (level 2, whose 8-deep
// boxes would leave half the CUs idle; and, with NT = 8 N-tiles per wave, the 128-channel
// blocks of levels 0-1: one staged halo feeds twice the MFMAs).  pieces pc = tid + T j; the
// wave-instructions wholly past the halo's 2 Halo pieces aim at a 1 KiB dummy slot
// (out-of-range source: no memory traffic) so every wave issues the same count; a buffer
// holds rows up to the last real piece.  Epilogue slice rows: NT x 16 channels bf16 + 16 B
// (conflict-free 2-B writes), 16 rows (one M-tile) per wave.
template <int BD, int NT = 4> struct B6G {
  static constexpr int T = BD * 64;
  static constexpr int CO = NT * 16;                                    // channels per workgroup
  static constexpr int Halo = (BD + 2) * kBgHH * kBgHW;                 // rows x 32 B
  static constexpr int Pieces = (2 * Halo + T - 1) / T;                 // DMA pieces / thread
  static constexpr int Buf = (2 * Halo + 63) / 64 * 1024;
  static constexpr int Row = CO * 2 + 16;
  static constexpr int Slice = 16 * Row;
  static constexpr int EpiStores = 8 * NT / 2;                          // 16-B stores per wave and box
  static constexpr int SliceOff = 2 * Buf + kBgDummy;
  static constexpr int RedOff = SliceOff + BD * Slice;
  static constexpr int Lds = RedOff + BD * CO * 3 * 4 + CO * 4;         // + bias
  static constexpr int BnOff = Lds;
  static constexpr int LdsBn = Lds + 2 * kBgBnMax * 4;
  // split-K form (fp32 partial rows): its own slice of 16 rows x CO fp32 (+ 16 B) per wave
  static constexpr int Row32 = CO * 4 + 16;
  static constexpr int LdsSplit = SliceOff + BD * 16 * Row32;
  static constexpr int EpiStores32 = 8 * CO / 16;                       // 16-B stores per wave and box
  static_assert(LdsSplit <= 160 * 1024, "LDS");
  static_assert(Pieces <= kB6Steps, "one piece per k-step");
  static_assert((Pieces - 2) * T + (BD - 1) * 64 < 2 * Halo, "dummy pieces in the last round only");
  static_assert(LdsBn <= 160 * 1024, "LDS");
};
static_assert(B6G<8>::Buf == kBgBuf && B6G<8>::Pieces == kBgPieces, "8-deep geometry");
static_assert(B6G<8>::Row == 144 && B6G<8>::EpiStores == 16, "64-channel slice rows");

// box w width WB: 16 (levels 0-2: an M-tile is one h-row of 16 w) or 8 (level 3: an M-tile is
// two h-rows of 8 w); the box is BD d-planes x (128 / WB) h x WB w, its halo plane HH x HW
// rows (10 x 18 or 18 x 10: 180 rows either way)
template <int WB> struct B6W {
  static constexpr int BH = 128 / WB, HH = BH + 2, HW = WB + 2;
  static constexpr int MTR = (16 / WB) * HW;  // halo rows between M-tiles
};
static_assert(B6W<16>::HH == kBgHH && B6W<16>::HW == kBgHW && B6W<8>::HH * B6W<8>::HW == kBgHH * kBgHW, "halo");
// halo row offset of tap t; the zero-weight 28th tap reads tap 26's rows
template <int WB = 16> __host__ __device__ constexpr int b6_tapoff(int t) {
  return t > 26 ? b6_tapoff<WB>(26) : ((t / 9) * B6W<WB>::HH + (t / 3) % 3) * B6W<WB>::HW + t % 3;
}
// retire the hidden loads of the B fragments of a step (and everything issued before)
template <int N> __device__ __forceinline__ void vm_wait4(s16x8_t (&b)[4]) {
  static_assert(N >= 0 && N <= 63, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void vm_wait4(s16x8_t (&b)[8]) {
  static_assert(N >= 0 && N <= 63, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7])
               : "n"(N) : "memory");
}
template <int P> constexpr int b6_piece(int s) { return ((s % kB6Steps) + kB6Steps) % kB6Steps < P ? 1 : 0; }
// vector-memory ops issued after the last of B(t)'s NT loads by the time step t waits for it:
// every step u issues B(u + D) (NT loads) then piece(u) (u < P)
template <int P, int Dist, int NT = 4> constexpr int b6_wait(int t) {
  int n = b6_piece<P>(t - Dist);
  for (int u = t - Dist + 1; u <= t; ++u) n += NT + b6_piece<P>(u);
  return n;
}

// WB: box w width (B6W).  SPLIT (level 3): the workgroups of a (slot, co block) cover 1 / nsplit of
// the input chunks each (p.chunks_per_split) and write fp32 partial rows p.yacc[split][vox][co]
// (no bias / statistics: pcms_split_epilogue sums the splits in a fixed order)
template <bool BNIN = false, int BD = 8, int NT = 4, int WB = 16, bool SPLIT = false>
__global__ void __launch_bounds__(BD * 64, 1) conv3_fwd_b16_kernel(Conv3Params p, uint32_t x0bytes,
                                                                  uint32_t x1bytes) {
  typedef B6G<BD, NT> G6;
  typedef B6W<WB> GW;
  static_assert(NT == 4 || (NT == 8 && BD == 4), "128-channel blocks: one wave per SIMD");
  static_assert(!SPLIT || (!BNIN && NT == 4), "split-K form: plain 64-channel blocks");
  constexpr int CO = G6::CO;
  // kT (64-channel blocks): the MFMA runs weights x activations, so a lane's accumulator holds
  // 4 consecutive output channels of one voxel (channel-major D) -- the epilogue stores them
  // straight from registers (8 B of bf16, or 16 B of fp32 partial rows) instead of transposing
  // through the LDS slice
  constexpr bool kT = NT == 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if PCMS_SETPRIO & 2
  if (BD == 8 && wave >= 4) __builtin_amdgcn_s_setprio(1);  // the younger wave of each SIMD pair
#endif
  const int Cout = p.Cout, ncob = Cout / CO;
  const int G = gridDim.x;
  const int lg = (G & 7) == 0 ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int nsplit = SPLIT ? p.nchunk / p.chunks_per_split : 1;
  const int cob = lg % ncob, split = SPLIT ? (lg / ncob) % nsplit : 0;
  const int slot = lg / ncob / nsplit, nslot = G / ncob / nsplit;
  const int nbox = p.N * p.nbd * p.nbh * p.nbw;
  const int co_base = cob * CO;
  auto origin = [&](int box, int& n, int& d0, int& h0, int& w0) {
    int q = box;
    const int bwi = q % p.nbw; q /= p.nbw;
    const int bhi = q % p.nbh; q /= p.nbh;
    const int bdi = q % p.nbd;
    n = q / p.nbd;
    d0 = bdi * BD; h0 = bhi * GW::BH; w0 = bwi * WB;
  };
  const i32x4_t xr0 = buffer_desc(p.x0, x0bytes);
  const i32x4_t xr1 = buffer_desc(p.x1 ? p.x1 : p.x0, x1bytes);
  const uint32_t lds0 = lds_addr(lds);
  // halo piece j of this thread: row pc / 2 (32 B), 16-B half pc & 1 (channels 8 half ..),
  // no swizzle; live = false: still issued (the vmcnt arithmetic), reads out of range = zeros.
  // The piece's voxel (pvox, -1 outside the volume) depends on the box only: formed when a
  // box's first chunk is staged (fresh) and reused for its other chunks (one multiply-add then);
  // 4-deep boxes only (one wave per SIMD: registers to spare; the 8-deep kernel spills with it)
  constexpr bool kCache = BD == 4;
  int pvox[kCache ? G6::Pieces : 1];
  auto stage_piece = [&](int n, int d0, int h0, int w0, int chunk, int buf, int j, bool live, bool fresh) {
    const int c = chunk * 16;
    const bool first = c < p.c0;
    const uint32_t stride = first ? p.c0 : p.c1;
    const uint32_t cofs = first ? c : c - p.c0;
    const int pc = opaque(tid) + j * G6::T;
    uint32_t voff = kOOB;
    if constexpr (kCache) {
      if (fresh) {
        const int hv = pc >> 1;
        const int hw_ = hv % GW::HW, t_ = hv / GW::HW, hh_ = t_ % GW::HH, hd_ = t_ / GW::HH;
        const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
        pvox[j] = (hv < G6::Halo && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H &&
                   (unsigned)gw < (unsigned)p.W) ? ((n * p.D + gd) * p.H + gh) * p.W + gw : -1;
      }
      if (live && pvox[j] >= 0) voff = ((uint32_t)pvox[j] * stride + cofs + (uint32_t)(pc & 1) * 8u) * 2u;
    } else {
      (void)fresh;
      const int hv = pc >> 1;
      const int hw_ = hv % GW::HW, t_ = hv / GW::HW, hh_ = t_ % GW::HH, hd_ = t_ / GW::HH;
      const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
      if (live && hv < G6::Halo && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H &&
          (unsigned)gw < (unsigned)p.W)
        voff = ((uint32_t)(((n * p.D + gd) * p.H + gh) * p.W + gw) * stride + cofs + (uint32_t)(pc & 1) * 8u) * 2u;
    }
    const bool dummy = j == G6::Pieces - 1 && j * G6::T + wave * 64 >= 2 * G6::Halo;
    const uint32_t lb = __builtin_amdgcn_readfirstlane(
        dummy ? lds0 + 2 * G6::Buf : lds0 + buf * G6::Buf + (wave * 64 + j * G6::T) * 16);
    dma16(first ? xr0 : xr1, lb, dummy ? kOOB : voff, 0);
    return !dummy && voff != kOOB ? 1u << j : 0u;
  };
  float* bnt = reinterpret_cast<float*>(lds + G6::BnOff);
  auto bn_apply = [&](int buf, int chunk, uint32_t pm) {
#pragma unroll
    for (int j = 0; j < G6::Pieces; ++j) {
      if (!((pm >> j) & 1)) continue;
      const int pc = tid + j * G6::T;
      u32x4_t* q = reinterpret_cast<u32x4_t*>(lds + buf * G6::Buf + pc * 16);
      const int c = chunk * 16 + (tid & 1) * 8;  // piece pc = tid + T j: its half is tid & 1
      const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(bnt + c), s1 = *reinterpret_cast<const f32x4_t*>(bnt + c + 4);
      const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(bnt + kBgBnMax + c);
      const f32x4_t h1 = *reinterpret_cast<const f32x4_t*>(bnt + kBgBnMax + c + 4);
      const float sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
      const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      u32x4_t v = *q;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = pack_bf16x2(bn_relu1(__uint_as_float(v[i] << 16), sc[2 * i], sh[2 * i]),
                           bn_relu1(__uint_as_float(v[i] & 0xffff0000u), sc[2 * i + 1], sh[2 * i + 1]));
      *q = v;
    }
  };
  if constexpr (BNIN) {
    if (tid < p.Cin) { bnt[tid] = p.isc[tid]; bnt[kBgBnMax + tid] = p.ish[tid]; }
    __syncthreads();
  }

  // B: pack16, (16-chunk c, step s) rows of Cout / 16 fragments of 1 KiB; this wave's NT
  // N-tiles are the workgroup's CO channels: bases off (+ 4 KiB) + immediates 0-3 KiB
  const int nchunk = p.Cin >> 4;  // (the pack's chunk count; SPLIT: this split's [cbeg, cend))
  const int cbeg = split * (SPLIT ? p.chunks_per_split : 0), cend = SPLIT ? cbeg + p.chunks_per_split : nchunk;
  const uint32_t step_bytes = (uint32_t)Cout * 64u;
  const i32x4_t wr = buffer_desc(p.w, (uint32_t)nchunk * kB6Steps * step_bytes);
  auto load_b = [&](s16x8_t (&dst)[NT], int chunk, int st, uint32_t boff) {
    const uint32_t off = boff + (uint32_t)(chunk * kB6Steps + st) * step_bytes;
#pragma unroll
    for (int h = 0; h < NT / 4; ++h) {
      bload16<0>(dst[4 * h + 0], wr, off + h * 4096u);
      bload16<1024>(dst[4 * h + 1], wr, off + h * 4096u);
      bload16<2048>(dst[4 * h + 2], wr, off + h * 4096u);
      bload16<3072>(dst[4 * h + 3], wr, off + h * 4096u);
    }
  };

  float* red = reinterpret_cast<float*>(lds + G6::RedOff);  // [wave][CO][mean, M2, n]
  float* bls = red + BD * CO * 3;
  if (tid < CO) bls[tid] = p.bias ? p.bias[co_base + tid] : 0.f;
  // outputs per 64-channel half h of the block: y0 below cy0, y1 from it (the dgrad's two Up3D
  // sources; cy0 % 64 == 0)
  auto ydst = [&](int h, long& ys, int& yc0) {
    const int cb = co_base + 64 * h;
    const bool to0 = cb < p.cy0;
    ys = to0 ? p.cy0 : Cout - p.cy0;
    yc0 = to0 ? cb : cb - p.cy0;
    return __builtin_amdgcn_make_buffer_rsrc(to0 ? p.y0 : p.y1, (short)0, (int)(p.nvox * ys * 2), 0x00020000);
  };
  char* slice = lds + G6::SliceOff + wave * (SPLIT ? 16 * G6::Row32 : G6::Slice);
  int nbdone = 0;

  f32x4_t acc[8][NT];
  constexpr int kB6Dist = b6_dist<BD, NT>();
  static_assert(kB6Steps % (kB6Dist + 1) == 0, "B ring index must continue across chunks");
  s16x8_t bset[kB6Dist + 1][NT];
  int box = slot;
  int n, d0, h0, w0;
  origin(box, n, d0, h0, w0);
  if (cend - cbeg <= 4)
    for (int i = 0; i < 2 * (slot & 3); ++i) __builtin_amdgcn_s_sleep(127);
  uint32_t pmask = 0;
#pragma unroll
  for (int j = 0; j < G6::Pieces; ++j) pmask |= stage_piece(n, d0, h0, w0, cbeg, 0, j, true, true);
  {
    const uint32_t boff0 = (uint32_t)(cob * NT * 1024 + lane * 16);
#pragma unroll
    for (int t = 0; t < kB6Dist; ++t) load_b(bset[t], cbeg, t, boff0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (BNIN) bn_apply(0, 0, pmask);
  __syncthreads();
  int buf = 0;
  while (true) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int nbx = box + nslot;
    const bool has_next = nbx < nbox;
    int nn = n, nd0 = d0, nh0 = h0, nw0 = w0;
    if (has_next) origin(nbx, nn, nd0, nh0, nw0);
    auto run_chunk = [&](int chunk, auto slack_tag) {
      constexpr bool Slack = decltype(slack_tag)::value;
      const bool last = chunk + 1 == cend;
      const bool live = !last || has_next;
      const int sn = last ? nn : n, sd = last ? nd0 : d0, sh = last ? nh0 : h0, sw = last ? nw0 : w0;
      const int schunk = last ? cbeg : chunk + 1;
      const int lo = opaque(lane);
      const uint32_t boff = (uint32_t)(cob * NT * 1024 + lo * 16);
      // A: this lane's halo row base -- box voxel (d = wave, h = 0, w = r16), its channel half
      // (g4 & 1) -- plus the row offset of its tap of the pair (g4 >> 1); M-tile mt = h-row mt
      // is an immediate (mt x 18 rows)
      const int r16 = lo & 15;  // the lane's voxel of an M-tile: h-row r16 / WB, w r16 % WB
      const uint32_t abase = lds0 + buf * G6::Buf +
                             (uint32_t)(((wave * GW::HH + r16 / WB) * GW::HW + r16 % WB) * 32 + ((lo >> 4) & 1) * 16);
      const bool hi_tap = (lo >> 5) & 1;
      // A fragment of (step st, M-tile mt); fragments are read two M-tiles ahead of their four
      // MFMAs through a 3-register rotation, across step boundaries (a deeper, per-step rolling
      // set made the compiler double-buffer it into spills)
      auto rd = [&](int st, int mt) {
        const uint32_t ad = abase + (uint32_t)(hi_tap ? b6_tapoff<WB>(2 * st + 1) : b6_tapoff<WB>(2 * st)) * 32u;
        return *reinterpret_cast<const LDS_AS s16x8_t*>((const LDS_AS char*)(uintptr_t)ad + mt * GW::MTR * 32);
      };
      s16x8_t ar[3];
      ar[0] = rd(0, 0);
      ar[1] = rd(0, 1);
      static_for<kB6Steps>([&](auto sc) {
        constexpr int st = decltype(sc)::value;
        constexpr int sn_ = st + kB6Dist;
        if constexpr (sn_ < kB6Steps) load_b(bset[sn_ % (kB6Dist + 1)], chunk, sn_, boff);
        else load_b(bset[sn_ % (kB6Dist + 1)], schunk, sn_ - kB6Steps, boff);
        if constexpr (st < G6::Pieces) {
          const uint32_t bits = stage_piece(sn, sd, sh, sw, schunk, buf ^ 1, st, live, last);
          if constexpr (BNIN) pmask = (st == 0 ? 0u : pmask) | bits;
        }
        s16x8_t (&b)[NT] = bset[st % (kB6Dist + 1)];
        constexpr int extra = (Slack && st < kB6Dist) ? (SPLIT ? G6::EpiStores32 : G6::EpiStores) : 0;
        vm_wait4<b6_wait<G6::Pieces, kB6Dist, NT>(st) + extra>(b);
        static_for<8>([&](auto mc) {
          constexpr int mt = decltype(mc)::value;
          constexpr int q = st * 8 + mt + 2;  // the fragment read now: position q (two ahead)
          if constexpr (q < kB6Steps * 8) ar[q % 3] = rd(q / 8, q % 8);
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            if constexpr (kT) acc[mt][j] = mfma16(b[j], ar[(st * 8 + mt) % 3], acc[mt][j]);
            else acc[mt][j] = mfma16(ar[(st * 8 + mt) % 3], b[j], acc[mt][j]);
          }
        });
        // keep the order (1 read, NT MFMAs per M-tile) and every step's work in its step
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
          if (st * 8 + mt + 2 < kB6Steps * 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
          __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);  // NT MFMA
        }
        __builtin_amdgcn_sched_barrier(0);
      });
      if (!last) vm_wait<NT * (kB6Steps - G6::Pieces)>();
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (BNIN && (BG_ABL & 128) == 0) bn_apply(buf ^ 1, schunk, pmask);  // (128: ablation)
      __syncthreads();
      buf ^= 1;
    };
    run_chunk(cbeg, std::true_type{});
    for (int chunk = cbeg + 1; chunk < cend; ++chunk) run_chunk(chunk, std::false_type{});

    if constexpr (SPLIT) {
      // fp32 partial rows of this split: one M-tile at a time through the wave's slice (16 rows
      // of CO fp32), read back as whole 256-B voxel rows, 16-B stores
      const int lane_o = opaque(lane);
      const int rr = lane_o & 15, gg = lane_o >> 4;
      const long vbase = (((long)n * p.D + d0 + wave) * p.H + h0) * p.W + w0;
      const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(
          p.yacc, (short)0, (int)((long)nsplit * p.nvox * Cout * 4), 0x00020000);
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if constexpr (kT) {  // lane (gg, rr): voxel rr, channels 16 j + 4 gg .. + 3
            *reinterpret_cast<f32x4_t*>(slice + rr * G6::Row32 + (16 * j + 4 * gg) * 4) = acc[mt][j];
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              *reinterpret_cast<float*>(slice + (4 * gg + i) * G6::Row32 + (16 * j + rr) * 4) = acc[mt][j][i];
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < CO / 16; ++k) {
          const int q = lane_o + 64 * k, vw = q >> 4, c4 = q & 15;
          const u32x4_t v = *reinterpret_cast<const u32x4_t*>(slice + vw * G6::Row32 + c4 * 16);
          const long vox = vbase + (long)(mt * (16 / WB) + vw / WB) * p.W + vw % WB;
          __builtin_amdgcn_raw_buffer_store_b128(v, ar, (int)((((long)split * p.nvox + vox) * Cout + co_base + c4 * 4) * 4),
                                                 0, 0);
        }
      }
      if (!has_next) break;
      box = nbx;
      n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
      continue;
    }

    // ---- epilogue of this box: lane (g4, r16) holds, per (M-tile mt, N-tile j), voxels w =
    // 4 g4 + i (i < 4) of h-row mt, channel 16 j + r16.  One M-tile at a time through the wave's
    // own slice (16 rows of Row B): + bias, bf16; read back as whole 128-B half rows (NT / 2 x
    // 16 B per lane, each store instruction inside one 64-channel half), 16-B stores.
    // BatchNorm moments shifted by K (the running mean; the bias before the first box), per
    // channel over the wave's 128 voxels, Chan-merged per (wave, channel).
    if constexpr ((BG_ABL & 64) != 0) {  // ablation: no epilogue at all
#pragma unroll
      for (int mt = 0; mt < 8; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j) asm volatile("" ::"v"(acc[mt][j]));
      if (!has_next) break;
      box = nbx;
      n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
      continue;
    }
    if constexpr (kT) {
      // lane (gg, rr) holds, per (M-tile mt, N-tile j), voxel rr of h-row(s) mt and channels
      // 16 j + 4 gg + i (i < 4): + bias, bf16, one 8-B store.  BatchNorm moments shifted by K
      // (the running mean; the bias before the first box) summed over the lane's 8 M-tiles,
      // then over the 16 lanes of its DPP row (the wave's 128 voxels), Chan-merged per (wave,
      // channel) as below
      const int lane_o = opaque(lane);
      const int rr = lane_o & 15, gg = lane_o >> 4;
      const long vbase = (((long)n * p.D + d0 + wave) * p.H + h0) * p.W + w0;
      const bool relu = p.accumulate & PCMS_CONV_RELU;
      const bool want_stats = p.stats != nullptr;  // (the dgrads: none)
      long ys;
      int yc0;
      const auto yr = ydst(0, ys, yc0);
      const float rn = (float)nbdone * 128.f;
      constexpr float nb = 128.f;  // voxels per wave and box
      const float nnew = rn + nb;
      // statistics N-tile by N-tile (4 channels x 2 sums live), then the values M-tile by
      // M-tile through the wave's slice: one 8-B LDS write per (M-tile, N-tile), read back as
      // whole 128-B half rows for 16-B stores (register-direct 8-B stores touch 16 lines per
      // instruction and ran slower)
      float bias4[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) bias4[j][i] = bls[16 * j + 4 * gg + i];
      if (want_stats) {
        // per-lane shifted sums of its 16 channels (m = 4 j + i) over its 8 voxels, then a
        // reduce-scatter over the 16 lanes of the row (4 DPP stages, halving the values each
        // time): lane rr ends with channel m = rr summed over the row's 128 voxels, and merges
        // that one channel
        // (channel pairs in packed fp32: v_pk_add_f32 / v_pk_fma_f32, the same IEEE results)
        float S1[4 * NT], S2[4 * NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int c0 = 16 * j + 4 * gg + 2 * q;
            const float k0 = nbdone ? red[(wave * CO + c0) * 3] : bias4[j][2 * q];
            const float k1 = nbdone ? red[(wave * CO + c0 + 1) * 3] : bias4[j][2 * q + 1];
            const f32x2_t sh = {bias4[j][2 * q] - k0, bias4[j][2 * q + 1] - k1};
            f32x2_t s1 = {0.f, 0.f}, s2 = {0.f, 0.f};
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
              const f32x2_t e = (f32x2_t){acc[mt][j][2 * q], acc[mt][j][2 * q + 1]} + sh;
              s1 += e;
              s2 = __builtin_elementwise_fma(e, e, s2);
            }
            S1[4 * j + 2 * q] = s1[0];
            S1[4 * j + 2 * q + 1] = s1[1];
            S2[4 * j + 2 * q] = s2[0];
            S2[4 * j + 2 * q + 1] = s2[1];
          }
        }
        auto stage = [&](auto nc, auto ctl, bool hi) __attribute__((always_inline)) {
          constexpr int h = decltype(nc)::value / 2;
          constexpr int c = decltype(ctl)::value;
#pragma unroll
          for (int k = 0; k < h; ++k) {
            const float k1 = hi ? S1[h + k] : S1[k], t1 = hi ? S1[k] : S1[h + k];
            const float k2 = hi ? S2[h + k] : S2[k], t2 = hi ? S2[k] : S2[h + k];
            S1[k] = k1 + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t1), c, 0xf, 0xf, true));
            S2[k] = k2 + __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t2), c, 0xf, 0xf, true));
          }
        };
        static_assert(NT == 4, "16 channels per lane");
        stage(std::integral_constant<int, 16>{}, std::integral_constant<int, 0x140>{}, (rr & 8) != 0);  // 15 - r
        stage(std::integral_constant<int, 8>{}, std::integral_constant<int, 0x141>{}, (rr & 4) != 0);   // 7 - r
        stage(std::integral_constant<int, 4>{}, std::integral_constant<int, 0x4e>{}, (rr & 2) != 0);    // r ^ 2
        stage(std::integral_constant<int, 2>{}, std::integral_constant<int, 0xb1>{}, (rr & 1) != 0);    // r ^ 1
        const int ch = 16 * (rr >> 2) + 4 * gg + (rr & 3);
        float* rme = red + (wave * CO + ch) * 3;
        const float K = nbdone ? rme[0] : bls[ch];
        const float s1 = S1[0], s2 = S2[0];
        const float mbox = K + s1 / nb;
        const float m2b = fmaxf(s2 - s1 * s1 / nb, 0.f);
        const float rmean = nbdone ? rme[0] : 0.f, rm2 = nbdone ? rme[1] : 0.f;
        const float delta = mbox - rmean;
        rme[0] = rmean + delta * (nb / nnew);
        rme[1] = rm2 + m2b + delta * delta * (rn * nb / nnew);
        rme[2] = nnew;
      }
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          uint32_t o[2];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            f32x2_t a = (f32x2_t){acc[mt][j][2 * k], acc[mt][j][2 * k + 1]} +
                        (f32x2_t){bias4[j][2 * k], bias4[j][2 * k + 1]};
            if (relu) a = (f32x2_t){fmaxf(a[0], 0.f), fmaxf(a[1], 0.f)};
            o[k] = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, bf16x2_t));
          }
          *reinterpret_cast<u32x2_t*>(slice + rr * G6::Row + (16 * j + 4 * gg) * 2) = (u32x2_t){o[0], o[1]};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < NT / 2; ++k) {
          const int vw = (k * 64 + lane_o) >> 3, c8 = lane_o & 7;
          const u32x4_t v = *reinterpret_cast<const u32x4_t*>(slice + vw * G6::Row + c8 * 16);
          const long vox = vbase + (long)(mt * (16 / WB) + vw / WB) * p.W + vw % WB;
          if constexpr ((BG_ABL & 2) == 0)
            __builtin_amdgcn_raw_buffer_store_b128(v, yr, (int)((vox * ys + yc0 + c8 * 8) * 2), 0, 0);
          else
            asm volatile("" ::"v"(v), "v"((int)vox));
        }
      }
      ++nbdone;
      if (!has_next) break;
      box = nbx;
      n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
      continue;
    }
    const int lane_o = opaque(lane);
    const int rr = lane_o & 15, gg = lane_o >> 4;
    const long plane = (long)p.H * p.W;
    const long vbase = (((long)n * p.D + d0 + wave) * p.H + h0) * p.W + w0;
    const bool relu = p.accumulate & PCMS_CONV_RELU;
    float bias_j[NT], K0[NT], S1[NT], S2[NT];
    const float rn = (float)nbdone * 128.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bias_j[j] = bls[16 * j + rr];
      K0[j] = nbdone ? red[(wave * CO + 16 * j + rr) * 3] : bias_j[j];
      S1[j] = 0.f;
      S2[j] = 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v0 = acc[mt][j][i];
          if constexpr ((BG_ABL & 32) == 0)
            *reinterpret_cast<bf16_t*>(slice + (4 * gg + i) * G6::Row + (16 * j + rr) * 2) =
                f2bf(relu ? fmaxf(v0 + bias_j[j], 0.f) : v0 + bias_j[j]);
          else
            asm volatile("" ::"v"(v0));
          const float e0 = v0 + (bias_j[j] - K0[j]);
          S1[j] += e0;
          S2[j] = fmaf(e0, e0, S2[j]);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 0; k < NT / 2; ++k) {
        const int h = k >> 1, vw = ((k & 1) * 64 + lane_o) >> 3, c8 = lane_o & 7;
        long ys;
        int yc0;
        const auto yr = ydst(h, ys, yc0);
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(slice + vw * G6::Row + (h * 8 + c8) * 16);
        const long vox = vbase + (long)(mt * (16 / WB) + vw / WB) * p.W + vw % WB;
        if constexpr ((BG_ABL & 2) == 0)
          __builtin_amdgcn_raw_buffer_store_b128(v, yr, (int)((vox * ys + yc0 + c8 * 8) * 2), 0, 0);
        else
          asm volatile("" ::"v"(v), "v"((int)vox));
      }
      (void)plane;
    }
    {
      constexpr float nb = 128.f;  // voxels per wave and box
      const float nnew = rn + nb;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        float s1 = S1[j], s2 = S2[j];
        s1 += __shfl_xor(s1, 16, 64);
        s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        const float mbox = K0[j] + s1 / nb;
        const float m2b = fmaxf(s2 - s1 * s1 / nb, 0.f);
        float* rme = red + (wave * CO + 16 * j + rr) * 3;
        const float rmean = nbdone ? rme[0] : 0.f, rm2 = nbdone ? rme[1] : 0.f;
        const float delta = mbox - rmean;
        if (gg == 0) {
          rme[0] = rmean + delta * (nb / nnew);
          rme[1] = rm2 + m2b + delta * delta * (rn * nb / nnew);
          rme[2] = nnew;
        }
      }
      ++nbdone;
    }
    if (!has_next) break;
    box = nbx;
    n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
  }

  if (SPLIT || !p.stats) return;
  __syncthreads();
  if (tid < CO) {
    float S = 0.f, Nn = 0.f;
#pragma unroll
    for (int w = 0; w < BD; ++w) {
      S += red[(w * CO + tid) * 3] * red[(w * CO + tid) * 3 + 2];
      Nn += red[(w * CO + tid) * 3 + 2];
    }
    const float m = S / Nn;
    float M2 = 0.f;
#pragma unroll
    for (int w = 0; w < BD; ++w) {
      const float c = red[(w * CO + tid) * 3 + 2];
      const float d = red[(w * CO + tid) * 3] - m;
      M2 += red[(w * CO + tid) * 3 + 1] + c * d * d;
    }
    float* st = p.stats + ((long)slot * Cout + co_base + tid) * 2;
    st[0] = S;
    st[1] = M2;
    if (tid == 0 && cob == 0) p.stats[(long)nslot * Cout * 2 + slot] = Nn;
  }
}

}  // namespace

// ---- 16x16x32 big-box path (conv3_fwd_b16_kernel) ----
// box depth pcms_conv3_fwd16 runs a conv with: 8 where its 8-deep boxes (x 64-channel blocks)
// fill every CU (levels 0-1; level 2's 512-channel outputs), else 4 where 4-deep boxes do
// (level 2's 256-channel outputs: one wave per SIMD, profiles/r5_deep_ab.txt), else 0
static bool b16_shape_ok(int bd, int N, int D, int H, int W, int c0, int c1) {
  const long nvox = (long)N * D * H * W;
  return D % bd == 0 && H % 8 == 0 && W % 16 == 0 && c0 % 16 == 0 && c1 % 16 == 0 && c0 >= 16 &&
         nvox < (1L << 30) && nvox * std::max(c0, c1) * 2 < (long)kOOB;
}
struct B16Cfg { int bd, nt; };
// 128-channel blocks on 4-deep boxes (B6G<4, 8>) where Cout allows and they fill the CUs (A/B
// switch pcms_conv3_b16_nt8; off: 12-20 % slower than 64-channel blocks on 8-deep boxes at
// every level-0/1 shape despite a 5-12 % higher clock -- one wave per SIMD with 64 MFMAs per
// k-step cannot hide its B fetches, profiles/r5_nt8_ab.txt)
static int g_b16_nt8 = 0;
static B16Cfg b16_config(int N, int D, int H, int W, int c0, int c1, int Cout) {
  if (Cout % 64 || (long)N * D * H * W * Cout * 2 >= (long)kOOB) return {0, 0};
  const long nb8 = (long)N * (D / 8) * (H / 8) * (W / 16), nb4 = (long)N * (D / 4) * (H / 8) * (W / 16);
  const long ncob = Cout / 64;
  if (g_b16_nt8 && Cout % 128 == 0 && b16_shape_ok(4, N, D, H, W, c0, c1) && nb4 * (Cout / 128) >= big_min_boxes())
    return {4, 8};
  if (big_fwd_ok(PCMS_BF16, N, D, H, W, c0, c1)) return {8, 4};
  if (b16_shape_ok(8, N, D, H, W, c0, c1) && nb8 * ncob >= big_min_boxes()) return {8, 4};
  if (b16_shape_ok(4, N, D, H, W, c0, c1) && nb4 * ncob >= big_min_boxes()) return {4, 4};
  return {0, 0};
}
static int b16_slots(B16Cfg c, int N, int D, int H, int W, int Cout) {
  const int nbox = N * (D / c.bd) * (H / 8) * (W / 16);
  const int G = big_max_wgs() > 0 ? big_max_wgs() : device_cus();
  return std::max(1, std::min(nbox, G / (Cout / (16 * c.nt))));
}

extern "C" {

// 1 when pcms_conv3_fwd16 runs this conv (bf16, one split); the engine keeps a pack16 for
// such convs
int pcms_conv3_big16_ok(int N, int D, int H, int W, int c0, int c1, int Cout) {
  return b16_config(N, D, H, W, c0, c1, Cout).bd ? 1 : 0;
}
// 128-channel blocks of the 16x16x32 kernel on (1) or off (0); v < 0 queries; returns the
// previous setting (set before any workspace query: it changes pcms_conv3_fwd16_rows)
int pcms_conv3_b16_nt8(int v) {
  const int old = g_b16_nt8;
  if (v >= 0) g_b16_nt8 = v;
  return old;
}
// BatchNorm partial rows pcms_conv3_fwd16 writes for this conv (0: not a fwd16 shape)
int pcms_conv3_fwd16_rows(int N, int D, int H, int W, int c0, int c1, int Cout) {
  const B16Cfg c = b16_config(N, D, H, W, c0, c1, Cout);
  return c.bd ? b16_slots(c, N, D, H, W, Cout) : 0;
}
// y = conv(x) + bias on the 16x16x32 big-box kernel (wpack16 = a pcms_conv3_pack16 form);
// arguments as pcms_conv3_fwd with splits = 1; isc / ish != NULL: the input's BatchNorm + ReLU
// applied in the staging (as pcms_conv3_fwd_bnin; one source of <= 128 channels).  -5 when
// pcms_conv3_big16_ok is 0.
int pcms_conv3_fwd16(const void* x0, int c0, const void* x1, int c1, const float* isc, const float* ish,
                     const void* wpack16, const float* bias, void* y0, void* y1, int cy0, float* stats, int flags,
                     int N, int D, int H, int W, int Cout, hipStream_t s) {
  const B16Cfg cf = b16_config(N, D, H, W, c0, c1, Cout);
  const int bd = cf.bd;
  if (!bd || (c1 > 0 && x1 == nullptr)) return -5;
  if (isc && (c1 != 0 || c0 > kBgBnMax || !ish)) return -1;
  if (stats && flags) return -6;
  if (flags & ~PCMS_CONV_RELU) return -8;
  if (y1 == nullptr) cy0 = Cout;
  if (cy0 % 64 != 0 && cy0 != Cout) return -2;
  Conv3Params p;
  p.x0 = x0; p.x1 = x1; p.c0 = c0; p.c1 = c1;
  p.isc = isc; p.ish = ish;
  p.w = wpack16; p.bias = bias; p.y0 = y0; p.y1 = y1; p.cy0 = cy0;
  p.yacc = nullptr; p.stats = stats; p.accumulate = flags;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = c0 + c1; p.Cout = Cout;
  p.nvox = (long)N * D * H * W;
  p.nchunk = p.Cin / 16; p.chunks_per_split = p.nchunk;
  p.nbd = D / bd; p.nbh = H / 8; p.nbw = W / 16;
  const int nslot = b16_slots(cf, N, D, H, W, Cout);
  auto kern = cf.nt == 8 ? (isc ? conv3_fwd_b16_kernel<true, 4, 8> : conv3_fwd_b16_kernel<false, 4, 8>)
              : bd == 8  ? (isc ? conv3_fwd_b16_kernel<true, 8> : conv3_fwd_b16_kernel<false, 8>)
                         : (isc ? conv3_fwd_b16_kernel<true, 4> : conv3_fwd_b16_kernel<false, 4>);
  const int ldsb = cf.nt == 8 ? (isc ? B6G<4, 8>::LdsBn : B6G<4, 8>::Lds)
                   : bd == 8  ? (isc ? B6G<8>::LdsBn : B6G<8>::Lds)
                              : (isc ? B6G<4>::LdsBn : B6G<4>::Lds);
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ldsb);
  hipLaunchKernelGGL(kern, dim3(nslot * (Cout / (16 * cf.nt))), dim3(bd * 64), ldsb, s, p,
                     (uint32_t)(p.nvox * c0 * 2), (uint32_t)(p.nvox * c1 * 2));
  PCMS_CHECK_LAUNCH();
}

// ---- split-K 16x16x32 form for level 3 (W = 8 rows): boxes of 4 d x 16 h x 8 w ----
// the split count pcms_conv3_fwd16_split uses for this conv (0: not such a shape -- whole
// 4-deep W8 boxes, fewer than 256 (box, 64-channel block) items, and a power-of-two split
// of the 16-channel chunks that brings them to >= 256 workgroups)
int pcms_conv3_fwd16_split_ok(int N, int D, int H, int W, int c0, int c1, int Cout) {
  const long nvox = (long)N * D * H * W;
  if (Cout % 64 || D % 4 || H % 16 || W % 8 || c0 % 16 || c1 % 16 || c0 < 16) return 0;
  if (nvox >= (1L << 30) || nvox * std::max(std::max(c0, c1), Cout) * 2 >= (long)kOOB) return 0;
  const long items = (long)N * (D / 4) * (H / 16) * (W / 8) * (Cout / 64);
  const int nchunk = (c0 + c1) / 16;
  if (items >= big_min_boxes()) return 0;
  int sp = 1;
  while (items * sp < big_min_boxes() && nchunk % (2 * sp) == 0) sp *= 2;
  if (sp == 1 || (long)sp * nvox * Cout * 4 >= (long)kOOB) return 0;
  return sp;
}

// yacc[split][vox][Cout] fp32 = this split's partial sums (no bias, no statistics; sum them
// with pcms_split_epilogue(yacc, splits, ...)); splits = pcms_conv3_fwd16_split_ok(...), -5 if
// that is 0
int pcms_conv3_fwd16_split(const void* x0, int c0, const void* x1, int c1, const void* wpack16, float* yacc,
                           int N, int D, int H, int W, int Cout, int splits, hipStream_t s) {
  if (splits < 2 || splits != pcms_conv3_fwd16_split_ok(N, D, H, W, c0, c1, Cout) || (c1 > 0 && x1 == nullptr))
    return -5;
  Conv3Params p;
  p.x0 = x0; p.x1 = x1; p.c0 = c0; p.c1 = c1;
  p.isc = nullptr; p.ish = nullptr;
  p.w = wpack16; p.bias = nullptr; p.y0 = nullptr; p.y1 = nullptr; p.cy0 = Cout;
  p.yacc = yacc; p.stats = nullptr; p.accumulate = 0;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = c0 + c1; p.Cout = Cout;
  p.nvox = (long)N * D * H * W;
  p.nchunk = p.Cin / 16; p.chunks_per_split = p.nchunk / splits;
  p.nbd = D / 4; p.nbh = H / 16; p.nbw = W / 8;
  const int nbox = N * p.nbd * p.nbh * p.nbw;
  const int G = big_max_wgs() > 0 ? big_max_wgs() : device_cus();
  const int nslot = std::max(1, std::min(nbox, G / ((Cout / 64) * splits)));
  auto kern = conv3_fwd_b16_kernel<false, 4, 4, 8, true>;
  const int ldsb = B6G<4>::LdsSplit;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ldsb);
  hipLaunchKernelGGL(kern, dim3(nslot * (Cout / 64) * splits), dim3(256), ldsb, s, p,
                     (uint32_t)(p.nvox * c0 * 2), (uint32_t)(p.nvox * c1 * 2));
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
