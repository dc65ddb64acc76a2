// 3x3x3 convolution, the persistent 32x32x16 big-box forward / dgrad kernel (conv3_fwd.hip's
// conv3_fwd_any launches it for the shapes big_fwd_ok accepts), NDHWC, gfx950.
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
// Big-box forward / dgrad (bf16; the level-0/1 hot case: D % 8 == H % 8 == 0, W % 16 == 0,
// input channels in 16-channel chunks), PERSISTENT: one 8-wave workgroup per CU, one grid of
// at most #CU workgroups; workgroup (slot, cob) computes 8 x 8 x 16 = 1024-voxel boxes
// slot, slot + nslot, ... for its 64 output channels.  Wave w = (M-group mg = w & 3, N-tile
// nt = w >> 2) owns voxel rows [256 mg, 256 mg + 256) = 8 M-tiles and output channels
// [32 nt, 32 nt + 32), so every B fragment (weights, L2-resident; one contiguous 1 KiB load
// from the fragment-major pack, round 5) feeds 8 MFMAs and the two waves of a SIMD overlap
// one's operand waits with the other's MFMAs.
// The 10 x 10 x 18 halo of a chunk (32-B rows; the two 16-B halves swapped on odd row octets,
// so 16 consecutive rows hit 16 distinct bank groups) is double-buffered: the next chunk's
// halo -- the NEXT BOX's first chunk during a box's last chunk -- streams in by buffer
// LDS-DMA, one piece per thread and tap over the first 8 taps, and A fragments of tap t + 1
// are read while tap t's 8 MFMAs run; B loads run Dist taps ahead across chunk and box
// boundaries.  So only the first box of a workgroup waits for its operands; every later box
// starts on a landed halo.  Epilogue per box: + bias, bf16 channels staged through the
// M-group's 8 KiB LDS slice (two M-tiles at a time, the pair's channel halves) and
// written back as 16-B stores of whole 128-B channel rows (16 store instructions per wave and
// box, issued without waiting: the B waits of the next box's first taps count them).
// BatchNorm partials: per (M-group, channel) a running Chan merge over the boxes (count,
// mean, M2); one stats row per slot at the end.
// ------------------------------------------------------------------------------------
// (box and halo geometry, kBgThreads .. kBgDummy: conv3_bigbox.h)
constexpr int kBgStage = 64 * 128;                                        // per-M-group store slice
constexpr int kBgRed = 4 * 64 * 3 * 4;                                    // BN moments
constexpr int kBgLds = 2 * kBgBuf + kBgDummy + 4 * kBgStage + kBgRed + 64 * 4;  // + bias
// BNIN: the input BatchNorm's scale / shift table [2][kBgBnMax] floats after that
constexpr int kBgBnOff = kBgLds;
constexpr int kBgLdsBn = kBgLds + 2 * kBgBnMax * 4;
#ifndef BG_DIST
#define BG_DIST 8  // 2: 1-1.5 % slower big-box launches (A/B, profiles/r4_bg_dist_ab.txt)
#endif
// (BG_ABL, the ablation bits: conv3_bigbox.h)
constexpr int kBgDist = BG_DIST;           // B prefetch distance (taps); (Dist + 1) | 27
constexpr int kBgEpiStores = kBgMT * 2;    // 16-B stores per wave and box
static_assert(27 % (kBgDist + 1) == 0, "B ring index must continue across chunks");
static_assert(kBgLdsBn <= 160 * 1024, "LDS");

// retire the hidden load of a B fragment (bload16) and everything issued before it
template <int N> __device__ __forceinline__ void vm_wait1(s16x8_t& a) {
  static_assert(N >= 0 && N <= 63, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory");
}
// vector-memory ops issued after B(t)'s load by the time tap t waits for it: every tap s
// issues B(s + D) then piece(s) (s < P, chunk-relative, every chunk alike)
template <int P> constexpr int bg_piece(int s) { return ((s % 27) + 27) % 27 < P ? 1 : 0; }
template <int P, int Dist> constexpr int bg_wait(int t) {
  int n = bg_piece<P>(t - Dist);
  for (int s = t - Dist + 1; s <= t; ++s) n += 1 + bg_piece<P>(s);
  return n;
}

// BNIN (pcms_conv3_fwd_bnin, single-source inputs of <= kBgBnMax channels): the input is
// relu(x * isc + ish) -- the previous BatchNorm + ReLU applied in the staging path instead of
// a separate HBM pass.  At a chunk's end each thread rewrites the pieces it staged for the
// next chunk in LDS (their DMA has landed by the chunk-end vmcnt wait; out-of-range pieces,
// the zero padding, are left zero), before the barrier that publishes the buffer.
template <bool BNIN = false>
__global__ void __launch_bounds__(kBgThreads, 1) conv3_fwd_big_kernel(Conv3Params p, uint32_t x0bytes,
                                                                     uint32_t x1bytes) {
  constexpr int MT = kBgMT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wave = (M-group mg: box voxel rows 256 mg ..; N-tile nt: output channels 32 nt .. 32 nt + 31)
  const int mg = wave & 3, nt = wave >> 2;
  const int Cout = p.Cout, ncob = Cout >> 6;
  // logical workgroup id: consecutive ids on one XCD (dispatch is round-robin over 8), output
  // channel block fastest, so the workgroups sharing a halo (and neighbouring boxes) share L2
  const int G = gridDim.x;
  const int lg = (G & 7) == 0 ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int cob = lg % ncob, slot = lg / ncob, nslot = G / ncob;
  const int nbox = p.N * p.nbd * p.nbh * p.nbw;
  // box walk: slot, slot + nslot, ... (a d-column walk and sc1 / nt output stores measured
  // no different, profiles/r5_big_walk_storepolicy_ab.txt)
  const int box_step = nslot, box_end = nbox, box0 = slot;
  const int co_base = cob * 64;
  auto origin = [&](int box, int& n, int& d0, int& h0, int& w0) {
    int q = box;
    const int bwi = q % p.nbw; q /= p.nbw;
    const int bhi = q % p.nbh; q /= p.nbh;
    const int bdi = q % p.nbd;
    n = q / p.nbd;
    d0 = bdi * kBgBD; h0 = bhi * 8; w0 = bwi * 16;
  };

  const i32x4_t xr0 = buffer_desc(p.x0, x0bytes);
  const i32x4_t xr1 = buffer_desc(p.x1 ? p.x1 : p.x0, x1bytes);
  const uint32_t lds0 = lds_addr(lds);
  // live = false (past the last box): the piece is still issued (the vmcnt arithmetic is the
  // same for every chunk) but reads out of range = zeros into the idle buffer
  auto stage_piece = [&](int n, int d0, int h0, int w0, int chunk, int buf, int j, bool live) {
    const int c = chunk * 16;
    const bool first = c < p.c0;  // workgroup-uniform: the chunk lies in x0 or in x1
    const uint32_t stride = first ? p.c0 : p.c1;
    const uint32_t cofs = first ? c : c - p.c0;
    // piece j of this thread: halo row hv = pc / 2, logical 16-B half (pc & 1) swapped on odd
    // row octets (recomputed per chunk: a few VALU against 432 MFMAs, no registers held)
    const int pc = opaque(tid) + j * kBgThreads;
    const int hv = pc >> 1;
    const int hw_ = hv % kBgHW, t_ = hv / kBgHW, hh_ = t_ % kBgHH, hd_ = t_ / kBgHH;
    const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
    uint32_t voff = kOOB;
    if (live && hv < kBgHalo && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H &&
        (unsigned)gw < (unsigned)p.W && !(BG_ABL & 1))
      voff = ((uint32_t)(((n * p.D + gd) * p.H + gh) * p.W + gw) * stride + cofs +
              (uint32_t)((pc & 1) ^ ((hw_ >> 3) & 1)) * 8u) * 2u;
    const bool dummy = j == kBgPieces - 1 && wave > 0;  // wave-uniform
    const uint32_t lb = __builtin_amdgcn_readfirstlane(
        dummy ? lds0 + 2 * kBgBuf : lds0 + buf * kBgBuf + (wave * 64 + j * kBgThreads) * 16);
    dma16(first ? xr0 : xr1, lb, dummy ? kOOB : voff, 0);
    // BNIN: bit j = a real piece; bit 8 + j = its logical channel half
    return (!dummy && voff != kOOB ? 1u << j : 0u) | ((uint32_t)((pc & 1) ^ ((hw_ >> 3) & 1)) << (8 + j));
  };
  // BNIN: the staged pieces of buffer `buf` (chunk `chunk`) -> relu(x sc + sh) in place
  float* bnt = reinterpret_cast<float*>(lds + kBgBnOff);  // reserved by kBgLdsBn (BNIN launches)
  auto bn_apply = [&](int buf, int chunk, uint32_t pm) {
#pragma unroll
    for (int j = 0; j < kBgPieces; ++j) {
      if (!((pm >> j) & 1)) continue;
      const int pc = tid + j * kBgThreads;
      u32x4_t* q = reinterpret_cast<u32x4_t*>(lds + buf * kBgBuf + pc * 16);
      const int c = chunk * 16 + ((pm >> (8 + j)) & 1) * 8;
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

  // A fragment byte offsets in a halo buffer: MFMA row r = 256 wave + 32 mt + perm32(lane)
  // is box voxel (2 wave + mt / 4, 2 (mt % 4) + prow / 16, prow % 16).  The half swizzle
  // depends on the halo w coordinate only, so for each kw the (kd, kh) part of a tap is a
  // constant row offset (kd * 10 + kh) * 18 * 32 bytes folded into the ds_read immediate.
  // One base register per kw (recomputed per chunk); the M-tile and (kd, kh) parts are
  // ds_read immediates.
  // B fragments (weights, packed [Cin/32][27][Cout][32]; 16-channel chunk c = half c & 1 of
  // 32-chunk c >> 1) come through hidden loads Dist taps ahead: vector-memory returns are
  // in order, so a wait on B(t) also retires every halo piece issued before it; the pieces
  // get >= Dist taps to arrive from HBM before anything waits on them.
  // B address: (chunk, tap) byte offset (uniform) + one per-lane byte offset, through a
  // descriptor over the whole pack
  const int nchunk = p.Cin >> 4;
  const uint32_t tap_bytes = (uint32_t)Cout * 64u;
  const i32x4_t wr = buffer_desc(p.w, (uint32_t)(p.Cin >> 5) * 27u * tap_bytes);
  bool bl_prologue = true;  // BG_ABL & 8: only the prologue's weight loads run
  auto load_b = [&](s16x8_t& dst, int chunk, int tap, uint32_t boff) {
    if ((BG_ABL & 8) && !bl_prologue) return;
    // fragment-major pack (pack_bf16_off): the (32-chunk, tap) rows, boff = this wave's row
    // tile and lane, then the k-step (chunk & 1): one contiguous 1 KiB per wave
    const uint32_t off = boff + (uint32_t)((chunk >> 1) * 27 + tap) * tap_bytes + (uint32_t)(chunk & 1) * 1024u;
    bload16<0>(dst, wr, off);
  };

  // epilogue constants: column j of N-tile nt = channel 32 nt + j; two-pointer output split at
  // cy0 (workgroup-uniform)
  // (bias and the running BatchNorm moments live in LDS between boxes, not in registers)
  float* red = reinterpret_cast<float*>(lds + 2 * kBgBuf + kBgDummy + 4 * kBgStage);  // [mg][64][3]
  float* bls = red + 4 * 64 * 3;                                           // [64]
  if (tid < 64) bls[tid] = p.bias ? p.bias[co_base + tid] : 0.f;
  const bool to0 = co_base < p.cy0;
  const long ys = to0 ? p.cy0 : Cout - p.cy0;
  const int yc0 = to0 ? co_base : co_base - p.cy0;
  // output through a descriptor too (stores out of range are dropped; the host checks
  // every byte offset fits 31 bits)
  const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(
      to0 ? p.y0 : p.y1, (short)0, (int)(p.nvox * ys * 2), 0x00020000);
  char* stg = lds + 2 * kBgBuf + kBgDummy + mg * kBgStage;  // shared by the M-group's two waves
  int nbdone = 0;  // boxes merged into the running moments (uniform: kept in an SGPR)

  f32x16_t acc[MT];
  s16x8_t bset[kBgDist + 1];
  int box = box0;
  int n, d0, h0, w0;
  origin(box, n, d0, h0, w0);
  // Short boxes (4 chunks): every CU would reach its box boundary -- the vmcnt(0), the 128 KiB
  // store burst and the next halo's first pieces -- at the same moment; starting slot s
  // (s % 4) x ~16k cycles late spreads those bursts (measured 517 -> 433 us at level 0,
  // 64 -> 64; no effect with 8+ chunks, so not applied there).
  if (nchunk <= 4)
    for (int i = 0; i < 2 * (slot & 3); ++i) __builtin_amdgcn_s_sleep(127);
  uint32_t pmask = 0;  // BNIN: the pieces staged for the next chunk (stage_piece bits)
#pragma unroll
  for (int j = 0; j < kBgPieces; ++j) pmask |= stage_piece(n, d0, h0, w0, 0, 0, j, true);
#pragma unroll
  for (int t = 0; t < kBgDist; ++t) load_b(bset[t], 0, t, (uint32_t)(((co_base >> 5) + nt) * 2048 + lane * 16));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  bl_prologue = false;
  if constexpr (BNIN) bn_apply(0, 0, pmask);
  __syncthreads();
  int buf = 0;
  while (true) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const int nbx = box + box_step;
    const bool has_next = nbx < box_end;
    int nn = n, nd0 = d0, nh0 = h0, nw0 = w0;
    if (has_next) origin(nbx, nn, nd0, nh0, nw0);
    // one chunk: 27 taps.  Chunk 0 (peeled, Slack): B(t < Dist) were issued before the
    // previous box's 32 epilogue stores, so those waits count them as well; in a workgroup's
    // first box the prologue's vmcnt(0) already retired B(t < Dist), the looser count is safe.
    auto run_chunk = [&](int chunk, auto slack_tag) {
      constexpr bool Slack = decltype(slack_tag)::value;
      const bool last = chunk + 1 == nchunk;
      const bool live = !last || has_next;
      const int sn = last ? nn : n, sd = last ? nd0 : d0, sh = last ? nh0 : h0, sw = last ? nw0 : w0;
      const int schunk = last ? 0 : chunk + 1;
      const char* hl = lds + buf * kBgBuf;
      const int lo = opaque(lane);
      const int prow = perm32(lo & 31), hs = lo >> 5;
      const int hbase = ((2 * mg * kBgHH + (prow >> 4)) * kBgHW + (prow & 15)) * 32;
      int swk[3];
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) swk[kw] = hbase + kw * 32 + ((hs ^ ((((prow & 15) + kw) >> 3) & 1)) << 4);
      const uint32_t boff = (uint32_t)(((co_base >> 5) + nt) * 2048 + lo * 16);
      auto read_a1 = [&](int tap, int mt) {
        if constexpr ((BG_ABL & 16) != 0) tap = 0;
        const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        return *reinterpret_cast<const s16x8_t*>(hl + swk[kw] + (kd * kBgHH + kh) * kBgHW * 32 +
                                                 ((mt >> 2) * kBgHH + 2 * (mt & 3)) * kBgHW * 32);
      };
      // A fragments roll through one register set: right after M-tile mt's two MFMAs of tap t
      // its fragment of tap t + 1 is read (14 MFMAs of slack before its first use)
      s16x8_t a[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = read_a1(0, mt);
      // per tap: B(tap + D) (the set index runs on across chunks: (D + 1) | 27), one halo
      // piece of the next chunk (taps < 15); wait for B(tap); 16 MFMAs
      static_for<27>([&](auto tc) {
        constexpr int tap = decltype(tc)::value;
        constexpr int tn = tap + kBgDist;
        if constexpr (tn < 27) load_b(bset[tn % (kBgDist + 1)], chunk, tn, boff);
        else load_b(bset[tn % (kBgDist + 1)], schunk, tn - 27, boff);
        if constexpr (tap < kBgPieces) {
          const uint32_t bits = stage_piece(sn, sd, sh, sw, schunk, buf ^ 1, tap, live);
          if constexpr (BNIN) pmask = (tap == 0 ? 0u : pmask) | bits;
        }
        s16x8_t& b = bset[tap % (kBgDist + 1)];
        constexpr int extra = (Slack && tap < kBgDist) ? kBgEpiStores : 0;
        vm_wait1<bg_wait<kBgPieces, kBgDist>(tap) + extra>(b);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if constexpr ((BG_ABL & 4) != 0) asm volatile("" ::"v"(a[mt]), "v"(b));
          else acc[mt] = mfma(a[mt], b, acc[mt]);
          if constexpr (tap + 1 < 27 && (BG_ABL & 16) == 0) a[mt] = read_a1(tap + 1, mt);
        }
      });
      // the next chunk's halo has landed (the newest piece is followed by the B loads of the
      // remaining taps) and every wave is done with buf.  After a box's last chunk retire
      // everything: the epilogue needs registers, and the compiler may move (or, after the
      // workgroup's last box, reuse) the destinations of the next box's B loads -- they
      // must hold landed data by then (costs one L2 round trip per box).
      if (!last) vm_wait<27 - kBgPieces>();
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (BNIN) bn_apply(buf ^ 1, schunk, pmask);
      __syncthreads();
      buf ^= 1;
    };
    run_chunk(0, std::true_type{});
    for (int chunk = 1; chunk < nchunk; ++chunk) run_chunk(chunk, std::false_type{});

    // ---- epilogue of this box, two M-tiles at a time: + bias, bf16 channels into the
    // M-group's LDS slice (row = 32 mm + C row, 128 B of 64 channels; the two waves of the
    // group write channels 0-31 / 32-63), read back as 4 x 16 B per lane and wave = whole
    // 128-B channel rows, 16-B stores.  BatchNorm moments in the same pass, shifted by K
    // (the running mean; the bias before the first box): box mean K + S1 / n, M2 = S2 -
    // S1^2 / n, Chan-merged into the running moments.
    // (lane-dependent offsets from an opaque lane copy: box-invariant, the compiler would
    // hoist them out of the box loop and spill them)
    const int lane_o = opaque(lane);
    const long plane = (long)p.H * p.W;
    const long vbase = (((long)n * p.D + d0) * p.H + h0) * p.W + w0;
    char* wst = stg + (lane_o & 31) * 2 + nt * 64 + (lane_o >> 5) * 512;
    float* rme = red + (mg * 64 + 32 * nt + (lane_o & 31)) * 3;  // [ch][mean, M2, n] of this wave's channel
    const float bias0 = bls[32 * nt + (lane_o & 31)];
    const bool relu = p.accumulate & PCMS_CONV_RELU;  // eval: BatchNorm folded (no stats then)
    const float rn = (float)nbdone * (32.f * MT);
    const float K0 = nbdone ? rme[0] : bias0;
    const float c0s = bias0 - K0;  // d = acc + bias - K
    float S1 = 0.f, S2 = 0.f;
#pragma unroll
    for (int pass = 0; pass < MT / 2; ++pass) {
#pragma unroll
      for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = mm * 32 + (e & 3) + 8 * (e >> 2);
          const float v0 = acc[2 * pass + mm][e];
          *reinterpret_cast<bf16_t*>(wst + row * 128) = f2bf(relu ? fmaxf(v0 + bias0, 0.f) : v0 + bias0);
          const float e0 = v0 + c0s;
          S1 += e0;
          S2 = fmaf(e0, e0, S2);
        }
      // both waves of the M-group have written their channels of the slice (raw barrier:
      // __syncthreads() would also drain this wave's stores of the previous pass)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = (4 * nt + k) * 8 + (lane_o >> 3), c16 = lane_o & 7;
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stg + row * 128 + c16 * 16);
        const int mt = 2 * pass + (row >> 5), pr = perm32(row & 31);
        const int rd = 2 * mg + (mt >> 2), rh = 2 * (mt & 3) + (pr >> 4), rw = pr & 15;
        const long vox = vbase + (long)rd * plane + (long)rh * p.W + rw;
        if constexpr ((BG_ABL & 2) == 0)
          __builtin_amdgcn_raw_buffer_store_b128(v, yr, (int)((vox * ys + yc0 + c16 * 8) * 2), 0, 0);
        else
          asm volatile("" ::"v"(v), "v"((int)vox));
      }
      // both waves are done reading the slice before the next pass rewrites it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    {
      constexpr float nb = 32.f * MT;  // voxels per wave and box
      const float nnew = rn + nb;
      const float s1 = S1 + __shfl_xor(S1, 32, 64);
      const float s2 = S2 + __shfl_xor(S2, 32, 64);
      const float mbox = K0 + s1 / nb;
      const float m2b = fmaxf(s2 - s1 * s1 / nb, 0.f);
      const float rmean = nbdone ? rme[0] : 0.f, rm2 = nbdone ? rme[1] : 0.f;
      const float delta = mbox - rmean;
      if ((lane_o >> 5) == 0) {
        rme[0] = rmean + delta * (nb / nnew);
        rme[1] = rm2 + m2b + delta * delta * (rn * nb / nnew);
        rme[2] = nnew;
      }
      ++nbdone;
    }
    if (!has_next) break;
    box = nbx;
    n = nn; d0 = nd0; h0 = nh0; w0 = nw0;
  }

  if (!p.stats) return;
  // one stats row per slot: Chan merge of the 4 waves' running moments (mean, M2, n)
  __syncthreads();
  if (tid < 64) {
    float S = 0.f, Nn = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      S += red[(w * 64 + tid) * 3] * red[(w * 64 + tid) * 3 + 2];
      Nn += red[(w * 64 + tid) * 3 + 2];
    }
    const float m = S / Nn;
    float M2 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float c = red[(w * 64 + tid) * 3 + 2];
      const float d = red[(w * 64 + tid) * 3] - m;
      M2 += red[(w * 64 + tid) * 3 + 1] + c * d * d;
    }
    float* st = p.stats + ((long)slot * Cout + co_base + tid) * 2;
    st[0] = S;
    st[1] = M2;
    if (tid == 0 && cob == 0) p.stats[(long)nslot * Cout * 2 + slot] = Nn;
  }
}

}  // namespace

// big-box forward: bf16, whole 8x8x16 boxes, 16-channel chunks of both sources, enough boxes
// to give every CU one (pcms_conv3_big_min_boxes), every byte offset inside a 32-bit voffset
static int g_big_min_boxes = 256;
static int g_big_max_wgs = 0;  // persistent grid cap (0: one workgroup per CU)
bool big_fwd_ok(int dtype, int N, int D, int H, int W, int c0, int c1) {
  if (dtype != PCMS_BF16 || D % kBgBD || H % 8 || W % 16 || c0 % 16 || c1 % 16 || c0 < 16) return false;
  const long nvox = (long)N * D * H * W;
  if ((long)N * (D / kBgBD) * (H / 8) * (W / 16) < g_big_min_boxes) return false;
  return nvox < (1L << 30) && nvox * std::max(c0, c1) * 2 < (long)kOOB;
}
// (the output descriptor additionally needs nvox * Cout * 2 < 2^31: checked at launch)
// box slots of the persistent grid (= BatchNorm stats rows): each slot's workgroups (one
// per 64-channel block) walk boxes slot, slot + nslot, ...
int big_slots(int N, int D, int H, int W, int Cout) {
  const int nbox = N * (D / kBgBD) * (H / 8) * (W / 16);
  const int G = g_big_max_wgs > 0 ? g_big_max_wgs : device_cus();
  return std::max(1, std::min(nbox, G / (Cout / 64)));
}
int big_min_boxes() { return g_big_min_boxes; }
int big_max_wgs() { return g_big_max_wgs; }

// the launch for a conv that passed big_fwd_ok and the output bound above; cp: the Conv3Params
// conv3_fwd_any filled (sources, pack, outputs, flags, grid), the box counts set here
int big_fwd_launch(const void* cp, hipStream_t s) {
  Conv3Params p = *static_cast<const Conv3Params*>(cp);
  p.nbd = p.D / kBgBD; p.nbh = p.H / 8; p.nbw = p.W / 16;
  const int nslot = big_slots(p.N, p.D, p.H, p.W, p.Cout);
  auto kern = p.isc ? conv3_fwd_big_kernel<true> : conv3_fwd_big_kernel<false>;
  const int ldsb = p.isc ? kBgLdsBn : kBgLds;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ldsb);
  hipLaunchKernelGGL(kern, dim3(nslot * (p.Cout / 64)), dim3(kBgThreads), ldsb, s, p,
                     (uint32_t)(p.nvox * p.c0 * 2), (uint32_t)(p.nvox * p.c1 * 2));
  PCMS_CHECK_LAUNCH();
}

extern "C" {

// Minimum box count for the big-box forward (tests lower it to reach small grids);
// v <= 0 only queries.  Returns the previous value.
int pcms_conv3_big_min_boxes(int v) {
  const int old = g_big_min_boxes;
  if (v > 0) g_big_min_boxes = v;
  return old;
}

// Workgroup cap of the persistent big-box grid (tests lower it so each workgroup walks
// several boxes); 0 restores one per CU, v < 0 only queries.  Returns the previous value.
int pcms_conv3_big_max_wgs(int v) {
  const int old = g_big_max_wgs;
  if (v >= 0) g_big_max_wgs = v;
  return old;
}

}  // extern "C"
