// 3x3x3 / stride 1 / pad 1 convolution, the weight gradient (the second backward product of
// aten::convolution_backward for nn.Conv3d(k=3, padding=1)), NDHWC, gfx950.
//
//   conv3_wgrad dW[tap, co, ci] += sum_v dY[v, co] * X[v + tap, ci]   (K = voxels)
//               Both MFMA operands need the voxel index contiguous: they are read from
//               natural NDHWC LDS tiles with ds_read_b64_tr_b16 (hardware transpose).
#include "common.h"
#include "pcms_hip.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "conv_common.h"
#include "conv3_units.h"

namespace {

// ------------------------------------------------------------------------------------
// weight-gradient kernel
// ------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4_t mfma16(s16x8_t a, s16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                 0, 0, 0);
}

constexpr int kWThreads = 512;          // 8 waves: wave = (co-tile, tap-group)
// ablation builds only (tests/tools/wgrad_abl.py; 0 in the product): bit 1 the direct flush's
// global stores dropped, 2 no staging after a workgroup's first box, 4 no MFMA phase, 8 no
// wait for the next box's DMA at a box's end, 16 the spread pieces' addresses computed but
// read nothing (zeros land in LDS), 32 the spread pieces read fixed in-range addresses (no
// address arithmetic) -- wrong results: timing only
#ifndef WGRAD_ABL
#define WGRAD_ABL 0
#endif
// A/B builds: bit 0 s_setprio 1 for waves 4-7 of the weight gradient, bit 1 of the 8-deep
// 16x16x32 conv (MI355X_MICROARCH.md, two waves per SIMD item 4); 0 in the product
#ifndef PCMS_SETPRIO
#define PCMS_SETPRIO 0
#endif
constexpr int kWHaloMax = 720;          // halo rows (box <= 256 voxels)

template <typename T> struct WTraits;
template <> struct WTraits<bf16_t> {
  static constexpr int BV = 256;        // voxels per staged box
  static constexpr int KV = 16;         // voxels per MFMA
  static constexpr int NBUF = 2;
  static constexpr int DYROW = 128;     // 64 co x 2 B
  static constexpr int XROW = 64;       // 32 ci x 2 B
  static constexpr int VEC = 8;
  static constexpr int HALO = kWHaloMax;
  static constexpr int NPART = 1;
  typedef s16x8_t Frag;
};
template <> struct WTraits<x6_t> {
  // boxes of <= 64 voxels (round 6): the h, m, l tiles (3 x 24 KB) plus the fp32 LDS-DMA
  // target of the NEXT box (48 KB) fit in LDS, so the box stream no longer stops the MFMAs
  static constexpr int BV = 64;         // voxels per staged box
  static constexpr int KV = 8;          // voxels per MFMA k-step (K halves concatenated)
  static constexpr int NBUF = 1;
  static constexpr int DYROW = 128;
  static constexpr int XROW = 64;
  static constexpr int VEC = 4;
  static constexpr int HALO = 256;
  static constexpr int NPART = 3;
  // the fp32 box as it arrives by LDS-DMA: dy [BV][64 co] then the x halo [HALO][32 ci] (+ one
  // wave-instruction of slack: a halo's last DMA may run past its rows, reading zeros)
  static constexpr int RAWDY = BV * 64 * 4;
  static constexpr int RAWBYTES = RAWDY + (HALO * 8 + 64) * 16;
  typedef s16x8_t Frag;
};
template <> struct WTraits<x3_t> {
  static constexpr int BV = 128;        // voxels per staged box (hi + lo tiles: 2 x 62 KB)
  static constexpr int KV = 16;
  static constexpr int NBUF = 1;
  static constexpr int DYROW = 128;     // LDS rows as bf16 (one tile per half)
  static constexpr int XROW = 64;
  static constexpr int VEC = 4;         // fp32 elements per 16-B global piece
  static constexpr int HALO = kWHaloMax;
  static constexpr int NPART = 2;
  typedef s16x8_t Frag;
};

struct WgradParams {
  const void* x0; const void* x1; int c0; int c1;
  const void* dy;
  float* dwt;            // fp32 workspace: one [27][Cout][Cin] partial row per split
  int N, D, H, W, Cin, Cout;
  int lbd, lbh, lbw, nbd, nbh, nbw;
  int nbox, boxes_per_split;
  int nco, nci;          // 64-channel output blocks, 32-channel input blocks
  int dma;               // bf16: stage by buffer LDS-DMA (byte sizes below < 2^31)
  uint32_t x0bytes, x1bytes, dybytes;
  float* dw;             // direct (one split, bf16): dw [Cout][cw][27] += through an LDS transpose
  int cw, direct;
  int store;             // PCMS_GRAD_STORE: dw = (the first writer of a fresh gradient), not +=
  int ntg;               // tap groups (TG kernels: 2, taps [0, 16) / [16, 27) per workgroup)
  // BNIN kernels (pcms_conv3_wgrad_bnin): x is relu(x0 * isc + ish) per input channel
  const float* isc = nullptr; const float* ish = nullptr;
};


// TG: the taps are split over two workgroups per (tile, split) -- for grids of few boxes,
// where splitting the voxels instead would add partial rows and a reduction pass
// BNIN (bf16, LDS-DMA staging, one source): the staged x halo is relu(x * isc + ish), applied
// in LDS by the thread that staged each piece, after its DMA landed and before the barrier that
// publishes the buffer (the BatchNorm + ReLU of the layer below, fused as in
// conv3_fwd_big_kernel<true>); out-of-range pieces (zero padding) stay zero
// K16 (bf16, compile-time box, no TG): v_mfma_f32_16x16x32_bf16 instead of 32x32x16 -- the same
// LDS reads per FLOP (K = 32 voxels per step: 8 A + 4 B transposed reads per tap pair of
// ci tiles), the MFMA shape that runs the power-capped big-box convs at a higher clock
// (profiles/r5_mfma_shape_probe.txt).  acc16[j][ct][t]: tap j, 16-co tile ct, 16-ci tile t.
template <typename T, int LBD, int LBH, int LBW, bool TG = false, bool P4 = false, bool BNIN = false,
          bool K16 = false>
__global__ void __launch_bounds__(kWThreads, 1) conv3_wgrad_kernel(WgradParams p) {
  static_assert(!K16 || (std::is_same<T, bf16_t>::value && LBW >= 2 && !TG), "K16: bf16 fixed boxes");
  const int lbd_ = LBW >= 0 ? LBD : p.lbd, lbh_ = LBW >= 0 ? LBH : p.lbh, lbw_ = LBW >= 0 ? LBW : p.lbw;
  typedef WTraits<T> Tr;
  typedef typename Tr::Frag Frag;
  constexpr int DYBYTES = Tr::BV * Tr::DYROW;
  constexpr int XBYTES = Tr::HALO * Tr::XROW;
  constexpr int BUFBYTES = DYBYTES + XBYTES;
  extern __shared__ __attribute__((aligned(16))) char wlds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hsel = lane >> 5;
#if PCMS_SETPRIO & 1
  // static priority for the second-dispatched half (waves 4-7: each SIMD's younger wave)
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
  // wave w owns taps w, w + 8, w + 16 (, w + 24) for BOTH co tiles, so each B (x) fragment
  // feeds 2 MFMAs: 1.5 LDS reads per MFMA instead of 2.3 (8 accumulators)
  // fp32 data, split-bf16 products: x3 (hi, lo tiles) / x6 (h, m, l tiles), the parts
  // BUFBYTES apart
  constexpr bool kX3 = std::is_same<T, x3_t>::value, kX6 = std::is_same<T, x6_t>::value;
  typedef typename std::conditional<kX3 || kX6, float, bf16_t>::type M;
  // 1-D grid, logical id XCD-aware (dispatch is round-robin over 8 XCDs: consecutive logical
  // ids land on one XCD at about the same time), tile (co block, ci block) fastest: the
  // workgroups of one split that share its dy boxes (and its halos) share an L2
  const int G = gridDim.x, ntile = p.nco * p.nci;
  const int lg = (G & 7) == 0 ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int tile = lg % ntile, split = lg / ntile / (TG ? 2 : 1);
  // the wave's taps: main taps tb + 8 j (j < NJ, accumulators j and 4 + j) and, where it
  // exists, one more at tb + 8 NJ (accumulators 3 and 7).  TG group 0: taps w, w + 8;
  // group 1: 16 + w, 24 + w (waves 0-2)
  const int tgrp = TG ? (lg / ntile) & 1 : 0;
  constexpr int NJ = TG ? 1 : 3;
  const int tb = 16 * tgrp + wave;
  const bool four = TG ? (tgrp == 0 || wave < 3) : wave < 3;
  auto owned = [&](int j) __attribute__((always_inline)) { return j < NJ || (j == 3 && four); };
  auto tapof = [&](int j) __attribute__((always_inline)) { return tb + 8 * (j < NJ ? j : NJ); };
  const int co_base = (tile % p.nco) * 64;
  const int ci_base = (tile / p.nco) * 32;
  // fp32 build, <= 8 input channels (the stem): the 32 MFMA columns hold 4 taps x 8 channels
  // (column n = tap 4 wave + n / 8, channel n % 8; waves 0-6 own the 7 tap groups) instead of
  // one tap x 32 channels of which 24 are padding -- 3.9x fewer MFMAs per box
  constexpr bool pack4 = kX6 && P4;  // the host launches P4 for Cin <= 8 only
  const int bd = 1 << lbd_, bh = 1 << lbh_, bw = 1 << lbw_;
  const int HH = bh + 2, HW = bw + 2;
  const int HV = (bd + 2) * HH * HW;
  const int boxvol = bd * bh * bw;
  const long plane = (long)p.H * p.W;
  const M* x0 = (const M*)p.x0;
  const M* x1 = (const M*)p.x1;
  const M* dy = (const M*)p.dy;

  const int b_beg = split * p.boxes_per_split;
  const int b_end = min(p.nbox, b_beg + p.boxes_per_split);

  f32x16_t acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  f32x4_t acc16[4][4][2];
  if constexpr (K16) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc16[j][c][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }

  // register staging: pieces of 16 B
  constexpr int DYP = Tr::BV * Tr::DYROW / 16;
  const int XP = HV * Tr::XROW / 16;
  constexpr int MAXP = Tr::NBUF == 2 ? (DYP + kWHaloMax * Tr::XROW / 16 + kWThreads - 1) / kWThreads : 1;
  u32x4_t stg[MAXP];

  auto box_origin = [&](int b, int& n, int& d0, int& h0, int& w0) {
    int bwi = b % p.nbw; b /= p.nbw;
    int bhi = b % p.nbh; b /= p.nbh;
    int bdi = b % p.nbd;
    n = b / p.nbd;
    d0 = bdi * bd; h0 = bhi * bh; w0 = bwi * bw;
  };
  auto stage_load = [&](int b) {
    int n, d0, h0, w0;
    box_origin(b, n, d0, h0, w0);
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      // one unconditional 16-B load per piece (invalid pieces read the zero page): a
      // conditional load merged with a zero default makes the compiler drain vmcnt before
      // the merge, serialising the prefetch with the compute it should overlap
      const int pc = tid + i * kWThreads;
      const void* src = g_zero16;
      if (pc < DYP) {
        const int r = pc / (Tr::DYROW / 16), q = pc % (Tr::DYROW / 16);
        if (r < boxvol) {
          const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
          const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
          if (gd < p.D && gh < p.H && gw < p.W) {
            const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
            src = dy + vox * p.Cout + co_base + q * Tr::VEC;
          }
        }
      } else if (pc < DYP + XP) {
        const int hp = pc - DYP;
        const int hv = hp / (Tr::XROW / 16), q = hp % (Tr::XROW / 16);
        const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
        const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
        const int c = ci_base + q * Tr::VEC;
        if (gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && c < p.Cin) {
          const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
          src = (c < p.c0) ? (const void*)(x0 + vox * p.c0 + c) : (const void*)(x1 + vox * p.c1 + (c - p.c0));
        }
      }
      stg[i] = *reinterpret_cast<const u32x4_t*>(src);
    }
  };
  auto stage_store = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int pc = tid + i * kWThreads;
      if (pc < DYP) {
        const int r = pc / (Tr::DYROW / 16), q = pc % (Tr::DYROW / 16);
        int off;
        if (sizeof(T) == 2) off = dy_off_bf16(r, q * 8);
        else off = r * Tr::DYROW + q * 16;
        *reinterpret_cast<u32x4_t*>(buf + off) = stg[i];
      } else if (pc < DYP + XP) {
        const int hp = pc - DYP;
        *reinterpret_cast<u32x4_t*>(buf + DYBYTES + hp * 16) = stg[i];
      }
    }
  };

  // fp32 build: every 16-B piece (4 fp32) of the box's dy tile and x halo loaded into
  // registers (all in flight), then split into the hi tile at buf and the lo tile at
  // buf + BUFBYTES (the bf16 layouts: dy_off_bf16 rows, 64-B halo rows)
  auto stage_x3 = [&](char* buf, int b) {
    int n, d0, h0, w0;
    box_origin(b, n, d0, h0, w0);
    constexpr int DYQ = Tr::BV * 16;                      // 64 co / 4 per piece
    constexpr int XQMAX = Tr::HALO * 8;                   // 32 ci / 4
    constexpr int PER = (DYQ + XQMAX + kWThreads - 1) / kWThreads;
    constexpr int RND = 8;                                // pieces in flight per thread (VGPRs)
    const int XQ = HV * 8;
#pragma unroll
    for (int i0 = 0; i0 < PER; i0 += RND) {
      f32x4_t v[RND];
#pragma unroll
      for (int i = 0; i < RND; ++i) {
        const int pc = tid + (i0 + i) * kWThreads;
        const float* src = reinterpret_cast<const float*>(g_zero16);
        if (pc < DYQ) {
          const int r = pc >> 4, q = pc & 15;
          const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
          const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
          if (r < boxvol && gd < p.D && gh < p.H && gw < p.W)
            src = reinterpret_cast<const float*>(dy) + (((long)n * p.D + gd) * plane + (long)gh * p.W + gw) * p.Cout + co_base + q * 4;
        } else if (pc < DYQ + XQ) {
          const int hp = pc - DYQ, hv = hp >> 3, q = hp & 7;
          const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
          const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
          const int c = ci_base + q * 4;
          if (gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && c < p.Cin) {
            const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
            src = (c < p.c0) ? reinterpret_cast<const float*>(x0) + vox * p.c0 + c
                             : reinterpret_cast<const float*>(x1) + vox * p.c1 + (c - p.c0);
          }
        }
        v[i] = *reinterpret_cast<const f32x4_t*>(src);
      }
#pragma unroll
      for (int i = 0; i < RND; ++i) {
        const int pc = tid + (i0 + i) * kWThreads;
        int off;
        if (pc < DYQ) off = dy_off_bf16(pc >> 4, (pc & 15) * 4);
        else if (pc < DYQ + XQ) off = DYBYTES + (pc - DYQ) * 8;
        else continue;
        if constexpr (kX6) {
          const float f[8] = {v[i][0], v[i][1], v[i][2], v[i][3], 0.f, 0.f, 0.f, 0.f};
          u32x4_t h, m, l;
          split3x8(f, h, m, l);
          *reinterpret_cast<u32x2_t*>(buf + off) = (u32x2_t){h[0], h[1]};
          *reinterpret_cast<u32x2_t*>(buf + BUFBYTES + off) = (u32x2_t){m[0], m[1]};
          *reinterpret_cast<u32x2_t*>(buf + 2 * BUFBYTES + off) = (u32x2_t){l[0], l[1]};
        } else {
          const u32x2_t h01 = split2(v[i][0], v[i][1]), h23 = split2(v[i][2], v[i][3]);
          *reinterpret_cast<u32x2_t*>(buf + off) = (u32x2_t){h01[0], h23[0]};
          *reinterpret_cast<u32x2_t*>(buf + BUFBYTES + off) = (u32x2_t){h01[1], h23[1]};
        }
      }
    }
  };

  // fp32 build with LDS-DMA (p.dma): the box's fp32 dy tile and x halo into the raw buffer
  // after the part tiles (16-B pieces, one wave-instruction of 64 consecutive pieces each;
  // padding / out-of-volume pieces read zeros), and the split of the landed box into the tiles
  auto stage_raw = [&](int b) __attribute__((always_inline)) {
    if constexpr (kX6) {
      int n, d0, h0, w0;
      box_origin(b, n, d0, h0, w0);
      const uint32_t lb0 = lds_addr(wlds + Tr::NPART * BUFBYTES);
      const bool first = ci_base < p.c0;  // a 32-channel block lies in one source
      const i32x4_t xr = buffer_desc(first ? p.x0 : p.x1, first ? p.x0bytes : p.x1bytes);
      const i32x4_t dr = buffer_desc(p.dy, p.dybytes);
      const int xs = first ? p.c0 : p.c1, xc = first ? ci_base : ci_base - p.c0;
      constexpr int DYQ = Tr::BV * 16;  // 16 pieces of 4 fp32 per voxel (64 co)
      constexpr int RP = (DYQ + Tr::HALO * 8 + kWThreads - 1) / kWThreads;
      static_assert(DYQ % 64 == 0, "dy pieces in whole wave-instructions");
      const int XQ = HV * 8;            // 8 pieces per halo voxel (32 ci)
#pragma unroll
      for (int i = 0; i < RP; ++i) {
        const int pc0 = (tid & ~63) + i * kWThreads;  // wave-uniform first piece
        if (pc0 >= DYQ + XQ) break;
        const int pc = pc0 + lane;
        uint32_t voff = kOOB;
        if (pc0 < DYQ) {
          const int r = pc >> 4, q = pc & 15;
          if (r < boxvol) {
            const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
            const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
            if (gd < p.D && gh < p.H && gw < p.W)
              voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * p.Cout + co_base + q * 4) * 4);
          }
          dma16(dr, __builtin_amdgcn_readfirstlane(lb0 + pc0 * 16), voff, 0);
        } else {
          const int hp = pc - DYQ, hv = hp >> 3, q = hp & 7;
          const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
          const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
          if (hp < XQ && gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && xc + q * 4 < xs)
            voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * xs + xc + q * 4) * 4);
          dma16(xr, __builtin_amdgcn_readfirstlane(lb0 + Tr::RAWDY + (pc0 - DYQ) * 16), voff, 0);
        }
      }
    } else {
      (void)b;
    }
  };
  auto split_raw = [&](char* buf) __attribute__((always_inline)) {
    if constexpr (kX6) {
      const char* raw = wlds + Tr::NPART * BUFBYTES;
      constexpr int DYQ = Tr::BV * 16;
      const int XQ = HV * 8;
      for (int pc = tid; pc < DYQ + XQ; pc += kWThreads) {
        const bool isdy = pc < DYQ;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(isdy ? raw + pc * 16 : raw + Tr::RAWDY + (pc - DYQ) * 16);
        const int off = isdy ? dy_off_bf16(pc >> 4, (pc & 15) * 4) : DYBYTES + (pc - DYQ) * 8;
        const float f[8] = {v[0], v[1], v[2], v[3], 0.f, 0.f, 0.f, 0.f};
        u32x4_t h, m, l;
        split3x8(f, h, m, l);
        *reinterpret_cast<u32x2_t*>(buf + off) = (u32x2_t){h[0], h[1]};
        *reinterpret_cast<u32x2_t*>(buf + BUFBYTES + off) = (u32x2_t){m[0], m[1]};
        *reinterpret_cast<u32x2_t*>(buf + 2 * BUFBYTES + off) = (u32x2_t){l[0], l[1]};
      }
    } else {
      (void)buf;
    }
  };

  // per-lane voxel-row helpers for the k index (voxel inside the box)
  auto halo_row = [&](int r) {
    const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
    return (rd * HH + rh) * HW + rw;
  };

  // generic box: one 16-voxel k-step at a time.  x3: the lo tiles sit BUFBYTES past the hi
  // tiles; per (co tile, tap) hi*hi + lo*hi + hi*lo
  auto compute = [&](const char* buf) {
    const char* xb = buf + DYBYTES;
#pragma unroll 2
    for (int k0 = 0; k0 < boxvol; k0 += Tr::KV) {
      const int g = (lane >> 4) & 1, qq = (lane & 15) >> 2, pp = lane & 3;
      auto frag = [](const char* base, int o0, int o1) __attribute__((always_inline)) {
        const s16x4_t l = tr_read(base, o0), h = tr_read(base, o1);
        return (s16x8_t){l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
      };
      if constexpr (kX6) {
        // 8 voxels per k-step, both K halves over the same voxels from different parts:
        // A1 = [dy h | dy m], A2 = [dy h | dy l]; B1 = [x h | x h], B2 = [x m | x h],
        // B3 = [x l | x m]; A1.B1 + A2.B2 + A1.B3 = hh + mh + hm + lh + hl + mm
        const int v_a = k0 + qq;
        const char* dA1 = buf + hsel * BUFBYTES;
        const char* dA2 = buf + hsel * 2 * BUFBYTES;
        s16x8_t a1[2], a2[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int co = ct * 32 + g * 16 + pp * 4;
          const int o0 = dy_off_bf16(v_a, co), o1 = dy_off_bf16(v_a + 4, co);
          a1[ct] = frag(dA1, o0, o1);
          a2[ct] = frag(dA2, o0, o1);
        }
        const int hr0 = halo_row(v_a), hr1 = halo_row(v_a + 4);
        const int ci = g * 16 + pp * 4;
        if constexpr (pack4) {
          if (wave < 7) {
            // the lane's 4 columns g 16 + pp 4 .. + 3 = tap 2 g + pp / 2 of the group, channels
            // (pp & 1) 4 .. + 3 (tap 27 of the last group reads tap 26; its column is dropped)
            const int tap = min(4 * wave + 2 * g + (pp >> 1), 26);
            const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            const int off = (kd * HH + kh) * HW + kw;
            const int o0 = (hr0 + off) * Tr::XROW + (pp & 1) * 8, o1 = (hr1 + off) * Tr::XROW + (pp & 1) * 8;
            const s16x8_t b1 = frag(xb, o0, o1);
            const s16x8_t b2 = frag(xb + (hsel ? 0 : BUFBYTES), o0, o1);
            const s16x8_t b3 = frag(xb + (hsel ? BUFBYTES : 2 * BUFBYTES), o0, o1);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
              acc[4 * ct] = mfma(a1[ct], b1, acc[4 * ct]);
              acc[4 * ct] = mfma(a2[ct], b2, acc[4 * ct]);
              acc[4 * ct] = mfma(a1[ct], b3, acc[4 * ct]);
            }
          }
          continue;
        }
        const char* xb1 = xb;                                     // B1: h | h
        const char* xb2 = xb + (hsel ? 0 : BUFBYTES);            // B2: m | h
        const char* xb3 = xb + (hsel ? BUFBYTES : 2 * BUFBYTES);  // B3: l | m
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (owned(j)) {
            const int tap = tapof(j);
            const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
            const int off = (kd * HH + kh) * HW + kw;
            const int o0 = (hr0 + off) * Tr::XROW + ci * 2, o1 = (hr1 + off) * Tr::XROW + ci * 2;
            const s16x8_t b1 = frag(xb1, o0, o1), b2 = frag(xb2, o0, o1), b3 = frag(xb3, o0, o1);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
              acc[4 * ct + j] = mfma(a1[ct], b1, acc[4 * ct + j]);
              acc[4 * ct + j] = mfma(a2[ct], b2, acc[4 * ct + j]);
              acc[4 * ct + j] = mfma(a1[ct], b3, acc[4 * ct + j]);
            }
          }
        }
        continue;
      }
      const int v_a = k0 + 8 * hsel + qq;
      s16x8_t a2[2], a2l[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int co = ct * 32 + g * 16 + pp * 4;
        a2[ct] = frag(buf, dy_off_bf16(v_a, co), dy_off_bf16(v_a + 4, co));
        if constexpr (kX3) a2l[ct] = frag(buf + BUFBYTES, dy_off_bf16(v_a, co), dy_off_bf16(v_a + 4, co));
      }
      const int hr0 = LBW >= 4 ? halo_row(k0) + 8 * hsel + qq : halo_row(v_a);
      const int hr1 = LBW >= 4 ? hr0 + 4 : halo_row(v_a + 4);
      const int ci = g * 16 + pp * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (owned(j)) {
          const int tap = tapof(j);
          const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
          const int off = (kd * HH + kh) * HW + kw;
          const int o0 = (hr0 + off) * Tr::XROW + ci * 2, o1 = (hr1 + off) * Tr::XROW + ci * 2;
          const s16x8_t b = frag(xb, o0, o1);
          acc[j] = mfma(a2[0], b, acc[j]);
          acc[4 + j] = mfma(a2[1], b, acc[4 + j]);
          if constexpr (kX3) {
            const s16x8_t bl = frag(xb + BUFBYTES, o0, o1);
            acc[j] = mfma(a2l[0], b, acc[j]);
            acc[4 + j] = mfma(a2l[1], b, acc[4 + j]);
            acc[j] = mfma(a2[0], bl, acc[j]);
            acc[4 + j] = mfma(a2[1], bl, acc[4 + j]);
          }
        }
      }
    }
  };

  // bf16 with a compile-time box (w = 8 or 16): the k loop fully unrolled.  Every fragment
  // address is a per-lane base (per box buffer) + an immediate: the dy half swap depends on the
  // lane's voxel inside a 16-voxel step only, a step starts a w-row, and the lane's voxels
  // (vl, vl + 4) lie in one w-row (vl % 8 < 4), so its halo rows are a lane constant plus the
  // step's compile-time row.  The
  // fragments of step s + 1 are read while step s's MFMAs run (two register sets), so the
  // LDS latency is behind the MFMAs instead of in front of each pair.  Taps wave + 8 j, j < 3
  // for every wave; the fourth (waves 0-2: taps 24-26) in a uniform branch at the step's end,
  // its fragment also one step ahead (one code path: no per-variant register allocation).
  auto compute_fixed = [&](const char* buf, auto&& mid, auto&& stage) __attribute__((always_inline)) {
    constexpr int LD = LBW >= 2 ? LBD : 0, LH = LBW >= 2 ? LBH : 0, LW = LBW >= 2 ? LBW : 4;
    constexpr int HHc = (1 << LH) + 2, HWc = (1 << LW) + 2;
    constexpr int NK = (1 << (LD + LH + LW)) / 16;
    // halo rows between a lane's two voxels vl and vl + 4: the same w-row (w >= 8: vl % 8 < 4)
    // or, at w = 4, the next h-row (LH >= 2: a 16-voxel step stays inside one d-plane)
    static_assert(LW >= 3 || (LW == 2 && LH >= 2), "compile-time wgrad box");
    constexpr int D4 = LW >= 3 ? 4 : HWc;
    const int g = (lane >> 4) & 1, qq = (lane & 15) >> 2, pp = lane & 3;
    const int vl = 8 * hsel + qq;  // the lane's first voxel inside a step
    const int vrow = (vl >> LW) * HWc + (vl & ((1 << LW) - 1));  // its halo row offset
    const char* ab0 = buf + dy_off_bf16(vl, g * 16 + pp * 4);
    const char* ab1 = buf + dy_off_bf16(vl, 32 + g * 16 + pp * 4);
    const char* bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tap = tapof(j);
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      bb[j] = buf + DYBYTES + (vrow + (kd * HHc + kh) * HWc + kw) * Tr::XROW + (g * 16 + pp * 4) * 2;
    }
    auto cat = [](s16x4_t lo, s16x4_t hi) __attribute__((always_inline)) {
      return (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto hro = [](int s) __attribute__((always_inline)) {  // the step's first halo row (w = 0)
      const int v0 = 16 * s, rd = v0 >> (LH + LW), rh = (v0 >> LW) & ((1 << LH) - 1);
      return (rd * HHc + rh) * HWc * Tr::XROW;
    };
    s16x8_t fa[2][2], fb[2][3], f3[2];
    auto load = [&](int s, int set) __attribute__((always_inline)) {
      fa[set][0] = cat(tr_read(ab0, s * 2048), tr_read(ab0, s * 2048 + 512));
      fa[set][1] = cat(tr_read(ab1, s * 2048), tr_read(ab1, s * 2048 + 512));
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[set][j] = cat(tr_read(bb[j], hro(s)), tr_read(bb[j], hro(s) + D4 * Tr::XROW));
    };
    auto load3 = [&](int s, int set) __attribute__((always_inline)) {
      f3[set] = cat(tr_read(bb[3], hro(s)), tr_read(bb[3], hro(s) + D4 * Tr::XROW));
    };
    load(0, 0);
    if (four) load3(0, 0);
    static_for<NK>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, cs = s & 1, ns = cs ^ 1;
      stage(sc);  // the next box's halo pieces of this step (their address VALU under the MFMAs)
      if constexpr (s == NK / 2) mid();  // BNIN: the next box's BN apply under this box's MFMAs
      if constexpr (s + 1 < NK) load(s + 1, ns);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        acc[j] = mfma(fa[cs][0], fb[cs][j], acc[j]);
        acc[4 + j] = mfma(fa[cs][1], fb[cs][j], acc[4 + j]);
      }
      if (four) {
        if constexpr (s + 1 < NK) load3(s + 1, ns);
        acc[3] = mfma(fa[cs][0], f3[cs], acc[3]);
        acc[7] = mfma(fa[cs][1], f3[cs], acc[7]);
      }
    });
  };
  // K16: 32-voxel steps; lane (G = lane / 16, q, pp) reads voxels 8 G + q and 8 G + q + 4 of a
  // step (one w-row, or two adjacent h-rows at w = 4), A = dy^T rows co 16 c + 4 pp.., B = x
  // columns ci 16 t + 4 pp.. of the tap's halo rows; MFMAs walk co tile c outermost.
  auto compute_fixed16 = [&](const char* buf, auto&& mid, auto&& stage) __attribute__((always_inline)) {
    constexpr int LD = LBW >= 2 ? LBD : 0, LH = LBW >= 2 ? LBH : 0, LW = LBW >= 2 ? LBW : 4;
    constexpr int HHc = (1 << LH) + 2, HWc = (1 << LW) + 2;
    constexpr int NK = (1 << (LD + LH + LW)) / 32;
    static_assert(LW >= 3 || (LW == 2 && LH >= 3), "K16 box: a 32-voxel step stays in one d-plane");
    constexpr int D4 = LW >= 3 ? 4 : HWc;
    const int G4 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int vl = 8 * G4 + q;
    const int vrow = (vl >> LW) * HWc + (vl & ((1 << LW) - 1));
    const char* ab[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) ab[c] = buf + dy_off_bf16(vl, c * 16 + pp * 4);
    const char* bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tap = tapof(j);
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      bb[j] = buf + DYBYTES + (vrow + (kd * HHc + kh) * HWc + kw) * Tr::XROW + pp * 8;
    }
    auto cat = [](s16x4_t lo, s16x4_t hi) __attribute__((always_inline)) {
      return (s16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto hro = [](int s) __attribute__((always_inline)) {
      const int v0 = 32 * s, rd = v0 >> (LH + LW), rh = (v0 >> LW) & ((1 << LH) - 1);
      return (rd * HHc + rh) * HWc * Tr::XROW;
    };
    // one register set per operand: co tile c's A fragment of step s + 1 is read right after
    // c's MFMAs of step s (a whole step of slack); tap j's B fragments after their last use
    // (c = 3), a few MFMAs before the next step needs them (the other wave of the SIMD covers)
    s16x8_t fa[4], fb[4][2];
    auto loadA = [&](int s, int c) __attribute__((always_inline)) {
      fa[c] = cat(tr_read(ab[c], s * 4096), tr_read(ab[c], s * 4096 + 512));
    };
    auto loadB = [&](int s, int j) __attribute__((always_inline)) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
        fb[j][t] = cat(tr_read(bb[j], hro(s) + t * 32), tr_read(bb[j], hro(s) + D4 * Tr::XROW + t * 32));
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) loadA(0, c);
#pragma unroll
    for (int j = 0; j < NJ; ++j) loadB(0, j);
    if (four) loadB(0, 3);
    static_for<NK>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value;
      stage(sc);
      if constexpr (s == NK / 2) mid();  // BNIN: the next box's BN apply under this box's MFMAs
      static_for<4>([&](auto ccc) __attribute__((always_inline)) {
        constexpr int c = decltype(ccc)::value;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
          for (int t = 0; t < 2; ++t) acc16[j][c][t] = mfma16(fa[c], fb[j][t], acc16[j][c][t]);
          if constexpr (c == 3 && s + 1 < NK) loadB(s + 1, j);
        }
        if (four) {
#pragma unroll
          for (int t = 0; t < 2; ++t) acc16[3][c][t] = mfma16(fa[c], fb[3][t], acc16[3][c][t]);
          if constexpr (c == 3 && s + 1 < NK) loadB(s + 1, 3);
        }
        if constexpr (s + 1 < NK) loadA(s + 1, c);
      });
    });
  };
  // mid(): work placed halfway through the box's MFMA steps (compute_fixed), or after them
  // stage(s): called at the start of every k-step of the compile-time-box loops
  constexpr bool kSpread = !kX3 && !kX6 && LBW >= 2;
  auto compute_box = [&](const char* buf, auto&& mid, auto&& stage) __attribute__((always_inline)) {
    if constexpr (K16) {
      compute_fixed16(buf, mid, stage);
    } else if constexpr (kSpread) {
      compute_fixed(buf, mid, stage);
    } else {
      compute(buf);
      mid();
    }
  };
  auto nomid = []() __attribute__((always_inline)) {};
  auto nostage = [](auto) __attribute__((always_inline)) {};

  // bf16 hot path: both tiles arrive by buffer LDS-DMA (no register staging); the next box
  // streams in while this one computes.  The dy tile keeps dy_off_bf16's half swap (applied
  // to the source address); each wave instruction is all-dy or all-halo (2048 dy pieces);
  // out-of-range pieces read zeros.
  // BNIN: bit i = piece i of this thread is a real (in-range) x-halo piece
  // piece i (16 B; i < MAXP) of this thread for the box at (n, d0, h0, w0) into buf; returns
  // bit i when it is a real (in-range) x-halo piece (BNIN)
  auto stage_piece = [&](char* buf, int i, int n, int d0, int h0, int w0) -> uint32_t {
    const int pc0 = (tid & ~63) + i * kWThreads;  // wave-uniform first piece
    if (pc0 >= DYP + XP) return 0u;
    const uint32_t lb0 = lds_addr(buf);
    const int pc = pc0 + lane;
    uint32_t voff = kOOB;
    if (pc0 < DYP) {
      const int r = pc >> 3, q = pc & 7;
      const int ql = q ^ (((r >> 1) & 1) << 2);
      if (r < boxvol) {
        const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
        const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
        if (gd < p.D && gh < p.H && gw < p.W)
          voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * p.Cout + co_base + ql * 8) * 2);
      }
      if constexpr (WGRAD_ABL & 16) { asm volatile("" ::"v"(voff)); voff = kOOB; }
      if constexpr (WGRAD_ABL & 32) voff = (uint32_t)(pc * 16);
      dma16(buffer_desc(p.dy, p.dybytes), __builtin_amdgcn_readfirstlane(lb0 + pc0 * 16), voff, 0);
      return 0u;
    }
    const bool first = ci_base < p.c0;  // a 32-channel block lies in one source
    const int xs = first ? p.c0 : p.c1, xc = first ? ci_base : ci_base - p.c0;
    const int hp = pc - DYP;
    const int hv = hp >> 2, q = hp & 3;
    const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
    const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
    if (hp < XP && gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && xc + q * 8 < xs)
      voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * xs + xc + q * 8) * 2);
    if constexpr (WGRAD_ABL & 16) { asm volatile("" ::"v"(voff)); voff = kOOB; }
    if constexpr (WGRAD_ABL & 32) voff = (uint32_t)(pc * 16);
    dma16(buffer_desc(first ? p.x0 : p.x1, first ? p.x0bytes : p.x1bytes),
          __builtin_amdgcn_readfirstlane(lb0 + DYBYTES + (pc0 - DYP) * 16), voff, 0);
    return voff != kOOB ? 1u << i : 0u;
  };
  // compile-time boxes: each piece's source offset relative to its box origin does not depend
  // on the box, so it is formed once (prel: elements past the box-origin voxel's first channel,
  // pco: the halo coordinates hd | hh << 8 | hw << 16 of an x piece, -1 for padding pieces);
  // a box then costs one add per piece, plus 3 compares on boxes that touch the volume's border.
  // (Measured neutral here -- 819 vs 823-832 us at level 0, profiles/r5_wgrad_prel_abl.txt:
  // with two waves per SIMD the VALU already hid under the other wave's MFMAs; what the
  // fixed-address ablation gained, profiles/r5_wgrad_addr_abl.txt, was L2 hits, not arithmetic.)
  int prel[kSpread ? MAXP : 1], pco[kSpread ? MAXP : 1];
  if constexpr (kSpread) {
    const bool first = ci_base < p.c0;
    const int xs = first ? p.c0 : p.c1, xc = first ? ci_base : ci_base - p.c0;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int pc = (tid & ~63) + i * kWThreads + lane;
      if ((tid & ~63) + i * kWThreads < DYP) {
        const int r = pc >> 3, q = pc & 7;
        const int ql = q ^ (((r >> 1) & 1) << 2);
        const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
        prel[i] = ((rd * p.H + rh) * p.W + rw) * p.Cout + co_base + ql * 8;
        pco[i] = r < boxvol ? (rd | (rh << 8) | (rw << 16)) : -1;
      } else {
        const int hp = pc - DYP, hv = hp >> 2, q = hp & 3;
        const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
        prel[i] = (((hd_ - 1) * p.H + (hh_ - 1)) * p.W + (hw_ - 1)) * xs + xc + q * 8;
        pco[i] = (hp < XP && xc + q * 8 < xs) ? (hd_ | (hh_ << 8) | (hw_ << 16)) : -1;
      }
    }
  }
  // piece i of the box at (n, d0, h0, w0): `inner` = the box and its halo lie inside the volume
  auto stage_piece_fast = [&](char* buf, int i, int n, int d0, int h0, int w0, bool inner) -> uint32_t {
    const int pc0 = (tid & ~63) + i * kWThreads;
    if (pc0 >= DYP + XP) return 0u;
    const uint32_t lb0 = lds_addr(buf);
    const int c = pco[i];
    const long vb = ((long)(n * p.D + d0) * p.H + h0) * p.W + w0;
    uint32_t voff;
    if (pc0 < DYP) {
      voff = (uint32_t)((vb * p.Cout + prel[i]) * 2);
      if (c < 0) voff = kOOB;
      else if (!inner && (d0 + (c & 255) >= p.D || h0 + ((c >> 8) & 255) >= p.H || w0 + (c >> 16) >= p.W)) voff = kOOB;
      dma16(buffer_desc(p.dy, p.dybytes), __builtin_amdgcn_readfirstlane(lb0 + pc0 * 16), voff, 0);
      return 0u;
    }
    const bool first = ci_base < p.c0;
    const int xs = first ? p.c0 : p.c1;
    voff = (uint32_t)((vb * xs + prel[i]) * 2);
    if (c < 0) {
      voff = kOOB;
    } else if (!inner) {
      const int gd = d0 + (c & 255) - 1, gh = h0 + ((c >> 8) & 255) - 1, gw = w0 + (c >> 16) - 1;
      if ((unsigned)gd >= (unsigned)p.D || (unsigned)gh >= (unsigned)p.H || (unsigned)gw >= (unsigned)p.W) voff = kOOB;
    }
    if constexpr (WGRAD_ABL & 16) { asm volatile("" ::"v"(voff)); voff = kOOB; }
    if constexpr (WGRAD_ABL & 32) voff = (uint32_t)((pc0 + lane) * 16);
    dma16(buffer_desc(first ? p.x0 : p.x1, first ? p.x0bytes : p.x1bytes),
          __builtin_amdgcn_readfirstlane(lb0 + DYBYTES + (pc0 - DYP) * 16), voff, 0);
    return voff != kOOB ? 1u << i : 0u;
  };
  // a whole box at once (runtime-geometry kernels and the first box)
  auto stage_dma = [&](char* buf, int b) -> uint32_t {
    uint32_t xm = 0;
    int n, d0, h0, w0;
    box_origin(b, n, d0, h0, w0);
    const uint32_t lb0 = lds_addr(buf);
    const bool first = ci_base < p.c0;  // a 32-channel block lies in one source
    const i32x4_t xr = buffer_desc(first ? p.x0 : p.x1, first ? p.x0bytes : p.x1bytes);
    const i32x4_t dr = buffer_desc(p.dy, p.dybytes);
    const int xs = first ? p.c0 : p.c1, xc = first ? ci_base : ci_base - p.c0;
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      const int pc0 = (tid & ~63) + i * kWThreads;  // wave-uniform first piece
      if (pc0 >= DYP + XP) break;
      const int pc = pc0 + lane;
      uint32_t voff = kOOB;
      if (pc0 < DYP) {
        const int r = pc >> 3, q = pc & 7;
        const int ql = q ^ (((r >> 1) & 1) << 2);
        if (r < boxvol) {
          const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
          const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
          if (gd < p.D && gh < p.H && gw < p.W)
            voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * p.Cout + co_base + ql * 8) * 2);
        }
        dma16(dr, __builtin_amdgcn_readfirstlane(lb0 + pc0 * 16), voff, 0);
      } else {
        const int hp = pc - DYP;
        const int hv = hp >> 2, q = hp & 3;
        const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
        const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
        if (hp < XP && gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && xc + q * 8 < xs)
          voff = (uint32_t)(((((n * p.D + gd) * p.H + gh) * p.W + gw) * xs + xc + q * 8) * 2);
        dma16(xr, __builtin_amdgcn_readfirstlane(lb0 + DYBYTES + (pc0 - DYP) * 16), voff, 0);
        if (voff != kOOB) xm |= 1u << i;
      }
    }
    return xm;
  };
  // BNIN: this thread's landed x pieces of buffer buf in place (every piece of a thread has
  // channel group q = tid & 3: DYP and the 512-piece rounds are multiples of 4)
  float* bnt = reinterpret_cast<float*>(wlds + Tr::NBUF * BUFBYTES);
  auto bn_x = [&](char* buf, uint32_t xm) {
    const int q = tid & 3;
    const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(bnt + q * 8), s1 = *reinterpret_cast<const f32x4_t*>(bnt + q * 8 + 4);
    const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(bnt + 32 + q * 8);
    const f32x4_t h1 = *reinterpret_cast<const f32x4_t*>(bnt + 32 + q * 8 + 4);
    const float sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
      if (!((xm >> i) & 1)) continue;
      u32x4_t* v = reinterpret_cast<u32x4_t*>(buf + DYBYTES + (tid + i * kWThreads - DYP) * 16);
      u32x4_t x = *v;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        x[k] = pack_bf16x2(bn_relu1(__uint_as_float(x[k] << 16), sc[2 * k], sh[2 * k]),
                           bn_relu1(__uint_as_float(x[k] & 0xffff0000u), sc[2 * k + 1], sh[2 * k + 1]));
      *v = x;
    }
  };
  if constexpr (BNIN) {
    if (tid < 32) {
      const int c = ci_base + tid;
      bnt[tid] = c < p.Cin ? p.isc[c] : 0.f;
      bnt[32 + tid] = c < p.Cin ? p.ish[c] : 0.f;
    }
    __syncthreads();
  }

  if (!kX6 && b_beg < b_end && p.dma) {
    if constexpr (Tr::NBUF == 2) {
      uint32_t xm = stage_dma(wlds, b_beg);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if constexpr (BNIN) bn_x(wlds, xm);
      __syncthreads();
      for (int b = b_beg; b < b_end; ++b) {
        const int cur = (b - b_beg) & 1;
        const bool nxt = b + 1 < b_end && !(WGRAD_ABL & 2);
        char* nbuf = wlds + (cur ^ 1) * BUFBYTES;
        // compile-time boxes: the next box's pieces are issued PPS per k-step over the first
        // SPW steps, so their address arithmetic runs on the VALU beside this box's MFMAs
        // instead of in a block before them (where both waves of a SIMD stalled the MFMA pipe
        // together); they land long before the box-end wait (BNIN: before its apply at NK / 2)
        int n1 = 0, d1 = 0, h1 = 0, w1 = 0;
        bool inner1 = false;
        if constexpr (kSpread && !(WGRAD_ABL & 4)) {
          if (nxt) {
            box_origin(b + 1, n1, d1, h1, w1);
            inner1 = d1 >= 1 && d1 + bd < p.D && h1 >= 1 && h1 + bh < p.H && w1 >= 1 && w1 + bw < p.W;
          }
          xm = 0;
        } else if (nxt) {
          xm = stage_dma(nbuf, b + 1);
        }
        auto stage = [&](auto sc) __attribute__((always_inline)) {
          if constexpr (kSpread) {
            constexpr int st = decltype(sc)::value;
            constexpr int NKc = (1 << (LBD + LBH + LBW)) / (K16 ? 32 : 16);
            constexpr int SPW = BNIN ? NKc / 4 : NKc / 2;
            constexpr int PPS = (MAXP + SPW - 1) / SPW;
            if constexpr (st * PPS < MAXP) {
              if (nxt) {
#pragma unroll
                for (int k = 0; k < PPS; ++k)
                  if (st * PPS + k < MAXP) xm |= stage_piece_fast(nbuf, st * PPS + k, n1, d1, h1, w1, inner1);
              }
            }
          }
        };
        if constexpr (BNIN) {
          // this thread's pieces of box b + 1 have landed once its vmcnt drains (LDS-DMA
          // completion is per wave); nobody reads buffer cur ^ 1 before the barrier below
          compute_box(wlds + cur * BUFBYTES, [&]() __attribute__((always_inline)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (b + 1 < b_end) bn_x(nbuf, xm);
          }, stage);
        } else if constexpr (!(WGRAD_ABL & 4)) {
          compute_box(wlds + cur * BUFBYTES, nomid, stage);
        }
        if constexpr (!(WGRAD_ABL & 8)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  } else if (kX6 && b_beg < b_end && p.dma) {
    if constexpr (kX6) {
      // fp32 build (bf16x6) with LDS-DMA: box b + 1 streams into the fp32 staging buffer while
      // box b's MFMAs run on its split tiles; between boxes every thread splits its pieces of
      // the landed box into the h / m / l tiles (the values stage_x3 writes)
      stage_raw(b_beg);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      for (int b = b_beg; b < b_end; ++b) {
        split_raw(wlds);
        __syncthreads();
        if (b + 1 < b_end) stage_raw(b + 1);
        compute(wlds);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  } else if (b_beg < b_end) {
    if constexpr (Tr::NBUF == 2) {
      stage_load(b_beg);
      stage_store(wlds);
      __syncthreads();
      for (int b = b_beg; b < b_end; ++b) {
        const int cur = (b - b_beg) & 1;
        if (b + 1 < b_end) stage_load(b + 1);
        compute_box(wlds + cur * BUFBYTES, nomid, nostage);
        if (b + 1 < b_end) stage_store(wlds + (cur ^ 1) * BUFBYTES);
        __syncthreads();
      }
    } else {
      // fp32 build: synchronous staging (all of a box's loads in flight, split on the way
      // into LDS), then the box's MFMAs
      for (int b = b_beg; b < b_end; ++b) {
        __syncthreads();
        stage_x3(wlds, b);
        __syncthreads();
        compute(wlds);
      }
    }
  }

  // flush: C[row = co][col = ci] of tap -> this split's partial row dwt[split][tap][co][ci]
  // with plain stores (two 128-B row segments per instruction); the splits are summed in a
  // fixed order by wgrad_group_sum_kernel / wgrad_reduce_kernel.  (fp32 atomics from every
  // split into one [27][Cout][Cin] image serialised on the contended addresses: 2-4x the
  // kernel's own time at level 0.)
  float* prow = p.dwt + (long)split * 27 * p.Cout * p.Cin;
  {
    if (p.direct) {
      // one split: no partial rows to reduce.  Per 32-row co half, the workgroup's
      // [32 co][32 ci][27 taps] tile is transposed through LDS (the staging buffers are free)
      // and added to the contiguous [ci][27] runs of the torch-layout dw.
      float* tile = reinterpret_cast<float*>(wlds);
      const int nci = min(32, p.cw - ci_base);
      for (int ct = 0; ct < 2; ++ct) {
        __syncthreads();
        if constexpr (pack4) {
          const int tap = 4 * wave + ((lane & 31) >> 3);
          if (wave < 7 && tap < 27)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int col = (e & 3) + 8 * (e >> 2) + 4 * hsel;
              tile[(col * 32 + (lane & 7)) * 27 + tap] = acc[ct * 4][e];
            }
        } else if constexpr (K16) {
          // acc16[j][c][t] element e: co 16 c + 4 (lane / 16) + e, ci 16 t + lane % 16
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!owned(j)) continue;
            const int tap = tapof(j);
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
              for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int col = cc * 16 + 4 * (lane >> 4) + e;
                  tile[(col * 32 + t * 16 + (lane & 15)) * 27 + tap] = acc16[j][2 * ct + cc][t][e];
                }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!owned(j)) continue;
            const int tap = tapof(j);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int col = (e & 3) + 8 * (e >> 2) + 4 * hsel;
              tile[(col * 32 + (lane & 31)) * 27 + tap] = acc[ct * 4 + j][e];
            }
          }
        }
        __syncthreads();
        if (TG) {
          // this group's taps only (the other group's workgroup writes the rest of each run)
          for (int i = tid; i < 32 * 32 * 27; i += kWThreads) {
            const int col = i / 864, r = i % 864, tap = r % 27;
            const int co = co_base + ct * 32 + col;
            if (co < p.Cout && r < nci * 27 && (tap >= 16) == (tgrp == 1)) {
              float* d = p.dw + ((long)co * p.cw + ci_base) * 27 + r;
              *d = p.store ? tile[i] : *d + tile[i];
            }
          }
        } else if (nci == 32) {
          // whole 32 x 864-float runs: 16-B read-modify-writes, all of a thread's loads in
          // flight before the first add (a dependent load -> add -> store chain per element
          // made the deep levels latency-bound)
          constexpr int kQ = 32 * 216, kPer = (kQ + kWThreads - 1) / kWThreads;
          f32x4_t g[kPer];
#pragma unroll
          for (int k = 0; k < kPer; ++k) {
            const int q4 = tid + k * kWThreads, row = q4 / 216, q = q4 % 216;
            g[k] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            if (q4 < kQ && !p.store)  // store: plain stores, nothing to read back
              g[k] = *reinterpret_cast<const f32x4_t*>(p.dw + ((long)(co_base + ct * 32 + row) * p.cw + ci_base) * 27 + 4 * q);
          }
#pragma unroll
          for (int k = 0; k < kPer; ++k) {
            const int q4 = tid + k * kWThreads, row = q4 / 216, q = q4 % 216;
#if WGRAD_ABL & 1  // ablation build: the flush's global stores dropped
            const f32x4_t o = g[k] + *reinterpret_cast<const f32x4_t*>(tile + row * 864 + 4 * q);
            if (q4 < kQ && o[0] == 1.2345e30f)
              *reinterpret_cast<f32x4_t*>(p.dw + ((long)(co_base + ct * 32 + row) * p.cw + ci_base) * 27 + 4 * q) = o;
#else
            if (q4 < kQ)
              *reinterpret_cast<f32x4_t*>(p.dw + ((long)(co_base + ct * 32 + row) * p.cw + ci_base) * 27 + 4 * q) =
                  g[k] + *reinterpret_cast<const f32x4_t*>(tile + row * 864 + 4 * q);
#endif
          }
        } else {
          for (int i = tid; i < 32 * 32 * 27; i += kWThreads) {
            const int col = i / 864, r = i % 864;  // r = ci * 27 + tap
            const int co = co_base + ct * 32 + col;
            if (co < p.Cout && r < nci * 27) {
              float* d = p.dw + ((long)co * p.cw + ci_base) * 27 + r;
              *d = p.store ? tile[i] : *d + tile[i];
            }
          }
        }
      }
      return;
    }
    if constexpr (pack4) {
      const int tap = 4 * wave + ((lane & 31) >> 3), ci = ci_base + (lane & 7);
      if (wave < 7 && tap < 27 && ci < p.Cin)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int co = co_base + ct * 32 + (e & 3) + 8 * (e >> 2) + 4 * hsel;
            if (co < p.Cout) prow[((long)tap * p.Cout + co) * p.Cin + ci] = acc[ct * 4][e];
          }
      return;
    }
    if constexpr (K16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!owned(j)) continue;
        const int tap = tapof(j);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int co = co_base + c * 16 + 4 * (lane >> 4) + e;
              const int ci = ci_base + t * 16 + (lane & 15);
              if (co < p.Cout && ci < p.Cin) prow[((long)tap * p.Cout + co) * p.Cin + ci] = acc16[j][c][t][e];
            }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!owned(j)) continue;
      const int tap = tapof(j);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int co = co_base + ct * 32 + (e & 3) + 8 * (e >> 2) + 4 * hsel;
          const int ci = ci_base + (lane & 31);
          if (co < p.Cout && ci < p.Cin) prow[((long)tap * p.Cout + co) * p.Cin + ci] = acc[ct * 4 + j][e];
        }
    }
  }
}

// Weight-gradient split reduction (deterministic, fixed order).  part: S rows of
// E = 27 * Cout * Cin floats ([split][tap][co][ci], Cin = stored channels).
// Stage 1 (S > 16): rows r*16 .. r*16+15 summed in place into row r*16.
__global__ void __launch_bounds__(256) wgrad_group_sum_kernel(float* part, int S, long E) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= E) return;
  const int r0 = blockIdx.y * 16, r1 = min(S, r0 + 16);
  part[(long)r0 * E + e] = sum_rows16(part + (long)r0 * E + e, E, r1 - r0);
}
// Stage 2: dw [Cout][Cw][27] (torch OIDHW, the weight's own input-channel count Cw <= Cin;
// stem: 5 of 8) += sum of R rows spaced `stride` rows apart.  Block = (co, 32 channels): the
// [27][32] tiles are read as 128-B rows, transposed through LDS, added to the contiguous
// 32 x 27 run of dw.
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* part, int R, int stride, float* dw,
                                                           int Cout, int Cin, int Cw, int store) {
  __shared__ float tile[27][33];
  const int co = blockIdx.x, ci0 = blockIdx.y * 32;
  const long rstep = (long)stride * 27 * Cout * Cin;
  for (int e = threadIdx.x; e < 27 * 32; e += 256) {
    const int t = e >> 5, c = e & 31, ci = ci0 + c;
    float sum = 0.f;
    if (ci < Cw) {
      sum = sum_rows16(part + ((long)t * Cout + co) * Cin + ci, rstep, R);
    }
    tile[t][c] = sum;
  }
  __syncthreads();
  float* dst = dw + ((long)co * Cw + ci0) * 27;
  const int n = min(32, Cw - ci0) * 27;
  for (int e = threadIdx.x; e < n; e += 256) dst[e] = store ? tile[e % 27][e / 27] : dst[e] + tile[e % 27][e / 27];
}

// Both stages in one launch, same sums bit for bit: the S split rows as G = ceil(S / 16)
// groups of 16, each group summed in row order by one thread, the G group sums then added in
// group order (= wgrad_group_sum_kernel + wgrad_reduce_kernel).  Block = (co, 32 channels) x
// GL group lanes: 256 element lanes (up to 4 of the 864 [27][32] elements each) per group
// lane, all of a group's rows for all of a thread's elements loaded before the first add
// (the two-stage form was a 57 MB pass plus a latency-bound 3.5 MB pass per level-0/1 layer).
// LDS: the [G][27 x 32] group sums.
constexpr int kWredMaxGroups = 16;  // and 16 rows x E floats per group below 2 GB (host check)
static int g_wred_fused = 1;  // 0: the two-stage reduction (A/B, bit-identity test)
template <int GL>
__global__ void __launch_bounds__(256 * GL) wgrad_reduce_fused_kernel(const float* part, int S, float* dw, int Cout,
                                                                      int Cin, int Cw, int store) {
  extern __shared__ float gsum[];  // [G][864]
  constexpr int NE = 27 * 32;
  const int co = blockIdx.x, ci0 = blockIdx.y * 32;
  const long E = 27L * Cout * Cin;
  const int G = (S + 15) / 16;
  const int el = threadIdx.x & 255, gl = threadIdx.x >> 8;
  // 32-bit byte offsets from the group's (uniform) first row: 16 rows x E floats < 2 GB
  uint32_t off[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = el + 256 * k, t = e >> 5, c = e & 31;
    ok[k] = e < NE && ci0 + c < Cw;
    off[k] = ok[k] ? (uint32_t)((((long)t * Cout + co) * Cin + ci0 + c) * 4) : 0u;
  }
  const uint32_t rowb = (uint32_t)(E * 4);
  for (int g = gl; g < G; g += GL) {
    const int r0 = g * 16, n = min(16, S - r0);
    // the group's rows through a descriptor: row offset in the SGPR soffset, element offset in
    // one VGPR (a 64-bit address per load held 128 VGPRs of addresses)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(part + (long)r0 * E), (short)0, (int)(n * rowb), 0x00020000);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 16; h += 8) {  // 8 rows x 4 elements in flight, added in row order
      float v[4][8];
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (h + r < n && ok[k])
            v[k][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)off[k], (int)((h + r) * rowb), 0));
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (h + r < n && ok[k]) s[k] += v[k][r];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = el + 256 * k;
      if (e < NE) gsum[g * NE + e] = s[k];
    }
  }
  __syncthreads();
  float* dst = dw + ((long)co * Cw + ci0) * 27;
  const int n = min(32, Cw - ci0) * 27;
  for (int o = threadIdx.x; o < n; o += 256 * GL) {
    const int c = o / 27, t = o % 27, e = t * 32 + c;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += gsum[g * NE + e];
    dst[o] = store ? s : dst[o] + s;
  }
}

}  // namespace

// bf16 grids of at most this many boxes split their taps over two workgroups (TG) before
// splitting their voxels (partial rows + a reduction pass); 0 disables
static int g_wgrad_tg_maxbox = 64;
// compile-time-box bf16 weight gradients on v_mfma_f32_16x16x32_bf16 (1) or 32x32x16 (0, the
// product: the 16x16x32 form ran at a higher clock but slower, profiles/r5_wgrad_k16_abl.txt)
static int g_wgrad_k16 = 0;
// the fp32 build's weight gradient streams its boxes by LDS-DMA into an fp32 staging buffer (1)
// or stages each box synchronously through registers (0, the product): with the 64-voxel boxes
// of round 6 both run the fp32 step in the same time (66.5 vs 66.2 ms, profiles/r6_x6_ab.txt) --
// the kernel is bound by its LDS fragment reads, not by the box stream
static int g_wgrad_x6_dma = 0;
// Weight-gradient launch plan: box geometry, boxes per split, split count (shared by the
// launch and its workspace query)
struct WgradPlan { Box b; int nbd, nbh, nbw, nbox, bps, splits, ntg; };
static WgradPlan wgrad_plan(int dtype, int N, int D, int H, int W, int Cin, int Cout, int target_wgs) {
  WgradPlan q;
  const int bv = dtype == PCMS_BF16 ? WTraits<bf16_t>::BV : dtype == PCMS_F32X3 ? WTraits<x3_t>::BV : WTraits<x6_t>::BV;
  const int halo = dtype == PCMS_F32 ? WTraits<x6_t>::HALO : kWHaloMax;
  q.b = choose_box(D, H, W, bv, halo, 4, 16);
  q.nbd = cdiv(D, 1 << q.b.lbd); q.nbh = cdiv(H, 1 << q.b.lbh); q.nbw = cdiv(W, 1 << q.b.lbw);
  q.nbox = N * q.nbd * q.nbh * q.nbw;
  const int tiles = (Cout / 64) * cdiv(Cin, 32);
  if (target_wgs <= 0) target_wgs = 512;
  q.ntg = dtype == PCMS_BF16 && q.nbox <= g_wgrad_tg_maxbox && tiles < target_wgs ? 2 : 1;
  const int splits = std::max(1, std::min(q.nbox, cdiv(target_wgs, tiles * q.ntg)));
  q.bps = cdiv(q.nbox, splits);
  q.splits = cdiv(q.nbox, q.bps);
  return q;
}

// Weight gradient: dw (torch layout [Cout][cin_w][27], fp32) += sum_v dy (x) x, where
// cin_w <= c0 + c1 is the weight's input-channel count (the stored input may be padded).
// dwt: pcms_conv3_wgrad_ws_floats(...) fp32 workspace (per-split partial rows, summed in a
// fixed order: the result is deterministic).
static int conv3_wgrad_any(int dtype, const void* x0, int c0, const void* x1, int c1, const float* isc,
                           const float* ish, const void* dy, float* dw, float* dwt, int N, int D, int H, int W,
                           int Cout, int cin_w, int target_wgs, int flags, hipStream_t s) {
  const int Cin = c0 + c1;
  if (cin_w <= 0 || cin_w > Cin) return -4;
  if (flags & ~PCMS_GRAD_STORE) return -8;
  const int VEC = dtype == PCMS_BF16 ? 8 : 4;
  if (Cout % 64 != 0 || c0 % VEC != 0 || c1 % VEC != 0) return -1;
  const WgradPlan q = wgrad_plan(dtype, N, D, H, W, Cin, Cout, target_wgs);
  WgradParams p;
  p.x0 = x0; p.x1 = x1; p.c0 = c0; p.c1 = c1; p.dy = dy; p.dwt = dwt;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.lbd = q.b.lbd; p.lbh = q.b.lbh; p.lbw = q.b.lbw;
  p.nbd = q.nbd; p.nbh = q.nbh; p.nbw = q.nbw;
  p.nbox = q.nbox;
  p.boxes_per_split = q.bps;
  const long nvox = (long)N * D * H * W;
  // LDS-DMA staging: bf16, and the fp32 (bf16x6) build's fp32 staging buffer (g_wgrad_x6_dma)
  const int es = dtype == PCMS_BF16 ? 2 : 4;
  p.dma = (dtype == PCMS_BF16 || (dtype == PCMS_F32 && g_wgrad_x6_dma)) && (c1 == 0 || c0 % 32 == 0) &&
          nvox * std::max(Cout, std::max(c0, c1)) * es < (long)kOOB;
  p.x0bytes = (uint32_t)(p.dma ? nvox * c0 * es : 0);
  p.x1bytes = (uint32_t)(p.dma ? nvox * c1 * es : 0);
  p.dybytes = (uint32_t)(p.dma ? nvox * Cout * es : 0);
  const int splits = q.splits;
  p.nco = Cout / 64;
  p.nci = cdiv(Cin, 32);
  p.dw = dw;
  p.cw = cin_w;
  p.direct = splits == 1;
  p.store = flags & PCMS_GRAD_STORE;
  p.ntg = q.ntg;
  p.isc = isc; p.ish = ish;
  if (isc && (!p.dma || c1 != 0 || q.ntg != 1)) return -5;  // BNIN: the LDS-DMA one-source kernels
  dim3 grid(splits * p.nco * p.nci * q.ntg);
  size_t lds;
  if (dtype == PCMS_BF16 && isc) {
    lds = (size_t)WTraits<bf16_t>::NBUF * (WTraits<bf16_t>::BV * WTraits<bf16_t>::DYROW + kWHaloMax * WTraits<bf16_t>::XROW) +
          64 * sizeof(float);
    auto kern = conv3_wgrad_kernel<bf16_t, -1, -1, -1, false, false, true>;
    const bool k16 = g_wgrad_k16;
    if (q.b.lbd == 2 && q.b.lbh == 2 && q.b.lbw == 4)
      kern = k16 ? conv3_wgrad_kernel<bf16_t, 2, 2, 4, false, false, true, true> : conv3_wgrad_kernel<bf16_t, 2, 2, 4, false, false, true>;
    else if (q.b.lbd == 1 && q.b.lbh == 3 && q.b.lbw == 4)
      kern = k16 ? conv3_wgrad_kernel<bf16_t, 1, 3, 4, false, false, true, true> : conv3_wgrad_kernel<bf16_t, 1, 3, 4, false, false, true>;
    else if (q.b.lbd == 2 && q.b.lbh == 3 && q.b.lbw == 3)
      kern = k16 ? conv3_wgrad_kernel<bf16_t, 2, 3, 3, false, false, true, true> : conv3_wgrad_kernel<bf16_t, 2, 3, 3, false, false, true>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(kWThreads), lds, s, p);
  } else if (dtype == PCMS_BF16) {
    lds = (size_t)WTraits<bf16_t>::NBUF * (WTraits<bf16_t>::BV * WTraits<bf16_t>::DYROW + kWHaloMax * WTraits<bf16_t>::XROW);
    auto kern = conv3_wgrad_kernel<bf16_t, -1, -1, -1>;
    if (q.ntg == 2) {
      kern = conv3_wgrad_kernel<bf16_t, -1, -1, -1, true>;
      if (q.b.lbd == 2 && q.b.lbh == 3 && q.b.lbw == 3) kern = conv3_wgrad_kernel<bf16_t, 2, 3, 3, true>;
    } else if (q.b.lbd == 2 && q.b.lbh == 2 && q.b.lbw == 4) {
      kern = g_wgrad_k16 ? conv3_wgrad_kernel<bf16_t, 2, 2, 4, false, false, false, true> : conv3_wgrad_kernel<bf16_t, 2, 2, 4>;
    } else if (q.b.lbd == 1 && q.b.lbh == 3 && q.b.lbw == 4) {
      kern = g_wgrad_k16 ? conv3_wgrad_kernel<bf16_t, 1, 3, 4, false, false, false, true> : conv3_wgrad_kernel<bf16_t, 1, 3, 4>;
    } else if (q.b.lbd == 2 && q.b.lbh == 3 && q.b.lbw == 3) {
      kern = g_wgrad_k16 ? conv3_wgrad_kernel<bf16_t, 2, 3, 3, false, false, false, true> : conv3_wgrad_kernel<bf16_t, 2, 3, 3>;
    } else if (q.b.lbd == 3 && q.b.lbh == 3 && q.b.lbw == 2) {  // level 4
      kern = g_wgrad_k16 ? conv3_wgrad_kernel<bf16_t, 3, 3, 2, false, false, false, true> : conv3_wgrad_kernel<bf16_t, 3, 3, 2>;
    }
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(kWThreads), lds, s, p);
  } else if (dtype == PCMS_F32X3) {
    typedef WTraits<x3_t> X;
    lds = (size_t)X::NPART * (X::BV * X::DYROW + X::HALO * X::XROW);
    (void)hipFuncSetAttribute((const void*)conv3_wgrad_kernel<x3_t, -1, -1, -1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((conv3_wgrad_kernel<x3_t, -1, -1, -1>), grid, dim3(kWThreads), lds, s, p);
  } else {
    typedef WTraits<x6_t> X;
    lds = (size_t)X::NPART * (X::BV * X::DYROW + X::HALO * X::XROW) + (p.dma ? X::RAWBYTES : 0);
    // the direct (one-split) flush transposes a [32 co][32 ci][27] fp32 tile through LDS
    if (p.direct) lds = std::max(lds, (size_t)32 * 32 * 27 * sizeof(float));
    auto kern = Cin <= 8 ? conv3_wgrad_kernel<x6_t, -1, -1, -1, false, true> : conv3_wgrad_kernel<x6_t, -1, -1, -1>;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(kWThreads), lds, s, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (p.direct) return 0;  // the kernel added into dw itself
  const long E = 27L * Cout * Cin;
  const int G = cdiv(splits, 16);
  if (g_wred_fused && G <= kWredMaxGroups && E * 16 * 4 < (1L << 31)) {
    const dim3 grid(Cout, cdiv(cin_w, 32));
    const size_t glds = (size_t)G * 27 * 32 * sizeof(float);
    if (G >= 4)
      hipLaunchKernelGGL(wgrad_reduce_fused_kernel<4>, grid, dim3(1024), glds, s, (const float*)dwt, splits, dw, Cout,
                         Cin, cin_w, p.store);
    else if (G >= 2)
      hipLaunchKernelGGL(wgrad_reduce_fused_kernel<2>, grid, dim3(512), glds, s, (const float*)dwt, splits, dw, Cout,
                         Cin, cin_w, p.store);
    else
      hipLaunchKernelGGL(wgrad_reduce_fused_kernel<1>, grid, dim3(256), glds, s, (const float*)dwt, splits, dw, Cout,
                         Cin, cin_w, p.store);
    PCMS_CHECK_LAUNCH();
  }
  int R = splits, stride = 1;
  if (splits > 16) {
    hipLaunchKernelGGL(wgrad_group_sum_kernel, dim3((unsigned)cdiv(E, 256), cdiv(splits, 16)), dim3(256), 0, s, dwt,
                       splits, E);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    R = cdiv(splits, 16);
    stride = 16;
  }
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(Cout, cdiv(cin_w, 32)), dim3(256), 0, s, (const float*)dwt, R, stride,
                     dw, Cout, Cin, cin_w, p.store);
  PCMS_CHECK_LAUNCH();
}

extern "C" {

// the compile-time-box bf16 weight gradients on 16x16x32 (1) or 32x32x16 (0) MFMAs; v < 0
// queries.  Returns the previous value.
int pcms_conv3_wgrad_k16(int v) {
  const int old = g_wgrad_k16;
  if (v >= 0) g_wgrad_k16 = v;
  return old;
}

// the fp32 (bf16x6) weight gradient's LDS-DMA box stream (1) or synchronous staging (0); v < 0
// queries.  Returns the previous value.
int pcms_conv3_wgrad_x6_dma(int v) {
  const int old = g_wgrad_x6_dma;
  if (v >= 0) g_wgrad_x6_dma = v;
  return old;
}

// the weight gradient's split rows summed by one launch (1) or by the two-stage group-sum +
// reduce pair (0), bit-identical; v < 0 queries.  Returns the previous value.
int pcms_conv3_wgrad_reduce_fused(int v) {
  const int old = g_wred_fused;
  if (v >= 0) g_wred_fused = v;
  return old;
}

// grids of at most v boxes split the taps of the bf16 weight gradient over two workgroups
// before splitting the voxels (0: never); v < 0 queries.  Returns the previous value.
int pcms_conv3_wgrad_tg_maxbox(int v) {
  const int old = g_wgrad_tg_maxbox;
  if (v >= 0) g_wgrad_tg_maxbox = v;
  return old;
}

// fp32 workspace floats pcms_conv3_wgrad needs: one [27][Cout][c0+c1] partial row per split
int pcms_conv3_wgrad_ws_floats(int dtype, int N, int D, int H, int W, int c0, int c1, int Cout, int target_wgs) {
  const int Cin = c0 + c1;
  return wgrad_plan(dtype, N, D, H, W, Cin, Cout, target_wgs).splits * 27 * Cout * Cin;
}

int pcms_conv3_wgrad(int dtype, const void* x0, int c0, const void* x1, int c1, const void* dy,
                     float* dw, float* dwt, int N, int D, int H, int W, int Cout, int cin_w, int target_wgs,
                     int flags, hipStream_t s) {
  return conv3_wgrad_any(dtype, x0, c0, x1, c1, nullptr, nullptr, dy, dw, dwt, N, D, H, W, Cout, cin_w, target_wgs,
                         flags, s);
}

// 1: pcms_conv3_fwd_bnin and pcms_conv3_wgrad_bnin (target_wgs) both run this bf16 layer
int pcms_conv3_bnin_ok(int N, int D, int H, int W, int cin, int Cout, int target_wgs) {
  const long nvox = (long)N * D * H * W;
  if (cin > kBgBnMax || cin % 16 || Cout % 64 || !big_fwd_ok(PCMS_BF16, N, D, H, W, cin, 0)) return 0;
  if (nvox * std::max(Cout, cin) * 2 >= (long)kOOB) return 0;
  return wgrad_plan(PCMS_BF16, N, D, H, W, cin, Cout, target_wgs).ntg == 1 ? 1 : 0;
}

// the weight gradient of the conv of relu(x * isc + ish) (pcms_conv3_fwd_bnin's forward):
// bf16, one source; the LDS-DMA shapes only (-5 otherwise)
int pcms_conv3_wgrad_bnin(int dtype, const void* x, int cin, const float* isc, const float* ish, const void* dy,
                          float* dw, float* dwt, int N, int D, int H, int W, int Cout, int cin_w, int target_wgs,
                          int flags, hipStream_t s) {
  if (!isc || !ish || dtype != PCMS_BF16) return -1;
  return conv3_wgrad_any(dtype, x, cin, nullptr, 0, isc, ish, dy, dw, dwt, N, D, H, W, Cout, cin_w, target_wgs,
                         flags, s);
}

}  // extern "C"
