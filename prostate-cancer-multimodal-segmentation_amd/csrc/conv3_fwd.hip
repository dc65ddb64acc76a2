// 3x3x3 / stride 1 / pad 1 convolution for the U-Net DoubleConv blocks, NDHWC, gfx950.
//
// Replaces nn.Conv3d(k=3, padding=1) of models/unet3d.py:29,35 (forward, and the two
// autograd backward products of aten::convolution_backward).
//
//   conv3_fwd   implicit GEMM  Y[v, co] = sum_{tap, ci} X[v + tap, ci] * W[co, ci, tap]
//               M = voxels (a spatial box of <= 512 voxels per workgroup), N = 64 output
//               channels per workgroup, K = 27 * Cin walked as (ci-chunk, tap).  The
//               chunk's (box + halo) input tile is staged once in LDS and re-read for all
//               27 taps through an LDS row offset; weights stream from L2 into registers.
//               Epilogue: + bias, store, per-workgroup BatchNorm partial sums (sum, sumsq).
//               Also serves dgrad (dX = conv(dY, W flipped + transposed)), with
//               `accumulate` and a two-pointer output for the concat split of Up3D.
//               This unit: the general kernel and the entry points; the big-box forms of
//               the hot levels are conv3_big.hip and conv3_b16.hip, the packs conv3_pack.hip.
//   conv3_wgrad (conv3_wgrad.hip)
//
// bf16 path: v_mfma_f32_32x32x16_bf16; fp32 path (parity build): v_mfma_f32_32x32x2_f32.
#include "common.h"
#include "pcms_hip.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "conv_common.h"
#include "conv3_units.h"

namespace {

// g_zero16 (conv_common.h) as the kernel below has always been compiled to reach it: a use the
// host can see makes the zero page an external symbol of the code object, addressed through
// the GOT (while all conv3 kernels were one translation unit, the weight gradient's staging
// lambdas were that use).  Kept so that this unit's eight kernels are the same instruction
// streams as before the split; without it they address the page pc-relative (two instructions
// fewer per reference, a change to time).
__host__ __device__ inline const void* conv3_zero16() { return g_zero16; }

// LBD/LBH/LBW >= 0: compile-time box geometry (the hot (4, 8, 16) box: halo decode and tap
// offsets become constant arithmetic); -1: runtime geometry from p.
// MTW: M-tiles per wave (4: 512-voxel boxes; 2: boxes of <= 256 voxels -- level 4's 8x8x4 --
// on all four waves instead of two)
// ablation builds of the general forward / dgrad (0 in the product): bit 1 the fp32 (split)
// chunks after a workgroup's first are not staged, 2 no MFMA phase for them
#ifndef CONV_ABL
#define CONV_ABL 0
#endif
template <typename T, int MINW, int LBD, int LBH, int LBW, int MTW = 4>
__global__ void __launch_bounds__(kThreads, MINW) conv3_fwd_kernel(Conv3Params p) {
  const int lbd_ = LBW >= 0 ? LBD : p.lbd, lbh_ = LBW >= 0 ? LBH : p.lbh, lbw_ = LBW >= 0 ? LBW : p.lbw;
  typedef Traits<T> Tr;
  typedef typename Tr::Frag Frag;
  __shared__ __attribute__((aligned(16))) char lds[kHaloMax * kRowBytes];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r_lane = lane & 31, hsel = lane >> 5;
  // 1-D grid of (box, co block, split), co block fastest in the logical id; the logical id is
  // XCD-aware (dispatch is round-robin over the 8 XCDs): an XCD runs consecutive logical ids,
  // i.e. every co block of a few adjacent boxes, which share their halos in its L2.  (The
  // other order -- an XCD holding every box of a few weight slices -- measured slower at
  // levels 2-3 in round 4: DESIGN.md §0c item 3(b).)
  const int nbox = p.N * p.nbd * p.nbh * p.nbw, nco = p.Cout >> 6;
  const int G = gridDim.x;
  const int lg = (G & 7) == 0 ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int bx = (lg / nco) % nbox, by = lg % nco;
  const int bz = lg / (nbox * nco);
  int mb = bx;
  const int bwi = mb % p.nbw; mb /= p.nbw;
  const int bhi = mb % p.nbh; mb /= p.nbh;
  const int bdi = mb % p.nbd;
  const int n = mb / p.nbd;
  const int co_base = by * 64;
  const int cbeg = bz * p.chunks_per_split;
  const int cend = min(p.nchunk, cbeg + p.chunks_per_split);
  const int bd = 1 << lbd_, bh = 1 << lbh_, bw = 1 << lbw_;
  const int boxvol = bd * bh * bw;
  const int d0 = bdi * bd, h0 = bhi * bh, w0 = bwi * bw;
  const int HH = bh + 2, HW = bw + 2;
  const int HV = (bd + 2) * HH * HW;

  const bool w16 = lbw_ == 4;
  const int prow = w16 ? perm32(r_lane) : r_lane;
  int hb[MTW];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    int r = wave * (32 * MTW) + mt * 32 + prow;
    if (r >= boxvol) r = 0;
    int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
    hb[mt] = (rd * HH + rh) * HW + rw;
  }
  const bool wave_active = wave * (32 * MTW) < boxvol;

  // fp32 data (x3_t / x6_t): the fp32 halo split into bf16 parts in LDS, three MFMAs per
  // (M-tile, N-tile, tap) instead of two
  constexpr bool kX3 = std::is_same<T, x3_t>::value, kX6 = std::is_same<T, x6_t>::value;
  constexpr bool kSplit = kX3 || kX6;
  typedef typename Tr::Mem M;
  f32x16_t acc[MTW][2];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const M* x0 = (const M*)p.x0;
  const M* x1 = (const M*)p.x1;
  const bf16_t* wp = (const bf16_t*)p.w;
  const long plane = (long)p.H * p.W;

  for (int chunk = cbeg; chunk < cend; ++chunk) {
#if CONV_ABL & 1  // ablation builds only (wrong results, timing): fp32 chunks after the first not staged
    if (kSplit && chunk > cbeg) goto compute_chunk;
#endif
    __syncthreads();
    // ---- stage the halo tile of this chunk by LDS-DMA: piece p (16 B) -> LDS [16p, 16p+16).
    // The LDS image is lane-linear, so the slot swizzle is applied to the SOURCE address
    // (physical slot qp of row hv holds logical slot qp ^ swz(hv)); out-of-range pieces
    // read the zero page.  All pieces are in flight at once (no register staging).
    for (int base = wave * 64; base < HV * 4; base += kThreads) {
      const int pc = base + lane;
      const int hv = pc >> 2;
      const int ql = (pc & 3) ^ swz(hv);
      const void* src = g_zero16;
      if (pc < HV * 4) {
        const int hw_ = hv % HW, t_ = hv / HW, hh_ = t_ % HH, hd_ = t_ / HH;
        const int gd = d0 + hd_ - 1, gh = h0 + hh_ - 1, gw = w0 + hw_ - 1;
        const int c = chunk * Tr::CK + ql * Tr::VEC;
        if (gd >= 0 && gd < p.D && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W && c < p.Cin &&
            ql * Tr::VEC < Tr::CK) {  // (x6: the row's slots 2, 3 stay zero)
          const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
          src = (c < p.c0) ? (const void*)(x0 + vox * p.c0 + c) : (const void*)(x1 + vox * p.c1 + (c - p.c0));
        }
      }
      __builtin_amdgcn_global_load_lds(src, (LDS_AS void*)(lds + base * 16), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (kX6) {
      // split every 8-channel fp32 row in place into logical slots [h | m | l | 0]
      for (int r = tid; r < HV; r += kThreads) {
        char* row = lds + r * kRowBytes;
        const int sw = swz(r);
        const f32x4_t q0 = *reinterpret_cast<const f32x4_t*>(row + ((0 ^ sw) * 16));
        const f32x4_t q1 = *reinterpret_cast<const f32x4_t*>(row + ((1 ^ sw) * 16));
        const float f[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
        u32x4_t h, m, l;
        split3x8(f, h, m, l);
        *reinterpret_cast<u32x4_t*>(row + ((0 ^ sw) * 16)) = h;
        *reinterpret_cast<u32x4_t*>(row + ((1 ^ sw) * 16)) = m;
        *reinterpret_cast<u32x4_t*>(row + ((2 ^ sw) * 16)) = l;
      }
      __syncthreads();
    }
    if constexpr (kX3) {
      // split every 16-channel fp32 row in place: logical 16-B slot s of the row (physical
      // s ^ swz) = [hi 0-7, hi 8-15, lo 0-7, lo 8-15], so lds_a(ks = 0 / 1) reads hi / lo
      for (int r = tid; r < HV; r += kThreads) {
        char* row = lds + r * kRowBytes;
        const int sw = swz(r);
        f32x4_t q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const f32x4_t*>(row + ((k ^ sw) * 16));
        u32x4_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const u32x2_t hl = split2(q[k][2 * i], q[k][2 * i + 1]);
            o[k >> 1][(k & 1) * 2 + i] = hl[0];
            o[2 + (k >> 1)][(k & 1) * 2 + i] = hl[1];
          }
#pragma unroll
        for (int s = 0; s < 4; ++s) *reinterpret_cast<u32x4_t*>(row + ((s ^ sw) * 16)) = o[s];
      }
      __syncthreads();
    }
#if CONV_ABL & 1
  compute_chunk:
#endif
    if (!wave_active) continue;
#if CONV_ABL & 2  // ablation builds only: no MFMA phase for the fp32 data
    if (kSplit) continue;
#endif

    const bf16_t* wchunk = wp + (long)chunk * 27 * p.Cout * Tr::WK;
    Frag bset[2][2][Tr::KS];
    auto load_b = [&](Frag (&dst)[2][Tr::KS], int tap) {
      if constexpr (std::is_same<T, bf16_t>::value) {
        // fragment-major pack (pack_bf16_off): block (row tile, ks) = one contiguous 1 KiB
        const bf16_t* wt = wchunk + ((long)tap * p.Cout + co_base) * 32 + lane * 8;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int ks = 0; ks < Tr::KS; ++ks)
            dst[nt][ks] = *reinterpret_cast<const s16x8_t*>(wt + nt * 1024 + ks * 512);
      } else {
        const bf16_t* wt = wchunk + ((long)tap * p.Cout + co_base + r_lane) * Tr::WK;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int ks = 0; ks < Tr::KS; ++ks) dst[nt][ks] = gl_b(wt + nt * 32 * Tr::WK, ks, hsel);
      }
    };
    load_b(bset[0], 0);
    // The A fragments roll through one register set: right after M-tile mt's MFMAs of tap t
    // its fragment of tap t + 1 is read (15 MFMAs of slack before its first use) instead of
    // one read -> wait -> two MFMAs per fragment.  B: two register sets, tap t + 1 loaded
    // while tap t computes (a third set, two taps ahead, pushed the kernel past 256 VGPRs into
    // spills with a reload inside this loop); taps walked two (kd, kh) rows per trip so every
    // set index is a compile-time constant.
    // x6: a[0] = [h|m], a[1] = [h|l] (logical slot 2 * hsel)
    auto frag1 = [&](int row) __attribute__((always_inline)) {
      if constexpr (kX6) return lds_slot(lds, row, 2 * hsel);
      else return lds_a(lds, row, 1, hsel);
    };
    s16x8_t a[2][MTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      a[0][mt] = lds_a(lds, hb[mt], 0, hsel);
      a[1][mt] = frag1(hb[mt]);
    }
    auto tap_step = [&](int tap, int set, const int (&hbk)[MTW]) {
      load_b(bset[set ^ 1], min(tap + 1, 26));
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this tap's MFMAs
      const int tn = tap + 1 < 27 ? tap + 1 : 0;
      const int offn = ((tn / 9) * HH + (tn / 3) % 3) * HW + tn % 3;
      if constexpr (kSplit) {
        // x3: hi*hi + lo*hi + hi*lo (a[0] = hi, a[1] = lo; B ks 0 = hi, 1 = lo)
        // x6: [h|m].[h|h] + [h|l].[m|h] + [h|m].[l|m] (a[0], a[1]; B ks 0, 1, 2)
        constexpr int b1 = kX6 ? 1 : 0, b2 = kX6 ? 2 : 1;
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma(a[0][mt], bset[set][nt][0], acc[mt][nt]);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma(a[1][mt], bset[set][nt][b1], acc[mt][nt]);
          a[1][mt] = frag1(hbk[mt] + offn);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma(a[0][mt], bset[set][nt][b2], acc[mt][nt]);
          a[0][mt] = lds_a(lds, hbk[mt] + offn, 0, hsel);
        }
#pragma unroll
        for (int i = 0; i < 2 * MTW; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);  // 3 MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma(a[ks][mt], bset[set][nt][ks], acc[mt][nt]);
            a[ks][mt] = lds_a(lds, hbk[mt] + offn, ks, hsel);
          }
        // (the scheduler would otherwise sink all eight reads below the last MFMA)
#pragma unroll
        for (int i = 0; i < 2 * MTW; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
        }
      }
    };
    for (int kdh = 0; kdh < 8; kdh += 2) {
      // row bases from an opaque copy: the fragment addresses are recomputed per trip rather
      // than hoisted out of the loops (and spilled)
      int hbk[MTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) hbk[mt] = opaque(hb[mt]);
#pragma unroll
      for (int j = 0; j < 6; ++j) tap_step(kdh * 3 + j, j & 1, hbk);
    }
    {
      int hbk[MTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) hbk[mt] = opaque(hb[mt]);
#pragma unroll
      for (int j = 0; j < 3; ++j) tap_step(24 + j, j & 1, hbk);
    }
  }

  // ---- epilogue ----
  // BatchNorm partials per workgroup row: (sum, M2 = sum of squared deviations from the
  // row's own mean) + the row's voxel count.  Each wave first forms its own per-channel
  // mean (two passes over the accumulator registers), waves are merged with Chan's formula:
  // no E[x^2] - E[x]^2 cancellation (BN over few voxels / large |mean| / std).
  float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
  float bias_l[2] = {0.f, 0.f};
  if (p.bias) {
    bias_l[0] = p.bias[co_base + r_lane];
    bias_l[1] = p.bias[co_base + 32 + r_lane];
  }
  const bool want_stats = p.stats && !p.yacc;
  const bool interior = d0 + bd <= p.D && h0 + bh <= p.H && w0 + bw <= p.W;
  uint64_t vmask = 0;  // bit mt * 16 + e: row valid
  if (wave_active) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = (e & 3) + 8 * (e >> 2) + 4 * hsel;
        const int r = wave * (32 * MTW) + mt * 32 + (w16 ? perm32(rr) : rr);
        bool valid = r < boxvol;
        if (valid && !interior) {
          const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
          valid = d0 + rd < p.D && h0 + rh < p.H && w0 + rw < p.W;
        }
        if (valid) vmask |= 1ull << (mt * 16 + e);
      }
  }
  constexpr int kRedOff = 512 * 64 * 2;  // bf16 C tile [512][64] occupies the first 64 KiB
  // (PCMS_CONV_RELU, eval with the BatchNorm folded into w / b: tested where used, from the
  // kernel argument -- a flag held across the epilogue cost a spill)
  if (!kSplit && !p.yacc && !(p.accumulate & PCMS_CONV_ACCUMULATE)) {
    // bf16 fast path: + bias, stats from the fp32 values, C tile -> LDS (box order), then
    // 16-byte coalesced stores (one box row = a contiguous w-run of voxels).
    __syncthreads();  // every wave is done reading the halo
    bf16_t* ct = reinterpret_cast<bf16_t*>(lds);
    if (wave_active) {
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rr = (e & 3) + 8 * (e >> 2) + 4 * hsel;
          const int r = wave * (32 * MTW) + mt * 32 + (w16 ? perm32(rr) : rr);
          const bool valid = (vmask >> (mt * 16 + e)) & 1;
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const float v = acc[mt][nt][e] + bias_l[nt];
            ct[r * 64 + nt * 32 + r_lane] = f2bf(v);
            if (valid) s1[nt] += v;
          }
        }
      }
    }
    __syncthreads();
    for (int pc = tid; pc < boxvol * 8; pc += kThreads) {
      const int r = pc >> 3, q = pc & 7;
      const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
      const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
      if (!interior && (gd >= p.D || gh >= p.H || gw >= p.W)) continue;
      const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
      const int co = co_base + q * 8;
      M* dst = (co < p.cy0) ? (M*)p.y0 + vox * p.cy0 + co : (M*)p.y1 + vox * (p.Cout - p.cy0) + (co - p.cy0);
      u32x4_t o = *reinterpret_cast<const u32x4_t*>(ct + r * 64 + q * 8);
      if (p.accumulate & PCMS_CONV_RELU) o = relu_bf16x8(o);
      *reinterpret_cast<u32x4_t*>(dst) = o;
    }
  } else if (wave_active) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (!((vmask >> (mt * 16 + e)) & 1)) continue;
        const int rr = (e & 3) + 8 * (e >> 2) + 4 * hsel;
        const int r = wave * (32 * MTW) + mt * 32 + (w16 ? perm32(rr) : rr);
        const int rd = r >> (lbh_ + lbw_), rh = (r >> lbw_) & (bh - 1), rw = r & (bw - 1);
        const int gd = d0 + rd, gh = h0 + rh, gw = w0 + rw;
        const long vox = ((long)n * p.D + gd) * plane + (long)gh * p.W + gw;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int co = co_base + nt * 32 + r_lane;
          float v = acc[mt][nt][e];
          if (p.yacc) {  // split-K: this split's own fp32 slab (summed in a fixed order later)
            p.yacc[((long)bz * p.nvox + vox) * p.Cout + co] = v;
            continue;
          }
          v += bias_l[nt];
          M* dst = (co < p.cy0) ? (M*)p.y0 + vox * p.cy0 + co
                                : (M*)p.y1 + vox * (p.Cout - p.cy0) + (co - p.cy0);
          if (p.accumulate & PCMS_CONV_ACCUMULATE) v += Elem<M>::ld(dst);  // (stats are refused with accumulate)
          if (p.accumulate & PCMS_CONV_RELU) v = fmaxf(v, 0.f);
          Elem<M>::st(dst, v);
          s1[nt] += v;
        }
      }
    }
  }
  if (want_stats) {
    // wave-level mean per channel (rows of a channel live in lanes r_lane and r_lane + 32)
    const float nw = (float)(__popcll(vmask) + __shfl_xor(__popcll(vmask), 32, 64));
    float mw[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s1[nt] += __shfl_xor(s1[nt], 32, 64);
      mw[nt] = nw > 0.f ? s1[nt] / nw : 0.f;
    }
    // squared deviations about the rounded wave mean, corrected by (sum d)^2 / n
    float sd[2] = {0.f, 0.f};
    if (wave_active) {
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if (!((vmask >> (mt * 16 + e)) & 1)) continue;
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const float d = acc[mt][nt][e] + bias_l[nt] - mw[nt];
            s2[nt] += d * d;
            sd[nt] += d;
          }
        }
    }
    __syncthreads();  // halo / C tile no longer read: reuse LDS for the cross-wave reduction
    float* red = reinterpret_cast<float*>(lds + (kSplit ? 0 : kRedOff));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s2[nt] += __shfl_xor(s2[nt], 32, 64);
      sd[nt] += __shfl_xor(sd[nt], 32, 64);
      if (nw > 0.f) s2[nt] -= sd[nt] * sd[nt] / nw;
      if (hsel == 0) {
        float* rp = red + (wave * 64 + nt * 32 + r_lane) * 3;
        rp[0] = s1[nt];
        rp[1] = s2[nt];
        rp[2] = nw;
      }
    }
    __syncthreads();
    if (tid < 64) {
      float S = 0.f, Nn = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        S += red[(w * 64 + tid) * 3 + 0];
        Nn += red[(w * 64 + tid) * 3 + 2];
      }
      const float m = Nn > 0.f ? S / Nn : 0.f;
      float M2 = 0.f, sdd = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float c = red[(w * 64 + tid) * 3 + 2];
        if (c > 0.f) {
          const float d = red[(w * 64 + tid) * 3 + 0] / c - m;
          M2 += red[(w * 64 + tid) * 3 + 1] + c * d * d;
          sdd += c * d;
        }
      }
      if (Nn > 0.f) M2 -= sdd * sdd / Nn;
      float* st = p.stats + ((long)bx * p.Cout + co_base + tid) * 2;
      st[0] = S;
      st[1] = M2;
      if (tid == 0 && by == 0) p.stats[(long)nbox * p.Cout * 2 + bx] = Nn;
    }
  }
}

}  // namespace

static int g_conv_mtw2 = 1;  // boxes of <= 256 voxels on 2 M-tiles per wave (A/B switch)
static int g_fwd_box_vol = 512;  // general forward / dgrad box volume (512 or 256; A/B switch)

// Forward (or dgrad) 3x3x3 conv. See Conv3Params.  splits > 1: every split writes its fp32
// partial sums into its own slab of yacc [splits][N*D*H*W][Cout] (plain stores, no zeroing
// needed); pcms_split_epilogue then sums the slabs in split order (deterministic), adds the
// bias, converts, and forms the BN statistics.
static int conv3_fwd_any(int dtype, const void* x0, int c0, const void* x1, int c1, const float* isc,
                         const float* ish, const void* wpack, const float* bias, void* y0, void* y1, int cy0,
                         float* yacc, float* stats, int flags, int N, int D, int H, int W, int Cout, int splits,
                         hipStream_t s) {
  const int accumulate = flags & PCMS_CONV_ACCUMULATE;
  const int Cin = c0 + c1;
  const int CK = pcms_conv3_chunk(dtype);
  const int VEC = dtype == PCMS_BF16 ? 8 : 4;
  if (Cout % 64 != 0 || c0 % VEC != 0 || c1 % VEC != 0 || (c1 > 0 && x1 == nullptr)) return -1;
  if (stats && flags) return -6;  // BN statistics describe a fresh, pre-activation output only
  if (flags & ~(PCMS_CONV_ACCUMULATE | PCMS_CONV_RELU)) return -8;
  if (y1 == nullptr) cy0 = Cout;
  if (cy0 % 64 != 0 && cy0 != Cout) return -2;
  Box b = fwd_box(D, H, W, g_fwd_box_vol);
  Conv3Params p;
  p.x0 = x0; p.x1 = x1; p.c0 = c0; p.c1 = c1;
  p.isc = isc; p.ish = ish;
  p.w = wpack; p.bias = bias; p.y0 = y0; p.y1 = y1; p.cy0 = cy0;
  p.yacc = splits > 1 ? yacc : nullptr;
  p.stats = stats; p.accumulate = flags;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.nvox = (long)N * D * H * W;
  p.nchunk = cdiv(Cin, CK);
  if (splits < 1) splits = 1;
  if (splits > p.nchunk) splits = p.nchunk;
  p.chunks_per_split = cdiv(p.nchunk, splits);
  splits = cdiv(p.nchunk, p.chunks_per_split);
  if (splits > 1 && yacc == nullptr) return -3;
  p.lbd = b.lbd; p.lbh = b.lbh; p.lbw = b.lbw;
  p.nbd = cdiv(D, 1 << b.lbd); p.nbh = cdiv(H, 1 << b.lbh); p.nbw = cdiv(W, 1 << b.lbw);
  if (splits > 1) p.yacc = yacc;
  if (splits == 1 && !accumulate && big_fwd_ok(dtype, N, D, H, W, c0, c1) &&
      (long)N * D * H * W * Cout * 2 < (long)kOOB)
    return big_fwd_launch(&p, s);
  if (p.isc) return -5;  // the input BatchNorm + ReLU runs on the big-box path only
  dim3 grid(N * p.nbd * p.nbh * p.nbw * (Cout / 64) * splits);
  const bool hot = b.lbd == 2 && b.lbh == 3 && b.lbw == 4;
  const bool small = b.lbd + b.lbh + b.lbw <= 8 && g_conv_mtw2;  // <= 256 voxels: 2 M-tiles per wave
  if (dtype == PCMS_BF16) {
    if (hot) hipLaunchKernelGGL((conv3_fwd_kernel<bf16_t, 2, 2, 3, 4>), grid, dim3(kThreads), 0, s, p);
    else if (small) hipLaunchKernelGGL((conv3_fwd_kernel<bf16_t, 2, -1, -1, -1, 2>), grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((conv3_fwd_kernel<bf16_t, 2, -1, -1, -1>), grid, dim3(kThreads), 0, s, p);
  } else if (dtype == PCMS_F32X3) {
    if (hot) hipLaunchKernelGGL((conv3_fwd_kernel<x3_t, 2, 2, 3, 4>), grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((conv3_fwd_kernel<x3_t, 2, -1, -1, -1>), grid, dim3(kThreads), 0, s, p);
  } else {
    if (hot) hipLaunchKernelGGL((conv3_fwd_kernel<x6_t, 2, 2, 3, 4>), grid, dim3(kThreads), 0, s, p);
    else if (small) hipLaunchKernelGGL((conv3_fwd_kernel<x6_t, 2, -1, -1, -1, 2>), grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL((conv3_fwd_kernel<x6_t, 2, -1, -1, -1>), grid, dim3(kThreads), 0, s, p);
  }
  PCMS_CHECK_LAUNCH();
}

extern "C" {

// Returns the m-block count (workgroups along M) of the general fwd kernel for a grid
// (an upper bound on every fwd path's BatchNorm row count; sizes the split decision).
int pcms_conv3_mblocks(int N, int D, int H, int W) {
  Box b = fwd_box(D, H, W, g_fwd_box_vol);
  return N * cdiv(D, 1 << b.lbd) * cdiv(H, 1 << b.lbh) * cdiv(W, 1 << b.lbw);
}

// BatchNorm partial rows an unsplit pcms_conv3_fwd with these sources writes
int pcms_conv3_fwd_rows(int dtype, int N, int D, int H, int W, int c0, int c1, int Cout) {
  if (Cout % 64 == 0 && big_fwd_ok(dtype, N, D, H, W, c0, c1) && (long)N * D * H * W * Cout * 2 < (long)kOOB)
    return big_slots(N, D, H, W, Cout);
  return pcms_conv3_mblocks(N, D, H, W);
}

// general-kernel forward / dgrad box volume: 512 or 256 voxels; v <= 0 queries; returns the
// previous setting (A/B switch: set before any workspace query)
int pcms_conv3_fwd_box_vol(int v) {
  const int old = g_fwd_box_vol;
  if (v == 256 || v == 512) g_fwd_box_vol = v;
  return old;
}

// general-kernel boxes of <= 256 voxels on four waves of 2 M-tiles (1) or two of 4 (0);
// v < 0 queries; returns the previous setting
int pcms_conv3_small_box_mtw2(int v) {
  const int old = g_conv_mtw2;
  if (v >= 0) g_conv_mtw2 = v;
  return old;
}

int pcms_conv3_chunk(int dtype) {
  return dtype == PCMS_BF16 ? Traits<bf16_t>::CK : dtype == PCMS_F32X3 ? Traits<x3_t>::CK : Traits<x6_t>::CK;
}

// Input-channel splits a split-K launch with `splits` requested actually uses (whole
// chunks per split): the slab count of yacc and of pcms_split_epilogue.
int pcms_conv3_splits(int dtype, int Cin, int splits) {
  const int nchunk = cdiv(Cin, pcms_conv3_chunk(dtype));
  splits = std::max(1, std::min(splits, nchunk));
  return cdiv(nchunk, cdiv(nchunk, splits));
}

int pcms_conv3_fwd(int dtype, const void* x0, int c0, const void* x1, int c1,
                   const void* wpack, const float* bias, void* y0, void* y1, int cy0,
                   float* yacc, float* stats, int flags,
                   int N, int D, int H, int W, int Cout, int splits, hipStream_t s) {
  return conv3_fwd_any(dtype, x0, c0, x1, c1, nullptr, nullptr, wpack, bias, y0, y1, cy0, yacc, stats, flags, N, D,
                       H, W, Cout, splits, s);
}

// the same with the input's BatchNorm + ReLU applied in the staging path: the conv of
// relu(x * isc + ish) (bf16, one source of <= 128 channels, the big-box shapes; -5 otherwise)
int pcms_conv3_fwd_bnin(int dtype, const void* x, int cin, const float* isc, const float* ish, const void* wpack,
                        const float* bias, void* y, float* stats, int N, int D, int H, int W, int Cout,
                        hipStream_t s) {
  if (!isc || !ish || cin > kBgBnMax || dtype != PCMS_BF16) return -1;
  return conv3_fwd_any(dtype, x, cin, nullptr, 0, isc, ish, wpack, bias, y, nullptr, Cout, nullptr, stats, 0, N, D,
                       H, W, Cout, 1, s);
}

}  // extern "C"
