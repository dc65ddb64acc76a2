// 3x3x3 convolution weight packs (the general kernels' fragment-major packs, the 16x16x32
// kernel's pack16) and the fused Adam + pack kernels, gfx950.
#include "common.h"
#include "pcms_hip.h"
#include <algorithm>
#include <type_traits>
#include <utility>

#include "conv_common.h"
#include "conv3_bigbox.h"

namespace {

// master fp32 W[Cout][Cin][27] -> packed T [chunk][27][J][CK]
//   fwd  (flip=0): J = Cout, k-index = ci
//   dgrad(flip=1): J = Cin,  k-index = co, tap mirrored (26 - t)
// One block per (chunk, 8 consecutive j): the 8 x CK x 27 source block is read with unit
// stride into LDS and written back with unit stride in the packed order.
template <typename T, int CK>
__global__ void __launch_bounds__(256) pack_conv3_kernel(const float* w, T* out, int Cout, int Cin, int flip) {
  __shared__ float tile[8][CK][27];
  const int J = flip ? Cin : Cout;
  const int Kdim = flip ? Cout : Cin;
  const int chunk = blockIdx.y;
  const int j0 = blockIdx.x * 8;
  constexpr int E = 8 * CK * 27;
  for (int e = threadIdx.x; e < E; e += 256) {
    int jj, k, t;
    if (!flip) { t = e % 27; k = (e / 27) % CK; jj = e / (27 * CK); }      // w[j][chunk*CK + k][t]
    else { t = e % 27; jj = (e / 27) % 8; k = e / (27 * 8); }             // w[chunk*CK + k][j][t]
    const int kk = chunk * CK + k, j = j0 + jj;
    float v = 0.f;
    if (kk < Kdim && j < J) v = flip ? w[((long)kk * Cin + j) * 27 + t] : w[((long)j * Cin + kk) * 27 + t];
    tile[jj][k][t] = v;
  }
  __syncthreads();
  if constexpr (std::is_same<T, x6_t>::value) {
    // one thread per packed row (t, jj): its 8 k values split once, the 96-B row
    // [h|h] [m|h] [l|m] written as six 16-B stores (consecutive threads: consecutive rows)
    static_assert(CK == 8, "x6 pack rows hold 8 k");
    const int jj = threadIdx.x % 8, t = threadIdx.x / 8;
    if (t < 27 && j0 + jj < J) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = flip ? tile[jj][k][26 - t] : tile[jj][k][t];
      u32x4_t h, m, l;
      split3x8(f, h, m, l);
      u32x4_t* o = reinterpret_cast<u32x4_t*>(reinterpret_cast<bf16_t*>(out) + (((long)chunk * 27 + t) * J + j0 + jj) * 48);
      o[0] = h; o[1] = h; o[2] = m; o[3] = h; o[4] = l; o[5] = m;
    }
    return;
  }
  for (int e = threadIdx.x; e < E; e += 256) {
    const int k = e % CK, jj = (e / CK) % 8, t = e / (CK * 8);
    if (j0 + jj >= J) continue;
    const float v = flip ? tile[jj][k][26 - t] : tile[jj][k][t];
    if constexpr (std::is_same<T, x3_t>::value) {
      // split-bf16 pack row [hi k = 0..15 | lo k = 0..15]
      bf16_t* o = reinterpret_cast<bf16_t*>(out) + (((long)chunk * 27 + t) * J + j0 + jj) * 2 * CK;
      const bf16_t hi = f2bf(v);
      o[k] = hi;
      o[CK + k] = f2bf(v - bf2f(hi));
    } else if constexpr (std::is_same<T, x6_t>::value) {
      // three-part pack row: the B fragments [h|h] [m|h] [l|m] (k = 0..7 each half)
      bf16_t* o = reinterpret_cast<bf16_t*>(out) + (((long)chunk * 27 + t) * J + j0 + jj) * 6 * CK;
      const bf16_t h = f2bf(v);
      const float r = v - bf2f(h);
      const bf16_t m = f2bf(r), l = f2bf(r - bf2f(m));
      o[k] = h; o[CK + k] = h;
      o[2 * CK + k] = m; o[3 * CK + k] = h;
      o[4 * CK + k] = l; o[5 * CK + k] = m;
    } else if constexpr (std::is_same<T, bf16_t>::value) {
      out[pack_bf16_off(chunk, t, j0 + jj, k, J)] = Elem<T>::cvt(v);
    } else {
      out[(((long)chunk * 27 + t) * J + j0 + jj) * CK + k] = Elem<T>::cvt(v);
    }
  }
}

// bf16 fast path (Kdim % 32 == 0, J % 8 == 0: every layer but the stem): the same block, read
// as 16-B vectors (the block's source is 8 contiguous 864-float runs (fwd) or 32 contiguous
// 216-float runs (dgrad)) and written as 16-B vectors of 8 packed k.
__global__ void __launch_bounds__(256) pack_conv3_bf16_kernel(const float* w, bf16_t* out, int Cout, int Cin,
                                                              int flip) {
  __shared__ float tile[8][32][27];
  const int J = flip ? Cin : Cout;
  const int chunk = blockIdx.y;
  const int j0 = blockIdx.x * 8;
  for (int e = threadIdx.x; e < 1728; e += 256) {
    int base, run, q;
    if (!flip) {  // w[j0 + jj][chunk*32 .. +32][27]: run jj of 864 floats
      run = e / 216; q = e % 216;
      base = ((j0 + run) * Cin + chunk * 32) * 27;
    } else {      // w[chunk*32 + k][j0 .. j0+8][27]: run k of 216 floats
      run = e / 54; q = e % 54;
      base = ((chunk * 32 + run) * Cin + j0) * 27;
    }
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(w + base + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = 4 * q + i;
      if (!flip) tile[run][idx / 27][idx % 27] = v[i];
      else tile[idx / 27][run][idx % 27] = v[i];
    }
  }
  __syncthreads();
  for (int g = threadIdx.x; g < 864; g += 256) {
    const int t = g >> 5, jj = (g >> 2) & 7, k8 = (g & 3) * 8;
    const int ts = flip ? 26 - t : t;
    u32x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(tile[jj][k8 + 2 * i][ts], tile[jj][k8 + 2 * i + 1][ts]);
    *reinterpret_cast<u32x4_t*>(out + pack_bf16_off(chunk, t, j0 + jj, k8, J)) = o;
  }
}

// Both bf16 packs of one conv from ONE read of the fp32 weight (Cin % 32 == Cout % 32 == 0).
// Block (co j0 .. j0+32, ci c*32 .. +32): the 32 contiguous 864-float runs w[co][c*32..][27]
// are converted to bf16 once into LDS (same rounding as pack_bf16x2), then both packs are
// written as 16-B pieces of the fragment-major layout (pack_bf16_off):
//   fwd   (c = ci/32, t, j = co, k = ci%32) = w[co][ci][t]
//   dgrad (c = co/32, t, j = ci, k = co%32) = w[co][ci][26 - t]
__global__ void __launch_bounds__(256) pack_conv3_bf16_both_kernel(const float* w, bf16_t* fwd, bf16_t* dgr,
                                                                   int Cout, int Cin) {
  __shared__ __attribute__((aligned(16))) uint16_t tb[32 * 864];
  const int chunk = blockIdx.y;
  const int j0 = blockIdx.x * 32;
  // all 27 loads of a thread in flight at once (the tile is 32 x 216 = 27 x 256 f32x4)
  f32x4_t v[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    const int e = threadIdx.x + i * 256, run = e / 216, q = e % 216;
    v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(w + ((long)(j0 + run) * Cin + chunk * 32) * 27) + q);
  }
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    const int e = threadIdx.x + i * 256, run = e / 216, q = e % 216;
    uint2 o;
    o.x = pack_bf16x2(v[i][0], v[i][1]);
    o.y = pack_bf16x2(v[i][2], v[i][3]);
    *reinterpret_cast<uint2*>(tb + run * 864 + 4 * q) = o;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < 27 * 128; g += 256) {
    const int t = g >> 7, co = (g >> 2) & 31, k8 = (g & 3) * 8;
    u32x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[i] = (uint32_t)tb[co * 864 + (k8 + 2 * i) * 27 + t] | ((uint32_t)tb[co * 864 + (k8 + 2 * i + 1) * 27 + t] << 16);
    *reinterpret_cast<u32x4_t*>(fwd + pack_bf16_off(chunk, t, j0 + co, k8, Cout)) = o;
  }
  for (int g = threadIdx.x; g < 27 * 128; g += 256) {
    const int t = g >> 7, ci = (g >> 2) & 31, k8 = (g & 3) * 8, ts = 26 - t;
    u32x4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[i] = (uint32_t)tb[(k8 + 2 * i) * 864 + ci * 27 + ts] | ((uint32_t)tb[(k8 + 2 * i + 1) * 864 + ci * 27 + ts] << 16);
    *reinterpret_cast<u32x4_t*>(dgr + pack_bf16_off(j0 >> 5, t, chunk * 32 + ci, k8, Cin)) = o;
  }
}

// the pack16 forms (pack16_off, conv3_bigbox.h) of one 32 co x 32 ci tile from its bf16 copy in LDS
__device__ void pack16_tile_store(const uint16_t* tb, bf16_t* fwd, bf16_t* dgr, int j0, int ci0, int Cout, int Cin) {
  // 2 chunks x 14 steps x 2 row tiles x 64 lanes = 3584 16-B pieces per direction
  for (int it = threadIdx.x; it < 2 * 3584; it += 256) {
    const int dir = it / 3584, q = it % 3584;
    bf16_t* out = dir ? dgr : fwd;
    if (!out) continue;
    const int l = q & 63, rt = (q >> 6) & 1, st = (q >> 7) % kB6Steps, cc = (q >> 7) / kB6Steps;
    const int g = l >> 4, jl = rt * 16 + (l & 15);             // row within the 32-row tile
    const int tap = 2 * st + (g >> 1);
    uint32_t o[4];
#pragma unroll
    for (int ee = 0; ee < 4; ++ee) {
      uint32_t v2 = 0;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int kl = cc * 16 + 8 * (g & 1) + 2 * ee + hh;  // k within the 32-wide tile
        uint16_t v = 0;
        if (tap < 27) v = dir ? tb[kl * 864 + jl * 27 + (26 - tap)] : tb[jl * 864 + kl * 27 + tap];
        v2 |= (uint32_t)v << (16 * hh);
      }
      o[ee] = v2;
    }
    const int J = dir ? Cin : Cout;
    const int jg = (dir ? ci0 : j0) + jl;                      // global row
    const int cg = ((dir ? j0 : ci0) >> 4) + cc;               // global 16-chunk
    *reinterpret_cast<u32x4_t*>(out + pack16_off(cg, st, jg, g, J)) = (u32x4_t){o[0], o[1], o[2], o[3]};
  }
}

// Adam + the bf16 packs in one pass over the conv weights (the flat master is read once per
// step instead of once for Adam and once more for the packs).  One block per (conv, 32 co x
// 32 ci) tile of a table entry [off, Cout, Cin, fwd pack, dgrad pack, first tile, fwd16 pack,
// dgrad16 pack] (int64 each): the tile's 32 contiguous 864-float runs w[co][ci0..ci0+32][27]
// are updated in place (p, m, v, and g when scaled), the new weights converted to bf16 into
// LDS, and each non-null pack written: the general kernel's two as in
// pack_conv3_bf16_both_kernel, the 16x16x32 kernel's two as in pack16_conv3_kernel.
__global__ void __launch_bounds__(256) adam_pack_conv3_kernel(float* P, float* Gr, float* Mo, float* Vo,
                                                              const long long* tab, int ntab, AdamCoef c,
                                                              const float* gmul) {
  __shared__ __attribute__((aligned(16))) uint16_t tb[32 * 864];
  int ei = 0;
  while (ei + 1 < ntab && tab[8 * (ei + 1) + 5] <= (long long)blockIdx.x) ++ei;
  const long long* e = tab + 8 * ei;
  const long off = (long)e[0];
  const int Cout = (int)e[1], Cin = (int)e[2];
  bf16_t* fwd = reinterpret_cast<bf16_t*>(e[3]);
  bf16_t* dgr = reinterpret_cast<bf16_t*>(e[4]);
  bf16_t* fwd16 = reinterpret_cast<bf16_t*>(e[6]);
  bf16_t* dgr16 = reinterpret_cast<bf16_t*>(e[7]);
  const int local = blockIdx.x - (int)e[5];
  const int j0 = (local % (Cout / 32)) * 32, chunk = local / (Cout / 32);
  const float s = gmul ? c.gscale * gmul[0] : c.gscale;
  // ADAM_U iterations' four streams loaded before any is used: 4 x ADAM_U 16-B loads in flight
  // per thread (the stores of an iteration could alias the next one's loads for the compiler,
  // so without the explicit batch it keeps one iteration's loads in flight)
#ifndef ADAM_U
#define ADAM_U 3
#endif
  static_assert(27 % ADAM_U == 0, "ADAM_U divides the 27 iterations");
  for (int i0 = 0; i0 < 27; i0 += ADAM_U) {
    f32x4_t pv[ADAM_U], gv[ADAM_U], mv[ADAM_U], vv[ADAM_U];
    long idx[ADAM_U];
    int tbo[ADAM_U];
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const int q4 = threadIdx.x + (i0 + u) * 256, run = q4 / 216, q = q4 % 216;
      idx[u] = off + ((long)(j0 + run) * Cin + chunk * 32) * 27 + 4 * q;
      tbo[u] = run * 864 + 4 * q;
      // the fp32 master / gradient / moment streams (1.4 GB per step) bypass the caches
      pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(P + idx[u]));
      gv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Gr + idx[u]));
      mv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Mo + idx[u]));
      vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Vo + idx[u]));
    }
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[u][k], gk = gv[u][k], mk = mv[u][k], vk = vv[u][k];
        adam_update(pk, gk, mk, vk, c, s);
        pv[u][k] = pk; gv[u][k] = gk; mv[u][k] = mk; vv[u][k] = vk;
      }
      __builtin_nontemporal_store(pv[u], reinterpret_cast<f32x4_t*>(P + idx[u]));
      __builtin_nontemporal_store(mv[u], reinterpret_cast<f32x4_t*>(Mo + idx[u]));
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4_t*>(Vo + idx[u]));
      if (s != 1.f) __builtin_nontemporal_store(gv[u], reinterpret_cast<f32x4_t*>(Gr + idx[u]));
      uint2 o;
      o.x = pack_bf16x2(pv[u][0], pv[u][1]);
      o.y = pack_bf16x2(pv[u][2], pv[u][3]);
      *reinterpret_cast<uint2*>(tb + tbo[u]) = o;
    }
  }
  __syncthreads();
  if (fwd)
    for (int g = threadIdx.x; g < 27 * 128; g += 256) {
      const int t = g >> 7, co = (g >> 2) & 31, k8 = (g & 3) * 8;
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = (uint32_t)tb[co * 864 + (k8 + 2 * i) * 27 + t] | ((uint32_t)tb[co * 864 + (k8 + 2 * i + 1) * 27 + t] << 16);
      *reinterpret_cast<u32x4_t*>(fwd + pack_bf16_off(chunk, t, j0 + co, k8, Cout)) = o;
    }
  if (dgr)
    for (int g = threadIdx.x; g < 27 * 128; g += 256) {
      const int t = g >> 7, ci = (g >> 2) & 31, k8 = (g & 3) * 8, ts = 26 - t;
      u32x4_t o;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = (uint32_t)tb[(k8 + 2 * i) * 864 + ci * 27 + ts] | ((uint32_t)tb[(k8 + 2 * i + 1) * 864 + ci * 27 + ts] << 16);
      *reinterpret_cast<u32x4_t*>(dgr + pack_bf16_off(j0 >> 5, t, chunk * 32 + ci, k8, Cin)) = o;
    }
  if (fwd16 || dgr16) pack16_tile_store(tb, fwd16, dgr16, j0, chunk * 32, Cout, Cin);
}

// fp32 build (bf16x6 packs): Adam + both three-part packs in one pass.  One block per (conv,
// 32 co x 16 ci) tile (the fp32 tile, 54 KiB, fits LDS where the 32 x 32 one would not): the
// 32 contiguous 432-float runs w[co][ci0..ci0+16][27] are updated in place as in
// adam_pack_conv3_kernel, the new fp32 weights kept in LDS, and each packed row -- 8 k
// values -> the B fragments [h|h] [m|h] [l|m] (split3x8, pack_conv3_kernel<x6_t>'s
// arithmetic) -- written as six 16-B stores:
//   fwd   [ci/8][t][co][48]   (k = ci)
//   dgrad [co/8][t][ci][48]   (k = co, tap mirrored)
__global__ void __launch_bounds__(256) adam_pack_conv3_x6_kernel(float* P, float* Gr, float* Mo, float* Vo,
                                                                 const long long* tab, int ntab, AdamCoef c,
                                                                 const float* gmul) {
  __shared__ float tf[32][16 * 27 + 1];  // [co][ci * 27 + t], rows padded by one float
  int ei = 0;
  while (ei + 1 < ntab && tab[8 * (ei + 1) + 5] <= (long long)blockIdx.x) ++ei;
  const long long* e = tab + 8 * ei;
  const long off = (long)e[0];
  const int Cout = (int)e[1], Cin = (int)e[2];
  bf16_t* fwd = reinterpret_cast<bf16_t*>(e[3]);
  bf16_t* dgr = reinterpret_cast<bf16_t*>(e[4]);
  const int local = blockIdx.x - (int)e[5];
  const int j0 = (local % (Cout / 32)) * 32, ci0 = (local / (Cout / 32)) * 16;
  const float s = gmul ? c.gscale * gmul[0] : c.gscale;
  // 32 runs of 108 f32x4 = 13.5 per thread: ADAM_X6_U iterations' four streams loaded before
  // any is used (adam_pack_conv3_kernel's batching; one iteration in flight per thread left
  // this kernel latency-bound at two 54-KiB blocks per CU)
#ifndef ADAM_X6_U
#define ADAM_X6_U 4
#endif
  for (int i0 = 0; i0 < 14; i0 += ADAM_X6_U) {
    f32x4_t pv[ADAM_X6_U], gv[ADAM_X6_U], mv[ADAM_X6_U], vv[ADAM_X6_U];
    long idx[ADAM_X6_U];
#pragma unroll
    for (int u = 0; u < ADAM_X6_U; ++u) {
      const int q4 = threadIdx.x + (i0 + u) * 256, run = q4 / 108, q = q4 % 108;
      idx[u] = off + ((long)(j0 + run) * Cin + ci0) * 27 + 4 * q;
      if (i0 + u < 14 && q4 < 32 * 108) {
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(P + idx[u]));
        gv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Gr + idx[u]));
        mv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Mo + idx[u]));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(Vo + idx[u]));
      }
    }
#pragma unroll
    for (int u = 0; u < ADAM_X6_U; ++u) {
      const int q4 = threadIdx.x + (i0 + u) * 256, run = q4 / 108, q = q4 % 108;
      if (i0 + u >= 14 || q4 >= 32 * 108) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pv[u][k], gk = gv[u][k], mk = mv[u][k], vk = vv[u][k];
        adam_update(pk, gk, mk, vk, c, s);
        pv[u][k] = pk; gv[u][k] = gk; mv[u][k] = mk; vv[u][k] = vk;
        tf[run][4 * q + k] = pk;
      }
      __builtin_nontemporal_store(pv[u], reinterpret_cast<f32x4_t*>(P + idx[u]));
      __builtin_nontemporal_store(mv[u], reinterpret_cast<f32x4_t*>(Mo + idx[u]));
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4_t*>(Vo + idx[u]));
      if (s != 1.f) __builtin_nontemporal_store(gv[u], reinterpret_cast<f32x4_t*>(Gr + idx[u]));
    }
  }
  __syncthreads();
  auto put = [](bf16_t* row, const float (&f)[8]) {
    u32x4_t h, m, l;
    split3x8(f, h, m, l);
    u32x4_t* o = reinterpret_cast<u32x4_t*>(row);
    o[0] = h; o[1] = h; o[2] = m; o[3] = h; o[4] = l; o[5] = m;
  };
  for (int r = threadIdx.x; r < 27 * 32 * 2; r += 256) {  // fwd rows (t, co, ci-chunk of 8)
    const int cc = r & 1, co = (r >> 1) & 31, t = r >> 6;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = tf[co][(cc * 8 + k) * 27 + t];
    put(fwd + ((((long)(ci0 / 8 + cc)) * 27 + t) * Cout + j0 + co) * 48, f);
  }
  for (int r = threadIdx.x; r < 27 * 16 * 4; r += 256) {  // dgrad rows (t, ci, co-chunk of 8)
    const int cc = r & 3, ci = (r >> 2) & 15, t = r >> 6;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = tf[cc * 8 + k][ci * 27 + 26 - t];
    put(dgr + ((((long)(j0 / 8 + cc)) * 27 + t) * Cin + ci0 + ci) * 48, f);
  }
}

// Both pack16 forms of the convs of a table, from the fp32 master (one block per 32 co x 32 ci
// tile, as pack_conv3_bf16_both_kernel): rows int64[8] = {weight ptr, Cout, Cin, fwd16 ptr (or
// 0), dgrad16 ptr (or 0), first tile, 0, 0}.  fwd16: J = Cout rows, k = Cin; dgrad16: J = Cin
// rows, k = Cout, taps mirrored (the dgrad conv is the transposed, flipped forward).
__global__ void __launch_bounds__(256) pack16_conv3_kernel(const long long* tab, int ntab) {
  __shared__ __attribute__((aligned(16))) uint16_t tb[32 * 864];
  int ei = 0;
  while (ei + 1 < ntab && tab[8 * (ei + 1) + 5] <= (long long)blockIdx.x) ++ei;
  const long long* e = tab + 8 * ei;
  const float* w = reinterpret_cast<const float*>(e[0]);
  const int Cout = (int)e[1], Cin = (int)e[2];
  bf16_t* fwd = reinterpret_cast<bf16_t*>(e[3]);
  bf16_t* dgr = reinterpret_cast<bf16_t*>(e[4]);
  const int local = blockIdx.x - (int)e[5];
  const int j0 = (local % (Cout / 32)) * 32, ci0 = (local / (Cout / 32)) * 32;
  // all 27 loads of a thread in flight at once (as pack_conv3_bf16_both_kernel)
  f32x4_t v[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    const int q4 = threadIdx.x + i * 256, run = q4 / 216, q = q4 % 216;
    v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(w + ((long)(j0 + run) * Cin + ci0) * 27) + q);
  }
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    const int q4 = threadIdx.x + i * 256, run = q4 / 216, q = q4 % 216;
    uint2 o;
    o.x = pack_bf16x2(v[i][0], v[i][1]);
    o.y = pack_bf16x2(v[i][2], v[i][3]);
    *reinterpret_cast<uint2*>(tb + run * 864 + 4 * q) = o;
  }
  __syncthreads();
  pack16_tile_store(tb, fwd, dgr, j0, ci0, Cout, Cin);
}

}  // namespace

extern "C" {

// elements (of the activation dtype: bf16, or fp32 for both split modes) of one conv weight
// pack with J output rows and Kdim input channels: [ceil(Kdim / CK)][27][J][WK] bf16
int pcms_conv3_pack_elems(int dtype, int J, int Kdim) {
  const int ck = pcms_conv3_chunk(dtype);
  const int wk = dtype == PCMS_BF16 ? Traits<bf16_t>::WK : dtype == PCMS_F32X3 ? Traits<x3_t>::WK : Traits<x6_t>::WK;
  const long bf16s = (long)cdiv(Kdim, ck) * 27 * J * wk;
  return (int)(dtype == PCMS_BF16 ? bf16s : bf16s / 2);
}

// forward and dgrad packs together (one weight read); other shapes / dtypes: the two packs
int pcms_conv3_pack2(int dtype, const float* w, void* fwd, void* dgrad, int Cout, int Cin, hipStream_t s) {
  if (dtype == PCMS_BF16 && Cin % 32 == 0 && Cout % 32 == 0) {
    hipLaunchKernelGGL(pack_conv3_bf16_both_kernel, dim3(Cout / 32, Cin / 32), dim3(256), 0, s, w, (bf16_t*)fwd,
                       (bf16_t*)dgrad, Cout, Cin);
    PCMS_CHECK_LAUNCH();
  }
  const int rc = pcms_conv3_pack(dtype, w, fwd, Cout, Cin, 0, s);
  return rc ? rc : pcms_conv3_pack(dtype, w, dgrad, Cout, Cin, 1, s);
}

// Adam over the conv weights of a table (see adam_pack_conv3_kernel; every entry has
// Cout % 32 == Cin % 32 == 0 and 16-B aligned offsets), writing both bf16 packs.
int pcms_adam_pack_conv3(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                         float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                         const float* gmul, hipStream_t s) {
  if (ntab <= 0 || ntiles <= 0) return 0;
  const AdamCoef c{step_size, b1, b2, eps, wd, bc2_sqrt, gscale};
  hipLaunchKernelGGL(adam_pack_conv3_kernel, dim3(ntiles), dim3(256), 0, s, p, g, m, v, table, ntab, c, gmul);
  PCMS_CHECK_LAUNCH();
}

// the same for the fp32 build: both bf16x6 packs (pcms_conv3_pack dtype 0 layouts); one tile
// per 32 co x 16 ci (ntiles = sum of Cout / 32 x Cin / 16)
int pcms_adam_pack_conv3_x6(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                            float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                            const float* gmul, hipStream_t s) {
  if (ntab <= 0 || ntiles <= 0) return 0;
  const AdamCoef c{step_size, b1, b2, eps, wd, bc2_sqrt, gscale};
  hipLaunchKernelGGL(adam_pack_conv3_x6_kernel, dim3(ntiles), dim3(256), 0, s, p, g, m, v, table, ntab, c, gmul);
  PCMS_CHECK_LAUNCH();
}

int pcms_conv3_pack(int dtype, const float* w, void* out, int Cout, int Cin, int flip, hipStream_t s) {
  const int CK = pcms_conv3_chunk(dtype);
  const int J = flip ? Cin : Cout;
  const int Kdim = flip ? Cout : Cin;
  if (dtype == PCMS_BF16 && J % 32) return -1;  // fragment-major rows come in 32-row tiles
  dim3 grid(cdiv(J, 8), cdiv(Kdim, CK));
  if (dtype == PCMS_BF16 && Kdim % 32 == 0 && J % 8 == 0)
    hipLaunchKernelGGL(pack_conv3_bf16_kernel, grid, dim3(256), 0, s, w, (bf16_t*)out, Cout, Cin, flip);
  else if (dtype == PCMS_BF16)
    hipLaunchKernelGGL((pack_conv3_kernel<bf16_t, 32>), grid, dim3(256), 0, s, w, (bf16_t*)out, Cout, Cin, flip);
  else if (dtype == PCMS_F32X3)
    hipLaunchKernelGGL((pack_conv3_kernel<x3_t, 16>), grid, dim3(256), 0, s, w, (x3_t*)out, Cout, Cin, flip);
  else
    hipLaunchKernelGGL((pack_conv3_kernel<x6_t, 8>), grid, dim3(256), 0, s, w, (x6_t*)out, Cout, Cin, flip);
  PCMS_CHECK_LAUNCH();
}

int pcms_conv3_pack16_elems(int J, int Kdim) { return (J % 16 || Kdim % 16) ? -1 : (Kdim / 16) * kB6Steps * J * 32; }
// pack16 forms (fwd16: rows = Cout, k = Cin; dgrad16: rows = Cin, k = Cout, taps mirrored) of the
// convs of a table: int64 rows {weight ptr, Cout, Cin, fwd16 ptr or 0, dgrad16 ptr or 0, first
// tile, 0, 0}, one tile per 32 co x 32 ci (ntiles = sum of Cout / 32 x Cin / 32)
int pcms_conv3_pack16(const long long* table, int ntab, int ntiles, hipStream_t s) {
  if (ntab <= 0 || ntiles <= 0) return 0;
  hipLaunchKernelGGL(pack16_conv3_kernel, dim3(ntiles), dim3(256), 0, s, table, ntab);
  PCMS_CHECK_LAUNCH();
}

}  // extern "C"
