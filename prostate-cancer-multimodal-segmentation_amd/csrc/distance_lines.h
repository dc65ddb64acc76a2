// Line routines of the exact Euclidean distance transform (distance.hip), written once for the
// device and for a host program (tests/tools/distance_host_check.cpp): every function is
// templated on a memory policy `Mem` that supplies the line it reads,
//   T load(int i) const      element i of the line, 0 <= i < the line's length
//
// The value defined (distance.edt_sq) is, per voxel p and spacing (sz, sy, sx),
//   min over feature voxels q of  fl( Z(|pd-qd|) + fl( Y(|ph-qh|) + X(|pw-qw|) ) )
//   X(k) = fl(fl(k sx) fl(k sx)), Y and Z alike                          (sq_term)
// and +inf without a feature voxel.  fp64 addition is monotone in each argument and X, Y, Z are
// monotone in k, so both inner minima commute with the outer additions and three passes give
// the same bits:
//   W  g1 = min |pw - qw| over the features of the row, an integer          (w_line_dist)
//   H  g2 = min over h' of fl(Y(|ph - h'|) + X(g1[h']))                     (h_line_min)
//   D  g3 = min over d' of fl(Z(|pd - d'|) + g2[d'])                        (d_line_min)
// Every product and sum rounds on its own: no contraction into FMAs in this file.
//
// Loop bounds.  Every loop here runs at most the line's length (w_line_dist: its number of
// 64-bit words) times; none waits on another thread.  The H and D walks go outward from the
// voxel's own position, k = 0, 1, 2, ..., and stop once the axis term alone, Y(k) or Z(k), is
// >= the best value so far: the other term is >= 0 and fl(a + b) >= a for b >= 0, so no
// candidate at distance >= k can be smaller.  A minimum does not depend on the order its
// candidates are visited in, so the early stop changes no bit.  The rule is looked at once per
// WALK distances: the up to 2 WALK candidates in between are independent loads, and a candidate
// examined beyond the stopping point is still a member of the set the minimum is taken over.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PCMS_HD __host__ __device__ __forceinline__
#else
#define PCMS_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#define PCMS_UNROLL _Pragma("unroll")
#else
#pragma STDC FP_CONTRACT OFF
#define PCMS_UNROLL
#endif

namespace pcms_edt {

// the longest axis the H / D passes stage in LDS (see distance.hip) and the W pass keeps as
// feature bits: 2048 positions = 32 words of 64
constexpr int MAX_AXIS = 2048;
constexpr int MAX_WORDS = MAX_AXIS / 64;
// distances examined between two looks at the stopping rule of the H and D walks
constexpr int WALK = 4;

// sentinels of the W pass for a row without a feature, in the two types it stores
constexpr int NONE8 = 0xff;     // W <= 255: distances <= 254 fit a byte
constexpr int NONE16 = 0xffff;  // W <= 2048

PCMS_HD double infinity() { return __builtin_huge_val(); }

// fl(fl(k s) fl(k s))
PCMS_HD double sq_term(int k, double s) {
  const double t = (double)k * s;
  return t * t;
}

// W pass, one voxel.  bits: the row's features, bit (p & 63) of word (p >> 6) for position p,
// zero past the row's end; nwords = ceil(W / 64).  The distance to the nearest feature of the
// row, or -1 when the row has none.
template <class Mem>
PCMS_HD int w_line_dist(const Mem& bits, int nwords, int pos) {
  const int c = pos >> 6, b = pos & 63;
  const uint64_t own = bits.load(c);
  int best = -1;
  uint64_t lo = own & (~0ull >> (63 - b));  // positions <= pos of the own word
  int at = c;
  for (int j = c - 1; j >= 0 && lo == 0; --j) {
    lo = bits.load(j);
    at = j;
  }
  if (lo != 0) best = pos - (at * 64 + 63 - __builtin_clzll(lo));
  uint64_t hi = own & (~0ull << b);  // positions >= pos
  at = c;
  for (int j = c + 1; j < nwords && hi == 0; ++j) {
    hi = bits.load(j);
    at = j;
  }
  if (hi != 0) {
    const int right = at * 64 + __builtin_ctzll(hi) - pos;
    if (best < 0 || right < best) best = right;
  }
  return best;
}

// H pass, one voxel at position p of a line of L integers g1 (`none` where the row had no
// feature): min over q of fl(Y(|p - q|) + X(g1[q])).
template <class Mem>
PCMS_HD double h_line_min(const Mem& g1, int L, int p, double sy, double sx, int none) {
  double best = infinity();
  {
    const int g = g1.load(p);
    if (g != none) best = sq_term(0, sy) + sq_term(g, sx);
  }
  for (int k = 1; k < L; k += WALK) {
    if (sq_term(k, sy) >= best || (p - k < 0 && p + k >= L)) break;
    PCMS_UNROLL
    for (int u = 0; u < WALK; ++u) {
      const int kk = k + u;
      const double yk = sq_term(kk, sy);
      if (p - kk >= 0) {
        const int g = g1.load(p - kk);
        if (g != none) {
          const double c = yk + sq_term(g, sx);
          best = c < best ? c : best;
        }
      }
      if (p + kk < L) {
        const int g = g1.load(p + kk);
        if (g != none) {
          const double c = yk + sq_term(g, sx);
          best = c < best ? c : best;
        }
      }
    }
  }
  return best;
}

// D pass, one voxel at position p of a line of L doubles g2 (+inf where the plane row had no
// feature): min over q of fl(Z(|p - q|) + g2[q]).
template <class Mem>
PCMS_HD double d_line_min(const Mem& g2, int L, int p, double sz) {
  double best = sq_term(0, sz) + g2.load(p);
  for (int k = 1; k < L; k += WALK) {
    if (sq_term(k, sz) >= best || (p - k < 0 && p + k >= L)) break;
    PCMS_UNROLL
    for (int u = 0; u < WALK; ++u) {
      const int kk = k + u;
      const double zk = sq_term(kk, sz);
      if (p - kk >= 0) {
        const double c = zk + g2.load(p - kk);
        best = c < best ? c : best;
      }
      if (p + kk < L) {
        const double c = zk + g2.load(p + kk);
        best = c < best ? c : best;
      }
    }
  }
  return best;
}

// surface(mask) of one voxel: foreground with a face neighbour that is background or outside.
// m.load(i): the mask byte at flat index i = (d H + h) W + w.
template <class Mem>
PCMS_HD bool on_surface(const Mem& m, int d, int h, int w, int D, int H, int W) {
  const long i = ((long)d * H + h) * W + w;
  if (m.load(i) == 0) return false;
  const long HW = (long)H * W;
  if (d == 0 || d == D - 1 || h == 0 || h == H - 1 || w == 0 || w == W - 1) return true;
  return m.load(i - 1) == 0 || m.load(i + 1) == 0 || m.load(i - W) == 0 || m.load(i + W) == 0 ||
         m.load(i - HW) == 0 || m.load(i + HW) == 0;
}

}  // namespace pcms_edt
