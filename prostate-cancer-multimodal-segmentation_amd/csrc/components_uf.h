// Union-find pieces of the connected-component labelling (components.hip), written once for the
// device and for a host program (tests/tools/components_host_check.cpp): every function is
// templated on a memory policy `Mem` that supplies
//   int  load(int i) const          the current parent of i (may be stale: see uf_union)
//   int  atomic_min(int i, int v)   parent[i] = min(parent[i], v), returns the old value
// Invariant, kept by every writer: parent[i] <= i, and parent[i] lies in i's component.  A root
// is an i with parent[i] == i.  A union links the LARGER root below the smaller one with
// atomic_min, so whatever the order of execution the root of a finished component is its
// minimum index.
//
// Termination.  uf_find: every step replaces x by parent[x] < x, so it ends within n steps on an
// array of n entries.  uf_union: a retry happens only after atomic_min(a, b) returned old != a,
// and old <= a by the invariant, so the retry continues from old < a: a + b strictly decreases,
// at most 2 n retries.  Both loops also carry these bounds as explicit iteration caps; running
// into one sets `bad`, which the kernels turn into a nonzero work[0].
#pragma once

#if defined(__HIPCC__)
#define PCMS_HD __host__ __device__ __forceinline__
#else
#define PCMS_HD inline
#endif

namespace pcms_cc {

// workgroup tile (voxels), W fastest: 4096 labels = 16 KiB of LDS
constexpr int TD = 8, TH = 16, TW = 32;
constexpr int TILE = TD * TH * TW;

// The neighbours that precede a voxel in scan order (half of the neighbourhood; the other half
// is reached from the other side): 3 with one nonzero offset, 6 with two, 4 with three.
constexpr int NFWD = 13;
PCMS_HD void fwd_offset(int k, int& dd, int& dh, int& dw) {
  constexpr signed char O[NFWD][3] = {{0, 0, -1},  {0, -1, 0},  {-1, 0, 0},  {0, -1, -1},  {0, -1, 1},
                                      {-1, 0, -1}, {-1, 0, 1},  {-1, -1, 0}, {-1, 1, 0},   {-1, -1, -1},
                                      {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};
  dd = O[k][0];
  dh = O[k][1];
  dw = O[k][2];
}
// 6 / 18 / 26 -> 3 / 9 / 13 forward neighbours, anything else -> 0
PCMS_HD int fwd_count(int connectivity) {
  return connectivity == 6 ? 3 : connectivity == 18 ? 9 : connectivity == 26 ? 13 : 0;
}

template <class Mem>
PCMS_HD int uf_find(const Mem& m, int x, long n, bool& bad) {
  for (long it = 0; it <= n; ++it) {
    const int p = m.load(x);
    if (p == x) return x;
    x = p;
  }
  bad = true;
  return x;
}

// A stale load can only make uf_find stop early at a former root; atomic_min then returns that
// entry's true parent (old != a) and the loop goes on from there, so stale reads cost retries,
// never correctness.
template <class Mem>
PCMS_HD void uf_union(Mem& m, int a, int b, long n, bool& bad) {
  for (long it = 0; it <= 2 * n; ++it) {
    a = uf_find(m, a, n, bad);
    b = uf_find(m, b, n, bad);
    if (bad || a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = m.atomic_min(a, b);
    if (old == a) return;  // a was a root and now hangs below b
    a = old;               // a had a parent already (old < a); whichever of old / b lost the min is joined next
  }
  bad = true;
}

// The local label a tile voxel starts from: the first voxel of its run of foreground along W
// (row_bits: bit p is set where the row's voxel p is foreground), so the W neighbours are joined
// before the first union and a solid row is one flat tree.
static_assert(TW == 32, "a tile row is the 32 bits of run_start");
PCMS_HD int run_start(unsigned row_bits, int lw) {
  const unsigned gaps = ~row_bits & ((1u << lw) - 1u);  // the background positions below lw
  return gaps == 0 ? 0 : 32 - __builtin_clz(gaps);
}

// Which unions are needed.  Offset 0 is the W neighbour.  A pair (t, u) of any other offset is
// left out when t - 1 and u - 1 exist and are foreground too: (t - 1, u - 1) is a pair of the
// same offset, t - 1 ~ t and u - 1 ~ u along W, so by induction over w the pair that is made at
// the start of the run stands for all of them.  W neighbours themselves are joined by run_start
// inside a tile and unconditionally by merge_voxel across a tile face.

// Tile phase, one voxel: t is the local index ((ld * TH + lh) * TW + lw) of a foreground voxel
// in a tile whose labels `lab` hold the local parent (foreground, initially t - lw +
// run_start) or -1 (background and voxels past the volume's end).  Joins it to its forward
// neighbours inside the tile.
template <class Mem>
PCMS_HD void tile_union_voxel(Mem& lab, int t, int nfwd, bool& bad) {
  const int ld = t / (TH * TW), lh = (t / TW) % TH, lw = t % TW;
  const bool left = lw > 0 && lab.load(t - 1) >= 0;
  for (int k = 1; k < nfwd; ++k) {
    int dd, dh, dw;
    fwd_offset(k, dd, dh, dw);
    const int nd = ld + dd, nh = lh + dh, nw = lw + dw;
    if (nd < 0 || nh < 0 || nh >= TH || nw < 0 || nw >= TW) continue;
    const int u = (nd * TH + nh) * TW + nw;
    if (lab.load(u) < 0) continue;
    if (left && nw > 0 && lab.load(u - 1) >= 0) continue;
    uf_union(lab, t, u, TILE, bad);
  }
}

// true where a voxel at local (ld, lh, lw) can have a forward neighbour in another tile
PCMS_HD bool on_merge_face(int ld, int lh, int lw) {
  return ld == 0 || lh == 0 || lh == TH - 1 || lw == 0 || lw == TW - 1;
}

// Merge phase, one voxel: (d, h, w) is a foreground voxel of the volume whose parents `par`
// hold global flat indices (foreground) or -1.  Joins it to its forward neighbours that lie in
// another tile.
template <class Mem>
PCMS_HD void merge_voxel(Mem& par, int d, int h, int w, int D, int H, int W, int nfwd, bool& bad) {
  const long n = (long)D * H * W;
  const int i = (d * H + h) * W + w;
  const bool left = w > 0 && par.load(i - 1) >= 0;
  for (int k = 0; k < nfwd; ++k) {
    int dd, dh, dw;
    fwd_offset(k, dd, dh, dw);
    const int nd = d + dd, nh = h + dh, nw = w + dw;
    if (nd < 0 || nh < 0 || nh >= H || nw < 0 || nw >= W) continue;
    if (nd / TD == d / TD && nh / TH == h / TH && nw / TW == w / TW) continue;  // the tile phase did it
    const int j = (nd * H + nh) * W + nw;
    if (par.load(j) < 0) continue;
    if (k > 0 && left && nw > 0 && par.load(j - 1) >= 0) continue;
    uf_union(par, i, j, n, bad);
  }
}

}  // namespace pcms_cc
