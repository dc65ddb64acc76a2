// Mask post-processing on the device (gfx950): components.py's host forms label_components /
// filter_components / fill_holes / postprocess, byte for byte.
//
//   pcms_components_label   canonical labels: 0 on background, 1 + the smallest flat index of
//                           the voxel's component on foreground
//   pcms_mask_postprocess   keep the largest components / drop small ones / fill enclosed holes
//
// Labelling is union-find with parent[i] <= i (components_uf.h has the functions, the invariant
// and the termination argument) in three launches:
//   tile     one workgroup labels an 8 x 16 x 32 tile in LDS: every voxel starts at the first
//            voxel of its run along W, the other forward neighbours are joined by LDS atomic
//            min; then every voxel's tile root is written as a global flat index (-1 on
//            background)
//   merge    voxels on a tile face join their forward neighbours in the next tile (global
//            atomic min)
//   flatten  every voxel finds its root and stores it over its parent; the same pass counts the
//            component sizes (wave-aggregated integer atomicAdd) or marks the roots of
//            components that touch a face of the volume (same-value stores)
// Nothing here depends on the order of execution: the root is the component's minimum index,
// integer sums commute, the top-k rounds take a maximum over unique keys.
//
// Workspace (int32): [0] status, [2..18) eight 64-bit top-k keys, [32, 32 + n) parents,
// [32 + n, 32 + 2 n) sizes / face marks.
#include "common.h"

#include "components_uf.h"
#include "pcms_hip.h"

namespace {

using namespace pcms_cc;

constexpr int TPB = 256;
constexpr int HDR = 32;                      // ints before the parents
constexpr long MAX_VOXELS = (1l << 30) - HDR;  // 2 n + HDR fits an int
constexpr int MAX_KEEP = 8;
typedef unsigned long long u64;

enum { ST_TILE = 1, ST_MERGE = 2, ST_FLATTEN = 3 };
enum { MODE_LABELS = 0, MODE_SIZES = 1, MODE_FACES = 2 };

// parents in LDS; loads are atomic so that a retry loop rereads them
struct LdsMem {
  int* p;
  __device__ __forceinline__ int load(int i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ int atomic_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
// parents in global memory while other workgroups link them: device-scope loads and atomics
struct GlobalMem {
  int* p;
  __device__ __forceinline__ int load(int i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ int atomic_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
// parents nobody links any more (the flatten pass): plain loads.  A concurrent flatten store
// replaces a parent by its root, which keeps the invariant.
struct FrozenMem {
  const int* p;
  __device__ __forceinline__ int load(int i) const { return p[i]; }
};

struct Tiles {
  int nh, nw;  // tiles along H and W
};
__device__ __forceinline__ void tile_origin(Tiles t, int& d0, int& h0, int& w0) {
  const int b = blockIdx.x;
  const int tw = b % t.nw, th = (b / t.nw) % t.nh, td = b / (t.nw * t.nh);
  d0 = td * TD;
  h0 = th * TH;
  w0 = tw * TW;
}

__global__ void __launch_bounds__(TPB) cc_init_kernel(int* __restrict__ work) {
  if (threadIdx.x < HDR) work[threadIdx.x] = 0;
}

// foreground is (mask != 0) != invert.  aux (sizes / marks) is zeroed here when given.
__global__ void __launch_bounds__(TPB) cc_tile_kernel(const uint8_t* __restrict__ mask, int invert, int nfwd,
                                                      int* __restrict__ par, int* __restrict__ aux,
                                                      int* __restrict__ work, int D, int H, int W, Tiles tiles) {
  __shared__ int lab[TILE];
  int d0, h0, w0;
  tile_origin(tiles, d0, h0, w0);
  unsigned fg = 0;  // bit k: this thread's k-th voxel is foreground
#pragma unroll
  for (int k = 0; k < TILE / TPB; ++k) {
    const int t = threadIdx.x + k * TPB;
    const int d = d0 + t / (TH * TW), h = h0 + (t / TW) % TH, w = w0 + t % TW;
    bool f = false;
    if (d < D && h < H && w < W) f = (mask[((long)d * H + h) * W + w] != 0) != (invert != 0);
    // a tile row is half a wave: its foreground bits give every voxel the start of its run
    const unsigned row = (unsigned)(__ballot(f) >> (threadIdx.x & 32));
    lab[t] = f ? t - t % TW + run_start(row, t % TW) : -1;
    fg |= (unsigned)f << k;
  }
  __syncthreads();
  LdsMem m{lab};
  bool bad = false;
#pragma unroll 1
  for (int k = 0; k < TILE / TPB; ++k)
    if (fg >> k & 1) tile_union_voxel(m, threadIdx.x + k * TPB, nfwd, bad);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < TILE / TPB; ++k) {
    const int t = threadIdx.x + k * TPB;
    const int d = d0 + t / (TH * TW), h = h0 + (t / TW) % TH, w = w0 + t % TW;
    if (d >= D || h >= H || w >= W) continue;
    const int i = (d * H + h) * W + w;
    int root = -1;
    if (fg >> k & 1) {
      const int r = uf_find(m, t, TILE, bad);
      root = ((d0 + r / (TH * TW)) * H + h0 + (r / TW) % TH) * W + w0 + r % TW;
    }
    par[i] = root;
    if (aux != nullptr) aux[i] = 0;
  }
  if (bad) work[0] = ST_TILE;
}

__global__ void __launch_bounds__(TPB) cc_merge_kernel(int* __restrict__ par, int nfwd, int* __restrict__ work, int D,
                                                       int H, int W, Tiles tiles) {
  int d0, h0, w0;
  tile_origin(tiles, d0, h0, w0);
  GlobalMem m{par};
  bool bad = false;
#pragma unroll 1
  for (int k = 0; k < TILE / TPB; ++k) {
    const int t = threadIdx.x + k * TPB;
    const int ld = t / (TH * TW), lh = (t / TW) % TH, lw = t % TW;
    const int d = d0 + ld, h = h0 + lh, w = w0 + lw;
    if (!on_merge_face(ld, lh, lw) || d >= D || h >= H || w >= W) continue;
    if (par[(d * H + h) * W + w] < 0) continue;  // foreground or not never changes
    merge_voxel(m, d, h, w, D, H, W, nfwd, bad);
  }
  if (bad) work[0] = ST_MERGE;
}

// MODE_LABELS: labels[i] = root + 1 or 0.  MODE_SIZES: aux[root] += 1 per voxel.  MODE_FACES:
// aux[root] = 1 for every component with a voxel on one of the six faces of the volume.
template <int MODE>
__global__ void __launch_bounds__(TPB) cc_flatten_kernel(int* __restrict__ par, int* __restrict__ dst,
                                                         int* __restrict__ work, int D, int H, int W) {
  const int n = D * H * W;
  FrozenMem m{par};
  bool bad = false;
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * TPB; base < n; base += (long)gridDim.x * TPB) {  // uniform per workgroup
    const long li = base + threadIdx.x;
    const int i = (int)li;
    int r = -1;
    if (li < n && par[i] >= 0) {
      r = uf_find(m, i, n, bad);
      par[i] = r;
    }
    if constexpr (MODE == MODE_LABELS) {
      if (li < n) dst[i] = r + 1;
    } else if constexpr (MODE == MODE_FACES) {
      if (r >= 0) {
        const int w = i % W, h = (i / W) % H, d = i / (W * H);
        if (d == 0 || d == D - 1 || h == 0 || h == H - 1 || w == 0 || w == W - 1) dst[r] = 1;
      }
    } else {
      // one atomicAdd per distinct root of the wave: at most 64 rounds, one per lane
      bool todo = r >= 0;
      for (int round = 0; round < 64; ++round) {
        const u64 open = __ballot(todo);
        if (open == 0) break;
        const int leader = __ffsll(open) - 1;
        const int r0 = __shfl(r, leader, 64);
        const bool mine = todo && r == r0;
        const u64 same = __ballot(mine);
        if (lane == leader) atomicAdd(dst + r0, __popcll(same));
        todo = todo && !mine;
      }
    }
  }
  if (bad) work[0] = ST_FLATTEN;
}

// rank key of a root: larger size first, then the smaller root (label)
__device__ __forceinline__ u64 rank_key(int size, int root) { return ((u64)(uint32_t)size << 32) | (uint32_t)~root; }

// round k of the top-k: win[k] = the largest key below win[k - 1] (0 when there is none left)
__global__ void __launch_bounds__(TPB) cc_topk_kernel(const int* __restrict__ par, const int* __restrict__ size,
                                                      u64* __restrict__ win, int k, int n) {
  const u64 below = k == 0 ? ~0ull : win[k - 1];
  u64 best = 0;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    if (par[i] != (int)i) continue;
    const u64 key = rank_key(size[i], (int)i);
    if (key < below && key > best) best = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && best != 0) atomicMax(win + k, best);
}

// out = foreground of a kept component.  keep > 0: win[keep - 1] is the smallest kept key
// (0 when there are fewer components than that: all stay).
__global__ void __launch_bounds__(TPB) cc_keep_kernel(const int* __restrict__ par, const int* __restrict__ size,
                                                      const u64* __restrict__ win, int keep, int min_voxels,
                                                      uint8_t* __restrict__ out, int n) {
  const u64 least = keep > 0 ? win[keep - 1] : 0;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const int r = par[i];
    uint8_t v = 0;
    if (r >= 0) {
      const int sz = size[r];
      v = sz >= min_voxels && rank_key(sz, r) >= least ? 1 : 0;
    }
    out[i] = v;
  }
}

__global__ void __launch_bounds__(TPB) cc_binarise_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out,
                                                          int n) {
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) out[i] = mask[i] != 0;
}

// par: flattened background components of out; a background voxel whose component is unmarked
// (touches no face of the volume) becomes 1
__global__ void __launch_bounds__(TPB) cc_fill_kernel(const int* __restrict__ par, const int* __restrict__ marked,
                                                      uint8_t* __restrict__ out, int n) {
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const int r = par[i];
    if (r >= 0 && marked[r] == 0) out[i] = 1;
  }
}

inline long voxels(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return -1;
  const long n = (long)D * H * W;
  return n > MAX_VOXELS ? -1 : n;
}
inline u64* winners(int* work) {  // the 8-byte-aligned keys inside the header
  return reinterpret_cast<u64*>((reinterpret_cast<uintptr_t>(work + 2) + 7) & ~(uintptr_t)7);
}

// tile + merge: par holds a forest whose roots are the components' minimum indices
int label_forest(const uint8_t* mask, int invert, int nfwd, int* par, int* aux, int* work, int D, int H, int W,
                 hipStream_t s) {
  const Tiles tiles{cdiv(H, TH), cdiv(W, TW)};
  const int ntiles = cdiv(D, TD) * tiles.nh * tiles.nw;
  PCMS_LAUNCH(cc_tile_kernel, dim3(ntiles), dim3(TPB), 0, s, mask, invert, nfwd, par, aux, work, D, H, W, tiles);
  if (ntiles > 1) PCMS_LAUNCH(cc_merge_kernel, dim3(ntiles), dim3(TPB), 0, s, par, nfwd, work, D, H, W, tiles);
  return 0;
}

}  // namespace

extern "C" {

int pcms_components_work_ints(int D, int H, int W) {
  const long n = voxels(D, H, W);
  return n < 0 ? -1 : (int)(HDR + 2 * n);
}

int pcms_components_label(const unsigned char* mask, int invert, int connectivity, int* labels, int* work, int D,
                          int H, int W, hipStream_t s) {
  const long n = voxels(D, H, W);
  const int nfwd = fwd_count(connectivity);
  if (mask == nullptr || labels == nullptr || work == nullptr || n < 0 || nfwd == 0) return -1;
  if (misaligned(labels, alignof(int)) || misaligned(work, alignof(int))) return -1;
  int* par = work + HDR;
  PCMS_LAUNCH(cc_init_kernel, dim3(1), dim3(TPB), 0, s, work);
  const int rc = label_forest(mask, invert, nfwd, par, nullptr, work, D, H, W, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(cc_flatten_kernel<MODE_LABELS>, dim3(grid_for(n, TPB)), dim3(TPB), 0, s, par, labels, work, D, H,
                     W);
  PCMS_CHECK_LAUNCH();
}

int pcms_mask_postprocess(const unsigned char* mask, unsigned char* out, int* work, int keep_largest, int min_voxels,
                          int fill_holes, int connectivity, int D, int H, int W, hipStream_t s) {
  const long n = voxels(D, H, W);
  const int nfwd = fwd_count(connectivity);
  if (mask == nullptr || out == nullptr || work == nullptr || n < 0 || nfwd == 0) return -1;
  if (misaligned(work, alignof(int)) || keep_largest < 0 || keep_largest > MAX_KEEP || min_voxels < 0) return -1;
  if (overlap(mask, n, out, n)) return -1;  // out may not alias mask
  int* par = work + HDR;
  int* aux = par + n;
  u64* win = winners(work);
  const int grid = grid_for(n, TPB);
  PCMS_LAUNCH(cc_init_kernel, dim3(1), dim3(TPB), 0, s, work);
  if (keep_largest == 0 && min_voxels <= 1) {
    PCMS_LAUNCH(cc_binarise_kernel, dim3(grid), dim3(TPB), 0, s, mask, out, (int)n);
  } else {
    const int rc = label_forest(mask, 0, nfwd, par, aux, work, D, H, W, s);
    if (rc != 0) return rc;
    PCMS_LAUNCH(cc_flatten_kernel<MODE_SIZES>, dim3(grid), dim3(TPB), 0, s, par, aux, work, D, H, W);
    for (int k = 0; k < keep_largest; ++k)
      PCMS_LAUNCH(cc_topk_kernel, dim3(grid_for(n, TPB * 4)), dim3(TPB), 0, s, (const int*)par, (const int*)aux,
                  win, k, (int)n);
    PCMS_LAUNCH(cc_keep_kernel, dim3(grid), dim3(TPB), 0, s, (const int*)par, (const int*)aux, (const u64*)win,
                keep_largest, min_voxels, out, (int)n);
  }
  if (fill_holes) {
    // the background of out at 6-connectivity (the dual of 26); its components off every face are holes
    const int rc = label_forest(out, 1, fwd_count(6), par, aux, work, D, H, W, s);
    if (rc != 0) return rc;
    PCMS_LAUNCH(cc_flatten_kernel<MODE_FACES>, dim3(grid), dim3(TPB), 0, s, par, aux, work, D, H, W);
    PCMS_LAUNCH(cc_fill_kernel, dim3(grid), dim3(TPB), 0, s, (const int*)par, (const int*)aux, out, (int)n);
  }
  return 0;
}

}  // extern "C"
