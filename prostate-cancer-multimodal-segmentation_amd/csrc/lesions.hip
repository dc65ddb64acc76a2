// The component table on the device (gfx950): lesions.py's component_table, on the bytes.
//
//   pcms_component_table   one row per component of a canonical label volume (0 on background,
//                          1 + the smallest flat index of the component elsewhere), in ascending
//                          label order: label, voxels, box, index sums, peak of prob
//
// lesions_table.h has the layout, the keys and the row update.  Six launches:
//   init     every row of the table gets the values the row update leaves unchanged; header[0] = 0
//   count    workgroup b counts the roots (labels[i] == i + 1) of its CHUNK consecutive voxels
//   scan     one workgroup turns the counts into exclusive offsets, tile after tile in index
//            order, and stores their total K in header[1]
//   scatter  workgroup b ranks its roots (offset + roots before it in the chunk, from ballots),
//            stores rank[root] in the workspace and label[rank] in the table
//   accum    every foreground voxel finds its row through rank[labels[i] - 1] and adds itself:
//            a lane first merges the voxels of its own that follow one another in a row, then the
//            wave reduces the lanes that hold the same row (leader loop, at most 64 rounds) and
//            the leader issues the integer atomics
//   decode   peak / peak_index from the 64-bit peak keys
// No atomics in the ranking; the accumulation's are integer add / min / max, which commute, so
// the table is a function of the inputs alone.  No loop waits on another wave.
//
// Workspace (int32): [0, n) rank (written at roots only), [n, n + chunks) chunk offsets.
#include "common.h"

#include "lesions_table.h"
#include "pcms_hip.h"

namespace {

using namespace pcms_lt;

constexpr int NWAVES = TPB / WAVE;
// a group of fewer lanes than this adds its voxels one by one: 11 atomics a lane cost less than
// the 6-step reduction of a 15-word part
constexpr int REDUCE_MIN = 4;

enum { ST_NOT_CANONICAL = 1 };

struct DevMem {
  __device__ __forceinline__ void add32(int* p, int v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void add64(long long* p, long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void min32(int* p, int v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void max32(int* p, int v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void max64(u64* p, u64 v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// the flat index of (chunk, wave, item, lane)
__device__ __forceinline__ long voxel_of(int k) {
  return (long)blockIdx.x * CHUNK + (threadIdx.x / WAVE) * WCHUNK + k * WAVE + (threadIdx.x & (WAVE - 1));
}

__global__ void __launch_bounds__(TPB) lt_init_kernel(Table t, int capacity, int with_prob, int* __restrict__ header) {
  const int r = blockIdx.x * TPB + threadIdx.x;
  if (r < capacity) row_init(t, r, with_prob != 0);
  if (r == 0) header[0] = 0;
}

__global__ void __launch_bounds__(TPB) lt_count_kernel(const int* __restrict__ labels, int* __restrict__ counts,
                                                       int n) {
  __shared__ int wave_roots[NWAVES];
  int roots = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long i = voxel_of(k);
    roots += __popcll(__ballot(i < n && is_root(labels, i)));
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) wave_roots[threadIdx.x / WAVE] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int q = 0; q < NWAVES; ++q) sum += wave_roots[q];
    counts[blockIdx.x] = sum;
  }
}

// counts -> exclusive offsets in place, header[1] = their total.  One workgroup; the loop runs
// cdiv(nchunks, TPB) times.
__global__ void __launch_bounds__(TPB) lt_scan_kernel(int* __restrict__ counts, int nchunks, int* __restrict__ header) {
  __shared__ int wave_sum[NWAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  int carry = 0;
  for (int base = 0; base < nchunks; base += TPB) {
    const int j = base + threadIdx.x;
    const int v = j < nchunks ? counts[j] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const int below = __shfl_up(inc, o, WAVE);
      if (lane >= o) inc += below;
    }
    if (lane == WAVE - 1) wave_sum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < NWAVES; ++q) {
      const int s = wave_sum[q];
      before += q < wave ? s : 0;
      total += s;
    }
    if (j < nchunks) counts[j] = carry + before + inc - v;
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next tile
  }
  if (threadIdx.x == 0) header[1] = carry;
}

__global__ void __launch_bounds__(TPB) lt_scatter_kernel(const int* __restrict__ labels,
                                                         const int* __restrict__ offsets, int* __restrict__ rank,
                                                         int* __restrict__ table_label, int capacity, int n) {
  __shared__ int wave_roots[NWAVES];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  u64 roots[ITEMS];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    const long i = voxel_of(k);
    roots[k] = __ballot(i < n && is_root(labels, i));
    mine += __popcll(roots[k]);
  }
  if (lane == 0) wave_roots[wave] = mine;
  __syncthreads();
  int next = offsets[blockIdx.x];
#pragma unroll
  for (int q = 0; q < NWAVES; ++q) next += q < wave ? wave_roots[q] : 0;
  const u64 below = ((u64)1 << lane) - 1;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    if (roots[k] >> lane & 1) {
      const long i = voxel_of(k);  // < n: the ballot's condition
      const int r = next + __popcll(roots[k] & below);
      rank[i] = r;
      if (r < capacity) table_label[r] = (int)i + 1;
    }
    next += __popcll(roots[k]);
  }
}

// butterfly over the 64 lanes: every lane ends with op over all of them (op commutes and associates)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    T other;
    if constexpr (sizeof(T) == 8) {
      const u64 b = (u64)v;
      const int lo = __shfl_xor((int)(uint32_t)b, o, WAVE), hi = __shfl_xor((int)(uint32_t)(b >> 32), o, WAVE);
      other = (T)(((u64)(uint32_t)hi << 32) | (uint32_t)lo);
    } else {
      other = __shfl_xor(v, o, WAVE);
    }
    v = op(v, other);
  }
  return v;
}

// The lanes with todo set add their parts to their rows.  One round per distinct row among
// them: the lowest open lane leads, the lanes with its row are retired -- the leader among them,
// so at most 64 rounds.
template <bool WITH_PROB>
__device__ __forceinline__ void wave_flush(const Table& t, bool todo, int r, const Part& p) {
  DevMem m;
  const int lane = threadIdx.x & (WAVE - 1);
  for (int round = 0; round < WAVE; ++round) {
    const u64 open = __ballot(todo);
    if (open == 0) break;
    const int leader = __ffsll(open) - 1;
    const int r0 = __shfl(r, leader, WAVE);
    const bool mine = todo && r == r0;
    const int lanes = __popcll(__ballot(mine));
    if (lanes < REDUCE_MIN) {  // uniform over the wave
      if (mine) row_add(m, t, r0, p, WITH_PROB);
    } else {
      // row_add's updates, one column at a time: reduce over the wave (the other lanes hold the
      // operation's neutral value), then the leader's atomic
      const bool lead = lane == leader;
      const int count = wave_reduce(mine ? p.count : 0, [](int a, int b) { return a + b; });
      if (lead) m.add32(t.voxels + r0, count);
      const long long s3[3] = {p.sd, p.sh, p.sw};
      const int lo3[3] = {p.d0, p.h0, p.w0}, hi3[3] = {p.d1, p.h1, p.w1};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long sum = wave_reduce(mine ? s3[a] : 0ll, [](long long x, long long y) { return x + y; });
        if (lead) m.add64(t.index_sum + 3l * r0 + a, sum);
        const int lo = wave_reduce(mine ? lo3[a] : BOX_MIN_INIT, [](int x, int y) { return y < x ? y : x; });
        if (lead) m.min32(t.bbox + 6l * r0 + 2 * a, lo);
        const int hi = wave_reduce(mine ? hi3[a] : BOX_MAX_INIT, [](int x, int y) { return y > x ? y : x; });
        if (lead) m.max32(t.bbox + 6l * r0 + 2 * a + 1, hi);
      }
      if constexpr (WITH_PROB) {
        const u64 key = wave_reduce(mine ? p.key : (u64)0, [](u64 x, u64 y) { return y > x ? y : x; });
        if (lead) m.max64(t.peak_key + r0, key);
      }
    }
    todo = todo && !mine;
  }
}

template <bool WITH_PROB>
__global__ void __launch_bounds__(TPB) lt_accum_kernel(const int* __restrict__ labels, const float* __restrict__ prob,
                                                       const int* __restrict__ rank, Table t, int capacity,
                                                       int* __restrict__ header, int H, int W, int n) {
  bool bad = false;
  Part acc = part_none();
  int acc_r = -1;  // the row acc belongs to; -1: acc is empty
#pragma unroll 1
  for (int k = 0; k <= ITEMS; ++k) {  // the last turn only hands in what is left
    const long i = voxel_of(k);
    const int r = k < ITEMS && i < n ? voxel_row(labels, rank, i, n, capacity, bad) : -1;
    // a lane whose row changes hands its part in first; background in between changes nothing
    const bool flush = acc_r >= 0 && (k == ITEMS || (r >= 0 && r != acc_r));
    if (__ballot(flush) != 0) wave_flush<WITH_PROB>(t, flush, acc_r, acc);
    if (flush) {
      acc = part_none();
      acc_r = -1;
    }
    if (r >= 0) {
      u64 key = 0;
      if constexpr (WITH_PROB) key = peak_pack(__float_as_uint(prob[i]), (int)i);
      part_merge(acc, part_of_voxel((int)i, H, W, key));
      acc_r = r;
    }
  }
  if (bad) header[0] = ST_NOT_CANONICAL;
}

__global__ void __launch_bounds__(TPB) lt_decode_kernel(Table t, int capacity) {
  const int r = blockIdx.x * TPB + threadIdx.x;
  if (r >= capacity) return;
  uint32_t bits;
  int index;
  peak_unpack(t.peak_key[r], bits, index);
  t.peak[r] = __uint_as_float(bits);
  t.peak_index[r] = index;
}

// voxels, or -1 for a bad dimension or a workspace whose bytes do not fit an int
inline long voxels(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return -1;
  const long n = (long)D * H * W;
  if (n > (1l << 30)) return -1;
  return 4 * (n + cdiv(n, CHUNK)) > 0x7fffffffl ? -1 : n;
}

}  // namespace

extern "C" {

int pcms_component_table_work_bytes(int D, int H, int W) {
  const long n = voxels(D, H, W);
  return n < 0 ? -1 : (int)(4 * (n + cdiv(n, CHUNK)));
}

int pcms_component_table_bytes(int capacity, int with_prob) {
  if (capacity < 1) return -1;
  const long b = table_bytes(capacity, with_prob != 0);
  return b > 0x7fffffffl ? -1 : (int)b;
}

int pcms_component_table(const int* labels, const float* prob, void* table, int capacity, int* header, void* work,
                         int D, int H, int W, hipStream_t s) {
  const long n = voxels(D, H, W);
  const int with_prob = prob != nullptr;
  const long tbytes = pcms_component_table_bytes(capacity, with_prob);
  if (labels == nullptr || table == nullptr || header == nullptr || work == nullptr || n < 0 || tbytes < 0) return -1;
  if (misaligned(labels, 4) || misaligned(prob, 4) || misaligned(table, 8) || misaligned(header, 4) ||
      misaligned(work, 4))
    return -1;
  const long wbytes = pcms_component_table_work_bytes(D, H, W);
  const void* bufs[] = {labels, prob, table, header, work};
  const long sizes[] = {4 * n, with_prob ? 4 * n : 0, tbytes, 8, wbytes};
  for (int a = 0; a < 5; ++a)
    for (int b = a < 2 ? 2 : a + 1; b < 5; ++b)  // the two inputs may be anything but written
      if (sizes[a] > 0 && overlap(bufs[a], sizes[a], bufs[b], sizes[b])) return -1;
  const int nchunks = cdiv(n, CHUNK);
  int* rank = static_cast<int*>(work);
  int* offsets = rank + n;
  const Table t = table_columns(table, capacity);
  const int rows = cdiv(capacity, TPB);
  PCMS_LAUNCH(lt_init_kernel, dim3(rows), dim3(TPB), 0, s, t, capacity, with_prob, header);
  PCMS_LAUNCH(lt_count_kernel, dim3(nchunks), dim3(TPB), 0, s, labels, offsets, (int)n);
  PCMS_LAUNCH(lt_scan_kernel, dim3(1), dim3(TPB), 0, s, offsets, nchunks, header);
  PCMS_LAUNCH(lt_scatter_kernel, dim3(nchunks), dim3(TPB), 0, s, labels, (const int*)offsets, rank, t.label, capacity,
              (int)n);
  if (with_prob) {
    PCMS_LAUNCH(lt_accum_kernel<true>, dim3(nchunks), dim3(TPB), 0, s, labels, prob, (const int*)rank, t, capacity,
                header, H, W, (int)n);
    PCMS_LAUNCH(lt_decode_kernel, dim3(rows), dim3(TPB), 0, s, t, capacity);
  } else {
    PCMS_LAUNCH(lt_accum_kernel<false>, dim3(nchunks), dim3(TPB), 0, s, labels, (const float*)nullptr,
                (const int*)rank, t, capacity, header, H, W, (int)n);
  }
  return 0;
}

}  // extern "C"
