// Pieces of the component table (lesions.hip), written once for the device and for a host
// program (tests/tools/lesions_host_check.cpp): the table's layout, the order-preserving key of a
// float, the partial row a group of voxels reduces to, and the row update, which is templated on
// a memory policy `Mem` that supplies
//   void add32(int* p, int v)            *p += v
//   void add64(long long* p, long long v)
//   void min32(int* p, int v)            *p = min(*p, v)
//   void max32(int* p, int v)
//   void max64(u64* p, u64 v)
// Every one of them is an integer operation that commutes and associates, so a row is a function
// of the set of voxels added to it, whatever the grouping and the order.
//
// Ranking.  Voxel i is a root iff labels[i] == i + 1; the row of a component is the number of
// roots below its own.  The volume is cut into chunks of CHUNK consecutive voxels, one per
// workgroup, a chunk into four runs of WCHUNK voxels, one per wave, and a run into ITEMS groups of
// 64 consecutive voxels: (chunk, wave, item, lane) order is flat-index order.
#pragma once

#include <stdint.h>

#ifndef PCMS_HD
#if defined(__HIPCC__)
#define PCMS_HD __host__ __device__ __forceinline__
#else
#define PCMS_HD inline
#endif
#endif

namespace pcms_lt {

typedef unsigned long long u64;

constexpr int TPB = 256, WAVE = 64, ITEMS = 8;
constexpr int WCHUNK = WAVE * ITEMS;  // consecutive voxels of one wave
constexpr int CHUNK = TPB * ITEMS;    // consecutive voxels of one workgroup
constexpr int BOX_MIN_INIT = 0x7fffffff, BOX_MAX_INIT = -1;

// Columns of `capacity` entries each, in this order (pcms_hip.h documents it).  The three peak
// columns are the tail: a table without prob ends before them.
struct Table {
  long long* index_sum;  // [capacity][3]  sums of d, h, w
  int* label;            // [capacity]
  int* voxels;           // [capacity]
  int* bbox;             // [capacity][6]  dmin, dmax, hmin, hmax, wmin, wmax
  u64* peak_key;         // [capacity]     (key << 32) | ~flat index of the peak; 0: none
  float* peak;           // [capacity]
  int* peak_index;       // [capacity]
};
PCMS_HD long table_bytes(int capacity, int with_prob) { return (long)capacity * (with_prob ? 72 : 56); }
PCMS_HD Table table_columns(void* base, int capacity) {
  char* b = static_cast<char*>(base);
  const long c = capacity;
  Table t;
  t.index_sum = reinterpret_cast<long long*>(b);
  t.label = reinterpret_cast<int*>(b + 24 * c);
  t.voxels = reinterpret_cast<int*>(b + 28 * c);
  t.bbox = reinterpret_cast<int*>(b + 32 * c);
  t.peak_key = reinterpret_cast<u64*>(b + 56 * c);
  t.peak = reinterpret_cast<float*>(b + 64 * c);
  t.peak_index = reinterpret_cast<int*>(b + 68 * c);
  return t;
}

// unsigned order of the keys = the total order of the floats: -nan < -inf < ... < -0 < +0 < ...
// < +inf < +nan
PCMS_HD uint32_t float_key(uint32_t bits) { return bits ^ ((bits >> 31) != 0 ? 0xFFFFFFFFu : 0x80000000u); }
// unique per voxel; the maximum is the largest value and, among equals, the smallest index.
// Never 0: the low word is ~i with i < 2^31.
PCMS_HD u64 peak_pack(uint32_t bits, int i) { return ((u64)float_key(bits) << 32) | (uint32_t)~i; }
PCMS_HD void peak_unpack(u64 packed, uint32_t& bits, int& index) {
  if (packed == 0) {  // a row no voxel was added to
    bits = 0;
    index = -1;
    return;
  }
  const uint32_t key = (uint32_t)(packed >> 32);
  bits = (key >> 31) != 0 ? key ^ 0x80000000u : ~key;
  index = (int)~(uint32_t)packed;
}

// what a set of voxels of one component adds to its row
struct Part {
  int count;
  long long sd, sh, sw;
  int d0, d1, h0, h1, w0, w1;
  u64 key;
};
PCMS_HD Part part_none() {
  return Part{0, 0, 0, 0, BOX_MIN_INIT, BOX_MAX_INIT, BOX_MIN_INIT, BOX_MAX_INIT, BOX_MIN_INIT, BOX_MAX_INIT, 0};
}
PCMS_HD Part part_of_voxel(int i, int H, int W, u64 key) {
  const int w = i % W, h = (i / W) % H, d = i / (W * H);
  return Part{1, d, h, w, d, d, h, h, w, w, key};
}
PCMS_HD void part_merge(Part& a, const Part& b) {
  a.count += b.count;
  a.sd += b.sd;
  a.sh += b.sh;
  a.sw += b.sw;
  a.d0 = b.d0 < a.d0 ? b.d0 : a.d0;
  a.d1 = b.d1 > a.d1 ? b.d1 : a.d1;
  a.h0 = b.h0 < a.h0 ? b.h0 : a.h0;
  a.h1 = b.h1 > a.h1 ? b.h1 : a.h1;
  a.w0 = b.w0 < a.w0 ? b.w0 : a.w0;
  a.w1 = b.w1 > a.w1 ? b.w1 : a.w1;
  a.key = b.key > a.key ? b.key : a.key;
}

template <class Mem>
PCMS_HD void row_add(Mem& m, const Table& t, int r, const Part& p, bool with_prob) {
  m.add32(t.voxels + r, p.count);
  m.add64(t.index_sum + 3l * r + 0, p.sd);
  m.add64(t.index_sum + 3l * r + 1, p.sh);
  m.add64(t.index_sum + 3l * r + 2, p.sw);
  int* box = t.bbox + 6l * r;
  m.min32(box + 0, p.d0);
  m.max32(box + 1, p.d1);
  m.min32(box + 2, p.h0);
  m.max32(box + 3, p.h1);
  m.min32(box + 4, p.w0);
  m.max32(box + 5, p.w1);
  if (with_prob) m.max64(t.peak_key + r, p.key);
}

// the initial row: what row_add's operations leave unchanged
PCMS_HD void row_init(const Table& t, int r, bool with_prob) {
  t.label[r] = 0;
  t.voxels[r] = 0;
  for (int k = 0; k < 3; ++k) t.index_sum[3l * r + k] = 0;
  for (int k = 0; k < 6; ++k) t.bbox[6l * r + k] = k % 2 == 0 ? BOX_MIN_INIT : BOX_MAX_INIT;
  if (with_prob) t.peak_key[r] = 0;
}

PCMS_HD bool is_root(const int* labels, long i) { return labels[i] == (int)i + 1; }

// The row of voxel i: -1 on background and for a row at or past capacity; -1 with bad = true
// where the label is not canonical (negative, past the volume, or not naming a root).  rank[] is
// read at roots only, which is where the ranking wrote it.
PCMS_HD int voxel_row(const int* labels, const int* rank, long i, long n, int capacity, bool& bad) {
  const int L = labels[i];
  if (L == 0) return -1;
  const long root = (long)L - 1;
  if (root < 0 || root >= n || labels[root] != L) {
    bad = true;
    return -1;
  }
  const int r = rank[root];
  return r < capacity ? r : -1;
}

}  // namespace pcms_lt
