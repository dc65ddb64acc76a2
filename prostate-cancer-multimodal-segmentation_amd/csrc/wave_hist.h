// The LDS histogram add that intensity.hip (digit counts of the radix select) and align.hip (the
// joint intensity histogram) share.
#pragma once
#include "common.h"

namespace {

// hist[digit] += 1 for every lane that is `on`.  An MR volume is mostly one value, so most lanes
// of a wave meet in one bin: the lanes that share the first active lane's bin are counted by a
// ballot and added once, only the others add for themselves.  Every lane of the wave must reach
// the call.
__device__ __forceinline__ void bin_add(uint32_t* hist, uint32_t digit, bool on, int lane) {
  const unsigned long long active = __ballot(on);
  if (active == 0) return;  // uniform over the wave
  const int leader = __ffsll(active) - 1;
  const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)digit, leader);
  const bool share = on && digit == d0;
  const uint32_t lanes = (uint32_t)__popcll(__ballot(share));
  if (lane == leader)
    __hip_atomic_fetch_add(hist + d0, lanes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else if (on && !share)
    __hip_atomic_fetch_add(hist + digit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace
