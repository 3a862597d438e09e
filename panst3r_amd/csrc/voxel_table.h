// The open-addressing table of the voxel stages (csrc/voxel.hip, csrc/components.hip): the 3 x 21-bit cell key, its hash, the bounded
// find-or-claim probe and the runs of equal keys inside a wave.  Integer code only.
#pragma once
#include "common.h"

namespace pst {

constexpr uint64_t VX_EMPTY = ~0ull;                               // no key is all ones: every 21-bit field is in [1, 2^21 - 1]
constexpr int VX_LIM = 1 << 20;

__device__ __forceinline__ uint64_t vx_hash(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

// lanes [head, tail] = the run of adjacent lanes that hold this lane's key.  Every lane of the wave must call it.
__device__ __forceinline__ void vx_run(uint64_t key, int lane, int& head, int& tail) {
  const uint64_t prev = __shfl_up((unsigned long long)key, 1);
  const uint64_t heads = __ballot(lane == 0 || prev != key);
  head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
  tail = above ? lane + __builtin_ctzll(above) : 63;
}

// the slot of `key`: claimed if it is not in the table yet.  -1 = the table is full (never: capacity >= 2 M), reported through *status.
__device__ __forceinline__ int vx_find_or_claim(uint64_t* __restrict__ keys, uint32_t mask, uint64_t key, int32_t* __restrict__ status) {
  uint32_t h = (uint32_t)vx_hash(key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    uint64_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == VX_EMPTY) k = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)VX_EMPTY, (unsigned long long)key);
    if (k == VX_EMPTY || k == key) return (int)h;
    h = (h + 1) & mask;
  }
  atomicOr(status, 1);
  return -1;
}

}  // namespace pst
