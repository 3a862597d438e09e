// The cell grid of the hash-grid stages (csrc/voxel.hip, csrc/components.hip, csrc/nearest.hip, csrc/meshdist.hip), written once: the cell of a
// point, the 3 x 21-bit cell key and its range test, the hash, the open-addressing table (the bounded claiming probe of a build, the read-only
// probe of a finished table), the per-cell lists (filled by arrival, guarded before they are read) and the launchers' capacity check.  (The runs
// of equal keys inside a wave, vx_run, are in wave_ops.h, which this header includes for its users.)  Integer code, and one fp32 multiply in
// vx_cell_of, which sets `fp contract(off)` for itself: whoever includes this header, and with whatever flags, the product is rounded on its own
// before the floor.
#pragma once
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "wave_ops.h"

namespace pst {

constexpr uint64_t VX_EMPTY = ~0ull;                               // no key is all ones: every 21-bit field is in [1, 2^21 - 1]
constexpr int VX_LIM = 1 << 20;
constexpr int VX_FULL = 1, VX_LISTS = 2;                           // the bits of a stage's status[0] that this header sets
static_assert(PST_VCC_FULL == VX_FULL && PST_NN_FULL == VX_FULL && PST_MESHDIST_FULL == VX_FULL, "one bit for a table without an empty slot");
static_assert(PST_NN_LISTS == VX_LISTS && PST_MESHDIST_LISTS == VX_LISTS, "one bit for a list that is not this build's");

__device__ __forceinline__ bool vx_in_range(int x, int y, int z) {
  return x > -VX_LIM && x < VX_LIM && y > -VX_LIM && y < VX_LIM && z > -VX_LIM && z < VX_LIM;
}
__device__ __forceinline__ uint64_t vx_key(int x, int y, int z) {     // only for cells in range: no field wraps
  return (uint64_t)(x + VX_LIM) | ((uint64_t)(y + VX_LIM) << 21) | ((uint64_t)(z + VX_LIM) << 42);
}

// the cell of a point: c = floor(x * inv) per axis (whole numbers as floats); finite = every |x| <= FLT_MAX, ok = finite and every |c| < 2^20
__device__ __forceinline__ void vx_cell_of(const float (&x)[3], float inv, float (&c)[3], bool& finite, bool& ok) {
#pragma clang fp contract(off)
  finite = ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = floorf(x[a] * inv);
    finite = finite && (fabsf(x[a]) <= PST_FMAX);                   // NaN fails the compare
    ok = ok && (fabsf(c[a]) < (float)VX_LIM);
  }
  ok = ok && finite;
}

__device__ __forceinline__ uint64_t vx_hash(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

// the slot of `key` while the table is being built: claimed if it is not in the table yet (*claimed, where given, tells which).
// -1 = the table is full (never: capacity >= 2 M), reported through *status.
__device__ __forceinline__ int vx_find_or_claim(uint64_t* __restrict__ keys, uint32_t mask, uint64_t key, int32_t* __restrict__ status,
                                                bool* claimed = nullptr) {
  uint32_t h = (uint32_t)vx_hash(key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    uint64_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == VX_EMPTY) k = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)VX_EMPTY, (unsigned long long)key);
    if (k == VX_EMPTY || k == key) {
      if (claimed) *claimed = k == VX_EMPTY;
      return (int)h;
    }
    h = (h + 1) & mask;
  }
  atomicOr(status, VX_FULL);
  return -1;
}

// the slot of `key` in a complete table (an earlier launch built it: plain loads), -1 if the key is absent.  A table without an empty slot
// (never: capacity >= 2 M) is reported through *status.
__device__ __forceinline__ int vx_find(const uint64_t* __restrict__ keys, uint32_t mask, uint64_t key, int32_t* __restrict__ status) {
  uint32_t h = (uint32_t)vx_hash(key) & mask;
  int slot = -1;
  uint32_t n = 0;
  for (; n <= mask; ++n) {
    const uint64_t k = keys[h];
    if (k == key) { slot = (int)h; break; }
    if (k == VX_EMPTY) break;
    h = (h + 1) & mask;
  }
  if (n > mask) atomicOr(status, VX_FULL);
  return slot;
}

// ---------------------------------------------------------------- the per-cell lists: rows[start[slot] + k] = the k-th arrival of the slot's cell, k < cell_count[slot]
// one more arrival into its cell's list: rows[its position] = value() (which position depends on arrival; nothing that leaves depends on it;
// `value` is called only for an arrival that is placed) -> the position, or -1 and the LISTS bit if the counts are not those of this insert:
// nothing is placed then.  The arrival that fills a list reports its length: status[2] = the longest list.
template <typename Value>
__device__ __forceinline__ int vx_list_place(int slot, const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count, int32_t* __restrict__ fill,
                                             int total, int32_t* __restrict__ rows, int32_t* __restrict__ status, Value value) {
  const int k = atomicAdd(&fill[slot], 1), n = cell_count[slot], pos = start[slot] + k;
  if ((unsigned)k >= (unsigned)n || (unsigned)pos >= (unsigned)total) { atomicOr(&status[0], VX_LISTS); return -1; }
  rows[pos] = value();
  if (k == n - 1) atomicMax(&status[2], n);
  return pos;
}

// the list of a slot before it is read: rows[b, b + cnt), cnt clamped to max_count (the caller refused a longer list before this launch).
// false and the LISTS bit for a list that leaves rows[0, total): not this build's.
__device__ __forceinline__ bool vx_list_range(int slot, const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count, int total, int max_count,
                                              int32_t* __restrict__ status, int& b, int& cnt) {
  b = start[slot];
  cnt = min(cell_count[slot], max_count);
  if ((unsigned)b > (unsigned)total || cnt < 0 || cnt > total - b) { atomicOr(&status[0], VX_LISTS); return false; }
  return true;
}

// ---------------------------------------------------------------- launcher side
static inline bool vx_cap_ok(int64_t n, int64_t cap) { return cap >= 2 * n && cap <= (1ll << 31) && (cap & (cap - 1)) == 0; }

// a table of the lists of `n` items: 1 .. max_n of them, capacity a power of two >= 2 n.  `name` = what the entry point calls n, `range` = its
// words for the limit
static inline int vx_table_ok(const char* what, int64_t n, int64_t max_n, int64_t capacity, const char* name, const char* range) {
  if (n <= 0 || n > max_n || !vx_cap_ok(n, capacity)) {
    set_error("%s: bad shape (%s=%lld: %s; capacity=%lld: a power of two >= 2 %s)", what, name, (long long)n, range, (long long)capacity, name);
    return PST_EINVAL;
  }
  return 0;
}

}  // namespace pst
