// The wait-free union-find on a parent[] array of rows, shared by csrc/components.hip (voxels joined through their neighbouring cells) and
// csrc/surface.hip (faces joined through their vertex rows).  parent[x] <= x always and values only decrease, so every loop ends, no thread ever
// waits for another thread's store, and the root of a finished component is its smallest row whatever the arrival order.  Every loop is bounded: an
// overflow sets PST_VCC_LOOP in status[0] and ends the loop.
#pragma once
#include "common.h"

namespace pst {

__device__ __forceinline__ int cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x as far as this thread can see, with path halving: parent[x] = its grandparent (atomicMin: values only decrease).  x falls in every step.
__device__ __forceinline__ int cc_find(int32_t* __restrict__ parent, int x, int bound, int32_t* __restrict__ status) {
  for (int it = 0; it < bound; ++it) {
    const int p = cc_load(&parent[x]);
    if (p == x) return x;
    const int g = cc_load(&parent[p]);
    if (g == p) return p;
    atomicMin(&parent[x], g);
    x = g;
  }
  atomicOr(status, PST_VCC_LOOP);
  return x;
}

// wait-free union: the larger of the two roots is hooked under the smaller.  When the atomic finds that `hi` was hooked by someone else (old < hi), hi now
// hangs under min(old, lo) and what is left is to unite old and lo: max(a, b) falls in every round, so there are at most `bound` of them.
__device__ __forceinline__ void cc_unite(int32_t* __restrict__ parent, int a, int b, int bound, int32_t* __restrict__ status) {
  a = cc_find(parent, a, bound, status);
  b = cc_find(parent, b, bound, status);
  for (int it = 0; it < bound && a != b; ++it) {                    // both finds agree: no atomic
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(&parent[hi], lo);
    if (old == hi) return;
    a = cc_find(parent, old, bound, status);
    b = cc_find(parent, lo, bound, status);
  }
  if (a != b) atomicOr(status, PST_VCC_LOOP);
}

}  // namespace pst
