// The square root of the mesh shading contract (include/panst3r_hip.h, mesh shading step 8), shared by csrc/mesh_normals.hip and pst_mesh_interp of
// csrc/mesh.hip: Heron's iteration from 1.0 on the argument scaled into [0.5, 2) by an even power of two.  Only fp64 add, multiply and divide in the
// order written, frexp and ldexp (both exact), so tests/mesh_shade_ref.py follows it bit for bit and nothing rests on how an fp64 sqrt is expanded.
// sqrt_heron sets `fp contract(off)` for itself, whoever includes this header.
#pragma once
#include "common.h"

namespace pst {

// finite x > 0 only (the callers test)
__device__ __forceinline__ double sqrt_heron(double x) {
#pragma clang fp contract(off)
  int e;
  (void)frexp(x, &e);
  const int e2 = e - (e & 1);                                       // even, also for a negative e (two's complement)
  const double r = ldexp(x, -e2);                                   // in [0.5, 2)
  double s = 1.0;
#pragma unroll
  for (int it = 0; it < 6; ++it) s = 0.5 * (s + r / s);
  return ldexp(s, e2 / 2);
}

}  // namespace pst
