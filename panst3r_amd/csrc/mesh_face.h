// What the surface sampler (csrc/nearest.hip) and the mesh distance (csrc/meshdist.hip) share about a triangle of an indexed mesh: which faces
// are kept (three indices inside the vertices, nine finite coordinates, a cross product of the edges that is not exactly zero in fp64) and the
// owner of an entry of a prefix sum over the faces.  mf_has_area sets `fp contract(off)` for itself: its fp64 operations are rounded one by one,
// in the order written, whoever includes this header.  (The rasteriser, csrc/mesh.hip, has a clip-space rule of its own.)
#pragma once
#include "common.h"

namespace pst {

struct MeshFace { int ok; float v[3][3]; };

__device__ __forceinline__ MeshFace mf_load(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int f) {
  MeshFace t;
  t.ok = 1;
  int idx[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k] = faces[(int64_t)f * 3 + k];
    if ((unsigned)idx[k] >= (unsigned)Nv) t.ok = 0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = t.ok ? vertices[(int64_t)idx[k] * 3 + a] : 0.f;
      if (!(fabsf(x) <= PST_FMAX)) t.ok = 0;                        // NaN fails the compare
      t.v[k][a] = x;
    }
  return t;
}

__device__ __forceinline__ bool mf_has_area(const MeshFace& t) {
#pragma clang fp contract(off)
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { e1[a] = (double)t.v[1][a] - (double)t.v[0][a]; e2[a] = (double)t.v[2][a] - (double)t.v[0][a]; }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  return !(cx == 0.0 && cy == 0.0 && cz == 0.0);
}

// the last face whose prefix is <= s: it holds entry s of the prefix sum (31 rounds at the most)
__device__ __forceinline__ int mf_prefix_owner(const int32_t* __restrict__ prefix, int F, int s) {
  int lo = 0, hi = F - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
    if (prefix[mid] <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace pst
