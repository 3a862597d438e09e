// The pinhole camera of the geometry stages (csrc/cloud.hip, consistency.hip, render.hip, mesh.hip, the ICP steps of nearest.hip and meshdist.hip),
// written once: the move of a point by a 3 x 4 fp32 matrix, the finite test, the perspective projection, the two layouts of the 16-float camera row,
// the workgroup -> view lookup of a pst_cloud_view table.  The arithmetic is contract (include/panst3r_hip.h), held bit for bit by the stages' tests;
// every operation is one of wave_ops.h's rn_*, which carry `fp contract(off)` themselves, whatever the including file sets.  What stays with each
// caller, under its own comment: the cull `three finite coordinates, then zc >= near` in that order, the pixel rule (floor(u) in the splatter,
// floor(u + 0.5) in the consistency count, rint(256 u) in the rasteriser) and the limit on |u|, |v| (2^20, 2^20, 2^14: three reasons).
#pragma once
#include "../../include/panst3r_hip.h"
#include "wave_ops.h"

namespace pst {

// floats per camera row of a device table: [R^T | -R^T t] row-major in [0, 12), then `f cx cy near` (engine.render.camera_table: the splatter and the
// consistency kernels) or `fx fy cx cy` (engine.mesh.mesh_camera_table: the rasteriser, whose near and far are arguments)
constexpr int PH_CAM = 16;
constexpr int PH_VIEW_WG = 1024;   // pixels per workgroup of every kernel that walks a pst_cloud_view table by first_wg (cloud.hip, consistency.hip)

// m_r = ((a_r0 x0 + a_r1 x1) + a_r2 x2) + a_r3 over the row-major 3 x 4 matrix a: every product and every sum rounded on its own, in this order
__device__ __forceinline__ void affine34(const float* a, const float (&x)[3], float (&m)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    m[r] = rn_add(rn_add(rn_add(rn_mul(a[4 * r + 0], x[0]), rn_mul(a[4 * r + 1], x[1])), rn_mul(a[4 * r + 2], x[2])), a[4 * r + 3]);
}
// three finite coordinates (a NaN fails every compare).  render_splat_kernel and ms_vertex write this test out at the call: inlined from here it
// arrives as one `and` of three compares, and the compiler no longer computes the zc row after the test on xc and yc (docs/experiments.md §17)
__device__ __forceinline__ bool finite3(const float (&p)[3]) { return fabsf(p[0]) <= PST_FMAX && fabsf(p[1]) <= PST_FMAX && fabsf(p[2]) <= PST_FMAX; }
// u = (fx xc) / zc + cx, v = (fy yc) / zc + cy: a rounded product, the quotient taken in fp64 and rounded once (rn_div), a rounded sum.
// -> |u| <= lim and |v| <= lim, which the caller tests BEFORE any conversion to int (a NaN or an infinity fails it)
__device__ __forceinline__ bool project(float fx, float fy, float cx, float cy, const float (&pc)[3], float lim, float& u, float& v) {
  u = rn_add(rn_div(rn_mul(fx, pc[0]), pc[2]), cx), v = rn_add(rn_div(rn_mul(fy, pc[1]), pc[2]), cy);
  return fabsf(u) <= lim && fabsf(v) <= lim;
}
// the view that owns workgroup wg: the last one whose first workgroup is <= wg (uniform: scalar loads)
__device__ __forceinline__ int view_of(const pst_cloud_view* views, int nviews, int wg) { return last_le(nviews, wg, [&](int v) { return views[v].first_wg; }); }

}  // namespace pst
