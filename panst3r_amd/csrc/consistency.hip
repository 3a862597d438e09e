// Cross-view depth consistency of a scene's pointmaps (stage f14; no counterpart in the reference): every pixel of every view projected into every
// OTHER view and compared with the depth that view measured there -> per pixel the number of views that agree with it, the number it violates (it
// lies in space they see through: a "floater") and the number of agreeing views that also give it the same panoptic id.  Restated in
// tests/consistency_ref.py [restated, parity unpinned]; the kernels are held to it bit for bit.  Two kernels over the cloud's device table of
// pst_cloud_view (a scene of mixed shapes is one launch; a workgroup of 256 threads covers 1024 consecutive pixels of one view, thread t the
// pixels t, t + 256, t + 512, t + 768 of them) plus two plain tables, cams float [V, 16] (engine.render.camera_table: rows of [R^T | -R^T t], f, cx,
// cy, near) and dims int32 [V, 2] = (H, W):
//   depth   one pass: the pixel's world point (pts3d, or with `local` pts3d_local moved by c2w: pinhole.h's affine34, as cloud_compact) seen from its OWN camera;
//           depth = zc if conf >= thr, the three camera coordinates are finite and zc >= near, else 0 = "this view measured nothing here"
//   count   a lane with depth 0 writes zeros; the others hold their world points in registers and loop over the target views j != own.  The loop
//           index and the skip are uniform over the workgroup: camera, dims and plane bases of the target come from scalar loads, and the only
//           vector memory traffic in the loop is the gather of the target's depth (and, with labels, of its panoptic id on an agreeing pair).
// The move, the finite test and the projection are pinhole.h's, one text with the splatter (csrc/render.hip); THE PIXEL is this file's: px = floor(u + 0.5), the
// NEAREST PIXEL CENTRE.  The pointmaps' convention puts pixel x at u = x exactly (estimate_focal_knowing_depth subtracts pp from integer pixel
// coordinates), so a view's own points project onto integers up to rounding; the splatter's floor(u), whose pixel (i, j) covers [j, j+1) x [i, i+1),
// would send half of them to their left neighbour.
// The arithmetic is part of the contract (include/panst3r_hip.h): contraction is off for the whole file, every fp32 product, sum and difference is
// rounded on its own (rn_* of wave_ops.h), the perspective quotient is rn_div.  Every test is a negated compare, so a NaN fails it.  No atomics at
// all; every result is written with plain vector stores; two calls return identical bytes.  No read falls outside a view's planes: the gather's
// index is formed only after the in-image test, and a target whose H W exceeds its npix takes no part.
// What bounds count: per (pixel, target) about 20 separately rounded fp32 operations, two IEEE quotients and one 4-byte gather whose lanes land on
// neighbouring target pixels (a few lines per wave, served by L2); the 12-byte source read is once per pixel.  The expectation is the quotients and
// the gathers' latency, not HBM (the measured times are in docs/experiments.md §6s).  Four pixels per thread keep four gathers in flight.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "pinhole.h"             // affine34, finite3, project, view_of, PH_CAM, PH_VIEW_WG; and through it wave_ops.h: rn_mul, rn_add, rn_sub

#pragma clang fp contract(off)

namespace pst {

constexpr int CS_T = 256, CS_PT = 4, CS_WG = CS_T * CS_PT;        // threads, pixels per thread, pixels per workgroup
static_assert(CS_WG == PH_VIEW_WG, "first_wg of a pst_cloud_view table counts workgroups of this many pixels");
constexpr float CS_LIM = 1048576.f;                               // |u|, |v| <= 2^20: px, py and py W + px are formed without overflow

// the world point of pixel i of view v
__device__ __forceinline__ void cs_world(const pst_cloud_view& v, int i, int local, float (&P)[3]) {
  if (local) {                                                     // uniform
    const float* p = v.pts3d_local + (int64_t)i * 3;
    const float x[3] = {p[0], p[1], p[2]};
    affine34(v.c2w, x, P);
  } else {
    const float* p = v.pts3d + (int64_t)i * 3;
    P[0] = p[0]; P[1] = p[1]; P[2] = p[2];
  }
}

__global__ __launch_bounds__(CS_T) void consist_depth_kernel(const pst_cloud_view* __restrict__ views, const float* __restrict__ cams, int nviews, float thr,
                                                             int local, float* __restrict__ depth) {
  const int wg = blockIdx.x;
  const int own = view_of(views, nviews, wg);
  const pst_cloud_view& v = views[own];
  const float* __restrict__ c = cams + (int64_t)own * PH_CAM;
  const float near = c[15];
  const int npix = v.npix;
  const int i0 = (wg - v.first_wg) * CS_WG + threadIdx.x;
#pragma unroll
  for (int k = 0; k < CS_PT; ++k) {
    const int i = i0 + k * CS_T;
    if (i >= npix) continue;
    float d = 0.f;
    if (v.conf[i] >= thr) {                                        // a NaN confidence measures nothing
      float P[3], pc[3];
      cs_world(v, i, local, P);
      affine34(c, P, pc);
      if (finite3(pc) && pc[2] >= near) d = pc[2];
    }
    depth[v.offset + i] = d;
  }
}

template <bool LABELS>
__global__ __launch_bounds__(CS_T) void consist_count_kernel(const pst_cloud_view* __restrict__ views, const float* __restrict__ cams, const int32_t* __restrict__ dims,
                                                             int nviews, float rel_tol, int local, const float* __restrict__ depth, int32_t* __restrict__ agree,
                                                             int32_t* __restrict__ violate, int32_t* __restrict__ same_label) {
  const int wg = blockIdx.x;
  const int own = view_of(views, nviews, wg);
  const pst_cloud_view& v = views[own];
  const int npix = v.npix;
  const int i0 = (wg - v.first_wg) * CS_WG + threadIdx.x;
  float P[CS_PT][3];
  int ag[CS_PT], vi[CS_PT], sl[CS_PT], lab[CS_PT];
  bool live[CS_PT];
#pragma unroll
  for (int k = 0; k < CS_PT; ++k) {
    const int i = i0 + k * CS_T;
    ag[k] = vi[k] = sl[k] = lab[k] = 0;
    P[k][0] = P[k][1] = P[k][2] = 0.f;
    live[k] = i < npix && !(depth[v.offset + i] == 0.f);
    if (live[k]) {
      cs_world(v, i, local, P[k]);
      if (LABELS && v.pan) lab[k] = v.pan[i];
    }
  }
  for (int j = 0; j < nviews; ++j) {
    if (j == own) continue;                                        // uniform
    const float* __restrict__ c = cams + (int64_t)j * PH_CAM;
    const int Hj = dims[2 * j], Wj = dims[2 * j + 1];
    if (Hj < 1 || Wj < 1 || (int64_t)Hj * Wj > views[j].npix) continue;               // uniform: a table that does not fit its planes is never indexed
    const float f = c[12], cx = c[13], cy = c[14], near = c[15];
    const float* __restrict__ dj = depth + views[j].offset;
    const int32_t* __restrict__ pj = LABELS ? views[j].pan : nullptr;
#pragma unroll
    for (int k = 0; k < CS_PT; ++k) {
      if (!live[k]) continue;
      float pc[3], u, w;
      affine34(c, P[k], pc);
      const float zc = pc[2];
      if (!finite3(pc) || !(zc >= near)) continue;
      if (!project(f, f, cx, cy, pc, CS_LIM, u, w)) continue;
      const int px = (int)floorf(rn_add(u, 0.5f)), py = (int)floorf(rn_add(w, 0.5f));   // the nearest pixel centre
      if (px < 0 || px >= Wj || py < 0 || py >= Hj) continue;      // unseen by j
      const int q = py * Wj + px;                                  // < Hj Wj <= npix of j
      const float d = dj[q];
      if (d == 0.f) continue;                                      // j measured nothing there
      const float tol = rn_mul(rel_tol, d);
      if (fabsf(rn_sub(zc, d)) <= tol) {                           // a tie agrees
        ++ag[k];
        if (LABELS && pj && lab[k] > 0 && pj[q] == lab[k]) ++sl[k];
      } else if (rn_sub(d, zc) > tol) {
        ++vi[k];                                                   // in front of what j measured along that ray
      }                                                            // else: occluded, counts for nothing
    }
  }
#pragma unroll
  for (int k = 0; k < CS_PT; ++k) {
    const int i = i0 + k * CS_T;
    if (i >= npix) continue;
    agree[v.offset + i] = ag[k];
    violate[v.offset + i] = vi[k];
    if (LABELS) same_label[v.offset + i] = sl[k];
  }
}

}  // namespace pst

static int consist_shape_ok(const char* what, int nviews, int nwg, int64_t N) {
  using namespace pst;
  if (nviews < 1 || nviews > 65535 || N < 1 || N > 0x7fffffffLL || nwg < 1 || nwg > N) {
    set_error("%s: bad shape (%d views in [1, 65535], N=%lld in [1, 2^31 - 1], %d workgroups in [1, N])", what, nviews, (long long)N, nwg);
    return PST_EINVAL;
  }
  return 0;
}

extern "C" int pst_consist_depth(const pst_cloud_view* views, const float* cams, int nviews, int nwg, int64_t N, float thr, int local, float* depth,
                                 void* stream) {
  using namespace pst;
  if (consist_shape_ok("consist_depth", nviews, nwg, N)) return PST_EINVAL;
  if (!views || !cams || !depth) { set_error("consist_depth: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(consist_depth_kernel, dim3((unsigned)nwg), dim3(CS_T), 0, (hipStream_t)stream, views, cams, nviews, thr, local, depth);
  return check_launch("consist_depth");
}

extern "C" int pst_consist_count(const pst_cloud_view* views, const float* cams, const int32_t* dims, int nviews, int nwg, int64_t N, float rel_tol, int local,
                                 const float* depth, int32_t* agree, int32_t* violate, int32_t* same_label, void* stream) {
  using namespace pst;
  if (consist_shape_ok("consist_count", nviews, nwg, N)) return PST_EINVAL;
  if (!(rel_tol >= 0.f && rel_tol < 1.f)) { set_error("consist_count: rel_tol=%g is not a number in [0, 1)", (double)rel_tol); return PST_EINVAL; }
  if (!views || !cams || !dims || !depth || !agree || !violate) { set_error("consist_count: null operand"); return PST_EINVAL; }
  if (same_label) hipLaunchKernelGGL(consist_count_kernel<true>, dim3((unsigned)nwg), dim3(CS_T), 0, (hipStream_t)stream, views, cams, dims, nviews, rel_tol, local,
                                     depth, agree, violate, same_label);
  else hipLaunchKernelGGL(consist_count_kernel<false>, dim3((unsigned)nwg), dim3(CS_T), 0, (hipStream_t)stream, views, cams, dims, nviews, rel_tol, local, depth,
                          agree, violate, same_label);
  return check_launch("consist_count");
}
