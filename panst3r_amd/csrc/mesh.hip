// A z-buffered triangle rasteriser: a mesh with one panoptic id per vertex (or per face) seen from B pinhole cameras -> per pixel the nearest face's
// depth, index and id, and after a per-view minimum-area filter the ground-truth maps that csrc/evaluate.hip scores against.  The reference renders
// them through pyrender / OpenGL (tools/preprocess_scannetpp.py:395-494); restated in tests/mesh_ref.py, [restated, parity unpinned].  The contract is
// the mesh section of include/panst3r_hip.h; everything is exact, so the outputs are held to the restatement bit for bit:
//   vertex    world -> camera in separately rounded fp32, the perspective quotient in fp64 rounded once (pinhole.h, one text with render.hip), then SNAPPED to 1/256
//             pixel: from here on coverage is integer arithmetic (int64 edge functions, the top-left rule), so a pixel centre on a shared edge belongs
//             to exactly one of the two faces - no crack, no double hit - whatever the order of evaluation.
//   depth     perspective-correct in fp64 from the integer edge values and the three 1 / zc: one rounding to fp32 at the end.
//   z-buffer  render.hip's: key = (bits(depth) << 32) | face, 64-bit atomicMin into a buffer the caller cleared to all ones.  INTEGER atomics only.
// Vertices are transformed per (camera, face), three per face, NOT once per (camera, vertex) into a buffer: that buffer is 12 bytes x B x Nv (2 GB
// for a chunk of 170 cameras of 384 x 512 and a million vertices) and a launch of its own, against roughly six times the arithmetic of a transform
// that is 9 multiplies, 9 additions and two divisions next to three scattered 12-byte gathers per face either way.
// Two raster paths:
//   lane  one lane per (camera, face), the camera on grid.y, loops over the face's pixel bounding box when it holds at most PST_MESH_LANE_PIXELS
//         pixels.  A larger face is appended to a compacted list (a 64-bit counter, vector atomics and stores) ...
//   wave  ... that a second launch walks one wave per entry, the 64 lanes striding over the box: one floor triangle that fills a 384 x 512 image is
//         3 072 passes of a wave instead of 196 608 iterations of one lane with 63 lanes idle.  The second launch has a fixed grid and reads the
//         count from the device: no host sync.  A full list is no error - the lane rasterises the face itself (the minimum is order-free).
// PST_MESH_LANE_PIXELS = 64, the width of a wave: the wave path needs at least one pass plus a second set-up of the face (index and vertex gathers,
// three transforms, a list append and read), so a box of up to 64 pixels cannot finish sooner there than one pass, while in the lane path it costs at
// most 64 iterations that the other lanes of the wave mostly share with faces of their own.  Above 64 the wave path's passes are ceil(n / 64) < n.
// `precheck`: as render.hip's - a relaxed load of the cell first, the atomic only for a key below what the load saw.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "pinhole.h"             // affine34, project, PH_CAM; and through it wave_ops.h: vx_run, id_row
#include "heron.h"               // sqrt_heron: the square root of the shading contract (pst_mesh_interp, at the end of this file)

#pragma clang fp contract(off)

namespace pst {

constexpr int MS_T = 256;
constexpr unsigned long long MS_EMPTY = ~0ull;
constexpr float MS_LIM = 16384.f;                                  // |u|, |v| <= 2^14: |X|, |Y| <= 2^22, every edge value below 2^47
constexpr int MS_BIG_BLOCKS = 2048;                                // the wave path's fixed grid: 8 192 waves stride the list

// a face set up for one camera: corner k's snapped position and 1 / zc, and per corner k the opposite edge a -> b
struct MsTri {
  int X[3], Y[3];
  double q[3], A;
  int dx[3], dy[3];                                                // edge k: d = (X_b - X_a, Y_b - Y_a), (a, b) = (1, 2), (2, 0), (0, 1)
  int least[3];                                                    // the smallest E_k that covers: 0 on a top or left edge, else 1
  bool swapped;                                                    // corners 1 and 2 were exchanged (A < 0 as listed)
  int j0, j1, i0, i1;                                              // the pixel bounding box, clipped to the image
};

__device__ __forceinline__ bool ms_vertex(const float* __restrict__ c, const float* __restrict__ vertices, int64_t vi, float near, int& X, int& Y, float& zc) {
  const float P[3] = {vertices[vi * 3 + 0], vertices[vi * 3 + 1], vertices[vi * 3 + 2]};
  float pc[3], u, v;
  affine34(c, P, pc);
  zc = pc[2];
  if (!(fabsf(pc[0]) <= PST_FMAX && fabsf(pc[1]) <= PST_FMAX && fabsf(zc) <= PST_FMAX) || !(zc >= near)) return false;      // finite3, written out: pinhole.h says why
  if (!project(c[12], c[13], c[14], c[15], pc, MS_LIM, u, v)) return false;
  X = (int)rintf(u * 256.f);                                        // the product is exact; rintf rounds half to even
  Y = (int)rintf(v * 256.f);
  return true;
}

// steps 2 and 3 and the clipped bounding box; false: the face leaves no trace in this camera
__device__ __forceinline__ bool ms_setup(const float* __restrict__ c, const float* __restrict__ vertices, int64_t Nv, const int32_t* __restrict__ faces, int64_t f,
                                         float near, int H, int W, MsTri& t) {
  float zc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t vi = faces[f * 3 + k];
    if (vi < 0 || vi >= Nv) return false;                           // no read outside the vertices
    if (!ms_vertex(c, vertices, vi, near, t.X[k], t.Y[k], zc[k])) return false;
  }
  int64_t A = (int64_t)(t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (int64_t)(t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
  if (A == 0) return false;
  t.swapped = A < 0;
  if (t.swapped) {
    int s = t.X[1]; t.X[1] = t.X[2]; t.X[2] = s;
    s = t.Y[1]; t.Y[1] = t.Y[2]; t.Y[2] = s;
    const float z = zc[1]; zc[1] = zc[2]; zc[2] = z;
    A = -A;
  }
  t.A = (double)A;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    t.q[k] = 1.0 / (double)zc[k];
    t.dx[k] = t.X[b] - t.X[a];
    t.dy[k] = t.Y[b] - t.Y[a];
    t.least[k] = (t.dy[k] < 0 || (t.dy[k] == 0 && t.dx[k] > 0)) ? 0 : 1;
  }
  const int xlo = min(t.X[0], min(t.X[1], t.X[2])), xhi = max(t.X[0], max(t.X[1], t.X[2]));
  const int ylo = min(t.Y[0], min(t.Y[1], t.Y[2])), yhi = max(t.Y[0], max(t.Y[1], t.Y[2]));
  // pixel j is sampled at 256 j + 128: j0 = ceil((xlo - 128) / 256), j1 = floor((xhi - 128) / 256); |X| <= 2^22, the shifts are arithmetic
  t.j0 = max((xlo + 127) >> 8, 0); t.j1 = min((xhi - 128) >> 8, W - 1);
  t.i0 = max((ylo + 127) >> 8, 0); t.i1 = min((yhi - 128) >> 8, H - 1);
  return t.j0 <= t.j1 && t.i0 <= t.i1;
}

// E_k at the centre of pixel (i, j): |values| < 2^47 for a pixel inside the bounding box
__device__ __forceinline__ void ms_edges(const MsTri& t, int i, int j, int64_t (&E)[3]) {
  const int64_t px = 256 * (int64_t)j + 128, py = 256 * (int64_t)i + 128;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3;
    E[k] = (int64_t)t.dx[k] * (py - t.Y[a]) - (int64_t)t.dy[k] * (px - t.X[a]);
  }
}

// steps 4 - 6 for one pixel of the box: 0 <= i < H, 0 <= j < W, so the cell is inside the camera's H x W
template <bool PRECHECK>
__device__ __forceinline__ void ms_sample(const MsTri& t, int i, int j, float near, float far, uint32_t face, unsigned long long* __restrict__ zb, int W) {
  int64_t E[3];
  ms_edges(t, i, j, E);
  if (E[0] < t.least[0] || E[1] < t.least[1] || E[2] < t.least[2]) return;
  const double s = ((double)E[0] * t.q[0] + (double)E[1] * t.q[1]) + (double)E[2] * t.q[2];
  const float depth = (float)(t.A / s);
  if (!(depth >= near && depth <= far)) return;                     // a NaN fails; far is finite
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)face;
  unsigned long long* p = zb + (int64_t)i * W + j;
  if constexpr (PRECHECK)
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin(p, key);
}

template <bool PRECHECK>
__global__ __launch_bounds__(MS_T) void mesh_raster_kernel(const float* __restrict__ vertices, int64_t Nv, const int32_t* __restrict__ faces, int64_t Nf,
                                                           const float* __restrict__ cams, int H, int W, float near, float far,
                                                           unsigned long long* __restrict__ zbuf, unsigned long long* __restrict__ big,
                                                           unsigned long long* __restrict__ big_count, int64_t big_capacity) {
  const int64_t f = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  if (f >= Nf) return;
  MsTri t;
  if (!ms_setup(cams + (int64_t)blockIdx.y * PH_CAM, vertices, Nv, faces, f, near, H, W, t)) return;
  const int64_t n = (int64_t)(t.j1 - t.j0 + 1) * (t.i1 - t.i0 + 1);
  if (n > PST_MESH_LANE_PIXELS) {
    const unsigned long long slot = atomicAdd(big_count, 1ull);
    if (slot < (unsigned long long)big_capacity) {                  // inside the list; a full list leaves the face to this lane
      big[slot] = ((unsigned long long)blockIdx.y << 32) | (unsigned long long)f;
      return;
    }
  }
  unsigned long long* __restrict__ zb = zbuf + (int64_t)blockIdx.y * H * W;
  for (int i = t.i0; i <= t.i1; ++i)
    for (int j = t.j0; j <= t.j1; ++j) ms_sample<PRECHECK>(t, i, j, near, far, (uint32_t)f, zb, W);
}

template <bool PRECHECK>
__global__ __launch_bounds__(MS_T) void mesh_raster_big_kernel(const float* __restrict__ vertices, int64_t Nv, const int32_t* __restrict__ faces, int64_t Nf,
                                                               const float* __restrict__ cams, int ncams, int H, int W, float near, float far,
                                                               unsigned long long* __restrict__ zbuf, const unsigned long long* __restrict__ big,
                                                               const unsigned long long* __restrict__ big_count, int64_t big_capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * MS_T + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * (MS_T / 64);
  const unsigned long long total = *big_count;
  const int64_t cnt = total < (unsigned long long)big_capacity ? (int64_t)total : big_capacity;
  for (int64_t k = wave; k < cnt; k += nwaves) {                    // uniform per wave
    const unsigned long long e = big[k];
    const int64_t cam = (int64_t)(e >> 32), f = (int64_t)(uint32_t)e;
    if (cam >= ncams || f >= Nf) continue;                          // (cannot happen for a list the lane kernel wrote)
    MsTri t;
    if (!ms_setup(cams + cam * PH_CAM, vertices, Nv, faces, f, near, H, W, t)) continue;
    const uint32_t bw = (uint32_t)(t.j1 - t.j0 + 1), n = bw * (uint32_t)(t.i1 - t.i0 + 1);      // n <= H W < 2^31
    unsigned long long* __restrict__ zb = zbuf + cam * H * W;
    for (uint32_t p = (uint32_t)lane; p < n; p += 64) ms_sample<PRECHECK>(t, t.i0 + (int)(p / bw), t.j0 + (int)(p % bw), near, far, (uint32_t)f, zb, W);
  }
}

__global__ __launch_bounds__(MS_T) void mesh_resolve_kernel(const unsigned long long* __restrict__ zbuf, int64_t npix, int H, int W, const float* __restrict__ vertices,
                                                            int64_t Nv, const int32_t* __restrict__ faces, int64_t Nf, const float* __restrict__ cams, float near,
                                                            const int32_t* __restrict__ vertex_ids, const int32_t* __restrict__ face_ids,
                                                            int64_t* __restrict__ face, float* __restrict__ depth, int32_t* __restrict__ pan) {
  const int64_t p = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  if (p >= npix) return;
  const unsigned long long key = zbuf[p];
  const int64_t f = (int64_t)(uint32_t)key;
  const bool hit = key != MS_EMPTY && f < Nf;                       // (f < Nf always holds for a buffer the raster kernels filled)
  int id = 0;
  if (hit && face_ids) id = face_ids[f];
  else if (hit && vertex_ids) {
    const int64_t hw = (int64_t)H * W, cam = p / hw, pix = p % hw;
    MsTri t;
    if (ms_setup(cams + cam * PH_CAM, vertices, Nv, faces, f, near, H, W, t)) {      // (true for a face that won a pixel of this camera)
      int64_t E[3];
      ms_edges(t, (int)(pix / W), (int)(pix % W), E);
      // the corner with the largest E_k, ties to the lowest position as listed: corner k stands at position k, 1 and 2 exchanged after a swap
      const int64_t e1 = t.swapped ? E[2] : E[1], e2 = t.swapped ? E[1] : E[2];
      int pos = 0;
      int64_t best = E[0];
      if (e1 > best) { best = e1; pos = 1; }
      if (e2 > best) pos = 2;
      id = vertex_ids[faces[f * 3 + pos]];                          // ms_setup checked the three indices
    }
  }
  face[p] = hit ? f : -1;
  depth[p] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
  pan[p] = id;
}

constexpr uint32_t MS_NONE = 0xffffffffu;

// counts[b, row] += 1 per pixel of a listed id.  Maps are piecewise constant and same-address atomics serialise: a run of adjacent lanes with one key
// adds its length with one atomic from its first lane (evaluate.hip's merge).  Every lane takes part in vx_run.
__global__ __launch_bounds__(MS_T) void mesh_area_count_kernel(const int32_t* __restrict__ pan, int64_t npix, int64_t hw, const int32_t* __restrict__ id2row, int ntab,
                                                               int S, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  uint32_t key = MS_NONE;
  if (p < npix) {
    const int r = id_row(pan[p], id2row, ntab, S, -1);                 // -1 = not listed
    if (r >= 0) key = (uint32_t)((p / hw) * S + r);                 // B S <= 2^31 - 1
  }
  int head, tail;
  vx_run(key, lane, head, tail);
  if (lane == head && key != MS_NONE) atomicAdd(&counts[key], tail - head + 1);
}

__global__ __launch_bounds__(MS_T) void mesh_area_apply_kernel(const int32_t* __restrict__ pan, int64_t npix, int64_t hw, const int32_t* __restrict__ id2row, int ntab,
                                                               int S, const int32_t* __restrict__ counts, int min_area, int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  if (p >= npix) return;
  const int id = pan[p];
  const int r = id_row(id, id2row, ntab, S, -1);
  out[p] = (r >= 0 && counts[(p / hw) * S + r] >= min_area) ? id : 0;
}

static bool ms_shape_ok(int ncams, int H, int W) {
  return ncams >= 1 && ncams <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffffLL / ncams;
}

}  // namespace pst

extern "C" int pst_mesh_lane_pixels(void) { return PST_MESH_LANE_PIXELS; }

extern "C" int pst_mesh_raster(const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams, int ncams, int H, int W, float near_z,
                               float far_z, uint64_t* zbuf, uint64_t* big, uint64_t* big_count, int64_t big_capacity, int precheck, void* stream) {
  using namespace pst;
  if (Nv <= 0 || Nv > 0x7fffffffLL || Nf <= 0 || Nf > 0x7fffffffLL || !ms_shape_ok(ncams, H, W) || big_capacity < 0) {
    set_error("mesh_raster: bad shape (Nv=%lld, Nf=%lld in [1, 2^31 - 1], %d cameras in [1, 65535], %d x %d pixels, cameras x pixels < 2^31, capacity %lld)",
              (long long)Nv, (long long)Nf, ncams, H, W, (long long)big_capacity);
    return PST_EINVAL;
  }
  if (!(near_z > 0.f) || !(far_z > near_z) || !(far_z <= PST_FMAX)) { set_error("mesh_raster: needs 0 < near < far, finite; got %g, %g", (double)near_z, (double)far_z); return PST_EINVAL; }
  if (!vertices || !faces || !cams || !zbuf || !big_count || (big_capacity > 0 && !big)) { set_error("mesh_raster: null operand"); return PST_EINVAL; }
  const dim3 grid(blocks_for(Nf, MS_T).x, (unsigned)ncams);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *zb = (unsigned long long*)zbuf, *bg = (unsigned long long*)big, *bc = (unsigned long long*)big_count;
  if (precheck) hipLaunchKernelGGL(mesh_raster_kernel<true>, grid, dim3(MS_T), 0, st, vertices, Nv, faces, Nf, cams, H, W, near_z, far_z, zb, bg, bc, big_capacity);
  else hipLaunchKernelGGL(mesh_raster_kernel<false>, grid, dim3(MS_T), 0, st, vertices, Nv, faces, Nf, cams, H, W, near_z, far_z, zb, bg, bc, big_capacity);
  if (big_capacity > 0) {
    const int64_t want = (big_capacity + MS_T / 64 - 1) / (MS_T / 64);
    const dim3 bgrid((unsigned)(want < MS_BIG_BLOCKS ? want : MS_BIG_BLOCKS));
    if (precheck) hipLaunchKernelGGL(mesh_raster_big_kernel<true>, bgrid, dim3(MS_T), 0, st, vertices, Nv, faces, Nf, cams, ncams, H, W, near_z, far_z, zb, bg, bc,
                                     big_capacity);
    else hipLaunchKernelGGL(mesh_raster_big_kernel<false>, bgrid, dim3(MS_T), 0, st, vertices, Nv, faces, Nf, cams, ncams, H, W, near_z, far_z, zb, bg, bc, big_capacity);
  }
  return check_launch("mesh_raster");
}

extern "C" int pst_mesh_resolve(const uint64_t* zbuf, int ncams, int H, int W, const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams,
                                float near_z, const int32_t* vertex_ids, const int32_t* face_ids, int64_t* face, float* depth, int32_t* pan, void* stream) {
  using namespace pst;
  if (Nv <= 0 || Nv > 0x7fffffffLL || Nf <= 0 || Nf > 0x7fffffffLL || !ms_shape_ok(ncams, H, W)) {
    set_error("mesh_resolve: bad shape (Nv=%lld, Nf=%lld in [1, 2^31 - 1], %d cameras in [1, 65535], %d x %d pixels, cameras x pixels < 2^31)", (long long)Nv,
              (long long)Nf, ncams, H, W);
    return PST_EINVAL;
  }
  if (vertex_ids && face_ids) { set_error("mesh_resolve: vertex_ids and face_ids are exclusive"); return PST_EINVAL; }
  if (!zbuf || !vertices || !faces || !cams || !face || !depth || !pan) { set_error("mesh_resolve: null operand"); return PST_EINVAL; }
  const int64_t npix = (int64_t)ncams * H * W;
  hipLaunchKernelGGL(mesh_resolve_kernel, blocks_for(npix, MS_T), dim3(MS_T), 0, (hipStream_t)stream, (const unsigned long long*)zbuf, npix, H, W,
                     vertices, Nv, faces, Nf, cams, near_z, vertex_ids, face_ids, face, depth, pan);
  return check_launch("mesh_resolve");
}

static bool ms_area_ok(const char* what, const void* pan, int ncams, int64_t hw, const void* id2row, int ntab, int S, const void* counts) {
  using namespace pst;
  if (ncams < 1 || ncams > 65535 || hw < 1 || hw > 0x7fffffffLL / ncams || ntab < 1 || S < 1 || S > 0x7fffffff / ncams) {
    set_error("%s: bad shape (%d cameras in [1, 65535], %lld pixels each, cameras x pixels < 2^31, ntab=%d, S=%d, cameras x S < 2^31)", what, ncams, (long long)hw, ntab, S);
    return false;
  }
  if (!pan || !id2row || !counts) { set_error("%s: null operand", what); return false; }
  return true;
}

extern "C" int pst_mesh_area_count(const int32_t* pan, int ncams, int64_t hw, const int32_t* id2row, int ntab, int S, int32_t* counts, void* stream) {
  using namespace pst;
  if (!ms_area_ok("mesh_area_count", pan, ncams, hw, id2row, ntab, S, counts)) return PST_EINVAL;
  const int64_t npix = ncams * hw;
  hipLaunchKernelGGL(mesh_area_count_kernel, blocks_for(npix, MS_T), dim3(MS_T), 0, (hipStream_t)stream, pan, npix, hw, id2row, ntab, S, counts);
  return check_launch("mesh_area_count");
}

extern "C" int pst_mesh_area_apply(const int32_t* pan, int ncams, int64_t hw, const int32_t* id2row, int ntab, int S, const int32_t* counts, int min_area, int32_t* out,
                                   void* stream) {
  using namespace pst;
  if (!ms_area_ok("mesh_area_apply", pan, ncams, hw, id2row, ntab, S, counts)) return PST_EINVAL;
  if (!out) { set_error("mesh_area_apply: null operand"); return PST_EINVAL; }
  const int64_t npix = ncams * hw;
  hipLaunchKernelGGL(mesh_area_apply_kernel, blocks_for(npix, MS_T), dim3(MS_T), 0, (hipStream_t)stream, pan, npix, hw, id2row, ntab, S, counts,
                     min_area, out);
  return check_launch("mesh_area_apply");
}

// ---------------------------------------------------------------- f17: per-vertex attributes and a headlight shade over a rendered face map
// The mesh shading section of include/panst3r_hip.h, steps 9 - 12.  One lane per pixel of a face map int64 [B, H, W] (MeshRender.face, or any values): the
// pixel's face is set up again for the pixel's camera with the rasteriser's own ms_setup / ms_edges, so the weights w_k = fp64(E_k) q_k and their sum s
// are the numbers the depth was made of.  A pixel whose entry is no face of the mesh, whose face leaves no trace in that camera or does not cover the
// pixel is a MISS: `fill` in every channel, shade 0 - so the outputs are defined for any map and s is never 0.  Plain vector stores, no atomics.
namespace pst {

constexpr int MS_MAX_CHANNELS = PST_MESH_INTERP_MAX_CHANNELS;

// N = (w0 a0 + w1 a1) + w2 a2 of three fp32 values widened to fp64
__device__ __forceinline__ double ms_blend(const double (&w)[3], float a0, float a1, float a2) {
  return (w[0] * (double)a0 + w[1] * (double)a1) + w[2] * (double)a2;
}

__global__ __launch_bounds__(MS_T) void mesh_interp_kernel(const int64_t* __restrict__ face, int64_t npix, int H, int W, const float* __restrict__ vertices, int64_t Nv,
                                                           const int32_t* __restrict__ faces, int64_t Nf, const float* __restrict__ cams, float near,
                                                           const float* __restrict__ attr, int C, float fill, float* __restrict__ out_attr, int shade_mode,
                                                           const float* __restrict__ normals, float* __restrict__ out_shade) {
  const int64_t p = (int64_t)blockIdx.x * MS_T + threadIdx.x;
  if (p >= npix) return;
  const int64_t hw = (int64_t)H * W, cam = p / hw, pix = p % hw, f = face[p];
  const int i = (int)(pix / W), j = (int)(pix % W);
  const float* __restrict__ c = cams + cam * PH_CAM;
  MsTri t;
  double w[3];
  bool hit = f >= 0 && f < Nf && ms_setup(c, vertices, Nv, faces, f, near, H, W, t);
  if (hit) hit = i >= t.i0 && i <= t.i1 && j >= t.j0 && j <= t.j1;   // a covered pixel lies in the box (mesh step 4); outside it the edge values are not bounded
  if (hit) {
    int64_t E[3];
    ms_edges(t, i, j, E);
    hit = E[0] >= t.least[0] && E[1] >= t.least[1] && E[2] >= t.least[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = (double)E[k] * t.q[k];
  }
  if (!hit) {
    if (out_attr)
      for (int ch = 0; ch < C; ++ch) out_attr[p * C + ch] = fill;
    if (out_shade) out_shade[p] = 0.f;
    return;
  }
  // the vertex at set-up corner k: listed position k, 1 and 2 exchanged after a swap (ms_setup checked the three indices)
  const int64_t v0 = faces[f * 3 + 0], v1 = faces[f * 3 + (t.swapped ? 2 : 1)], v2 = faces[f * 3 + (t.swapped ? 1 : 2)];
  if (out_attr) {
    const double s = (w[0] + w[1]) + w[2];                          // the depth's own sum: E0 + E1 + E2 = A > 0 and every q_k > 0
    for (int ch = 0; ch < C; ++ch) out_attr[p * C + ch] = (float)(ms_blend(w, attr[v0 * C + ch], attr[v1 * C + ch], attr[v2 * C + ch]) / s);
  }
  if (out_shade) {
    double N[3];
    if (shade_mode == PST_MESH_SHADE_SMOOTH) {
#pragma unroll
      for (int a = 0; a < 3; ++a) N[a] = ms_blend(w, normals[v0 * 3 + a], normals[v1 * 3 + a], normals[v2 * 3 + a]);
    } else {                                                        // flat: e1 x e2 of the corners AS LISTED, as mesh_face.h writes it
      const int64_t l1 = faces[f * 3 + 1], l2 = faces[f * 3 + 2];
      double e1[3], e2[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        e1[a] = (double)vertices[l1 * 3 + a] - (double)vertices[v0 * 3 + a];
        e2[a] = (double)vertices[l2 * 3 + a] - (double)vertices[v0 * 3 + a];
      }
      N[0] = e1[1] * e2[2] - e1[2] * e2[1]; N[1] = e1[2] * e2[0] - e1[0] * e2[2]; N[2] = e1[0] * e2[1] - e1[1] * e2[0];
    }
    double n[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) n[r] = ((double)c[4 * r] * N[0] + (double)c[4 * r + 1] * N[1]) + (double)c[4 * r + 2] * N[2];
    const double d0 = (((double)j + 0.5) - (double)c[14]) / (double)c[12], d1 = (((double)i + 0.5) - (double)c[15]) / (double)c[13];
    const double dot = (n[0] * d0 + n[1] * d1) + n[2], nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dd = (d0 * d0 + d1 * d1) + 1.0;
    const double x = nn * dd;
    out_shade[p] = (x > 0.0 && x <= 1.7976931348623157e308) ? (float)(fabs(dot) / sqrt_heron(x)) : 0.f;      // zero, NaN or infinite: 0
  }
}

}  // namespace pst

extern "C" int pst_mesh_interp(const int64_t* face, int ncams, int H, int W, const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams,
                               float near_z, const float* attr, int C, float fill, float* out_attr, int shade_mode, const float* normals, float* out_shade,
                               void* stream) {
  using namespace pst;
  if (Nv <= 0 || Nv > 0x7fffffffLL || Nf <= 0 || Nf > 0x7fffffffLL || !ms_shape_ok(ncams, H, W)) {
    set_error("mesh_interp: bad shape (Nv=%lld, Nf=%lld in [1, 2^31 - 1], %d cameras in [1, 65535], %d x %d pixels, cameras x pixels < 2^31)", (long long)Nv,
              (long long)Nf, ncams, H, W);
    return PST_EINVAL;
  }
  if (!(near_z > 0.f) || !(near_z <= PST_FMAX)) { set_error("mesh_interp: needs 0 < near, finite; got %g", (double)near_z); return PST_EINVAL; }
  if (!face || !vertices || !faces || !cams) { set_error("mesh_interp: null operand"); return PST_EINVAL; }
  if ((attr != nullptr) != (out_attr != nullptr)) { set_error("mesh_interp: attr and out_attr go together"); return PST_EINVAL; }
  if (attr && (C < 1 || C > MS_MAX_CHANNELS || !(fabsf(fill) <= PST_FMAX))) {
    set_error("mesh_interp: needs 1 <= C <= %d channels and a finite fill; got %d, %g", MS_MAX_CHANNELS, C, (double)fill);
    return PST_EINVAL;
  }
  if (shade_mode != PST_MESH_SHADE_NONE && shade_mode != PST_MESH_SHADE_FLAT && shade_mode != PST_MESH_SHADE_SMOOTH) {
    set_error("mesh_interp: shade_mode is 0 (none), 1 (flat) or 2 (smooth), got %d", shade_mode);
    return PST_EINVAL;
  }
  if ((shade_mode != PST_MESH_SHADE_NONE) != (out_shade != nullptr) || (shade_mode == PST_MESH_SHADE_SMOOTH) != (normals != nullptr)) {
    set_error("mesh_interp: out_shade goes with a shade mode, normals with the smooth mode (mode %d)", shade_mode);
    return PST_EINVAL;
  }
  if (!out_attr && !out_shade) { set_error("mesh_interp: neither attributes nor a shade asked for"); return PST_EINVAL; }
  const int64_t npix = (int64_t)ncams * H * W;
  hipLaunchKernelGGL(mesh_interp_kernel, blocks_for(npix, MS_T), dim3(MS_T), 0, (hipStream_t)stream, face, npix, H, W, vertices, Nv, faces, Nf, cams, near_z, attr,
                     attr ? C : 0, fill, out_attr, shade_mode, normals, out_shade);
  return check_launch("mesh_interp");
}
