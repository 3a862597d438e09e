// The pointmap grids of a scene triangulated into one labelled surface mesh (no counterpart in the reference; the contract is the surface section of
// include/panst3r_hip.h, restated in tests/surface_ref.py, [restated, parity unpinned]).  The vertices ARE the rows of the panoptic cloud; this file
// only makes faces:
//   rows      row[p] = the cloud row of scene pixel p, -1 for a pixel the confidence filter dropped (a fill and a scatter of the cloud's index)
//   count     one thread per quad of the pixel grid, a workgroup of 256 threads takes 256 consecutive quads of one view in raster order (a device
//             table of per-view numbers makes a mixed-shape scene one launch, as in cloud.hip): the corner loads run along x, rows y and y + 1 are
//             each read by two neighbouring quads out of cache.  A quad yields up to two triangles T0, T1; two ballots per wave, one count per
//             workgroup.
//   scan      pst_cloud_scan of the workgroup counts
//   emit      the second pass RE-EVALUATES the quad (four int32 and up to four fp32 loads that the count pass left in L2, against a one-byte code per
//             quad that would have to be written and read back) and stores its triangles at
//             base[wg] + waves below + popc(m0 & lanes below) + popc(m1 & lanes below) (+ its own T0): the order is fixed by construction.
//   islands   faces that share a vertex row are one component: the wait-free union-find of union_find.h on the vertex rows (unite(v0, v1),
//             unite(v0, v2) per face; the root is the component's smallest row), the faces of every root counted with int32 atomicAdd (a sum of
//             integers: no order), and the same count / scan / emit compaction of the faces whose component is large enough.
// No atomics in rows / count / emit; integer atomics only in the islands; every result written with plain vector stores.  The only float work is
// one subtraction, one product and compares: contraction is off for the whole file all the same.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "union_find.h"
#include "wave_ops.h"            // rn_mul, rn_sub, wg_rank, last_le

#pragma clang fp contract(off)

namespace pst {

constexpr int SF_T = PST_SURFACE_WG;                               // threads = quads (or faces) per workgroup
static_assert(SF_T == 256, "four waves per workgroup");

// the view that owns quad workgroup wg: the last one whose first workgroup is <= wg (a view without quads owns none).  dims int32 [V, 4] = H, W, first_wg, 0
__device__ __forceinline__ int sf_view_of(const int32_t* __restrict__ dims, int nviews, int wg) {
  return last_le(nviews, wg, [&](int v) { return dims[v * 4 + 2]; });
}

template <typename T>
__device__ __forceinline__ T sf_sel(const T (&v)[4], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// the four triangles of a quad with corners a = 0, b = 1, c = 2, d = 3, two bits per corner: all wound towards the source camera
constexpr int SF_ACD = 0 | 2 << 2 | 3 << 4, SF_ADB = 0 | 3 << 2 | 1 << 4, SF_ACB = 0 | 2 << 2 | 1 << 4, SF_BCD = 1 | 2 << 2 | 3 << 4;

struct SfTri { int keep, v[3]; };
struct SfQuad { SfTri t[2]; int64_t quad; };

// candidate triangle `code` of the quad: kept iff zmin > 0 && zmax <= zmin * k (NaN fails, equality keeps)
__device__ __forceinline__ SfTri sf_triangle(int code, const int (&r)[4], const float (&z)[4], float k) {
  SfTri t;
  float zz[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int c = (code >> (2 * j)) & 3;
    t.v[j] = sf_sel(r, c);
    zz[j] = sf_sel(z, c);
  }
  const bool pos = zz[0] > 0.f && zz[1] > 0.f && zz[2] > 0.f;      // no NaN beyond this point
  const float zmin = fminf(fminf(zz[0], zz[1]), zz[2]), zmax = fmaxf(fmaxf(zz[0], zz[1]), zz[2]);
  t.keep = pos && zmax <= rn_mul(zmin, k);
  return t;
}

// quad `tid` of workgroup wg (contract steps 2 and 3)
__device__ __forceinline__ SfQuad sf_quad(const pst_cloud_view* __restrict__ views, const int32_t* __restrict__ dims, int nviews, int wg, int tid,
                                          const int32_t* __restrict__ row, float k) {
  SfQuad q;
  q.t[0].keep = q.t[1].keep = 0;
  q.quad = 0;
  const int v = sf_view_of(dims, nviews, wg);
  const int H = dims[v * 4], W = dims[v * 4 + 1];
  const int i = (wg - dims[v * 4 + 2]) * SF_T + tid;
  if (H < 2 || W < 2 || i >= (H - 1) * (W - 1)) return q;          // (H - 1)(W - 1) < npix < 2^31
  const int y = i / (W - 1), x = i - y * (W - 1);
  const int pa = y * W + x;
  const int px[4] = {pa, pa + 1, pa + W, pa + W + 1};              // a, b, c, d: all inside the view
  const int64_t off = views[v].offset;
  const float* __restrict__ loc = views[v].pts3d_local;
  q.quad = off + pa;
  int r[4], n = 0;
  float z[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r[c] = row[off + px[c]];
    z[c] = 0.f;
    if (r[c] >= 0) { z[c] = loc[(int64_t)px[c] * 3 + 2]; ++n; }
  }
  if (n == 4) {
    const bool bc = fabsf(rn_sub(z[1], z[2])) < fabsf(rn_sub(z[0], z[3]));      // a tie or a NaN: diagonal a-d
    q.t[0] = sf_triangle(bc ? SF_ACB : SF_ACD, r, z, k);
    q.t[1] = sf_triangle(bc ? SF_BCD : SF_ADB, r, z, k);
  } else if (n == 3) {
    const int code = r[3] < 0 ? SF_ACB : r[0] < 0 ? SF_BCD : r[1] < 0 ? SF_ACD : SF_ADB;
    q.t[0] = sf_triangle(code, r, z, k);
  }
  return q;
}

__global__ __launch_bounds__(SF_T) void surface_fill_kernel(int32_t* __restrict__ row, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * SF_T + threadIdx.x;
  if (i < n) row[i] = -1;
}

__global__ __launch_bounds__(SF_T) void surface_rows_kernel(const int64_t* __restrict__ index, int M, int64_t N, int32_t* __restrict__ row) {
  const int i = blockIdx.x * SF_T + threadIdx.x;
  if (i >= M) return;
  const int64_t p = index[i];
  if (p >= 0 && p < N) row[p] = i;                                  // the cloud's indices are distinct: one writer per entry
}

__global__ __launch_bounds__(SF_T) void surface_count_kernel(const pst_cloud_view* __restrict__ views, const int32_t* __restrict__ dims, int nviews,
                                                             const int32_t* __restrict__ row, float k, int32_t* __restrict__ counts) {
  __shared__ int wtot[SF_T / 64];
  const SfQuad q = sf_quad(views, dims, nviews, blockIdx.x, threadIdx.x, row, k);
  int total;
  wg_rank<SF_T, 2>(q.t[0].keep | q.t[1].keep << 1, wtot, total);   // two items per lane: T0, then T1
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__device__ __forceinline__ int sf_face_id(int a, int b, int c) { return (a == b || a == c) ? a : (b == c ? b : 0); }

__global__ __launch_bounds__(SF_T) void surface_emit_kernel(const pst_cloud_view* __restrict__ views, const int32_t* __restrict__ dims, int nviews,
                                                            const int32_t* __restrict__ row, float k, const int32_t* __restrict__ vertex_ids,
                                                            const int32_t* __restrict__ base, int32_t* __restrict__ faces, int32_t* __restrict__ face_ids,
                                                            int64_t* __restrict__ quad) {
  __shared__ int wtot[SF_T / 64];
  const int64_t b0 = base[blockIdx.x];
  if (base[blockIdx.x + 1] == (int)b0) return;                      // uniform: nothing to write
  const SfQuad q = sf_quad(views, dims, nviews, blockIdx.x, threadIdx.x, row, k);
  int total;
  int64_t s = b0 + wg_rank<SF_T, 2>(q.t[0].keep | q.t[1].keep << 1, wtot, total);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (q.t[j].keep) {
      const int a = q.t[j].v[0], b = q.t[j].v[1], c = q.t[j].v[2];
      faces[s * 3] = a; faces[s * 3 + 1] = b; faces[s * 3 + 2] = c;
      face_ids[s] = sf_face_id(vertex_ids[a], vertex_ids[b], vertex_ids[c]);
      quad[s] = q.quad;
      ++s;
    }
}

// ---------------------------------------------------------------- islands
__global__ __launch_bounds__(SF_T) void surface_parent_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ size, int M) {
  const int v = blockIdx.x * SF_T + threadIdx.x;
  if (v < M) { parent[v] = v; size[v] = 0; }
}

__global__ __launch_bounds__(SF_T) void surface_link_kernel(const int32_t* __restrict__ faces, int F, int M, int32_t* __restrict__ parent,
                                                            int32_t* __restrict__ status) {
  const int f = blockIdx.x * SF_T + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
  if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M || (unsigned)c >= (unsigned)M) { atomicOr(status, PST_VCC_RANGE); return; }
  cc_unite(parent, a, b, M, status);
  cc_unite(parent, a, c, M, status);
}

// component[f] = the root of the face's first vertex (the links are final: plain loads, nothing written to parent), one count per face on its root.
// A face with ANY corner outside the rows was joined to nothing by the link: it belongs to no component and is counted on none.
__global__ __launch_bounds__(SF_T) void surface_root_kernel(const int32_t* __restrict__ faces, int F, int M, const int32_t* __restrict__ parent,
                                                            int32_t* __restrict__ component, int32_t* __restrict__ size, int32_t* __restrict__ status) {
  const int f = blockIdx.x * SF_T + threadIdx.x;
  if (f >= F) return;
  int x = faces[(int64_t)f * 3];
  const int b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
  if ((unsigned)x >= (unsigned)M || (unsigned)b >= (unsigned)M || (unsigned)c >= (unsigned)M) { atomicOr(status, PST_VCC_RANGE); component[f] = -1; return; }
  int r = parent[x], it = 0;
  for (; it < M && r != x; ++it) { x = r; r = parent[x]; }
  if (r != x) { atomicOr(status, PST_VCC_LOOP); component[f] = -1; return; }
  component[f] = r;
  atomicAdd(&size[r], 1);
}

__device__ __forceinline__ int sf_survives(const int32_t* __restrict__ component, const int32_t* __restrict__ size, int F, int min_faces, int f) {
  if (f >= F) return 0;
  const int r = component[f];
  return r >= 0 && size[r] >= min_faces;
}

__global__ __launch_bounds__(SF_T) void surface_keep_count_kernel(const int32_t* __restrict__ component, const int32_t* __restrict__ size, int F, int min_faces,
                                                                  int32_t* __restrict__ counts) {
  __shared__ int wtot[SF_T / 64];
  int total;
  wg_rank<SF_T, 1>(sf_survives(component, size, F, min_faces, blockIdx.x * SF_T + threadIdx.x), wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(SF_T) void surface_keep_emit_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ face_ids,
                                                                 const int64_t* __restrict__ quad, const int32_t* __restrict__ component,
                                                                 const int32_t* __restrict__ size, int F, int min_faces, const int32_t* __restrict__ base,
                                                                 int32_t* __restrict__ out_faces, int32_t* __restrict__ out_face_ids, int64_t* __restrict__ out_quad) {
  __shared__ int wtot[SF_T / 64];
  const int f = blockIdx.x * SF_T + threadIdx.x;
  const int keep = sf_survives(component, size, F, min_faces, f);
  int total;
  const int64_t s = (int64_t)base[blockIdx.x] + wg_rank<SF_T, 1>(keep, wtot, total);
  if (!keep) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) out_faces[s * 3 + j] = faces[(int64_t)f * 3 + j];
  out_face_ids[s] = face_ids[f];
  out_quad[s] = quad[f];
}

constexpr int64_t SF_MAX_PIXELS = 1ll << 30, SF_MAX_FACES = 0x7fffff00ll;       // (a grid of 256-thread workgroups over F faces stays inside int32)
static bool sf_faces_ok(int64_t F, int64_t M) { return F > 0 && F <= SF_MAX_FACES && M > 0 && M <= SF_MAX_PIXELS; }

}  // namespace pst

extern "C" int pst_surface_rows(const int64_t* index, int64_t M, int64_t N, int32_t* row, void* stream) {
  using namespace pst;
  if (!row || N <= 0 || N > SF_MAX_PIXELS || M < 0 || M > N || (M > 0 && !index)) {
    set_error("surface_rows: bad shape (M=%lld, N=%lld: at most 2^30 pixels) or null operand", (long long)M, (long long)N); return PST_EINVAL;
  }
  hipLaunchKernelGGL(surface_fill_kernel, blocks_for(N, SF_T), dim3(SF_T), 0, (hipStream_t)stream, row, N);
  const int rc = check_launch("surface_rows (fill)");
  if (rc || M == 0) return rc;
  hipLaunchKernelGGL(surface_rows_kernel, blocks_for(M, SF_T), dim3(SF_T), 0, (hipStream_t)stream, index, (int)M, N, row);
  return check_launch("surface_rows");
}

static int surface_quads_ok(const char* what, const void* views, const void* dims, int nviews, int nwg, const void* row, float k) {
  using namespace pst;
  if (!views || !dims || !row || nviews <= 0 || nwg <= 0 || !(k >= 1.f)) {
    set_error("%s: bad shape (nviews=%d, nwg=%d), ratio bound %g (k >= 1) or null operand", what, nviews, nwg, (double)k); return PST_EINVAL;
  }
  return 0;
}

extern "C" int pst_surface_count(const pst_cloud_view* views, const int32_t* dims, int nviews, int nwg, const int32_t* row, float k, int32_t* counts, void* stream) {
  using namespace pst;
  if (surface_quads_ok("surface_count", views, dims, nviews, nwg, row, k)) return PST_EINVAL;
  if (!counts) { set_error("surface_count: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(surface_count_kernel, dim3((unsigned)nwg), dim3(SF_T), 0, (hipStream_t)stream, views, dims, nviews, row, k, counts);
  return check_launch("surface_count");
}

extern "C" int pst_surface_emit(const pst_cloud_view* views, const int32_t* dims, int nviews, int nwg, const int32_t* row, float k, const int32_t* vertex_ids,
                                const int32_t* base, int32_t* faces, int32_t* face_ids, int64_t* quad, void* stream) {
  using namespace pst;
  if (surface_quads_ok("surface_emit", views, dims, nviews, nwg, row, k)) return PST_EINVAL;
  if (!vertex_ids || !base || !faces || !face_ids || !quad) { set_error("surface_emit: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(surface_emit_kernel, dim3((unsigned)nwg), dim3(SF_T), 0, (hipStream_t)stream, views, dims, nviews, row, k, vertex_ids, base, faces, face_ids,
                     quad);
  return check_launch("surface_emit");
}

extern "C" int pst_surface_link(const int32_t* faces, int64_t F, int64_t M, int32_t* parent, int32_t* size, int32_t* status, void* stream) {
  using namespace pst;
  if (!faces || !parent || !size || !status || !sf_faces_ok(F, M)) {
    set_error("surface_link: bad shape (F=%lld, M=%lld) or null operand", (long long)F, (long long)M); return PST_EINVAL;
  }
  hipLaunchKernelGGL(surface_parent_kernel, blocks_for(M, SF_T), dim3(SF_T), 0, (hipStream_t)stream, parent, size, (int)M);
  const int rc = check_launch("surface_link (parent)");
  if (rc) return rc;
  hipLaunchKernelGGL(surface_link_kernel, blocks_for(F, SF_T), dim3(SF_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, parent, status);
  return check_launch("surface_link");
}

extern "C" int pst_surface_components(const int32_t* faces, int64_t F, int64_t M, const int32_t* parent, int32_t* component, int32_t* size, int32_t* status,
                                      void* stream) {
  using namespace pst;
  if (!faces || !parent || !component || !size || !status || !sf_faces_ok(F, M)) {
    set_error("surface_components: bad shape (F=%lld, M=%lld) or null operand", (long long)F, (long long)M); return PST_EINVAL;
  }
  hipLaunchKernelGGL(surface_root_kernel, blocks_for(F, SF_T), dim3(SF_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, parent, component, size, status);
  return check_launch("surface_components");
}

extern "C" int pst_surface_keep_count(const int32_t* component, const int32_t* size, int64_t F, int min_faces, int32_t* counts, void* stream) {
  using namespace pst;
  if (!component || !size || !counts || F <= 0 || F > SF_MAX_FACES || min_faces < 1) {
    set_error("surface_keep_count: bad shape (F=%lld), min_faces %d or null operand", (long long)F, min_faces); return PST_EINVAL;
  }
  hipLaunchKernelGGL(surface_keep_count_kernel, blocks_for(F, SF_T), dim3(SF_T), 0, (hipStream_t)stream, component, size, (int)F, min_faces, counts);
  return check_launch("surface_keep_count");
}

extern "C" int pst_surface_keep_emit(const int32_t* faces, const int32_t* face_ids, const int64_t* quad, const int32_t* component, const int32_t* size, int64_t F,
                                     int min_faces, const int32_t* base, int32_t* out_faces, int32_t* out_face_ids, int64_t* out_quad, void* stream) {
  using namespace pst;
  if (!faces || !face_ids || !quad || !component || !size || !base || !out_faces || !out_face_ids || !out_quad || F <= 0 || F > SF_MAX_FACES ||
      min_faces < 1) {
    set_error("surface_keep_emit: bad shape (F=%lld), min_faces %d or null operand", (long long)F, min_faces); return PST_EINVAL;
  }
  hipLaunchKernelGGL(surface_keep_emit_kernel, blocks_for(F, SF_T), dim3(SF_T), 0, (hipStream_t)stream, faces, face_ids, quad, component, size, (int)F, min_faces, base,
                     out_faces, out_face_ids, out_quad);
  return check_launch("surface_keep_emit");
}
