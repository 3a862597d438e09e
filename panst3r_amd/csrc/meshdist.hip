// The exact distance from a point to a triangle mesh within a radius (engine/meshdist.py; no counterpart in the reference; the contract is the meshdist
// section of include/panst3r_hip.h, restated in tests/meshdist_ref.py, [restated, parity unpinned]):
//   count    one lane per face: the face's cell box (its fp32 bounding box in cells of edge `radius`, dilated by one cell), the number of its cells into
//            counts, dropped faces counted, the total added up in int64 (one integer atomic per wave)
//   scan     pst_cloud_scan of the per-face counts
//   insert   one lane per (face, cell) pair: its face by binary search in the prefix, its cell from the pair's local index -> key -> slot of the
//            open-addressing table, one int32 atomicAdd on the slot's count
//            (offsets: a prefix sum of the slot counts, made by the caller)
//   scatter  the pair's face into its cell's list (the position inside the list depends on arrival; nothing that leaves depends on it)
//   query    one lane per query: the list of the query's OWN cell, every candidate's closest point in fp64 (Ericson's region sequence), the minimum of
//            (bits(float32 d2) << 32) | face, the winner's closest point once more for the output
//   plane    one fused point-to-plane ICP step (the icp-plane section of the header, restated in tests/icp_plane_ref.py): a block per PST_ICP_CHUNK
//            source rows, 16 rows per lane: the row moved by the 3 x 4 matrix in fp32, the query's list walk (the same __device__ function), then the
//            winner's plane terms once - the unnormalised normal, its weight 1 / |N|^2, the seven derivatives - and the 38 live moments of the
//            normal equations in fp64 registers; the fixed order of the sums and the reducer are icp_sum.h, shared with icp_step of csrc/nearest.hip
// Which faces are kept and the search in the prefix are mesh_face.h, shared with the surface sampler of csrc/nearest.hip; the cell of a query, the
// key, the table's probes and the per-cell lists are voxel_table.h, shared by every hash-grid stage.
// Integer atomics only, every probe / candidate / search loop bounded by a number known before the launch, refusals through the status words, every
// result written with plain vector stores, no float atomics: two calls return identical bytes.  Contraction is off for the whole file: every fp32 and fp64 operation is
// rounded on its own, in the order written.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // and through it wave_ops.h: wave_count_add, wave_sum
#include "mesh_face.h"
#include "icp_sum.h"

#pragma clang fp contract(off)

namespace pst {

constexpr int MD_T = 256;
constexpr int64_t MD_MAX = 1ll << 30;                                // queries, faces and pairs of one call
constexpr int64_t MD_FACE_CAP = PST_MESHDIST_FACE_CAP;               // a face's count saturates here: one such face is beyond every legal total

// ---------------------------------------------------------------- the cell box of a face, its pairs
// the cell box [lo, lo + ext) of a loaded face: cell(min corner) - 1 .. cell(max corner) + 1 per axis; false if a cell of it leaves (-2^20, 2^20)
__device__ __forceinline__ bool md_box(const MeshFace& t, float inv, int (&lo)[3], int (&ext)[3]) {
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float mn = fminf(fminf(t.v[0][a], t.v[1][a]), t.v[2][a]), mx = fmaxf(fmaxf(t.v[0][a], t.v[1][a]), t.v[2][a]);
    const float cl = floorf(mn * inv) - 1.f, ch = floorf(mx * inv) + 1.f;      // whole numbers below 2^24, or far beyond the range
    in = in && cl > -(float)VX_LIM && ch < (float)VX_LIM;
    lo[a] = in ? (int)cl : 0;
    ext[a] = in ? (int)ch - (int)cl + 1 : 0;
  }
  return in;
}

// the number of (face, cell) pairs of face f, 0 = dropped, saturated at MD_FACE_CAP
__device__ __forceinline__ int64_t md_pairs(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int f, float inv, int (&lo)[3],
                                            int (&ext)[3]) {
  const MeshFace t = mf_load(vertices, Nv, faces, f);
  if (!t.ok || !mf_has_area(t) || !md_box(t, inv, lo, ext)) return 0;
  const int64_t n = (int64_t)ext[0] * ext[1] * ext[2];                // three factors below 2^21
  return n < MD_FACE_CAP ? n : MD_FACE_CAP;
}

__global__ __launch_bounds__(MD_T) void meshdist_count_kernel(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int F, float inv,
                                                              int32_t* __restrict__ counts, int64_t* __restrict__ total, int32_t* __restrict__ status) {
  const int f = blockIdx.x * MD_T + threadIdx.x;
  int64_t c = 0;
  int dropped = 0;
  if (f < F) {
    int lo[3], ext[3];
    c = md_pairs(vertices, Nv, faces, f, inv, lo, ext);
    dropped = c == 0;
    counts[f] = (int)c;
  }
  const long long sum = wave_sum(c);                                 // 64 faces of at most 2^31 - 1 pairs
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd((unsigned long long*)total, (unsigned long long)sum);
  wave_count_add(dropped, &status[1]);
}

__global__ __launch_bounds__(MD_T) void meshdist_insert_kernel(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int F, float inv,
                                                               const int32_t* __restrict__ prefix, int P, uint64_t* __restrict__ keys, uint32_t mask,
                                                               int32_t* __restrict__ cell_count, int32_t* __restrict__ pair_slot,
                                                               int32_t* __restrict__ status) {
  if (prefix[F] != P) {                                             // uniform: the prefix is not the one the caller sized the workspaces by
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[0], PST_MESHDIST_TOTAL);
    return;
  }
  const int p = blockIdx.x * MD_T + threadIdx.x;
  if (p >= P) return;
  const int f = mf_prefix_owner(prefix, F, p), t = p - prefix[f], cnt = prefix[f + 1] - prefix[f];
  int lo[3], ext[3];
  int slot = -1;
  if (md_pairs(vertices, Nv, faces, f, inv, lo, ext) != (int64_t)cnt || t < 0 || t >= cnt) atomicOr(&status[0], PST_MESHDIST_LISTS);      // not this mesh's prefix
  else {
    const int x = lo[0] + t % ext[0], y = lo[1] + (t / ext[0]) % ext[1], z = lo[2] + t / (ext[0] * ext[1]);      // ext0 ext1 <= cnt: inside int32
    slot = vx_find_or_claim(keys, mask, vx_key(x, y, z), status);
    if (slot >= 0) atomicAdd(&cell_count[slot], 1);
  }
  pair_slot[p] = slot;
}

// the pair's face into its cell's list; status[2] = the longest list
__global__ __launch_bounds__(MD_T) void meshdist_scatter_kernel(const int32_t* __restrict__ pair_slot, const int32_t* __restrict__ prefix, int F, int P,
                                                                const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count,
                                                                int32_t* __restrict__ fill, int32_t* __restrict__ rows, int32_t* __restrict__ status) {
  if (prefix[F] != P) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[0], PST_MESHDIST_TOTAL);
    return;
  }
  const int p = blockIdx.x * MD_T + threadIdx.x;
  if (p >= P) return;
  const int slot = pair_slot[p];
  if (slot < 0) return;
  vx_list_place(slot, start, cell_count, fill, P, rows, status, [&] { return mf_prefix_owner(prefix, F, p); });
}

// ---------------------------------------------------------------- the closest point of a triangle, in fp64, in the order the header writes out
__device__ __forceinline__ double md_dot(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ __forceinline__ double md_clamp(double t) { return t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0; }      // NaN -> 0

// -> the squared distance; cp = the closest point; the corners and the query widened once by the caller
__device__ __forceinline__ double md_closest(const double (&a)[3], const double (&b)[3], const double (&c)[3], const double (&q)[3], double (&cp)[3]) {
  double ab[3], ac[3], ap[3], bp[3], cq[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = q[k] - a[k]; bp[k] = q[k] - b[k]; cq[k] = q[k] - c[k]; }
  const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap), d3 = md_dot(ab, bp), d4 = md_dot(ac, bp), d5 = md_dot(ab, cq), d6 = md_dot(ac, cq);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0 && d2 <= 0.0) {                                      // A
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = a[k];
  } else if (d3 >= 0.0 && d4 <= d3) {                                // B
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = b[k];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                  // AB
    const double t = md_clamp(d1 / (d1 - d3));
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = a[k] + t * ab[k];
  } else if (d6 >= 0.0 && d5 <= d6) {                                // C
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = c[k];
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                  // AC
    const double t = md_clamp(d2 / (d2 - d6));
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = a[k] + t * ac[k];
  } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {        // BC
    const double t = md_clamp((d4 - d3) / ((d4 - d3) + (d5 - d6)));
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = b[k] + t * (c[k] - b[k]);
  } else {                                                           // the interior
    const double den = 1.0 / ((va + vb) + vc), v = md_clamp(vb * den), w = md_clamp(vc * den);
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = (a[k] + v * ab[k]) + w * ac[k];
  }
  const double dx = q[0] - cp[0], dy = q[1] - cp[1], dz = q[2] - cp[2];
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double md_face_distance(const MeshFace& t, const double (&q)[3], double (&cp)[3]) {
  double a[3], b[3], c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = (double)t.v[0][k]; b[k] = (double)t.v[1][k]; c[k] = (double)t.v[2][k]; }
  return md_closest(a, b, c, q, cp);
}

// step 6 of the contract for one lane, shared by meshdist_query and icp_plane_step: every face of the list of the cell c of the point q (ok = q is
// finite and c in range) -> the minimum of (bits(fp32 D2) << 32) | face, all ones without a candidate.  Nothing here is collective: lanes may
// call it divergently.
__device__ __forceinline__ uint64_t md_search(const double (&q)[3], const float (&c)[3], bool ok, const float* __restrict__ vertices, int Nv,
                                              const int32_t* __restrict__ faces, int F, const uint64_t* __restrict__ keys, uint32_t mask,
                                              const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count, const int32_t* __restrict__ rows,
                                              int P, int max_cell_faces, int32_t* __restrict__ status) {
  uint64_t best = ~0ull;
  if (!ok) return best;                                              // a query outside the range has no cell of a kept face
  const int slot = vx_find(keys, mask, vx_key((int)c[0], (int)c[1], (int)c[2]), status);
  int b, cnt;
  if (slot >= 0 && vx_list_range(slot, start, cell_count, P, max_cell_faces, status, b, cnt))
    for (int j = 0; j < cnt; ++j) {
      const int f = rows[b + j];
      if ((unsigned)f >= (unsigned)F) { atomicOr(&status[0], PST_MESHDIST_LISTS); continue; }
      const MeshFace t = mf_load(vertices, Nv, faces, f);
      if (!t.ok) { atomicOr(&status[0], PST_MESHDIST_LISTS); continue; }       // a listed face was kept by the build
      double cp[3];
      const float d2 = (float)md_face_distance(t, q, cp);         // >= +0, never NaN: its bits order as an unsigned integer
      const uint64_t cand = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)f;
      best = cand < best ? cand : best;
    }
  return best;
}

__global__ __launch_bounds__(MD_T) void meshdist_query_kernel(const float* __restrict__ queries, int Nq, const float* __restrict__ vertices, int Nv,
                                                              const int32_t* __restrict__ faces, int F, float inv, float r2,
                                                              const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ start,
                                                              const int32_t* __restrict__ cell_count, const int32_t* __restrict__ rows, int P,
                                                              int max_cell_faces, float* __restrict__ d2_out, int32_t* __restrict__ face_out,
                                                              float* __restrict__ closest, int32_t* __restrict__ status) {
  const int i = blockIdx.x * MD_T + threadIdx.x;
  const bool in = i < Nq;
  float x[3] = {0.f, 0.f, 0.f}, c[3];
  bool finite = true, ok = true;
  if (in) {
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = queries[(int64_t)i * 3 + a];
    vx_cell_of(x, inv, c, finite, ok);
  }
  wave_count_add(in && !finite, &status[3]);
  if (!in) return;
  const double q[3] = {(double)x[0], (double)x[1], (double)x[2]};
  const uint64_t best = md_search(q, c, ok, vertices, Nv, faces, F, keys, mask, start, cell_count, rows, P, max_cell_faces, status);
  const float d2 = __uint_as_float((uint32_t)(best >> 32));
  const bool hit = best != ~0ull && d2 <= r2;
  d2_out[i] = hit ? d2 : __uint_as_float(0x7f800000u);
  face_out[i] = hit ? (int)(uint32_t)best : -1;
  if (closest) {
    float out[3] = {x[0], x[1], x[2]};                               // without a hit: the query itself
    if (hit) {
      double cp[3];
      md_face_distance(mf_load(vertices, Nv, faces, (int)(uint32_t)best), q, cp);
#pragma unroll
      for (int a = 0; a < 3; ++a) out[a] = (float)cp[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) closest[(int64_t)i * 3 + a] = out[a];
  }
}

// ---------------------------------------------------------------- one fused point-to-plane ICP step (the icp-plane section of include/panst3r_hip.h)
constexpr int PL_LIVE = 38;                                          // the moments that are sums; [38], [39] are +0.0
static_assert(MD_T == ICP_T && PL_LIVE + 2 == PST_ICP_PLANE_MOMENTS, "the fixed order of the header (icp_sum.h)");

struct PlaneCentre { float c[3]; };

// step 3 of the section: the terms of one matched source into the lane's accumulators.  a, b, c the winner's corners, m the moved point, c0 the
// centre, all widened once; every product and sum below is rounded on its own, in the order written.
__device__ __forceinline__ void pl_accumulate(const MeshFace& t, const float (&mf)[3], const PlaneCentre& C, float d2, double (&acc)[PL_LIVE]) {
  double e1[3], e2[3], p[3], u[3], J[7];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = (double)t.v[0][k], m = (double)mf[k];
    e1[k] = (double)t.v[1][k] - a;
    e2[k] = (double)t.v[2][k] - a;
    p[k] = m - (double)C.c[k];
    u[k] = m - a;
  }
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};      // as mf_has_area writes them
  const double w = 1.0 / ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);                                                      // a kept face: n != 0
  const double rN = md_dot(n, u);
  J[0] = p[1] * n[2] - p[2] * n[1];
  J[1] = p[2] * n[0] - p[0] * n[2];
  J[2] = p[0] * n[1] - p[1] * n[0];
  J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
  J[6] = md_dot(n, p);
  acc[0] += 1.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const double g = w * J[i];
#pragma unroll
    for (int j = i; j < 7; ++j) acc[1 + 7 * i - i * (i - 1) / 2 + (j - i)] += g * J[j];      // the upper triangle, row-major: [1, 29)
    acc[29 + i] += g * rN;
  }
  acc[36] += (w * rN) * rN;
  acc[37] += (double)d2;
}

__global__ __launch_bounds__(MD_T) void icp_plane_step_kernel(const float* __restrict__ source, int N, IcpMatrix A, PlaneCentre C,
                                                              const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int F,
                                                              float inv, float r2, const uint64_t* __restrict__ keys, uint32_t mask,
                                                              const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count,
                                                              const int32_t* __restrict__ rows, int P, int max_cell_faces, float* __restrict__ d2_out,
                                                              int32_t* __restrict__ face_out, double* __restrict__ partials, int32_t* __restrict__ status) {
  const int first = blockIdx.x * PST_ICP_CHUNK + threadIdx.x;        // N <= 2^30: no row leaves int32
  double acc[PL_LIVE];
#pragma unroll
  for (int s = 0; s < PL_LIVE; ++s) acc[s] = 0.0;
  int bad = 0;
  for (int j = 0; j < ICP_ROWS; ++j) {                               // (per lane: nothing collective inside)
    const int i = first + MD_T * j;
    if (i >= N) break;
    float x[3], m[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = source[(int64_t)i * 3 + a];
    affine34(&A.a[0][0], x, m);
    bool finite, ok;
    vx_cell_of(m, inv, c, finite, ok);
    bad += !finite;
    const double q[3] = {(double)m[0], (double)m[1], (double)m[2]};
    const uint64_t best = md_search(q, c, ok, vertices, Nv, faces, F, keys, mask, start, cell_count, rows, P, max_cell_faces, status);
    const float d2 = __uint_as_float((uint32_t)(best >> 32));
    const bool hit = best != ~0ull && d2 <= r2;
    if (d2_out) {
      d2_out[i] = hit ? d2 : __uint_as_float(0x7f800000u);
      face_out[i] = hit ? (int)(uint32_t)best : -1;
    }
    if (!hit) continue;
    pl_accumulate(mf_load(vertices, Nv, faces, (int)(uint32_t)best), m, C, d2, acc);      // (the walk took the face from rows and checked it)
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) bad += __shfl_xor(bad, k);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&status[3], bad);
  icp_block_sum<PL_LIVE, PST_ICP_PLANE_MOMENTS>(acc, partials + (int64_t)blockIdx.x * PST_ICP_PLANE_MOMENTS);
}

static int md_mesh_ok(const char* what, const void* vertices, const void* faces, int64_t Nv, int64_t F, float inv) {
  if (!vertices || !faces || Nv <= 0 || Nv > 0x7fffffffll || F <= 0 || F > MD_MAX || !(inv > 0.f) || !(inv <= PST_FMAX)) {
    set_error("%s: bad shape (Nv=%lld, F=%lld: 1 .. 2^30 faces), inverse radius %g (positive, finite) or null mesh", what, (long long)Nv, (long long)F,
              (double)inv);
    return PST_EINVAL;
  }
  return 0;
}

}  // namespace pst

extern "C" int pst_meshdist_count(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, int32_t* counts, int64_t* total,
                                  int32_t* status, void* stream) {
  using namespace pst;
  if (md_mesh_ok("meshdist_count", vertices, faces, Nv, F, inv)) return PST_EINVAL;
  if (!counts || !total || !status) { set_error("meshdist_count: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(meshdist_count_kernel, blocks_for(F, MD_T), dim3(MD_T), 0, (hipStream_t)stream, vertices, (int)Nv, faces, (int)F, inv, counts, total, status);
  return check_launch("meshdist_count");
}

extern "C" int pst_meshdist_insert(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, const int32_t* prefix, int64_t total,
                                   uint64_t* keys, int64_t capacity, int32_t* cell_count, int32_t* pair_slot, int32_t* status, void* stream) {
  using namespace pst;
  if (md_mesh_ok("meshdist_insert", vertices, faces, Nv, F, inv) || vx_table_ok("meshdist_insert", total, MD_MAX, capacity, "total", "1 .. 2^30 pairs")) return PST_EINVAL;
  if (!prefix || !keys || !cell_count || !pair_slot || !status) { set_error("meshdist_insert: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(meshdist_insert_kernel, blocks_for(total, MD_T), dim3(MD_T), 0, (hipStream_t)stream, vertices, (int)Nv, faces, (int)F, inv, prefix, (int)total,
                     keys, (uint32_t)(capacity - 1), cell_count, pair_slot, status);
  return check_launch("meshdist_insert");
}

extern "C" int pst_meshdist_scatter(const int32_t* pair_slot, const int32_t* prefix, int64_t F, int64_t total, const int32_t* start,
                                    const int32_t* cell_count, int32_t* fill, int32_t* rows, int32_t* status, void* stream) {
  using namespace pst;
  if (!pair_slot || !prefix || !start || !cell_count || !fill || !rows || !status || F <= 0 || F > MD_MAX || total <= 0 || total > MD_MAX) {
    set_error("meshdist_scatter: bad shape (F=%lld, total=%lld: 1 .. 2^30) or null operand", (long long)F, (long long)total); return PST_EINVAL;
  }
  hipLaunchKernelGGL(meshdist_scatter_kernel, blocks_for(total, MD_T), dim3(MD_T), 0, (hipStream_t)stream, pair_slot, prefix, (int)F, (int)total, start, cell_count,
                     fill, rows, status);
  return check_launch("meshdist_scatter");
}

extern "C" int pst_meshdist_query(const float* queries, int64_t Nq, const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, float r2,
                                  const uint64_t* keys, int64_t capacity, const int32_t* start, const int32_t* cell_count, const int32_t* rows,
                                  int64_t total, int max_cell_faces, float* d2, int32_t* face, float* closest, int32_t* status, void* stream) {
  using namespace pst;
  if (md_mesh_ok("meshdist_query", vertices, faces, Nv, F, inv) || vx_table_ok("meshdist_query", total, MD_MAX, capacity, "total", "1 .. 2^30 pairs")) return PST_EINVAL;
  if (!queries || !keys || !start || !cell_count || !rows || !d2 || !face || !status || Nq <= 0 || Nq > MD_MAX || !(r2 >= 0.f) ||
      !(r2 <= PST_FMAX) || max_cell_faces < 1) {
    set_error("meshdist_query: bad shape (Nq=%lld: 1 .. 2^30 queries), squared radius %g (finite), max_cell_faces %d (>= 1) or null operand",
              (long long)Nq, (double)r2, max_cell_faces);
    return PST_EINVAL;
  }
  hipLaunchKernelGGL(meshdist_query_kernel, blocks_for(Nq, MD_T), dim3(MD_T), 0, (hipStream_t)stream, queries, (int)Nq, vertices, (int)Nv, faces, (int)F, inv, r2, keys,
                     (uint32_t)(capacity - 1), start, cell_count, rows, (int)total, max_cell_faces, d2, face, closest, status);
  return check_launch("meshdist_query");
}

extern "C" int pst_plane_icp_step(const float* source, int64_t N, float a00, float a01, float a02, float a03, float a10, float a11, float a12, float a13,
                                  float a20, float a21, float a22, float a23, float c0x, float c0y, float c0z, const float* vertices, int64_t Nv,
                                  const int32_t* faces, int64_t F, float inv, float r2, const uint64_t* keys, int64_t capacity, const int32_t* start,
                                  const int32_t* cell_count, const int32_t* rows, int64_t total, int max_cell_faces, float* d2, int32_t* face,
                                  double* partials, double* out, int32_t* status, void* stream) {
  using namespace pst;
  if (md_mesh_ok("plane_icp_step", vertices, faces, Nv, F, inv) || vx_table_ok("plane_icp_step", total, MD_MAX, capacity, "total", "1 .. 2^30 pairs")) return PST_EINVAL;
  if (!source || !keys || !start || !cell_count || !rows || !partials || !out || !status || (d2 == nullptr) != (face == nullptr) || N < 1 || N > MD_MAX ||
      !(r2 >= 0.f) || !(r2 <= PST_FMAX) || !(fabsf(c0x) <= PST_FMAX) || !(fabsf(c0y) <= PST_FMAX) || !(fabsf(c0z) <= PST_FMAX) || max_cell_faces < 1) {
    set_error("plane_icp_step: bad shape (N=%lld: 1 .. 2^30 source points), squared radius %g (finite), centre (%g, %g, %g) (finite), max_cell_faces %d "
              "(>= 1), one of d2 / face without the other, or null operand", (long long)N, (double)r2, (double)c0x, (double)c0y, (double)c0z, max_cell_faces);
    return PST_EINVAL;
  }
  const IcpMatrix A = {{{a00, a01, a02, a03}, {a10, a11, a12, a13}, {a20, a21, a22, a23}}};
  const PlaneCentre C = {{c0x, c0y, c0z}};
  const int P = (int)((N + PST_ICP_CHUNK - 1) / PST_ICP_CHUNK);
  hipLaunchKernelGGL(icp_plane_step_kernel, dim3((unsigned)P), dim3(MD_T), 0, (hipStream_t)stream, source, (int)N, A, C, vertices, (int)Nv, faces, (int)F, inv,
                     r2, keys, (uint32_t)(capacity - 1), start, cell_count, rows, (int)total, max_cell_faces, d2, face, partials, status);
  if (int rc = check_launch("plane_icp_step")) return rc;
  hipLaunchKernelGGL((icp_reduce_kernel<PL_LIVE, PST_ICP_PLANE_MOMENTS>), dim3(1), dim3(MD_T), 0, (hipStream_t)stream, (const double*)partials, P, out);
  return check_launch("plane_icp_step (reduce)");
}
