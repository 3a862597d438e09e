// One fused surface out of all views (stage f15; no counterpart in the reference): a truncated signed distance averaged over the views on the lattice
// nodes around the occupied voxels, free space carved by the views that see through it, and ONE sheet extracted by naive surface nets (no case
// table).  Restated in tests/tsdf_ref.py [restated, parity unpinned]; the kernels are held to it bit for bit.  The contract is the tsdf section of
// include/panst3r_hip.h.  Seven kernels over the integer cells of a VoxelCloud and the cloud's own pst_cloud_view table:
//   insert     one lane per (voxel row, offset) pair: the node's key into an open-addressing table (voxel_table.h), atomicMin of the pair index into
//              the slot.  The CANONICAL ORDER of the nodes is the order of their smallest pair index: pst_voxel_count / pst_cloud_scan /
//              pst_voxel_rank of csrc/voxel.hip turn `first` into ranks (a pair is a point there, a node a voxel): nothing that leaves the stage
//              depends on arrival order.
//   nodes      per rank the node's coordinates; per voxel the rank of the node at its cell: voxel_row.
//   integrate  THE HOT KERNEL.  One lane per node in rank order, four nodes per thread (as consistency.hip's CS_PT: four gathers in flight), a loop
//              over the views that is uniform over the workgroup: camera, dims and plane base of the view come from scalar loads, and the only
//              vector memory traffic in the loop is the gather of the view's depth.  Per (node, view) about 20 separately rounded fp32 operations,
//              two IEEE quotients and one 4-byte gather whose lanes land on neighbouring pixels: the same bound as consist_count (the expectation,
//              the measured times are in docs/experiments.md §6t).  No atomics, plain vector stores.
//   cells      per node: is the cell whose lowest corner it is a surface cell (eight corners in the table and valid, signs mixed) -> flag, count
//   vertices   per surface cell, in rank order: the mean of the edge crossings in fp64, and the id and colour of a voxel
//   face_count per node and axis: the lattice edge changes sign between valid nodes and its four cells are surface cells -> mask, count
//   face_emit  two triangles per such edge, wound so that the normal points from inside to outside
// The move and the projection are pinhole.h's, the rounded operations wave_ops.h's, the pixel is consistency.hip's floor(u + 0.5); contraction is
// off for the whole file; every test is a negated compare or written so that a NaN fails it.  No read falls outside a view's planes: the gather's
// index is formed only after the in-image test, and a view whose H W exceeds its npix takes no part.  Every probe is bounded by the capacity.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // vx_key, vx_in_range, vx_find_or_claim, vx_find, vx_table_ok; and through it wave_ops.h: rn_*, wg_rank
#include "pinhole.h"             // affine34, finite3, project, PH_CAM

#pragma clang fp contract(off)

namespace pst {

constexpr int TS_T = 256, TS_PT = 4, TS_WG = TS_T * TS_PT;        // threads, nodes per thread, nodes per workgroup (pst_cloud_scan's workgroups)
constexpr float TS_LIM = 1048576.f;                               // |u|, |v| <= 2^20: the consistency stage's limit
constexpr int64_t TS_MAX = 0x3fffffffLL;                          // pairs, and so nodes: what pst_voxel_count / pst_voxel_rank take
static_assert(PST_TSDF_FULL == VX_FULL && PST_TSDF_RANGE == PST_VCC_RANGE, "the status bits of the hash-grid stages");
static_assert(TS_WG == 1024, "pst_cloud_scan's callers count per 1024 items");

// the rank of the node (x, y, z), -1 if it is not active
__device__ __forceinline__ int ts_rank(const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ slot_rank, int x, int y, int z,
                                       int32_t* __restrict__ status) {
  if (!vx_in_range(x, y, z)) return -1;
  const int s = vx_find(keys, mask, vx_key(x, y, z), status);
  return s < 0 ? -1 : slot_rank[s];
}

__global__ __launch_bounds__(TS_T) void tsdf_insert_kernel(const int32_t* __restrict__ cells, int64_t P, int band, uint64_t* __restrict__ keys, uint32_t mask,
                                                           int32_t* __restrict__ first, int32_t* __restrict__ pair_slot, int32_t* __restrict__ status) {
  const int64_t p = (int64_t)blockIdx.x * TS_T + threadIdx.x;
  if (p >= P) return;
  const int side = 2 * band, K = side * side * side;
  const int64_t row = p / K;
  const int off = (int)(p - row * K);
  const int o[3] = {off % side, (off / side) % side, off / (side * side)};                   // x fastest
  long long n[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = (long long)cells[row * 3 + a] + o[a] - band + 1;
  int slot = -1;
  if (n[0] > -VX_LIM && n[0] < VX_LIM && n[1] > -VX_LIM && n[1] < VX_LIM && n[2] > -VX_LIM && n[2] < VX_LIM) {
    slot = vx_find_or_claim(keys, mask, vx_key((int)n[0], (int)n[1], (int)n[2]), status);
    if (slot >= 0) atomicMin(&first[slot], (int)p);
  } else {
    atomicOr(status, PST_TSDF_RANGE);
  }
  pair_slot[p] = slot;
}

__global__ __launch_bounds__(TS_T) void tsdf_nodes_kernel(const int32_t* __restrict__ cells, int Mv, int band, const int32_t* __restrict__ first_pair, int Nn,
                                                          const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ slot_rank,
                                                          int32_t* __restrict__ nodes, int32_t* __restrict__ voxel_row, int32_t* __restrict__ status) {
  const int i = blockIdx.x * TS_T + threadIdx.x;
  if (i < Nn) {
    const int side = 2 * band, K = side * side * side;
    const int p = first_pair[i], row = p / K, off = p - row * K;
    nodes[(int64_t)i * 3 + 0] = cells[(int64_t)row * 3 + 0] + off % side - band + 1;
    nodes[(int64_t)i * 3 + 1] = cells[(int64_t)row * 3 + 1] + (off / side) % side - band + 1;
    nodes[(int64_t)i * 3 + 2] = cells[(int64_t)row * 3 + 2] + off / (side * side) - band + 1;
  }
  if (i < Mv) {                                                     // the node n = c of a voxel's cell is one of the voxel's own: cells are unique per voxel
    const int r = ts_rank(keys, mask, slot_rank, cells[(int64_t)i * 3], cells[(int64_t)i * 3 + 1], cells[(int64_t)i * 3 + 2], status);
    if (r >= 0 && r < Nn) voxel_row[r] = i;
  }
}

__global__ __launch_bounds__(TS_T) void tsdf_integrate_kernel(const int32_t* __restrict__ nodes, int Nn, float vs, float tau, const pst_cloud_view* __restrict__ views,
                                                              const float* __restrict__ cams, const int32_t* __restrict__ dims, int nviews,
                                                              const float* __restrict__ depth, float* __restrict__ sdf, int32_t* __restrict__ weight) {
  const int i0 = blockIdx.x * TS_WG + threadIdx.x;
  float P[TS_PT][3], S[TS_PT];
  int W[TS_PT];
  bool live[TS_PT];
#pragma unroll
  for (int k = 0; k < TS_PT; ++k) {
    const int i = i0 + k * TS_T;
    live[k] = i < Nn;
    S[k] = 0.f; W[k] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) P[k][a] = live[k] ? rn_mul((float)nodes[(int64_t)i * 3 + a], vs) : 0.f;
  }
  const float ntau = -tau;
  for (int j = 0; j < nviews; ++j) {
    const float* __restrict__ c = cams + (int64_t)j * PH_CAM;
    const int Hj = dims[2 * j], Wj = dims[2 * j + 1];
    if (Hj < 1 || Wj < 1 || (int64_t)Hj * Wj > views[j].npix) continue;               // uniform: a table that does not fit its planes is never indexed
    const float f = c[12], cx = c[13], cy = c[14], near = c[15];
    const float* __restrict__ dj = depth + views[j].offset;
#pragma unroll
    for (int k = 0; k < TS_PT; ++k) {
      if (!live[k]) continue;
      float pc[3], u, w;
      affine34(c, P[k], pc);
      const float zc = pc[2];
      if (!finite3(pc) || !(zc >= near)) continue;
      if (!project(f, f, cx, cy, pc, TS_LIM, u, w)) continue;
      const int px = (int)floorf(rn_add(u, 0.5f)), py = (int)floorf(rn_add(w, 0.5f));   // the nearest pixel centre
      if (px < 0 || px >= Wj || py < 0 || py >= Hj) continue;      // outside the image of j
      const float d = dj[py * Wj + px];                            // the index is < Hj Wj <= npix of j
      if (d == 0.f) continue;                                      // j measured nothing there
      const float s = rn_sub(d, zc);
      if (s < ntau) continue;                                      // occluded: behind what j measured by more than the band
      S[k] = rn_add(S[k], fminf(s, tau));
      ++W[k];
    }
  }
#pragma unroll
  for (int k = 0; k < TS_PT; ++k) {
    const int i = i0 + k * TS_T;
    if (i >= Nn) continue;
    sdf[i] = W[k] > 0 ? rn_div(S[k], (float)W[k]) : 0.f;
    weight[i] = W[k];
  }
}

// the eight corner nodes (x fastest) of the cell at node r: their ranks; true iff all are active and valid
__device__ __forceinline__ bool ts_corners(const int32_t* __restrict__ nodes, int r, const uint64_t* __restrict__ keys, uint32_t mask,
                                           const int32_t* __restrict__ slot_rank, const int32_t* __restrict__ weight, int min_weight, int32_t* __restrict__ status,
                                           int (&c)[3], int (&q)[8]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = nodes[(int64_t)r * 3 + a];
  bool all = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    q[k] = k == 0 ? r : ts_rank(keys, mask, slot_rank, c[0] + (k & 1), c[1] + ((k >> 1) & 1), c[2] + (k >> 2), status);
    all = all && q[k] >= 0 && weight[q[k]] >= min_weight;
    if (!all) break;
  }
  return all;
}

__device__ __forceinline__ int ts_cell_mask(const int32_t* __restrict__ nodes, int Nn, int i0, const uint64_t* __restrict__ keys, uint32_t mask,
                                            const int32_t* __restrict__ slot_rank, const float* __restrict__ sdf, const int32_t* __restrict__ weight, int min_weight,
                                            int32_t* __restrict__ status) {
  int m = 0;
  for (int k = 0; k < TS_PT; ++k) {
    const int r = i0 + k;
    if (r >= Nn) break;
    int c[3], q[8];
    if (!ts_corners(nodes, r, keys, mask, slot_rank, weight, min_weight, status, c, q)) continue;
    int inside = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) inside += sdf[q[e]] < 0.f ? 1 : 0;
    if (inside > 0 && inside < 8) m |= 1 << k;
  }
  return m;
}

__global__ __launch_bounds__(TS_T) void tsdf_cells_kernel(const int32_t* __restrict__ nodes, int Nn, const uint64_t* __restrict__ keys, uint32_t mask,
                                                          const int32_t* __restrict__ slot_rank, const float* __restrict__ sdf, const int32_t* __restrict__ weight,
                                                          int min_weight, int32_t* __restrict__ cell_vertex, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ status) {
  __shared__ int wtot[TS_T / 64];
  const int i0 = blockIdx.x * TS_WG + threadIdx.x * TS_PT;
  const int m = ts_cell_mask(nodes, Nn, i0, keys, mask, slot_rank, sdf, weight, min_weight, status);
#pragma unroll
  for (int k = 0; k < TS_PT; ++k)
    if (i0 + k < Nn) cell_vertex[i0 + k] = (m >> k) & 1;            // the flag; tsdf_vertices turns it into the vertex row or -1
  int total;
  wg_rank<TS_T, TS_PT>(m, wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(TS_T) void tsdf_vertices_kernel(const int32_t* __restrict__ nodes, int Nn, const uint64_t* __restrict__ keys, uint32_t mask,
                                                             const int32_t* __restrict__ slot_rank, const float* __restrict__ sdf,
                                                             const int32_t* __restrict__ weight, int min_weight, const int32_t* __restrict__ voxel_row,
                                                             const int32_t* __restrict__ vox_count, const int32_t* __restrict__ vox_pan,
                                                             const float* __restrict__ vox_colors, int Mv, double vs, const int32_t* __restrict__ base,
                                                             int32_t* __restrict__ cell_vertex, float* __restrict__ vertices, int32_t* __restrict__ vertex_ids,
                                                             float* __restrict__ colors, int32_t* __restrict__ status) {
  __shared__ int wtot[TS_T / 64];
  const int i0 = blockIdx.x * TS_WG + threadIdx.x * TS_PT;
  int m = 0;
#pragma unroll
  for (int k = 0; k < TS_PT; ++k)
    if (i0 + k < Nn && cell_vertex[i0 + k] == 1) m |= 1 << k;
  int total;
  int v = base[blockIdx.x] + wg_rank<TS_T, TS_PT>(m, wtot, total);
  for (int k = 0; k < TS_PT; ++k) {
    const int r = i0 + k;
    if (r >= Nn) break;
    if (!((m >> k) & 1)) { cell_vertex[r] = -1; continue; }
    int c[3], q[8];
    float D[8];
    const bool ok = ts_corners(nodes, r, keys, mask, slot_rank, weight, min_weight, status, c, q);
#pragma unroll
    for (int e = 0; e < 8; ++e) D[e] = ok ? sdf[q[e]] : 0.f;
    // the crossings of the twelve edges: axis x, y, z; within an axis the (b, c) offsets 00, 10, 01, 11 (a, b, c cyclic)
    double sum[3] = {0.0, 0.0, 0.0};
    int n = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, cc = (a + 2) % 3;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ob = e & 1, oc = e >> 1;
        const int lo = (ob << b) | (oc << cc), hi = lo | (1 << a);
        const float Da = D[lo], Db = D[hi];
        if ((Da < 0.f) == (Db < 0.f)) continue;
        const double t = (double)Da / ((double)Da - (double)Db);
        double pos[3];
        pos[a] = t; pos[b] = (double)ob; pos[cc] = (double)oc;
        sum[0] = sum[0] + pos[0]; sum[1] = sum[1] + pos[1]; sum[2] = sum[2] + pos[2];
        ++n;
      }
    }
    const double dn = (double)(n > 0 ? n : 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) vertices[(int64_t)v * 3 + a] = (float)(((double)c[a] + sum[a] / dn) * vs);
    // the voxel of the cell, else the fullest voxel among the 26 neighbouring cells (ties to the smaller row), else none
    int vr = voxel_row[r];
    if (vr < 0) {
      int best = 0;
      for (int d = 0; d < 27; ++d) {
        if (d == 13) continue;
        const int g = ts_rank(keys, mask, slot_rank, c[0] + d % 3 - 1, c[1] + (d / 3) % 3 - 1, c[2] + d / 9 - 1, status);
        if (g < 0) continue;
        const int w = voxel_row[g];
        if (w < 0 || w >= Mv) continue;
        const int n2 = vox_count[w];
        if (vr < 0 || n2 > best || (n2 == best && w < vr)) { vr = w; best = n2; }
      }
    }
    const bool has = vr >= 0 && vr < Mv;
    vertex_ids[v] = has ? vox_pan[vr] : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) colors[(int64_t)v * 3 + a] = has ? vox_colors[(int64_t)vr * 3 + a] : 0.f;
    cell_vertex[r] = v;
    ++v;
  }
}

// the four cells around the lattice edge from node n along axis a, (b, c) offsets (0,0), (-1,0), (-1,-1), (0,-1): their vertex rows; true iff all
// four are surface cells
__device__ __forceinline__ bool ts_edge_cells(const int (&n)[3], int a, const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ slot_rank,
                                              const int32_t* __restrict__ cell_vertex, int32_t* __restrict__ status, int (&v)[4]) {
  const int b = (a + 1) % 3, c = (a + 2) % 3;
  const int ob[4] = {0, -1, -1, 0}, oc[4] = {0, 0, -1, -1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int x[3] = {n[0], n[1], n[2]};
    x[b] += ob[k]; x[c] += oc[k];
    const int g = ts_rank(keys, mask, slot_rank, x[0], x[1], x[2], status);
    v[k] = g < 0 ? -1 : cell_vertex[g];
    if (v[k] < 0) return false;
  }
  return true;
}

// bit 3 k + a = the edge from node i0 + k along axis a emits its two triangles
__global__ __launch_bounds__(TS_T) void tsdf_face_count_kernel(const int32_t* __restrict__ nodes, int Nn, const uint64_t* __restrict__ keys, uint32_t mask,
                                                               const int32_t* __restrict__ slot_rank, const float* __restrict__ sdf,
                                                               const int32_t* __restrict__ weight, int min_weight, const int32_t* __restrict__ cell_vertex,
                                                               int32_t* __restrict__ face_mask, int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ int wtot[TS_T / 64];
  const int i0 = blockIdx.x * TS_WG + threadIdx.x * TS_PT;
  int m = 0;
  for (int k = 0; k < TS_PT; ++k) {
    const int r = i0 + k;
    if (r >= Nn) break;
    int fm = 0;
    if (weight[r] >= min_weight) {
      const int n[3] = {nodes[(int64_t)r * 3], nodes[(int64_t)r * 3 + 1], nodes[(int64_t)r * 3 + 2]};
      const bool in = sdf[r] < 0.f;
      for (int a = 0; a < 3; ++a) {
        const int g = ts_rank(keys, mask, slot_rank, n[0] + (a == 0), n[1] + (a == 1), n[2] + (a == 2), status);
        if (g < 0 || weight[g] < min_weight || (sdf[g] < 0.f) == in) continue;
        int v[4];
        if (ts_edge_cells(n, a, keys, mask, slot_rank, cell_vertex, status, v)) fm |= 1 << a;
      }
    }
    face_mask[r] = fm;
    m |= fm << (3 * k);
  }
  int total;
  wg_rank<TS_T, 3 * TS_PT>(m, wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = 2 * total;
}

__device__ __forceinline__ int ts_face_id(int a, int b, int c) { return (a == b || a == c) ? a : (b == c ? b : 0); }      // f9's rule (csrc/surface.hip)

__global__ __launch_bounds__(TS_T) void tsdf_face_emit_kernel(const int32_t* __restrict__ nodes, int Nn, const uint64_t* __restrict__ keys, uint32_t mask,
                                                              const int32_t* __restrict__ slot_rank, const float* __restrict__ sdf,
                                                              const int32_t* __restrict__ cell_vertex, const int32_t* __restrict__ face_mask,
                                                              const int32_t* __restrict__ vertex_ids, const int32_t* __restrict__ base,
                                                              int32_t* __restrict__ faces, int32_t* __restrict__ face_ids, int64_t* __restrict__ edge,
                                                              int32_t* __restrict__ status) {
  __shared__ int wtot[TS_T / 64];
  const int i0 = blockIdx.x * TS_WG + threadIdx.x * TS_PT;
  int m = 0;
#pragma unroll
  for (int k = 0; k < TS_PT; ++k)
    if (i0 + k < Nn) m |= (face_mask[i0 + k] & 7) << (3 * k);
  int total;
  int64_t s = (int64_t)base[blockIdx.x] + 2 * (int64_t)wg_rank<TS_T, 3 * TS_PT>(m, wtot, total);
  for (int k = 0; k < TS_PT; ++k) {
    const int r = i0 + k;
    if (r >= Nn) break;
    if (!((m >> (3 * k)) & 7)) continue;
    const int n[3] = {nodes[(int64_t)r * 3], nodes[(int64_t)r * 3 + 1], nodes[(int64_t)r * 3 + 2]};
    const bool in = sdf[r] < 0.f;
    for (int a = 0; a < 3; ++a) {
      if (!((m >> (3 * k + a)) & 1)) continue;
      int v[4];
      const bool ok = ts_edge_cells(n, a, keys, mask, slot_rank, cell_vertex, status, v);
      // inside -> outside runs along +a from an inside node: (q0, q1, q2), (q0, q2, q3); against it from an outside one: (q0, q2, q1), (q0, q3, q2)
      const int t[2][3] = {{v[0], in ? v[1] : v[2], in ? v[2] : v[1]}, {v[0], in ? v[2] : v[3], in ? v[3] : v[2]}};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int e = 0; e < 3; ++e) faces[(s + h) * 3 + e] = ok ? t[h][e] : 0;
        face_ids[s + h] = ok ? ts_face_id(vertex_ids[t[h][0]], vertex_ids[t[h][1]], vertex_ids[t[h][2]]) : 0;
        edge[s + h] = 3 * (int64_t)r + a;
      }
      s += 2;
    }
  }
}

}  // namespace pst

static int tsdf_table_ok(const char* what, int64_t Nn, int64_t cap) {
  return pst::vx_table_ok(what, Nn, pst::TS_MAX, cap, "nodes", "1 .. 2^30 - 1");
}

extern "C" int pst_tsdf_insert(const int32_t* cells, int64_t Mv, int band, uint64_t* keys, int64_t cap, int32_t* first, int32_t* pair_slot, int32_t* status,
                               void* stream) {
  using namespace pst;
  if (!cells || !keys || !first || !pair_slot || !status) { set_error("tsdf_insert: null operand"); return PST_EINVAL; }
  if (band < 1 || band > PST_TSDF_MAX_BAND || Mv < 1 || Mv > TS_MAX / (8 * band * band * band)) {
    set_error("tsdf_insert: bad shape (band=%d in [1, %d], Mv=%lld: Mv (2 band)^3 pairs in [1, 2^30 - 1])", band, PST_TSDF_MAX_BAND, (long long)Mv);
    return PST_EINVAL;
  }
  const int64_t P = Mv * 8 * band * band * band;
  if (vx_table_ok("tsdf_insert", P, TS_MAX, cap, "pairs", "1 .. 2^30 - 1")) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_insert_kernel, blocks_for(P, TS_T), dim3(TS_T), 0, (hipStream_t)stream, cells, P, band, keys, (uint32_t)(cap - 1), first, pair_slot, status);
  return check_launch("tsdf_insert");
}

extern "C" int pst_tsdf_nodes(const int32_t* cells, int64_t Mv, int band, const int32_t* first_pair, int64_t Nn, const uint64_t* keys, int64_t cap,
                              const int32_t* slot_rank, int32_t* nodes, int32_t* voxel_row, int32_t* status, void* stream) {
  using namespace pst;
  if (!cells || !first_pair || !keys || !slot_rank || !nodes || !voxel_row || !status) { set_error("tsdf_nodes: null operand"); return PST_EINVAL; }
  if (band < 1 || band > PST_TSDF_MAX_BAND || Mv < 1 || Mv > TS_MAX / (8 * band * band * band) || Nn > Mv * 8 * band * band * band) {
    set_error("tsdf_nodes: bad shape (band=%d in [1, %d], Mv=%lld, nodes=%lld <= Mv (2 band)^3 <= 2^30 - 1)", band, PST_TSDF_MAX_BAND, (long long)Mv, (long long)Nn);
    return PST_EINVAL;
  }
  if (tsdf_table_ok("tsdf_nodes", Nn, cap)) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_nodes_kernel, blocks_for(Nn > Mv ? Nn : Mv, TS_T), dim3(TS_T), 0, (hipStream_t)stream, cells, (int)Mv, band, first_pair, (int)Nn, keys,
                     (uint32_t)(cap - 1), slot_rank, nodes, voxel_row, status);
  return check_launch("tsdf_nodes");
}

extern "C" int pst_tsdf_integrate(const int32_t* nodes, int64_t Nn, float voxel_size, int band, const pst_cloud_view* views, const float* cams, const int32_t* dims,
                                  int nviews, const float* depth, float* sdf, int32_t* weight, void* stream) {
  using namespace pst;
  if (!nodes || !views || !cams || !dims || !depth || !sdf || !weight) { set_error("tsdf_integrate: null operand"); return PST_EINVAL; }
  if (Nn < 1 || Nn > TS_MAX || nviews < 1 || nviews > 65535 || band < 1 || band > PST_TSDF_MAX_BAND || !(voxel_size > 0.f && voxel_size <= PST_FMAX)) {
    set_error("tsdf_integrate: bad shape (nodes=%lld in [1, 2^30 - 1], %d views in [1, 65535], band=%d in [1, %d]) or voxel size %g", (long long)Nn, nviews, band,
              PST_TSDF_MAX_BAND, (double)voxel_size);
    return PST_EINVAL;
  }
  const float tau = (float)band * voxel_size;                      // one rounded product: rn_mul((float)band, vs)
  hipLaunchKernelGGL(tsdf_integrate_kernel, blocks_for(Nn, TS_WG), dim3(TS_T), 0, (hipStream_t)stream, nodes, (int)Nn, voxel_size, tau, views, cams, dims, nviews,
                     depth, sdf, weight);
  return check_launch("tsdf_integrate");
}

extern "C" int pst_tsdf_cells(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf, const int32_t* weight,
                              int min_weight, int32_t* cell_vertex, int32_t* counts, int32_t* status, void* stream) {
  using namespace pst;
  if (!nodes || !keys || !slot_rank || !sdf || !weight || !cell_vertex || !counts || !status) { set_error("tsdf_cells: null operand"); return PST_EINVAL; }
  if (min_weight < 1) { set_error("tsdf_cells: min_weight=%d must be >= 1", min_weight); return PST_EINVAL; }
  if (tsdf_table_ok("tsdf_cells", Nn, cap)) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_cells_kernel, blocks_for(Nn, TS_WG), dim3(TS_T), 0, (hipStream_t)stream, nodes, (int)Nn, keys, (uint32_t)(cap - 1), slot_rank, sdf, weight,
                     min_weight, cell_vertex, counts, status);
  return check_launch("tsdf_cells");
}

extern "C" int pst_tsdf_vertices(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf,
                                 const int32_t* weight, int min_weight, const int32_t* voxel_row, const int32_t* vox_count, const int32_t* vox_pan,
                                 const float* vox_colors, int64_t Mv, double voxel_size, const int32_t* base, int32_t* cell_vertex, float* vertices,
                                 int32_t* vertex_ids, float* colors, int32_t* status, void* stream) {
  using namespace pst;
  if (!nodes || !keys || !slot_rank || !sdf || !weight || !voxel_row || !vox_count || !vox_pan || !vox_colors || !base || !cell_vertex || !vertices || !vertex_ids ||
      !colors || !status) {
    set_error("tsdf_vertices: null operand"); return PST_EINVAL;
  }
  if (min_weight < 1 || Mv < 1 || Mv > TS_MAX || !(voxel_size > 0.0 && voxel_size <= (double)PST_FMAX)) {     // positive and finite, as pst_tsdf_integrate's
    set_error("tsdf_vertices: bad shape (min_weight=%d >= 1, Mv=%lld in [1, 2^30 - 1]) or voxel size", min_weight, (long long)Mv); return PST_EINVAL;
  }
  if (tsdf_table_ok("tsdf_vertices", Nn, cap)) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_vertices_kernel, blocks_for(Nn, TS_WG), dim3(TS_T), 0, (hipStream_t)stream, nodes, (int)Nn, keys, (uint32_t)(cap - 1), slot_rank, sdf, weight,
                     min_weight, voxel_row, vox_count, vox_pan, vox_colors, (int)Mv, voxel_size, base, cell_vertex, vertices, vertex_ids, colors, status);
  return check_launch("tsdf_vertices");
}

extern "C" int pst_tsdf_face_count(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf,
                                   const int32_t* weight, int min_weight, const int32_t* cell_vertex, int32_t* face_mask, int32_t* counts, int32_t* status,
                                   void* stream) {
  using namespace pst;
  if (!nodes || !keys || !slot_rank || !sdf || !weight || !cell_vertex || !face_mask || !counts || !status) { set_error("tsdf_face_count: null operand"); return PST_EINVAL; }
  if (min_weight < 1) { set_error("tsdf_face_count: min_weight=%d must be >= 1", min_weight); return PST_EINVAL; }
  if (tsdf_table_ok("tsdf_face_count", Nn, cap)) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_face_count_kernel, blocks_for(Nn, TS_WG), dim3(TS_T), 0, (hipStream_t)stream, nodes, (int)Nn, keys, (uint32_t)(cap - 1), slot_rank, sdf,
                     weight, min_weight, cell_vertex, face_mask, counts, status);
  return check_launch("tsdf_face_count");
}

extern "C" int pst_tsdf_face_emit(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf,
                                  const int32_t* cell_vertex, const int32_t* face_mask, const int32_t* vertex_ids, const int32_t* base, int32_t* faces,
                                  int32_t* face_ids, int64_t* edge, int32_t* status, void* stream) {
  using namespace pst;
  if (!nodes || !keys || !slot_rank || !sdf || !cell_vertex || !face_mask || !vertex_ids || !base || !faces || !face_ids || !edge || !status) {
    set_error("tsdf_face_emit: null operand"); return PST_EINVAL;
  }
  if (tsdf_table_ok("tsdf_face_emit", Nn, cap)) return PST_EINVAL;
  hipLaunchKernelGGL(tsdf_face_emit_kernel, blocks_for(Nn, TS_WG), dim3(TS_T), 0, (hipStream_t)stream, nodes, (int)Nn, keys, (uint32_t)(cap - 1), slot_rank, sdf,
                     cell_vertex, face_mask, vertex_ids, base, faces, face_ids, edge, status);
  return check_launch("tsdf_face_emit");
}
