// The two primitives of the 3-D scores (engine/score3d.py; no counterpart in the reference; the contract is the score3d section of
// include/panst3r_hip.h, restated in tests/nearest_ref.py, [restated, parity unpinned]):
//   mesh sampler   count  one lane per face: the face's subdivision n (a binary search over [1, max_subdiv] decided by fp64 compares, no sqrt), n^2 into
//                         counts, dropped and clamped faces counted, the total added up in int64 (one integer atomic per wave)
//                  scan   pst_cloud_scan of the per-face counts
//                  emit   one lane per sample: its face by binary search in the prefix, the sub-triangle's integer weights, one fp64 combination
//                  (which faces are kept, and the search in the prefix: mesh_face.h, shared with csrc/meshdist.hip)
//   nearest point  insert one lane per target: cell -> key -> slot of the open-addressing table, one int32 atomicAdd on the slot's count
//                  (the cell rule, the key, the table's probes and the per-cell lists: voxel_table.h, shared by every hash-grid stage)
//                  (offsets: a prefix sum of the slot counts, made by the caller)
//                  scatter the target's row into its cell's list (the position inside the list depends on arrival; nothing that leaves depends on it)
//                  query  one lane per query: the 27 cells around it, every candidate's fp32 distance, the minimum of (bits(d2) << 32) | row
//   icp step       step   a block per PST_ICP_CHUNK source rows, 16 rows per lane: the row moved by the 3 x 4 matrix in fp32, the query's search (the same
//                         __device__ function), the 18 live moments of the matched pairs in fp64 registers; a butterfly per wave, the four waves added
//                         in order, one row of 20 per block
//                  reduce one block adds the rows of the blocks the same way
//                  (the move: pinhole.h; the fixed order of the sums: icp_sum.h, shared with the point-to-plane step of csrc/meshdist.hip)
// Integer atomics only, no float sum whose order depends on arrival (the moments are added in the order the header fixes), every probe / candidate / search loop bounded by a number known before the launch,
// refusals through the status words, every result written with plain vector stores: two calls return identical bytes.  Contraction is off for the
// whole file: every fp32 and fp64 operation is rounded on its own, in the order written.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // and through it wave_ops.h: rn_mul / rn_add / rn_sub, wave_count_add, wave_sum
#include "mesh_face.h"
#include "icp_sum.h"

#pragma clang fp contract(off)

namespace pst {

constexpr int NN_T = 256;
constexpr int MS_MAX_SUBDIV = PST_MESH_SAMPLE_MAX_SUBDIV;
static_assert(MS_MAX_SUBDIV == 1 << 15, "n^2 and 3n stay inside int32");

// ---------------------------------------------------------------- mesh surface sampler
__device__ __forceinline__ double ms_edge2(const double (&a)[3], const double (&b)[3]) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// the face's sample count n^2 (0 = dropped); clamped = the face wanted more than max_subdiv
__device__ __forceinline__ int ms_count(const MeshFace& t, double s2, int max_subdiv, int& clamped) {
  clamped = 0;
  if (!t.ok || !mf_has_area(t)) return 0;
  double v[3][3];                                                   // (widening a float is exact: the same values as the loader's)
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) v[k][a] = (double)t.v[k][a];
  const double L2 = fmax(fmax(ms_edge2(v[1], v[0]), ms_edge2(v[2], v[1])), ms_edge2(v[0], v[2]));
  // enough(n) = n n s2 >= L2 is monotone in n: the smallest n of [1, max_subdiv] that is enough, max_subdiv if none is.  At most 16 rounds.
  int lo = 1, hi = max_subdiv;
  if (!(((double)hi * (double)hi) * s2 >= L2)) { clamped = 1; return hi * hi; }
  for (int it = 0; it < 16 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if (((double)mid * (double)mid) * s2 >= L2) hi = mid; else lo = mid + 1;
  }
  return hi * hi;
}

__global__ __launch_bounds__(NN_T) void mesh_sample_count_kernel(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int F,
                                                                 double s2, int max_subdiv, int32_t* __restrict__ counts, int64_t* __restrict__ total,
                                                                 int32_t* __restrict__ status) {
  const int f = blockIdx.x * NN_T + threadIdx.x;
  int c = 0, clamped = 0, dropped = 0;
  if (f < F) {
    c = ms_count(mf_load(vertices, Nv, faces, f), s2, max_subdiv, clamped);
    dropped = c == 0;
    counts[f] = c;
  }
  const long long sum = wave_sum(c);                                 // 64 faces of at most 2^30 samples
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd((unsigned long long*)total, (unsigned long long)sum);
  wave_count_add(dropped, &status[1]);
  wave_count_add(clamped, &status[2]);
}

__global__ __launch_bounds__(NN_T) void mesh_sample_emit_kernel(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int F,
                                                                const int32_t* __restrict__ prefix, int total, const int32_t* __restrict__ vertex_ids,
                                                                const int32_t* __restrict__ face_ids, float* __restrict__ points,
                                                                int32_t* __restrict__ face, int32_t* __restrict__ ids, int32_t* __restrict__ status) {
  if (prefix[F] != total) {                                         // uniform: the prefix is not the one the caller sized the outputs by
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[0], PST_MESH_SAMPLE_TOTAL);
    return;
  }
  const int s = blockIdx.x * NN_T + threadIdx.x;
  if (s >= total) return;
  const int f = mf_prefix_owner(prefix, F, s), t = s - prefix[f], cnt = prefix[f + 1] - prefix[f];
  int n = (int)sqrt((double)cnt);                                   // cnt = n^2 exactly: a first guess, settled by integer compares
  if ((int64_t)n * n > cnt) --n;
  if ((int64_t)(n + 1) * (n + 1) <= cnt) ++n;
  int r = (int)sqrt((double)t);
  if ((int64_t)r * r > t) --r;
  if ((int64_t)(r + 1) * (r + 1) <= t) ++r;
  const int c = t - r * r, k = c >> 1;
  int w[3];
  if (c & 1) { w[0] = 3 * (n - r) - 1; w[1] = 3 * (r - k) - 1; w[2] = 3 * k + 2; }
  else       { w[0] = 3 * (n - r) - 2; w[1] = 3 * (r - k) + 1; w[2] = 3 * k + 1; }
  const MeshFace tri = mf_load(vertices, Nv, faces, f);             // (a face with samples has passed these checks)
  const double den = (double)(3 * n);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double p = (((double)w[0] * (double)tri.v[0][a] + (double)w[1] * (double)tri.v[1][a]) + (double)w[2] * (double)tri.v[2][a]) / den;
    points[(int64_t)s * 3 + a] = (float)p;
  }
  face[s] = f;
  int id = 0;
  if (face_ids) id = face_ids[f];
  else if (vertex_ids) {
    const int best = (w[1] > w[0] ? (w[2] > w[1] ? 2 : 1) : (w[2] > w[0] ? 2 : 0));      // the largest weight, ties to the lower corner
    id = vertex_ids[faces[(int64_t)f * 3 + best]];
  }
  ids[s] = id;
}

// ---------------------------------------------------------------- fixed-radius nearest neighbour
__device__ __forceinline__ void nn_cell(const float* __restrict__ p, float inv, float (&x)[3], float (&c)[3], bool& finite, bool& ok) {
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = p[a];
  vx_cell_of(x, inv, c, finite, ok);
}

__global__ __launch_bounds__(NN_T) void nn_insert_kernel(const float* __restrict__ targets, int M, float inv, uint64_t* __restrict__ keys, uint32_t mask,
                                                         int32_t* __restrict__ cell_count, int32_t* __restrict__ point_slot, int32_t* __restrict__ status) {
  const int i = blockIdx.x * NN_T + threadIdx.x;
  const bool in = i < M;
  float x[3], c[3];
  bool finite = false, ok = false;
  if (in) nn_cell(targets + (int64_t)i * 3, inv, x, c, finite, ok);
  wave_count_add(in && !ok, &status[1]);
  if (!in) return;
  int slot = -1;
  if (ok) {
    slot = vx_find_or_claim(keys, mask, vx_key((int)c[0], (int)c[1], (int)c[2]), status);
    if (slot >= 0) atomicAdd(&cell_count[slot], 1);
  }
  point_slot[i] = slot;
}

// the target's row into its cell's list; status[2] = the largest occupancy
__global__ __launch_bounds__(NN_T) void nn_scatter_kernel(const int32_t* __restrict__ point_slot, int M, const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ cell_count, int32_t* __restrict__ fill, int32_t* __restrict__ rows,
                                                          int32_t* __restrict__ status) {
  const int i = blockIdx.x * NN_T + threadIdx.x;
  if (i >= M) return;
  const int slot = point_slot[i];
  if (slot < 0) return;
  vx_list_place(slot, start, cell_count, fill, M, rows, status, [&] { return i; });
}

// step 3 of the fixed-radius contract for one lane, shared by nn_query and icp_step: every candidate of the 27 cells around the cell c of the point q
// -> the minimum of (bits(d2) << 32) | row, all ones without a candidate.  Nothing here is collective: lanes may call it divergently.
__device__ __forceinline__ uint64_t nn_search(const float (&q)[3], const float (&c)[3], bool finite, const float* __restrict__ targets, int M,
                                              const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ start,
                                              const int32_t* __restrict__ cell_count, const int32_t* __restrict__ rows, int max_cell_points,
                                              int32_t* __restrict__ status) {
  uint64_t best = ~0ull;
  // a finite query whose cell is not within one cell of the range has no target cell among its 27
  if (finite && fabsf(c[0]) <= (float)VX_LIM && fabsf(c[1]) <= (float)VX_LIM && fabsf(c[2]) <= (float)VX_LIM) {
    const int cx = (int)c[0], cy = (int)c[1], cz = (int)c[2];
    for (int nb = 0; nb < 27; ++nb) {
      const int x = cx + nb % 3 - 1, y = cy + (nb / 3) % 3 - 1, z = cz + nb / 9 - 1;
      if (!vx_in_range(x, y, z)) continue;                          // no such cell: never looked up
      const int slot = vx_find(keys, mask, vx_key(x, y, z), status);
      int b, cnt;
      if (slot < 0 || !vx_list_range(slot, start, cell_count, M, max_cell_points, status, b, cnt)) continue;
      for (int j = 0; j < cnt; ++j) {
        const int p = rows[b + j];
        if ((unsigned)p >= (unsigned)M) { atomicOr(&status[0], PST_NN_LISTS); continue; }
        const float dx = rn_sub(q[0], targets[(int64_t)p * 3]), dy = rn_sub(q[1], targets[(int64_t)p * 3 + 1]),
                    dz = rn_sub(q[2], targets[(int64_t)p * 3 + 2]);
        const float d2 = rn_add(rn_add(rn_mul(dx, dx), rn_mul(dy, dy)), rn_mul(dz, dz));      // >= +0, never NaN: its bits order as an unsigned integer
        const uint64_t cand = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)p;
        best = cand < best ? cand : best;
      }
    }
  }
  return best;
}

__global__ __launch_bounds__(NN_T) void nn_query_kernel(const float* __restrict__ queries, int Nq, const float* __restrict__ targets, int M, float inv,
                                                        float r2, const uint64_t* __restrict__ keys, uint32_t mask, const int32_t* __restrict__ start,
                                                        const int32_t* __restrict__ cell_count, const int32_t* __restrict__ rows, int max_cell_points,
                                                        float* __restrict__ d2_out, int32_t* __restrict__ row_out, int32_t* __restrict__ status) {
  const int i = blockIdx.x * NN_T + threadIdx.x;
  const bool in = i < Nq;
  float q[3], c[3];
  bool finite = false, ok = false;
  if (in) nn_cell(queries + (int64_t)i * 3, inv, q, c, finite, ok);
  wave_count_add(in && !finite, &status[3]);
  if (!in) return;
  const uint64_t best = nn_search(q, c, finite, targets, M, keys, mask, start, cell_count, rows, max_cell_points, status);
  const float d2 = __uint_as_float((uint32_t)(best >> 32));
  const bool hit = best != ~0ull && d2 <= r2;
  d2_out[i] = hit ? d2 : __uint_as_float(0x7f800000u);
  row_out[i] = hit ? (int)(uint32_t)best : -1;
}

// ---------------------------------------------------------------- one fused ICP step (the icp section of include/panst3r_hip.h)
constexpr int ICP_LIVE = 18;                                         // the moments that are sums; [18], [19] are +0.0
static_assert(NN_T == ICP_T && ICP_LIVE + 2 == PST_ICP_MOMENTS, "the fixed order of the header (icp_sum.h: the block sum and the reducer)");

__global__ __launch_bounds__(NN_T) void icp_step_kernel(const float* __restrict__ source, int N, IcpMatrix A, const float* __restrict__ targets, int M,
                                                        float inv, float r2, const uint64_t* __restrict__ keys, uint32_t mask,
                                                        const int32_t* __restrict__ start, const int32_t* __restrict__ cell_count,
                                                        const int32_t* __restrict__ rows, int max_cell_points, float* __restrict__ d2_out,
                                                        int32_t* __restrict__ row_out, double* __restrict__ partials, int32_t* __restrict__ status) {
  const int first = blockIdx.x * PST_ICP_CHUNK + threadIdx.x;        // N <= 2^30: no row leaves int32
  double acc[ICP_LIVE];
#pragma unroll
  for (int s = 0; s < ICP_LIVE; ++s) acc[s] = 0.0;
  int bad = 0;
  for (int j = 0; j < ICP_ROWS; ++j) {                               // (per lane: nothing collective inside)
    const int i = first + NN_T * j;
    if (i >= N) break;
    float x[3], m[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = source[(int64_t)i * 3 + a];
    affine34(&A.a[0][0], x, m);
    bool finite, ok;
    vx_cell_of(m, inv, c, finite, ok);
    bad += !finite;
    const uint64_t best = nn_search(m, c, finite, targets, M, keys, mask, start, cell_count, rows, max_cell_points, status);
    const float d2 = __uint_as_float((uint32_t)(best >> 32));
    const bool hit = best != ~0ull && d2 <= r2;
    if (d2_out) {
      d2_out[i] = hit ? d2 : __uint_as_float(0x7f800000u);
      row_out[i] = hit ? (int)(uint32_t)best : -1;
    }
    if (!hit) continue;
    const int p = (int)(uint32_t)best;                               // (the search took it from rows and checked it against M)
    double xd[3], yd[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { xd[a] = (double)x[a]; yd[a] = (double)targets[(int64_t)p * 3 + a]; }
    acc[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { acc[1 + a] += xd[a]; acc[4 + a] += yd[a]; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int a = 0; a < 3; ++a) acc[7 + 3 * r + a] += yd[r] * xd[a];      // a product of two widened fp32 values is exact
    acc[16] += (xd[0] * xd[0] + xd[1] * xd[1]) + xd[2] * xd[2];
    acc[17] += (double)d2;
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) bad += __shfl_xor(bad, k);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&status[3], bad);
  icp_block_sum<ICP_LIVE, PST_ICP_MOMENTS>(acc, partials + (int64_t)blockIdx.x * PST_ICP_MOMENTS);
}

constexpr int64_t NN_MAX_POINTS = 1ll << 30;

}  // namespace pst

extern "C" int pst_mesh_sample_count(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float spacing, int max_subdiv, int32_t* counts,
                                     int64_t* total, int32_t* status, void* stream) {
  using namespace pst;
  if (!vertices || !faces || !counts || !total || !status || Nv <= 0 || Nv > 0x7fffffffll || F <= 0 || F > NN_MAX_POINTS || !(spacing > 0.f) ||
      !(spacing <= PST_FMAX) || max_subdiv < 1 || max_subdiv > MS_MAX_SUBDIV) {
    set_error("mesh_sample_count: bad shape (Nv=%lld, F=%lld: at most 2^30 faces), spacing %g (positive, finite), max_subdiv %d (1 .. %d) or null operand",
              (long long)Nv, (long long)F, (double)spacing, max_subdiv, MS_MAX_SUBDIV);
    return PST_EINVAL;
  }
  const double s2 = (double)spacing * (double)spacing;              // exact: two 24-bit significands
  hipLaunchKernelGGL(mesh_sample_count_kernel, blocks_for(F, NN_T), dim3(NN_T), 0, (hipStream_t)stream, vertices, (int)Nv, faces, (int)F, s2, max_subdiv, counts, total,
                     status);
  return check_launch("mesh_sample_count");
}

extern "C" int pst_mesh_sample_emit(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, const int32_t* prefix, int64_t total, int64_t capacity,
                                    const int32_t* vertex_ids, const int32_t* face_ids, float* points, int32_t* face, int32_t* ids, int32_t* status,
                                    void* stream) {
  using namespace pst;
  if (!vertices || !faces || !prefix || !points || !face || !ids || !status || Nv <= 0 || Nv > 0x7fffffffll || F <= 0 || F > NN_MAX_POINTS || total <= 0 ||
      (vertex_ids && face_ids)) {
    set_error("mesh_sample_emit: bad shape (Nv=%lld, F=%lld, total=%lld), both kinds of ids or null operand", (long long)Nv, (long long)F, (long long)total);
    return PST_EINVAL;
  }
  if (total > capacity || total > 0x7fffff00ll) {                   // before anything is written
    set_error("mesh_sample_emit: %lld samples exceed the capacity of %lld (2^31 - 256 at the most): a larger spacing or a smaller max_subdiv gives fewer",
              (long long)total, (long long)capacity);
    return PST_EINVAL;
  }
  hipLaunchKernelGGL(mesh_sample_emit_kernel, blocks_for(total, NN_T), dim3(NN_T), 0, (hipStream_t)stream, vertices, (int)Nv, faces, (int)F, prefix, (int)total,
                     vertex_ids, face_ids, points, face, ids, status);
  return check_launch("mesh_sample_emit");
}

extern "C" int pst_nn_insert(const float* targets, int64_t M, float inv, uint64_t* keys, int64_t capacity, int32_t* cell_count, int32_t* point_slot,
                             int32_t* status, void* stream) {
  using namespace pst;
  if (vx_table_ok("nn_insert", M, NN_MAX_POINTS, capacity, "M", "at most 2^30 targets")) return PST_EINVAL;
  if (!targets || !keys || !cell_count || !point_slot || !status || !(inv > 0.f) || !(inv <= PST_FMAX)) {
    set_error("nn_insert: inverse radius %g (positive, finite) or null operand", (double)inv); return PST_EINVAL;
  }
  hipLaunchKernelGGL(nn_insert_kernel, blocks_for(M, NN_T), dim3(NN_T), 0, (hipStream_t)stream, targets, (int)M, inv, keys, (uint32_t)(capacity - 1), cell_count,
                     point_slot, status);
  return check_launch("nn_insert");
}

extern "C" int pst_nn_scatter(const int32_t* point_slot, int64_t M, const int32_t* start, const int32_t* cell_count, int32_t* fill, int32_t* rows,
                              int32_t* status, void* stream) {
  using namespace pst;
  if (!point_slot || !start || !cell_count || !fill || !rows || !status || M <= 0 || M > NN_MAX_POINTS) {
    set_error("nn_scatter: bad shape (M=%lld) or null operand", (long long)M); return PST_EINVAL;
  }
  hipLaunchKernelGGL(nn_scatter_kernel, blocks_for(M, NN_T), dim3(NN_T), 0, (hipStream_t)stream, point_slot, (int)M, start, cell_count, fill, rows, status);
  return check_launch("nn_scatter");
}

extern "C" int pst_nn_query(const float* queries, int64_t Nq, const float* targets, int64_t M, float inv, float r2, const uint64_t* keys, int64_t capacity,
                            const int32_t* start, const int32_t* cell_count, const int32_t* rows, int max_cell_points, float* d2, int32_t* row,
                            int32_t* status, void* stream) {
  using namespace pst;
  if (vx_table_ok("nn_query", M, NN_MAX_POINTS, capacity, "M", "at most 2^30 targets")) return PST_EINVAL;
  if (!queries || !targets || !keys || !start || !cell_count || !rows || !d2 || !row || !status || Nq <= 0 || Nq > NN_MAX_POINTS || !(inv > 0.f) ||
      !(inv <= PST_FMAX) || !(r2 >= 0.f) || !(r2 <= PST_FMAX) || max_cell_points < 1) {
    set_error("nn_query: bad shape (Nq=%lld: at most 2^30 queries), inverse radius %g, squared radius %g (finite), max_cell_points %d (>= 1) or null operand",
              (long long)Nq, (double)inv, (double)r2, max_cell_points);
    return PST_EINVAL;
  }
  hipLaunchKernelGGL(nn_query_kernel, blocks_for(Nq, NN_T), dim3(NN_T), 0, (hipStream_t)stream, queries, (int)Nq, targets, (int)M, inv, r2, keys,
                     (uint32_t)(capacity - 1), start, cell_count, rows, max_cell_points, d2, row, status);
  return check_launch("nn_query");
}

extern "C" int pst_icp_chunk(void) { return PST_ICP_CHUNK; }

extern "C" int pst_icp_step(const float* source, int64_t N, float a00, float a01, float a02, float a03, float a10, float a11, float a12, float a13, float a20,
                            float a21, float a22, float a23, const float* targets, int64_t M, float inv, float r2, const uint64_t* keys, int64_t capacity,
                            const int32_t* start, const int32_t* cell_count, const int32_t* rows, int max_cell_points, float* d2, int32_t* row,
                            double* partials, double* out, int32_t* status, void* stream) {
  using namespace pst;
  if (vx_table_ok("icp_step", M, NN_MAX_POINTS, capacity, "M", "at most 2^30 targets")) return PST_EINVAL;
  if (!source || !targets || !keys || !start || !cell_count || !rows || !partials || !out || !status || (d2 == nullptr) != (row == nullptr) || N < 1 ||
      N > NN_MAX_POINTS || !(inv > 0.f) || !(inv <= PST_FMAX) || !(r2 >= 0.f) || !(r2 <= PST_FMAX) || max_cell_points < 1) {
    set_error("icp_step: bad shape (N=%lld: 1 .. 2^30 source points), inverse cell edge %g, squared radius %g (finite), max_cell_points %d (>= 1), one of "
              "d2 / row without the other, or null operand", (long long)N, (double)inv, (double)r2, max_cell_points);
    return PST_EINVAL;
  }
  const IcpMatrix A = {{{a00, a01, a02, a03}, {a10, a11, a12, a13}, {a20, a21, a22, a23}}};
  const int P = (int)((N + PST_ICP_CHUNK - 1) / PST_ICP_CHUNK);
  hipLaunchKernelGGL(icp_step_kernel, dim3((unsigned)P), dim3(NN_T), 0, (hipStream_t)stream, source, (int)N, A, targets, (int)M, inv, r2, keys,
                     (uint32_t)(capacity - 1), start, cell_count, rows, max_cell_points, d2, row, partials, status);
  if (int rc = check_launch("icp_step")) return rc;
  hipLaunchKernelGGL((icp_reduce_kernel<ICP_LIVE, PST_ICP_MOMENTS>), dim3(1), dim3(NN_T), 0, (hipStream_t)stream, (const double*)partials, P, out);
  return check_launch("icp_step (reduce)");
}
