// Mesh simplification by vertex clustering (Rossignac-Borrel) on the cell grid of the voxel stage (f18; no counterpart in the reference; the contract
// is the mesh simplification section of include/panst3r_hip.h, restated in tests/simplify_ref.py, [restated, parity unpinned]).  The vertex half IS
// the voxel stage (pst_voxel_* on the vertex table, unchanged); this file only prepares its input and rewrites the faces:
//   used      one thread per face: used[corner] = 1 for its three corners (every writer stores the same word); a corner outside [0, M) sets the
//             RANGE bit and nothing is read or written through it.
//   mask      one thread per vertex: the vertex itself where it is used, NaN where no face names it - the voxel stage leaves a non-finite point out,
//             so an unused vertex joins no cluster and the rows keep their order.  The used vertices are counted, one atomic per wave.
//   remap     one thread per face: its corners through cluster[]; left out (a corner -1), degenerate (two new corners equal) or a candidate.  With
//             dedupe a candidate's sorted corners, 3 x 21 bits (each corner + 1, so no field is all ones), go into voxel_table.h's open-addressing
//             table and the face index into the slot by a 32-bit atomicMin: the smallest original index of every unordered triple.  Runs of adjacent
//             lanes with one key (the faces of neighbouring quads that collapsed onto one triple) are merged first: the run's first lane holds its
//             smallest index and is the only one that probes.
//   count     a candidate survives iff it is its slot's winner (without dedupe: every candidate): counted per 256 faces,
//   scan      pst_cloud_scan of the counts,
//   emit      and stored in the order of the originals with the remapped corners in their original order, the original's quad and index, and the
//             id two new corners share, else 0.
// Integer work only: no float arithmetic at all (mask copies bits or stores a NaN).  Integer atomics only; every result a plain vector store; every
// probe loop is vx_find_or_claim's, bounded by the capacity.  Two calls return equal bytes: the winner is a minimum, the order a scan.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // and through it wave_ops.h: wg_rank, vx_run, wave_count_add

namespace pst {

constexpr int SM_T = PST_SURFACE_WG;                               // threads = faces (or vertices) per workgroup
static_assert(SM_T == 256, "four waves per workgroup");
constexpr int SM_LEFT_OUT = -1, SM_DEGENERATE = -2;                // face_slot of a face that is no candidate
constexpr int64_t SM_MAX_FACES = 0x7fffff00ll, SM_MAX_VERTICES = 1ll << 30, SM_MAX_KEYED = (1ll << 21) - 2;
static_assert(PST_SIMPLIFY_FULL == VX_FULL, "one bit for a table without an empty slot");

__device__ __forceinline__ bool sm_in(int v, int n) { return (unsigned)v < (unsigned)n; }

// the sorted triple, 21 bits each of corner + 1 in [1, 2^21 - 1]: never VX_EMPTY
__device__ __forceinline__ uint64_t sm_key(int a, int b, int c) {
  const int lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = a + b + c - lo - hi;
  return (uint64_t)(lo + 1) | ((uint64_t)(mid + 1) << 21) | ((uint64_t)(hi + 1) << 42);
}

__global__ __launch_bounds__(SM_T) void simplify_used_kernel(const int32_t* __restrict__ faces, int F, int M, int32_t* __restrict__ used,
                                                             int32_t* __restrict__ status) {
  const int f = blockIdx.x * SM_T + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(int64_t)f * 3], b = faces[(int64_t)f * 3 + 1], c = faces[(int64_t)f * 3 + 2];
  if (!sm_in(a, M) || !sm_in(b, M) || !sm_in(c, M)) { atomicOr(&status[0], PST_SIMPLIFY_RANGE); return; }
  used[a] = 1; used[b] = 1; used[c] = 1;
}

__global__ __launch_bounds__(SM_T) void simplify_mask_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ used, int M,
                                                             float* __restrict__ masked, int32_t* __restrict__ status) {
  const int v = blockIdx.x * SM_T + threadIdx.x;
  const bool u = v < M && used[v] != 0;
  wave_count_add(u, &status[1]);
  if (v >= M) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) masked[(int64_t)v * 3 + a] = u ? vertices[(int64_t)v * 3 + a] : __builtin_nanf("");
}

// the new corners of face f; false = no candidate (`why` = SM_LEFT_OUT or SM_DEGENERATE).  A corner outside [0, M) or a cluster outside [-1, Mv)
// is reported and left out: nothing is read through it.
__device__ __forceinline__ bool sm_corners(const int32_t* __restrict__ faces, const int32_t* __restrict__ cluster, int f, int M, int Mv, int (&n)[3],
                                           int& why, int32_t* __restrict__ status) {
  why = SM_LEFT_OUT;
  bool bad = false, out = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int v = faces[(int64_t)f * 3 + j];
    n[j] = -1;
    if (!sm_in(v, M)) { bad = true; continue; }
    n[j] = cluster[v];
    if (n[j] == -1) out = true;
    else if (!sm_in(n[j], Mv)) { bad = true; n[j] = -1; }
  }
  if (bad && status) atomicOr(&status[0], PST_SIMPLIFY_RANGE);
  if (bad || out) return false;
  if (n[0] == n[1] || n[0] == n[2] || n[1] == n[2]) { why = SM_DEGENERATE; return false; }
  return true;
}

template <bool DEDUPE, bool MERGE>
__global__ __launch_bounds__(SM_T) void simplify_remap_kernel(const int32_t* __restrict__ faces, int F, int M, const int32_t* __restrict__ cluster, int Mv,
                                                              uint64_t* __restrict__ keys, uint32_t mask, int32_t* __restrict__ winner,
                                                              int32_t* __restrict__ face_slot, int32_t* __restrict__ status) {
  const int f = blockIdx.x * SM_T + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = f < F;
  int n[3] = {-1, -1, -1}, why = SM_LEFT_OUT;
  const bool cand = in && sm_corners(faces, cluster, f, M, Mv, n, why, status);
  wave_count_add(in && !cand && why == SM_LEFT_OUT, &status[2]);
  wave_count_add(in && !cand && why == SM_DEGENERATE, &status[3]);
  wave_count_add(cand, &status[4]);
  int slot = cand ? 0 : why;
  if constexpr (DEDUPE) {
    const uint64_t key = cand ? sm_key(n[0], n[1], n[2]) : VX_EMPTY;
    if constexpr (MERGE) {
      int head, tail;
      vx_run(key, lane, head, tail);
      int s = -1;
      if (cand && head == lane) {                                    // the run's first lane holds its smallest face index
        s = vx_find_or_claim(keys, mask, key, status);
        if (s >= 0) atomicMin(&winner[s], f);
      }
      s = __shfl(s, head);
      if (cand) slot = s >= 0 ? s : SM_LEFT_OUT;                     // a full table (never: capacity >= 2 F) is reported, the face not emitted
    } else if (cand) {
      const int s = vx_find_or_claim(keys, mask, key, status);
      if (s >= 0) atomicMin(&winner[s], f);
      slot = s >= 0 ? s : SM_LEFT_OUT;
    }
  }
  if (in) face_slot[f] = slot;
}

template <bool DEDUPE>
__device__ __forceinline__ int sm_survives(const int32_t* __restrict__ face_slot, const int32_t* __restrict__ winner, int F, int f) {
  if (f >= F) return 0;
  const int s = face_slot[f];
  if (s < 0) return 0;
  if constexpr (DEDUPE) return winner[s] == f;
  return 1;
}

template <bool DEDUPE>
__global__ __launch_bounds__(SM_T) void simplify_count_kernel(const int32_t* __restrict__ face_slot, const int32_t* __restrict__ winner, int F,
                                                              int32_t* __restrict__ counts) {
  __shared__ int wtot[SM_T / 64];
  int total;
  wg_rank<SM_T, 1>(sm_survives<DEDUPE>(face_slot, winner, F, blockIdx.x * SM_T + threadIdx.x), wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__device__ __forceinline__ int sm_face_id(int a, int b, int c) { return (a == b || a == c) ? a : (b == c ? b : 0); }

template <bool DEDUPE>
__global__ __launch_bounds__(SM_T) void simplify_emit_kernel(const int32_t* __restrict__ faces, const int64_t* __restrict__ quad,
                                                             const int32_t* __restrict__ cluster, const int32_t* __restrict__ vertex_ids,
                                                             const int32_t* __restrict__ face_slot, const int32_t* __restrict__ winner, int F, int M, int Mv,
                                                             const int32_t* __restrict__ base, int32_t* __restrict__ out_faces,
                                                             int32_t* __restrict__ out_face_ids, int64_t* __restrict__ out_quad, int32_t* __restrict__ src_face) {
  __shared__ int wtot[SM_T / 64];
  const int f = blockIdx.x * SM_T + threadIdx.x;
  int keep = sm_survives<DEDUPE>(face_slot, winner, F, f);
  int total;
  const int64_t s = (int64_t)base[blockIdx.x] + wg_rank<SM_T, 1>(keep, wtot, total);
  if (!keep) return;
  int n[3], why;
  if (!sm_corners(faces, cluster, f, M, Mv, n, why, nullptr)) return;  // never: remap found this face a candidate on the same operands
  out_faces[s * 3] = n[0]; out_faces[s * 3 + 1] = n[1]; out_faces[s * 3 + 2] = n[2];
  out_face_ids[s] = sm_face_id(vertex_ids[n[0]], vertex_ids[n[1]], vertex_ids[n[2]]);
  out_quad[s] = quad[f];
  src_face[s] = f;
}

static bool sm_mesh_ok(int64_t F, int64_t M) { return F > 0 && F <= SM_MAX_FACES && M > 0 && M <= SM_MAX_VERTICES; }

}  // namespace pst

extern "C" int pst_simplify_used(const int32_t* faces, int64_t F, int64_t M, int32_t* used, int32_t* status, void* stream) {
  using namespace pst;
  if (!faces || !used || !status || !sm_mesh_ok(F, M)) {
    set_error("simplify_used: bad shape (F=%lld, M=%lld) or null operand", (long long)F, (long long)M); return PST_EINVAL;
  }
  hipLaunchKernelGGL(simplify_used_kernel, blocks_for(F, SM_T), dim3(SM_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, used, status);
  return check_launch("simplify_used");
}

extern "C" int pst_simplify_mask(const float* vertices, const int32_t* used, int64_t M, float* masked, int32_t* status, void* stream) {
  using namespace pst;
  if (!vertices || !used || !masked || !status || M <= 0 || M > SM_MAX_VERTICES) {
    set_error("simplify_mask: bad shape (M=%lld) or null operand", (long long)M); return PST_EINVAL;
  }
  hipLaunchKernelGGL(simplify_mask_kernel, blocks_for(M, SM_T), dim3(SM_T), 0, (hipStream_t)stream, vertices, used, (int)M, masked, status);
  return check_launch("simplify_mask");
}

extern "C" int pst_simplify_remap(const int32_t* faces, int64_t F, int64_t M, const int32_t* cluster, int64_t Mv, int dedupe, uint64_t* keys, int64_t cap,
                                  int32_t* winner, int32_t* face_slot, int32_t* status, int merge, void* stream) {
  using namespace pst;
  if (!faces || !cluster || !face_slot || !status || !sm_mesh_ok(F, M) || Mv <= 0 || Mv > M) {
    set_error("simplify_remap: bad shape (F=%lld, M=%lld, Mv=%lld) or null operand", (long long)F, (long long)M, (long long)Mv); return PST_EINVAL;
  }
  const dim3 grid = blocks_for(F, SM_T);
  if (!dedupe) {
    hipLaunchKernelGGL((simplify_remap_kernel<false, false>), grid, dim3(SM_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, cluster, (int)Mv,
                       (uint64_t*)nullptr, 0u, (int32_t*)nullptr, face_slot, status);
    return check_launch("simplify_remap");
  }
  if (!keys || !winner) { set_error("simplify_remap: null operand"); return PST_EINVAL; }
  if (Mv > SM_MAX_KEYED) {
    set_error("simplify_remap: %lld new vertices exceed the 2^21 - 2 that a 3 x 21-bit face key takes (dedupe)", (long long)Mv); return PST_EINVAL;
  }
  if (vx_table_ok("simplify_remap", F, SM_MAX_FACES, cap, "F", "1 .. 2^31 - 256")) return PST_EINVAL;
  if (merge) hipLaunchKernelGGL((simplify_remap_kernel<true, true>), grid, dim3(SM_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, cluster, (int)Mv, keys,
                                (uint32_t)(cap - 1), winner, face_slot, status);
  else hipLaunchKernelGGL((simplify_remap_kernel<true, false>), grid, dim3(SM_T), 0, (hipStream_t)stream, faces, (int)F, (int)M, cluster, (int)Mv, keys,
                          (uint32_t)(cap - 1), winner, face_slot, status);
  return check_launch("simplify_remap");
}

extern "C" int pst_simplify_count(const int32_t* face_slot, const int32_t* winner, int64_t F, int dedupe, int32_t* counts, void* stream) {
  using namespace pst;
  if (!face_slot || !counts || (dedupe && !winner) || F <= 0 || F > SM_MAX_FACES) {
    set_error("simplify_count: bad shape (F=%lld) or null operand", (long long)F); return PST_EINVAL;
  }
  if (dedupe) hipLaunchKernelGGL(simplify_count_kernel<true>, blocks_for(F, SM_T), dim3(SM_T), 0, (hipStream_t)stream, face_slot, winner, (int)F, counts);
  else hipLaunchKernelGGL(simplify_count_kernel<false>, blocks_for(F, SM_T), dim3(SM_T), 0, (hipStream_t)stream, face_slot, winner, (int)F, counts);
  return check_launch("simplify_count");
}

extern "C" int pst_simplify_emit(const int32_t* faces, const int64_t* quad, const int32_t* cluster, const int32_t* vertex_ids, const int32_t* face_slot,
                                 const int32_t* winner, int64_t F, int64_t M, int64_t Mv, int dedupe, const int32_t* base, int32_t* out_faces,
                                 int32_t* out_face_ids, int64_t* out_quad, int32_t* src_face, void* stream) {
  using namespace pst;
  if (!faces || !quad || !cluster || !vertex_ids || !face_slot || (dedupe && !winner) || !base || !out_faces || !out_face_ids || !out_quad || !src_face ||
      !sm_mesh_ok(F, M) || Mv <= 0 || Mv > M) {
    set_error("simplify_emit: bad shape (F=%lld, M=%lld, Mv=%lld) or null operand", (long long)F, (long long)M, (long long)Mv); return PST_EINVAL;
  }
  if (dedupe) hipLaunchKernelGGL(simplify_emit_kernel<true>, blocks_for(F, SM_T), dim3(SM_T), 0, (hipStream_t)stream, faces, quad, cluster, vertex_ids,
                                 face_slot, winner, (int)F, (int)M, (int)Mv, base, out_faces, out_face_ids, out_quad, src_face);
  else hipLaunchKernelGGL(simplify_emit_kernel<false>, blocks_for(F, SM_T), dim3(SM_T), 0, (hipStream_t)stream, faces, quad, cluster, vertex_ids, face_slot,
                          winner, (int)F, (int)M, (int)Mv, base, out_faces, out_face_ids, out_quad, src_face);
  return check_launch("simplify_emit");
}
