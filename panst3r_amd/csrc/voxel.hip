// Voxel fusion of the panoptic point cloud with multi-view label votes (no counterpart in the reference, whose viewer shows the raw concatenation;
// restated in tests/voxel_ref.py, [restated, parity unpinned]).  One pass over the cloud that csrc/cloud.hip left on the device:
//   insert      every point's cell -> a 64-bit key (3 x 21 bits) in an open-addressing table (linear probing, slots claimed by 64-bit compare-and-swap,
//               every probe loop bounded by the capacity; the cell rule, the key and the table are voxel_table.h); atomicMin of the point's row into
//               the slot: the voxel's FIRST row.  A point left out (non-finite, or a cell outside +-2^20) gets slot -1 and is counted.
//   count/rank  a point is its voxel's first one iff first[slot] == its row: counted per 1024 points, turned into output ranks by pst_cloud_scan, so
//               the voxels come out in the order of their first rows without a sort.
//   accumulate  per point, into arrays indexed by the voxel's rank: count, three sums of the 16-bit in-cell offsets, three colour sums - 64-bit
//               INTEGER atomics - and one vote in a second table keyed by (rank, panoptic id).
//   vote        one pass over the pair table: 64-bit atomicMax of (votes << 32) | (0xFFFFFFFF - id) per voxel = most votes, ties to the smallest id.
//   emit        per voxel: mean position and colour in fp64 from the integer sums, the voted id, the blended colour, plain vector stores.
// The contract (include/panst3r_hip.h) is integer arithmetic plus separately rounded fp32 / fp64 operations: contraction is off for the whole file,
// no float atomics, no float sum whose order depends on arrival - two calls return identical bytes.
// `merge`: adjacent lanes of a wave that hold the same key (neighbouring pixels of one view fall into one voxel) are merged before the global
// atomics - the run's first lane inserts, its last lane adds the run's sums (a wave-wide prefix sum, differenced at the run's ends).  Same results.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // and through it wave_ops.h: rn_mul / rn_add / rn_sub, wg_rank, wave_scan, vx_run, wave_count_add

#pragma clang fp contract(off)

namespace pst {

constexpr int VX_T = 256, VX_PT = 4, VX_WG = VX_T * VX_PT;         // count / rank: the 1024-point workgroups of pst_cloud_scan's callers
constexpr int VX_MAX_COLORS = 4096;

// cell (as floats, exact integers) and in-cell offset q = floor((t - c) * 65536) in [0, 65536] of a point; false = the point is left out
__device__ __forceinline__ bool vx_cell(const float* __restrict__ p, float inv, float (&c)[3], int (&q)[3]) {
  const float x[3] = {p[0], p[1], p[2]};
  bool finite, ok;
  vx_cell_of(x, inv, c, finite, ok);
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = (int)floorf(rn_mul(rn_sub(rn_mul(x[a], inv), c[a]), 65536.f));      // t = x * inv: the product vx_cell_of floors
  return ok;
}

template <bool MERGE>
__global__ __launch_bounds__(VX_T) void voxel_insert_kernel(const float* __restrict__ points, int M, float inv, uint64_t* __restrict__ keys, uint32_t mask,
                                                            int32_t* __restrict__ first, int32_t* __restrict__ point_slot, int32_t* __restrict__ status) {
  const int i = blockIdx.x * VX_T + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = i < M;
  float c[3]; int q[3];
  bool ok = false;
  if (in) ok = vx_cell(points + (int64_t)i * 3, inv, c, q);
  const uint64_t key = ok ? vx_key((int)c[0], (int)c[1], (int)c[2]) : VX_EMPTY;
  wave_count_add(in && !ok, &status[1]);
  int slot = -1;
  if constexpr (MERGE) {
    int head, tail;
    vx_run(key, lane, head, tail);
    if (ok && head == lane) {                                       // the run's first lane holds its smallest row
      slot = vx_find_or_claim(keys, mask, key, status);
      if (slot >= 0) atomicMin(&first[slot], i);
    }
    slot = __shfl(slot, head);
  } else if (ok) {
    slot = vx_find_or_claim(keys, mask, key, status);
    if (slot >= 0) atomicMin(&first[slot], i);
  }
  if (in) point_slot[i] = slot;
}

// bit k = point i0 + k is the first one of its voxel
__device__ __forceinline__ int vx_first_mask(const int32_t* __restrict__ point_slot, const int32_t* __restrict__ first, int M, int i0) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < VX_PT; ++k)
    if (i0 + k < M) {
      const int s = point_slot[i0 + k];
      if (s >= 0 && first[s] == i0 + k) m |= 1 << k;
    }
  return m;
}

__global__ __launch_bounds__(VX_T) void voxel_count_kernel(const int32_t* __restrict__ point_slot, const int32_t* __restrict__ first, int M,
                                                           int32_t* __restrict__ counts) {
  __shared__ int wtot[VX_T / 64];
  int total;
  wg_rank<VX_T, VX_PT>(vx_first_mask(point_slot, first, M, blockIdx.x * VX_WG + threadIdx.x * VX_PT), wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// rank of every first point = workgroup base + wave base + lane prefix (stable: ranks follow the rows) -> slot_rank[slot], first_row[rank]
__global__ __launch_bounds__(VX_T) void voxel_rank_kernel(const int32_t* __restrict__ point_slot, const int32_t* __restrict__ first, int M,
                                                          const int32_t* __restrict__ base, int32_t* __restrict__ slot_rank, int32_t* __restrict__ first_row) {
  __shared__ int wtot[VX_T / 64];
  const int tid = threadIdx.x, i0 = blockIdx.x * VX_WG + tid * VX_PT;
  const int m = vx_first_mask(point_slot, first, M, i0);
  int total;
  int r = base[blockIdx.x] + wg_rank<VX_T, VX_PT>(m, wtot, total);
#pragma unroll
  for (int k = 0; k < VX_PT; ++k)
    if ((m >> k) & 1) {
      slot_rank[point_slot[i0 + k]] = r;
      first_row[r] = i0 + k;
      ++r;
    }
}

__device__ __forceinline__ void vx_vote(uint64_t* __restrict__ pkeys, int32_t* __restrict__ pcnt, uint32_t mask, uint64_t pkey, int n,
                                        int32_t* __restrict__ status) {
  const int s = vx_find_or_claim(pkeys, mask, pkey, status);
  if (s >= 0) atomicAdd(&pcnt[s], n);
}

// uchar of a colour channel: floor(clamp(x, 0, 1) * 255 + 0.5) in fp32, a NaN counts as 0
__device__ __forceinline__ uint32_t vx_u8(float x) { return (uint32_t)floorf(rn_add(rn_mul(fminf(fmaxf(x, 0.f), 1.f), 255.f), 0.5f)); }

template <bool MERGE>
__global__ __launch_bounds__(VX_T) void voxel_accumulate_kernel(const float* __restrict__ points, const float* __restrict__ rgb, const int32_t* __restrict__ pan,
                                                                int M, float inv, const int32_t* __restrict__ point_slot, const int32_t* __restrict__ slot_rank,
                                                                const int32_t* __restrict__ id2row, int ntab, int32_t* __restrict__ cnt,
                                                                unsigned long long* __restrict__ sums, uint64_t* __restrict__ pkeys, int32_t* __restrict__ pcnt,
                                                                uint32_t mask, int32_t* __restrict__ point_voxel, int32_t* __restrict__ status) {
  const int i = blockIdx.x * VX_T + threadIdx.x, lane = threadIdx.x & 63;
  int r = -1, id = 0;
  int q[3] = {0, 0, 0};
  uint32_t u[3] = {0, 0, 0};
  if (i < M) {
    const int s = point_slot[i];
    if (s >= 0) {
      r = slot_rank[s];
      float c[3];
      vx_cell(points + (int64_t)i * 3, inv, c, q);
#pragma unroll
      for (int a = 0; a < 3; ++a) u[a] = vx_u8(rgb[(int64_t)i * 3 + a]);
      const int p = pan[i];
      if (p > 0 && p < ntab && id2row[p] >= 0) id = p;                // everything else votes void
    }
    point_voxel[i] = r;
  }
  const uint64_t pkey = id > 0 ? ((uint64_t)(uint32_t)r << 32) | (uint32_t)id : VX_EMPTY;
  if constexpr (MERGE) {
    int head, tail;
    vx_run(r >= 0 ? (uint64_t)r : VX_EMPTY, lane, head, tail);
    // a wave's totals fit 32 bits: 64 x 65536 per offset, 64 x 255 per channel
    uint32_t v[5] = {(uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], u[0] | (u[1] << 16), u[2] | (1u << 16)};
    const int src = max(head - 1, 0);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const uint32_t s = wave_scan(v[k], lane);
      const uint32_t b = __shfl(s, src);
      v[k] = s - (head > 0 ? b : 0u);
    }
    if (r >= 0 && lane == tail) {
      atomicAdd(&cnt[r], (int)(v[4] >> 16));
      unsigned long long* sp = sums + (int64_t)r * 6;
      atomicAdd(sp + 0, (unsigned long long)v[0]); atomicAdd(sp + 1, (unsigned long long)v[1]); atomicAdd(sp + 2, (unsigned long long)v[2]);
      atomicAdd(sp + 3, (unsigned long long)(v[3] & 0xffffu)); atomicAdd(sp + 4, (unsigned long long)(v[3] >> 16));
      atomicAdd(sp + 5, (unsigned long long)(v[4] & 0xffffu));
    }
    vx_run(pkey, lane, head, tail);
    if (id > 0 && lane == head) vx_vote(pkeys, pcnt, mask, pkey, tail - head + 1, status);
  } else if (r >= 0) {
    atomicAdd(&cnt[r], 1);
    unsigned long long* sp = sums + (int64_t)r * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicAdd(sp + a, (unsigned long long)q[a]); atomicAdd(sp + 3 + a, (unsigned long long)u[a]); }
    if (id > 0) vx_vote(pkeys, pcnt, mask, pkey, 1, status);
  }
}

__global__ __launch_bounds__(VX_T) void voxel_vote_kernel(const uint64_t* __restrict__ pkeys, const int32_t* __restrict__ pcnt, int64_t cap,
                                                          unsigned long long* __restrict__ best) {
  for (int64_t s = (int64_t)blockIdx.x * VX_T + threadIdx.x; s < cap; s += (int64_t)gridDim.x * VX_T) {
    const uint64_t k = pkeys[s];
    if (k == VX_EMPTY) continue;                                     // (a pass over every slot, not a probe: those are voxel_table.h's)
    atomicMax(&best[k >> 32], ((unsigned long long)(uint32_t)pcnt[s] << 32) | (0xFFFFFFFFu - (uint32_t)k));
  }
}

__global__ __launch_bounds__(VX_T) void voxel_emit_kernel(const float* __restrict__ points, const int64_t* __restrict__ index, const int32_t* __restrict__ first_row,
                                                          const int32_t* __restrict__ mv_ptr, float inv, double voxel_size, const int32_t* __restrict__ cnt,
                                                          const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ best,
                                                          const float* __restrict__ colors, int ncolors, float w1, float w2, float* __restrict__ out_points,
                                                          float* __restrict__ out_rgb, int32_t* __restrict__ out_pan, float* __restrict__ out_colors,
                                                          int32_t* __restrict__ out_votes, int64_t* __restrict__ out_first) {
  const int r = blockIdx.x * VX_T + threadIdx.x;
  if (r >= *mv_ptr) return;
  const int i = first_row[r];
  float c[3]; int q[3];
  vx_cell(points + (int64_t)i * 3, inv, c, q);                      // every member of the voxel has this cell
  const int n = cnt[r];
  const double dn = (double)n;
  const unsigned long long b = best[r];
  const int id = b ? (int)(0xFFFFFFFFu - (uint32_t)b) : 0;
  const bool known = id > 0 && id < ncolors;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double off = ((double)sums[(int64_t)r * 6 + a] / dn) * 0x1p-16;
    out_points[(int64_t)r * 3 + a] = (float)(((double)c[a] + off) * voxel_size);
    const float g = (float)(((double)sums[(int64_t)r * 6 + 3 + a] / dn) / 255.0);
    out_rgb[(int64_t)r * 3 + a] = g;
    out_colors[(int64_t)r * 3 + a] = rn_add(rn_mul(w1, g), rn_mul(w2, known ? colors[id * 3 + a] : 0.f));
  }
  out_pan[r] = id;
  out_votes[r] = b ? (int)(b >> 32) : n;                            // only void votes: all of them
  out_first[r] = index[i];
}

}  // namespace pst

extern "C" int pst_voxel_insert(const float* points, int64_t M, float inv, uint64_t* keys, int64_t cap, int32_t* first, int32_t* point_slot, int32_t* status,
                                int merge, void* stream) {
  using namespace pst;
  if (!points || !keys || !first || !point_slot || !status) { set_error("voxel_insert: null operand"); return PST_EINVAL; }
  if (M <= 0 || M > 0x3fffffffLL || !vx_cap_ok(M, cap) || !(inv > 0.f)) {
    set_error("voxel_insert: bad shape (M=%lld, capacity=%lld: a power of two >= 2 M) or inverse voxel size", (long long)M, (long long)cap); return PST_EINVAL;
  }
  const dim3 grid = blocks_for(M, VX_T);
  if (merge) hipLaunchKernelGGL(voxel_insert_kernel<true>, grid, dim3(VX_T), 0, (hipStream_t)stream, points, (int)M, inv, keys, (uint32_t)(cap - 1), first, point_slot, status);
  else hipLaunchKernelGGL(voxel_insert_kernel<false>, grid, dim3(VX_T), 0, (hipStream_t)stream, points, (int)M, inv, keys, (uint32_t)(cap - 1), first, point_slot, status);
  return check_launch("voxel_insert");
}

extern "C" int pst_voxel_count(const int32_t* point_slot, const int32_t* first, int64_t M, int32_t* counts, void* stream) {
  using namespace pst;
  if (!point_slot || !first || !counts || M <= 0 || M > 0x3fffffffLL) { set_error("voxel_count: bad shape / null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(voxel_count_kernel, blocks_for(M, VX_WG), dim3(VX_T), 0, (hipStream_t)stream, point_slot, first, (int)M, counts);
  return check_launch("voxel_count");
}

extern "C" int pst_voxel_rank(const int32_t* point_slot, const int32_t* first, int64_t M, const int32_t* base, int32_t* slot_rank, int32_t* first_row,
                              void* stream) {
  using namespace pst;
  if (!point_slot || !first || !base || !slot_rank || !first_row || M <= 0 || M > 0x3fffffffLL) { set_error("voxel_rank: bad shape / null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(voxel_rank_kernel, blocks_for(M, VX_WG), dim3(VX_T), 0, (hipStream_t)stream, point_slot, first, (int)M, base, slot_rank,
                     first_row);
  return check_launch("voxel_rank");
}

extern "C" int pst_voxel_accumulate(const float* points, const float* rgb, const int32_t* pan, int64_t M, float inv, const int32_t* point_slot,
                                    const int32_t* slot_rank, const int32_t* id2row, int ntab, int32_t* cnt, uint64_t* sums, uint64_t* pair_keys,
                                    int32_t* pair_cnt, int64_t cap, int32_t* point_voxel, int32_t* status, int merge, void* stream) {
  using namespace pst;
  if (!points || !rgb || !pan || !point_slot || !slot_rank || !id2row || !cnt || !sums || !pair_keys || !pair_cnt || !point_voxel || !status) {
    set_error("voxel_accumulate: null operand"); return PST_EINVAL;
  }
  if (M <= 0 || M > 0x3fffffffLL || !vx_cap_ok(M, cap) || ntab < 1) {
    set_error("voxel_accumulate: bad shape (M=%lld, capacity=%lld, ntab=%d)", (long long)M, (long long)cap, ntab); return PST_EINVAL;
  }
  const dim3 grid = blocks_for(M, VX_T);
  if (merge) hipLaunchKernelGGL(voxel_accumulate_kernel<true>, grid, dim3(VX_T), 0, (hipStream_t)stream, points, rgb, pan, (int)M, inv, point_slot, slot_rank, id2row,
                                ntab, cnt, (unsigned long long*)sums, pair_keys, pair_cnt, (uint32_t)(cap - 1), point_voxel, status);
  else hipLaunchKernelGGL(voxel_accumulate_kernel<false>, grid, dim3(VX_T), 0, (hipStream_t)stream, points, rgb, pan, (int)M, inv, point_slot, slot_rank, id2row,
                          ntab, cnt, (unsigned long long*)sums, pair_keys, pair_cnt, (uint32_t)(cap - 1), point_voxel, status);
  return check_launch("voxel_accumulate");
}

extern "C" int pst_voxel_vote(const uint64_t* pair_keys, const int32_t* pair_cnt, int64_t cap, uint64_t* best, void* stream) {
  using namespace pst;
  if (!pair_keys || !pair_cnt || !best || cap <= 0 || cap > (1ll << 31)) { set_error("voxel_vote: bad shape / null operand"); return PST_EINVAL; }
  const int64_t nwg = (cap + VX_T - 1) / VX_T;
  hipLaunchKernelGGL(voxel_vote_kernel, dim3((unsigned)(nwg < 8192 ? nwg : 8192)), dim3(VX_T), 0, (hipStream_t)stream, pair_keys, pair_cnt, cap,
                     (unsigned long long*)best);
  return check_launch("voxel_vote");
}

extern "C" int pst_voxel_emit(const float* points, const int64_t* index, const int32_t* first_row, const int32_t* mv_ptr, int64_t max_voxels, float inv,
                              double voxel_size, const int32_t* cnt, const uint64_t* sums, const uint64_t* best, const float* colors, int ncolors, float w1,
                              float w2, float* out_points, float* out_rgb, int32_t* out_pan, float* out_colors, int32_t* out_votes, int64_t* out_first,
                              void* stream) {
  using namespace pst;
  if (!points || !index || !first_row || !mv_ptr || !cnt || !sums || !best || !colors || !out_points || !out_rgb || !out_pan || !out_colors || !out_votes ||
      !out_first) {
    set_error("voxel_emit: null operand"); return PST_EINVAL;
  }
  if (max_voxels <= 0 || max_voxels > 0x3fffffffLL || ncolors < 1 || ncolors > VX_MAX_COLORS || !(voxel_size > 0.0)) {
    set_error("voxel_emit: bad shape (max_voxels=%lld, ncolors=%d) or voxel size", (long long)max_voxels, ncolors); return PST_EINVAL;
  }
  hipLaunchKernelGGL(voxel_emit_kernel, blocks_for(max_voxels, VX_T), dim3(VX_T), 0, (hipStream_t)stream, points, index, first_row, mv_ptr, inv,
                     voxel_size, cnt, (const unsigned long long*)sums, (const unsigned long long*)best, colors, ncolors, w1, w2, out_points, out_rgb, out_pan,
                     out_colors, out_votes, out_first);
  return check_launch("voxel_emit");
}
