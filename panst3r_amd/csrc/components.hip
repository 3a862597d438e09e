// 3-D connected components of the voxel cloud and the despeckling of its labels (no counterpart in the reference; restated in tests/vcc_ref.py,
// [restated, parity unpinned]).  On the voxels that csrc/voxel.hip left on the device:
//   cells     the integer cell of every voxel's first point (step 1 of the voxel contract), written while the fusion's workspace is alive
//   build     cell key -> voxel row in an open-addressing table of its own (capacity >= 2 Mv; the key, the hash and both probes are voxel_table.h):
//             keys are unique, so a compare-and-swap claim plus a plain store of the row; parent[v] = v (void: -1)
//   link      one voxel per lane looks up the lexicographically positive half of its neighbourhood (3, 9 or 13 cells) and unites itself with every
//             neighbour of its own id in parent[]: find with path halving, hook the larger root under the smaller with atomicMin, go on from the value
//             the atomic returned when another thread got there first.  Parent values only decrease and parent[x] <= x, so every loop ends, no thread
//             ever waits for another thread's store, and a finished component's root is its smallest row whatever the arrival order.
//   flatten   root[v] = find(v) (read only), then size, points and the cell box of the component: integer atomicAdd / atomicMin / atomicMax on arrays
//             indexed by the root's row.  `merge`: runs of adjacent lanes with one root are reduced inside the wave first (a segmented scan), the run's
//             last lane issues the eight atomics.  Same results.
//   count / rank  a row is a root iff root[v] == v: counted per 1024 rows, turned into ranks by pst_cloud_scan (the pattern of voxel_count / voxel_rank),
//             the table compacted in the same pass; component[v] = rank of root[v].
//   votes     every voxel of a small component (size < min_voxels) looks up ALL its neighbours; one vote per (voxel, neighbour) pair whose neighbour is
//             non-void and lies in a component that is not small, into a pair table keyed by (root << 32) | id.  pst_voxel_vote picks the winner per root.
//   apply     the new id of every voxel (a small component without a vote becomes void) and its re-blended colour.
// Integer atomics only, every probe / find / union loop bounded (an overflow sets a bit of status[0] and ends the loop), plain vector stores for results.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "voxel_table.h"         // and through it wave_ops.h: rn_mul / rn_add, wg_rank, wave_scan, vx_run, wave_count_add
#include "union_find.h"          // cc_load, cc_find, cc_unite

#pragma clang fp contract(off)

namespace pst {

constexpr int CC_T = 256, CC_PT = 4, CC_WG = CC_T * CC_PT;         // count / rank: 1024 rows per workgroup, as pst_cloud_scan's other callers
constexpr int CC_DUP = PST_VCC_DUPLICATE, CC_RANGE = PST_VCC_RANGE, CC_LOOP = PST_VCC_LOOP;
constexpr int CC_MAX_COLORS = 4096;

// the row stored for `key`, -1 if the cell is empty
__device__ __forceinline__ int cc_lookup(const uint64_t* __restrict__ keys, const int32_t* __restrict__ rows, uint32_t mask, uint64_t key,
                                         int32_t* __restrict__ status) {
  const int slot = vx_find(keys, mask, key, status);
  return slot >= 0 ? rows[slot] : -1;
}

// offset k in [0, 27) of the 3 x 3 x 3 neighbourhood -> (dx, dy, dz) and the number of axes that differ; k > 13 is the lexicographically positive half
__device__ __forceinline__ int cc_offset(int k, int& dx, int& dy, int& dz) {
  dx = k % 3 - 1; dy = (k / 3) % 3 - 1; dz = k / 9 - 1;
  return (dx != 0) + (dy != 0) + (dz != 0);
}

__global__ __launch_bounds__(CC_T) void vcc_cells_kernel(const float* __restrict__ points, const int32_t* __restrict__ first_row, const int32_t* __restrict__ mv_ptr,
                                                         float inv, int32_t* __restrict__ cells) {
  const int r = blockIdx.x * CC_T + threadIdx.x;
  if (r >= *mv_ptr) return;
  const float* p = points + (int64_t)first_row[r] * 3;
  const float x[3] = {p[0], p[1], p[2]};
  float c[3];
  bool finite, ok;
  vx_cell_of(x, inv, c, finite, ok);                                // ok: the fusion kept the point
#pragma unroll
  for (int a = 0; a < 3; ++a) cells[(int64_t)r * 3 + a] = (int)c[a];
}

__global__ __launch_bounds__(CC_T) void vcc_build_kernel(const int32_t* __restrict__ cells, const int32_t* __restrict__ pan, int Mv, uint64_t* __restrict__ keys,
                                                         int32_t* __restrict__ rows, uint32_t mask, int32_t* __restrict__ parent, int32_t* __restrict__ status) {
  const int v = blockIdx.x * CC_T + threadIdx.x;
  if (v >= Mv) return;
  parent[v] = pan[v] > 0 ? v : -1;
  const int x = cells[(int64_t)v * 3], y = cells[(int64_t)v * 3 + 1], z = cells[(int64_t)v * 3 + 2];
  if (!vx_in_range(x, y, z)) { atomicOr(status, CC_RANGE); return; }
  bool claimed;
  const int slot = vx_find_or_claim(keys, mask, vx_key(x, y, z), status, &claimed);
  if (slot < 0) return;                                             // (a full table: reported by the probe)
  if (claimed) rows[slot] = v;                                      // the only writer of this slot's row
  else atomicOr(status, CC_DUP);                                    // two voxels in one cell: not a voxel cloud
}

__global__ __launch_bounds__(CC_T) void vcc_link_kernel(const int32_t* __restrict__ cells, const int32_t* __restrict__ pan, int Mv, const uint64_t* __restrict__ keys,
                                                        const int32_t* __restrict__ rows, uint32_t mask, int max_axes, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ status) {
  const int v = blockIdx.x * CC_T + threadIdx.x;
  if (v >= Mv) return;
  const int id = pan[v];
  if (id <= 0) return;
  const int x = cells[(int64_t)v * 3], y = cells[(int64_t)v * 3 + 1], z = cells[(int64_t)v * 3 + 2];
  if (!vx_in_range(x, y, z)) return;                                // (reported by build)
  for (int k = 14; k < 27; ++k) {
    int dx, dy, dz;
    if (cc_offset(k, dx, dy, dz) > max_axes) continue;
    if (!vx_in_range(x + dx, y + dy, z + dz)) continue;             // no such cell: never looked up
    const int n = cc_lookup(keys, rows, mask, vx_key(x + dx, y + dy, z + dz), status);
    if (n >= 0 && pan[n] == id) cc_unite(parent, v, n, Mv, status);
  }
}

template <bool MERGE>
__global__ __launch_bounds__(CC_T) void vcc_flatten_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ count, const int32_t* __restrict__ cells,
                                                           int Mv, int32_t* __restrict__ root, int32_t* __restrict__ size, unsigned long long* __restrict__ points,
                                                           int32_t* __restrict__ lo, int32_t* __restrict__ hi, int32_t* __restrict__ status) {
  const int v = blockIdx.x * CC_T + threadIdx.x, lane = threadIdx.x & 63;
  int r = -1;
  if (v < Mv) {
    r = parent[v];                                                  // -1: void
    if (r >= 0) {
      int x = v, it = 0;
      for (; it < Mv && r != x; ++it) { x = r; r = parent[x]; }    // the links are final: plain loads, nothing written
      if (r != x) { atomicOr(status, CC_LOOP); r = -1; }
    }
    root[v] = r;
  }
  int n = 0, c[3] = {0, 0, 0};
  long long pts = 0;
  if (r >= 0) {
    n = 1; pts = count[v];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cells[(int64_t)v * 3 + a];
  }
  if constexpr (MERGE) {
    int head, tail;
    vx_run(r >= 0 ? (uint64_t)r : VX_EMPTY, lane, head, tail);
    const auto add = [](auto p, auto q) { return p + q; };
    const auto mn = [](int p, int q) { return min(p, q); };
    const auto mx = [](int p, int q) { return max(p, q); };
    n = wave_scan(n, lane, head, add);
    pts = wave_scan(pts, lane, head, add);
    int l[3], h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { l[a] = wave_scan(c[a], lane, head, mn); h[a] = wave_scan(c[a], lane, head, mx); }
    if (r >= 0 && lane == tail) {
      atomicAdd(&size[r], n);
      atomicAdd(&points[r], (unsigned long long)pts);
#pragma unroll
      for (int a = 0; a < 3; ++a) { atomicMin(&lo[(int64_t)r * 3 + a], l[a]); atomicMax(&hi[(int64_t)r * 3 + a], h[a]); }
    }
  } else if (r >= 0) {
    atomicAdd(&size[r], 1);
    atomicAdd(&points[r], (unsigned long long)pts);
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&lo[(int64_t)r * 3 + a], c[a]); atomicMax(&hi[(int64_t)r * 3 + a], c[a]); }
  }
}

// bit k = row i0 + k is the root of a component
__device__ __forceinline__ int cc_root_mask(const int32_t* __restrict__ root, int Mv, int i0) {
  int m = 0;
#pragma unroll
  for (int k = 0; k < CC_PT; ++k)
    if (i0 + k < Mv && root[i0 + k] == i0 + k) m |= 1 << k;
  return m;
}

__global__ __launch_bounds__(CC_T) void vcc_count_kernel(const int32_t* __restrict__ root, int Mv, int32_t* __restrict__ counts) {
  __shared__ int wtot[CC_T / 64];
  int total;
  wg_rank<CC_T, CC_PT>(cc_root_mask(root, Mv, blockIdx.x * CC_WG + threadIdx.x * CC_PT), wtot, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// rank of every root = workgroup base + wave base + lane prefix (ranks follow the rows) -> rank_of[row] and the component's row of the table
__global__ __launch_bounds__(CC_T) void vcc_rank_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ pan, int Mv, const int32_t* __restrict__ base,
                                                        const int32_t* __restrict__ size, const int64_t* __restrict__ points, const int32_t* __restrict__ lo,
                                                        const int32_t* __restrict__ hi, int32_t* __restrict__ rank_of, int32_t* __restrict__ t_root,
                                                        int32_t* __restrict__ t_pan, int32_t* __restrict__ t_size, int64_t* __restrict__ t_points,
                                                        int32_t* __restrict__ t_lo, int32_t* __restrict__ t_hi) {
  __shared__ int wtot[CC_T / 64];
  const int tid = threadIdx.x, i0 = blockIdx.x * CC_WG + tid * CC_PT;
  const int m = cc_root_mask(root, Mv, i0);
  int total;
  int r = base[blockIdx.x] + wg_rank<CC_T, CC_PT>(m, wtot, total);
#pragma unroll
  for (int k = 0; k < CC_PT; ++k)
    if ((m >> k) & 1) {
      const int v = i0 + k;
      rank_of[v] = r;
      t_root[r] = v; t_pan[r] = pan[v]; t_size[r] = size[v]; t_points[r] = points[v];
#pragma unroll
      for (int a = 0; a < 3; ++a) { t_lo[(int64_t)r * 3 + a] = lo[(int64_t)v * 3 + a]; t_hi[(int64_t)r * 3 + a] = hi[(int64_t)v * 3 + a]; }
      ++r;
    }
}

__global__ __launch_bounds__(CC_T) void vcc_component_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ rank_of, int Mv,
                                                             int32_t* __restrict__ component) {
  const int v = blockIdx.x * CC_T + threadIdx.x;
  if (v >= Mv) return;
  const int r = root[v];
  component[v] = r >= 0 ? rank_of[r] : -1;
}

__global__ __launch_bounds__(CC_T) void vcc_votes_kernel(const int32_t* __restrict__ cells, const int32_t* __restrict__ pan, const int32_t* __restrict__ root,
                                                         const int32_t* __restrict__ size, int Mv, const uint64_t* __restrict__ keys,
                                                         const int32_t* __restrict__ rows, uint32_t mask, int max_axes, int min_voxels,
                                                         uint64_t* __restrict__ pkeys, int32_t* __restrict__ pcnt, uint32_t pmask, int32_t* __restrict__ status) {
  const int v = blockIdx.x * CC_T + threadIdx.x;
  if (v >= Mv) return;
  const int r = root[v];
  if (r < 0 || size[r] >= min_voxels) return;                       // void, or a component that stays
  const int x = cells[(int64_t)v * 3], y = cells[(int64_t)v * 3 + 1], z = cells[(int64_t)v * 3 + 2];
  if (!vx_in_range(x, y, z)) return;
  for (int k = 0; k < 27; ++k) {
    int dx, dy, dz;
    const int axes = cc_offset(k, dx, dy, dz);
    if (axes == 0 || axes > max_axes) continue;
    if (!vx_in_range(x + dx, y + dy, z + dz)) continue;
    const int n = cc_lookup(keys, rows, mask, vx_key(x + dx, y + dy, z + dz), status);
    if (n < 0) continue;
    const int id = pan[n], rn = root[n];
    if (id <= 0 || rn < 0 || size[rn] < min_voxels) continue;       // void and small neighbours do not vote
    const int s = vx_find_or_claim(pkeys, pmask, ((uint64_t)(uint32_t)r << 32) | (uint32_t)id, status);
    if (s >= 0) atomicAdd(&pcnt[s], 1);
  }
}

__global__ __launch_bounds__(CC_T) void vcc_apply_kernel(const int32_t* __restrict__ pan, const int32_t* __restrict__ root, const int32_t* __restrict__ size,
                                                         const unsigned long long* __restrict__ best, int Mv, int min_voxels, const float* __restrict__ rgb,
                                                         const float* __restrict__ colors, int ncolors, float w1, float w2, int32_t* __restrict__ out_pan,
                                                         float* __restrict__ out_colors, int32_t* __restrict__ status) {
  const int v = blockIdx.x * CC_T + threadIdx.x;
  int id = 0;
  bool small = false;
  if (v < Mv) {
    id = pan[v];
    const int r = root[v];
    small = r >= 0 && size[r] < min_voxels;
    if (small) {
      const unsigned long long b = best[r];
      id = b ? (int)(0xFFFFFFFFu - (uint32_t)b) : 0;                // no vote: a floater, void
    }
    const bool known = id > 0 && id < ncolors;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      out_colors[(int64_t)v * 3 + a] = rn_add(rn_mul(w1, rgb[(int64_t)v * 3 + a]), rn_mul(w2, known ? colors[id * 3 + a] : 0.f));
    out_pan[v] = id;
  }
  wave_count_add(small && id > 0, &status[1]);                      // moved
  wave_count_add(small && id == 0, &status[2]);                     // gone
}

static bool cc_pow2(int64_t cap) { return cap >= 2 && cap <= (1ll << 31) && (cap & (cap - 1)) == 0; }
static int cc_axes(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }
constexpr int64_t CC_MAX_ROWS = 0x3fffffffLL;

}  // namespace pst

extern "C" int pst_vcc_cells(const float* points, const int32_t* first_row, const int32_t* mv_ptr, int64_t max_voxels, float inv, int32_t* cells, void* stream) {
  using namespace pst;
  if (!points || !first_row || !mv_ptr || !cells || max_voxels <= 0 || max_voxels > CC_MAX_ROWS || !(inv > 0.f)) {
    set_error("vcc_cells: bad shape (max_voxels=%lld), inverse voxel size or null operand", (long long)max_voxels); return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_cells_kernel, blocks_for(max_voxels, CC_T), dim3(CC_T), 0, (hipStream_t)stream, points, first_row, mv_ptr, inv, cells);
  return check_launch("vcc_cells");
}

extern "C" int pst_vcc_build(const int32_t* cells, const int32_t* pan, int64_t Mv, uint64_t* keys, int32_t* rows, int64_t capacity, int32_t* parent,
                             int32_t* status, void* stream) {
  using namespace pst;
  if (!cells || !pan || !keys || !rows || !parent || !status) { set_error("vcc_build: null operand"); return PST_EINVAL; }
  if (Mv <= 0 || Mv > CC_MAX_ROWS || !vx_cap_ok(Mv, capacity)) {
    set_error("vcc_build: bad shape (Mv=%lld, capacity=%lld: a power of two >= 2 Mv)", (long long)Mv, (long long)capacity); return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_build_kernel, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, cells, pan, (int)Mv, keys, rows, (uint32_t)(capacity - 1), parent, status);
  return check_launch("vcc_build");
}

extern "C" int pst_vcc_link(const int32_t* cells, const int32_t* pan, int64_t Mv, const uint64_t* keys, const int32_t* rows, int64_t capacity, int connectivity,
                            int32_t* parent, int32_t* status, void* stream) {
  using namespace pst;
  if (!cells || !pan || !keys || !rows || !parent || !status) { set_error("vcc_link: null operand"); return PST_EINVAL; }
  if (Mv <= 0 || Mv > CC_MAX_ROWS || !vx_cap_ok(Mv, capacity) || !cc_axes(connectivity)) {
    set_error("vcc_link: bad shape (Mv=%lld, capacity=%lld) or connectivity %d (6, 18 or 26)", (long long)Mv, (long long)capacity, connectivity); return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_link_kernel, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, cells, pan, (int)Mv, keys, rows, (uint32_t)(capacity - 1),
                     cc_axes(connectivity), parent, status);
  return check_launch("vcc_link");
}

extern "C" int pst_vcc_flatten(const int32_t* parent, const int32_t* count, const int32_t* cells, int64_t Mv, int32_t* root, int32_t* size, int64_t* points,
                               int32_t* cell_lo, int32_t* cell_hi, int32_t* status, int merge, void* stream) {
  using namespace pst;
  if (!parent || !count || !cells || !root || !size || !points || !cell_lo || !cell_hi || !status || Mv <= 0 || Mv > CC_MAX_ROWS) {
    set_error("vcc_flatten: bad shape (Mv=%lld) or null operand", (long long)Mv); return PST_EINVAL;
  }
  if (merge) hipLaunchKernelGGL(vcc_flatten_kernel<true>, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, parent, count, cells, (int)Mv, root, size,
                                (unsigned long long*)points, cell_lo, cell_hi, status);
  else hipLaunchKernelGGL(vcc_flatten_kernel<false>, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, parent, count, cells, (int)Mv, root, size,
                          (unsigned long long*)points, cell_lo, cell_hi, status);
  return check_launch("vcc_flatten");
}

extern "C" int pst_vcc_count(const int32_t* root, int64_t Mv, int32_t* counts, void* stream) {
  using namespace pst;
  if (!root || !counts || Mv <= 0 || Mv > CC_MAX_ROWS) { set_error("vcc_count: bad shape / null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(vcc_count_kernel, blocks_for(Mv, CC_WG), dim3(CC_T), 0, (hipStream_t)stream, root, (int)Mv, counts);
  return check_launch("vcc_count");
}

extern "C" int pst_vcc_rank(const int32_t* root, const int32_t* pan, int64_t Mv, const int32_t* base, const int32_t* size, const int64_t* points,
                            const int32_t* cell_lo, const int32_t* cell_hi, int32_t* rank_of, int32_t* component, int32_t* t_root, int32_t* t_pan,
                            int32_t* t_size, int64_t* t_points, int32_t* t_lo, int32_t* t_hi, void* stream) {
  using namespace pst;
  if (!root || !pan || !base || !size || !points || !cell_lo || !cell_hi || !rank_of || !component || !t_root || !t_pan || !t_size || !t_points || !t_lo || !t_hi ||
      Mv <= 0 || Mv > CC_MAX_ROWS) {
    set_error("vcc_rank: bad shape / null operand"); return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_rank_kernel, blocks_for(Mv, CC_WG), dim3(CC_T), 0, (hipStream_t)stream, root, pan, (int)Mv, base, size, points, cell_lo,
                     cell_hi, rank_of, t_root, t_pan, t_size, t_points, t_lo, t_hi);
  const int rc = check_launch("vcc_rank");
  if (rc) return rc;
  hipLaunchKernelGGL(vcc_component_kernel, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, root, rank_of, (int)Mv, component);
  return check_launch("vcc_rank (component)");
}

extern "C" int pst_vcc_votes(const int32_t* cells, const int32_t* pan, const int32_t* root, const int32_t* size, int64_t Mv, const uint64_t* keys,
                             const int32_t* rows, int64_t capacity, int connectivity, int min_voxels, uint64_t* pair_keys, int32_t* pair_cnt,
                             int64_t pair_capacity, int32_t* status, void* stream) {
  using namespace pst;
  if (!cells || !pan || !root || !size || !keys || !rows || !pair_keys || !pair_cnt || !status) { set_error("vcc_votes: null operand"); return PST_EINVAL; }
  if (Mv <= 0 || Mv > CC_MAX_ROWS || !vx_cap_ok(Mv, capacity) || !cc_pow2(pair_capacity) || !cc_axes(connectivity) || min_voxels < 1) {
    set_error("vcc_votes: bad shape (Mv=%lld, capacity=%lld, pair_capacity=%lld), connectivity %d or min_voxels %d", (long long)Mv, (long long)capacity,
              (long long)pair_capacity, connectivity, min_voxels);
    return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_votes_kernel, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, cells, pan, root, size, (int)Mv, keys, rows, (uint32_t)(capacity - 1),
                     cc_axes(connectivity), min_voxels, pair_keys, pair_cnt, (uint32_t)(pair_capacity - 1), status);
  return check_launch("vcc_votes");
}

extern "C" int pst_vcc_apply(const int32_t* pan, const int32_t* root, const int32_t* size, const uint64_t* best, int64_t Mv, int min_voxels, const float* rgb,
                             const float* colors, int ncolors, float w1, float w2, int32_t* out_pan, float* out_colors, int32_t* status, void* stream) {
  using namespace pst;
  if (!pan || !root || !size || !best || !rgb || !colors || !out_pan || !out_colors || !status) { set_error("vcc_apply: null operand"); return PST_EINVAL; }
  if (Mv <= 0 || Mv > CC_MAX_ROWS || min_voxels < 1 || ncolors < 1 || ncolors > CC_MAX_COLORS) {
    set_error("vcc_apply: bad shape (Mv=%lld, ncolors=%d) or min_voxels %d", (long long)Mv, ncolors, min_voxels); return PST_EINVAL;
  }
  hipLaunchKernelGGL(vcc_apply_kernel, blocks_for(Mv, CC_T), dim3(CC_T), 0, (hipStream_t)stream, pan, root, size, (const unsigned long long*)best, (int)Mv, min_voxels, rgb,
                     colors, ncolors, w1, w2, out_pan, out_colors, status);
  return check_launch("vcc_apply");
}
