// The small device helpers of the geometry stages (csrc/cloud.hip, voxel.hip, components.hip, surface.hip, render.hip, mesh.hip, evaluate.hip,
// nearest.hip, meshdist.hip; voxel_table.h and pinhole.h include it for their users), written once: separately rounded fp32 operations, the stable rank of a lane's
// kept items inside its wave and its workgroup, the inclusive wave scan (plain and segmented), the runs of equal keys inside a wave, one atomic per
// wave for a count of flagged lanes, the integer wave sum, and two table lookups.  Integer code but for the rn_* operations, which set
// `fp contract(off)` for themselves: whoever includes this header, and with whatever flags, each of them is rounded on its own.
// A workgroup is one-dimensional and a whole number of 64-lane waves: lane = threadIdx.x & 63, wave = threadIdx.x >> 6.
// Left out on purpose: pq_count_kernel (csrc/evaluate.hip) keeps its own run heads - they depend on `uniform` of this lane and of the one below as
// well as on the key, and an 8-byte composite key for vx_run read no simpler; icp_block_sum (icp_sum.h) keeps its fp64 order, which is contract.
#pragma once
#include "common.h"

namespace pst {

// ---------------------------------------------------------------- separately rounded fp32 operations
// product, sum and difference that no multiply-add can be formed from: the pragma stands inside each function (the HIP header's __fmul_rn /
// __fadd_rn are plain operators compiled under the default contraction and DO fuse after inlining)
__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
// the contracts' quotient: fp64 division rounded once to fp32.  (For two fp32 operands that IS the correctly rounded fp32 quotient - 53 >= 2 x 24 + 2
// bits make the double rounding innocuous - and numpy's float32 division gives the same.  hipcc does narrow it: the gfx950 code holds, per quotient,
// v_div_scale_f32 x2 / v_rcp_f32 / five fma / v_div_fmas_f32 / v_div_fixup_f32, the IEEE expansion, with fp32 denormals on (float_denorm_mode_32 = 3)
// and no fast-math flag in the build - the same value by either route, which is why the contracts can name the fp64 form.)
__device__ __forceinline__ float rn_div(float a, float b) { return (float)((double)a / (double)b); }

// ---------------------------------------------------------------- stable ranks
// bit k of `mask` = this lane holds its k-th item (PT items per lane, in lane order) -> the items of the lower lanes of this wave, one ballot per
// bit, and the wave's total.  Every lane of the wave must call it.
template <int PT>
__device__ __forceinline__ int lane_rank(int mask, int& wave_total) {
  int pre = 0;
  wave_total = 0;
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    const uint64_t b = __ballot((mask >> k) & 1);
    pre += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0));
    wave_total += __popcll(b);
  }
  return pre;
}

// the same inside a workgroup of T threads: the items of every lower thread (= the slot of this lane's first item) and the workgroup's total.
// wtot = T / 64 ints of LDS.  Holds ONE __syncthreads(): every lane of the workgroup must call it, and what the workgroup wrote to LDS before the
// call is visible after it.
template <int T, int PT>
__device__ __forceinline__ int wg_rank(int mask, int* wtot, int& total) {
  static_assert(T % 64 == 0, "whole waves");
  int wave_total;
  int r = lane_rank<PT>(mask, wave_total);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wtot[wave] = wave_total;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) {
    const int t = wtot[w];
    if (w < wave) r += t;
    total += t;
  }
  return r;
}

// ---------------------------------------------------------------- scans, runs and sums over a wave.  Every lane of the wave must call them.
// segmented inclusive scan: op over the lanes [head, lane] of this lane's run (head as vx_run gives it): the run's last lane holds the run's total
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, int lane, int head, Op op) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane - o >= head) v = op(v, t);
  }
  return v;
}
// inclusive prefix sum over the wave
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
  return wave_scan(v, lane, 0, [](T a, T b) { return a + b; });
}

// lanes [head, tail] = the run of adjacent lanes that hold this lane's key
template <typename K>
__device__ __forceinline__ void vx_run(K key, int lane, int& head, int& tail) {
  const K prev = __shfl_up(key, 1);
  const uint64_t heads = __ballot(lane == 0 || prev != key);
  head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
  tail = above ? lane + __builtin_ctzll(above) : 63;
}

// *word += the number of lanes of this wave with `flag`: one atomic, issued by the first such lane, none without one
__device__ __forceinline__ void wave_count_add(bool flag, int32_t* word) {
  const int lane = threadIdx.x & 63;
  const uint64_t b = __ballot(flag);
  if (b && lane == (int)__builtin_ctzll(b)) atomicAdd(word, (int)__popcll(b));
}

// the sum of v over the wave, in every lane (integers: no order)
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---------------------------------------------------------------- table lookups
// the last entry i of [0, n) with first_of(i) <= x (first_of ascending, first_of(0) <= x): the view that owns a workgroup, the slab that owns a pixel
template <typename X, typename First>
__device__ __forceinline__ int last_le(int n, X x, First first_of) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first_of(mid) <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// id -> its row tab[id] in [0, n); `none` for void (id <= 0), an id outside the table (never used as an index) or an entry outside [0, n)
__device__ __forceinline__ int id_row(int id, const int32_t* __restrict__ tab, int ntab, int n, int none) {
  if (id <= 0 || id >= ntab) return none;
  const int r = tab[id];
  return (r >= 0 && r < n) ? r : none;
}

}  // namespace pst
