// What the two fused ICP steps share (icp_step of csrc/nearest.hip, point to point; icp_plane_step of csrc/meshdist.hip, point to plane), written
// once: the 3 x 4 fp32 matrix that moves a source point (step 1 of the icp section of include/panst3r_hip.h; the move is pinhole.h's affine34) and the fixed order in which the
// fp64 moments are added (step 4 of that section): the butterfly inside a wave, the four waves in order, one row per block, and the one-block
// reducer over the rows.  Templated on the number of live moments, so that both files instantiate the same text.  The sums set
// `fp contract(off)` for themselves, the move is rn_* throughout: every operation is rounded on its own, in the order written, whoever includes this header.
#pragma once
#include "pinhole.h"             // affine34, the move of the two steps; and through it common.h and include/panst3r_hip.h

namespace pst {

constexpr int ICP_T = PST_ICP_LANES;                                // lanes per block of a step and of its reducer
constexpr int ICP_ROWS = PST_ICP_CHUNK / ICP_T;                     // source rows per lane
static_assert(ICP_T == 256 && PST_ICP_CHUNK % ICP_T == 0, "four waves of 64 lanes, whole rows per lane: the fixed order of the header");

struct IcpMatrix { float a[3][4]; };                               // row-major 3 x 4: a source row is moved by affine34(&A.a[0][0], x, m)

// six butterfly steps inside every wave, then ((w0 + w1) + w2) + w3 -> row[0, LIVE); row[LIVE, MOMENTS) = +0.0.  Every lane of the block calls it.
template <int LIVE, int MOMENTS>
__device__ __forceinline__ void icp_block_sum(const double (&acc)[LIVE], double* __restrict__ row) {
#pragma clang fp contract(off)
  static_assert(LIVE <= MOMENTS && MOMENTS <= ICP_T, "one lane per moment writes the row");
  __shared__ double waves[ICP_T / 64][LIVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < LIVE; ++s) {
    double v = acc[s];
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v += __shfl_xor(v, k);
    if (lane == 0) waves[wave][s] = v;
  }
  __syncthreads();
  const int s = threadIdx.x;
  if (s < LIVE) row[s] = ((waves[0][s] + waves[1][s]) + waves[2][s]) + waves[3][s];
  else if (s < MOMENTS) row[s] = 0.0;
}

// one block; lane l adds the rows l, l + 256, ... of the partials in ascending order, then the same butterfly and the same wave order
template <int LIVE, int MOMENTS>
__global__ __launch_bounds__(ICP_T) void icp_reduce_kernel(const double* __restrict__ partials, int P, double* __restrict__ out) {
#pragma clang fp contract(off)
  double acc[LIVE];
#pragma unroll
  for (int s = 0; s < LIVE; ++s) acc[s] = 0.0;
  for (int r = threadIdx.x; r < P; r += ICP_T)
#pragma unroll
    for (int s = 0; s < LIVE; ++s) acc[s] += partials[(int64_t)r * MOMENTS + s];
  icp_block_sum<LIVE, MOMENTS>(acc, out);
}

}  // namespace pst
