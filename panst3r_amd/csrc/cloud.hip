// The labelled 3-D panoptic point cloud of a scene (reference tools/demo_panst3r.py:279-300 and ViserVisualizer.show_pointcloud :622-687, which
// build it on the host in numpy; restated in tests/cloud_ref.py, [restated, parity unpinned]).  Four steps on tensors that already sit on the device:
//   count     one pass over the conf planes of ALL views (a device table of per-view pointers makes a mixed-shape scene one launch): a
//             workgroup of 256 threads covers 1024 consecutive points of one view (a 16-byte load per thread), ballots conf >= thr, writes its count
//   scan      exclusive prefix sum of the workgroup counts by one workgroup -> every workgroup's output base, M at the end
//   compact   second pass, stable: slot = workgroup base + wave base + mbcnt of the ballots.  Per kept point: pts3d, pts3d_local (moved to the
//             world frame), rgb, pan, blended colour, scene index.  Every output is staged through LDS in slot order, so the global stores are
//             contiguous runs and not 64 scattered 12-byte rows.
//   median    exact per-segment, per-axis median of points_local by radix select on the order-preserving key of a float, most significant byte
//             first, four passes: LDS histograms flushed with INTEGER atomics (order-independent), then a small kernel that narrows the ranks
//             (radix_select.h, shared with csrc/depth_eval.hip).
// The arithmetic of compact is part of the contract (every product and every sum rounded on its own; the move of points_local is pinhole.h's
// affine34, the workgroup -> view lookup its view_of, both shared with csrc/consistency.hip): contraction is off for the whole file.
// No float atomics, every result written with plain vector stores.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "pinhole.h"             // affine34, view_of, PH_VIEW_WG; and through it wave_ops.h: rn_mul, rn_add, wg_rank, wave_scan
#include "radix_select.h"        // the median's select: keys, tally, flush, the narrow kernel and the loop over the four passes

#pragma clang fp contract(off)

namespace pst {

constexpr int CL_T = 256, CL_PT = 4, CL_WG = CL_T * CL_PT;        // threads, points per thread, points per workgroup
static_assert(CL_WG == PH_VIEW_WG, "first_wg of a pst_cloud_view table counts workgroups of this many points");
constexpr int CL_MAX_COLORS = 4096;                               // colour table rows that fit in LDS next to the staging buffer (48 + 12 KiB)
constexpr int MD_SB = 8;                                          // segments per workgroup of the histogram pass: 8 x 3 axes x 2 ranks x 256 counters = 48 KiB
constexpr int MD_SLICE = 32768;                                   // points per workgroup of the histogram pass
constexpr int MD_ROW = 3 * RS_SLOT;                               // counters per segment: one select slot per axis

// bit k = point i0 + k exists and conf >= thr (a NaN confidence is dropped, as `conf >= thr` drops it in numpy)
__device__ __forceinline__ int keep_mask(const float* __restrict__ conf, int npix, int i0, float thr) {
  int m = 0;
  if (i0 + 3 < npix && (((uintptr_t)conf) & 15) == 0) {
    const float4 c = *(const float4*)(conf + i0);
    m = (c.x >= thr ? 1 : 0) | (c.y >= thr ? 2 : 0) | (c.z >= thr ? 4 : 0) | (c.w >= thr ? 8 : 0);
  } else {
#pragma unroll
    for (int k = 0; k < CL_PT; ++k)
      if (i0 + k < npix && conf[i0 + k] >= thr) m |= 1 << k;
  }
  return m;
}

__global__ __launch_bounds__(CL_T) void cloud_count_kernel(const pst_cloud_view* __restrict__ views, int nviews, float thr, int32_t* __restrict__ counts) {
  __shared__ int wtot[CL_T / 64];
  const int wg = blockIdx.x;
  const pst_cloud_view& v = views[view_of(views, nviews, wg)];
  const int i0 = (wg - v.first_wg) * CL_WG + threadIdx.x * CL_PT;
  int total;
  wg_rank<CL_T, CL_PT>(keep_mask(v.conf, v.npix, i0, thr), wtot, total);
  if (threadIdx.x == 0) counts[wg] = total;
}

// base[i] = counts[0] + ... + counts[i - 1], base[n] = M.  One workgroup of 1024 threads, 1024 counts per round with a running carry.
__global__ __launch_bounds__(1024) void cloud_scan_kernel(const int32_t* __restrict__ counts, int n, int32_t* __restrict__ base) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += 1024) {
    const int i = r0 + tid;
    const int c = i < n ? counts[i] : 0;
    const int s = wave_scan(c, lane);
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    int wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int t = wsum[w];
      if (w < wave) wbase += t;
      tot += t;
    }
    const int carry = carry_s;
    if (i < n) base[i] = carry + wbase + s - c;
    __syncthreads();                             // every thread has read carry_s and wsum
    if (tid == 0) carry_s = carry + tot;
    __syncthreads();
  }
  if (tid == 0) base[n] = carry_s;
}

// rows of DW dwords, one per kept point, through LDS in slot order and out as one contiguous run
template <int DW>
__device__ __forceinline__ void stage_out(uint32_t* stage, const uint32_t (&val)[CL_PT][DW], int m, int slot, int cnt, uint32_t* __restrict__ out) {
  int s = slot;
#pragma unroll
  for (int k = 0; k < CL_PT; ++k)
    if ((m >> k) & 1) {
#pragma unroll
      for (int d = 0; d < DW; ++d) stage[s * DW + d] = val[k][d];
      ++s;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < cnt * DW; i += CL_T) out[i] = stage[i];
  __syncthreads();
}

__global__ __launch_bounds__(CL_T) void cloud_compact_kernel(const pst_cloud_view* __restrict__ views, int nviews, float thr, const int32_t* __restrict__ base,
                                                             const float* __restrict__ colors, int ncolors, float w1, float w2,
                                                             float* __restrict__ points, float* __restrict__ points_local, float* __restrict__ rgb,
                                                             int32_t* __restrict__ pan_out, float* __restrict__ col_out, int64_t* __restrict__ index) {
  extern __shared__ float ctab[];                                  // [ncolors][3]
  __shared__ uint32_t stage[CL_WG * 3];
  __shared__ int wtot[CL_T / 64];
  const int wg = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = base[wg];
  const int cnt = base[wg + 1] - (int)b0;
  if (cnt == 0) return;                                            // uniform
  for (int i = tid; i < ncolors * 3; i += CL_T) ctab[i] = colors[i];
  const pst_cloud_view& v = views[view_of(views, nviews, wg)];
  const int npix = v.npix;
  const int i0 = (wg - v.first_wg) * CL_WG + tid * CL_PT;
  const int m = keep_mask(v.conf, npix, i0, thr);
  int total;
  const int slot = wg_rank<CL_T, CL_PT>(m, wtot, total);           // its barrier also publishes the colour table in LDS

  float R[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) R[j] = v.c2w[j];
  uint32_t val[CL_PT][3];

  // points (pts3d as it is)
#pragma unroll
  for (int k = 0; k < CL_PT; ++k)
    if ((m >> k) & 1) {
      const uint32_t* p = (const uint32_t*)(v.pts3d + (int64_t)(i0 + k) * 3);
      val[k][0] = p[0]; val[k][1] = p[1]; val[k][2] = p[2];
    }
  stage_out<3>(stage, val, m, slot, cnt, (uint32_t*)(points + b0 * 3));

  // points_local in the world frame: pinhole.h's move by c2w
#pragma unroll
  for (int k = 0; k < CL_PT; ++k)
    if ((m >> k) & 1) {
      const float* p = v.pts3d_local + (int64_t)(i0 + k) * 3;
      float w[3], x[3] = {p[0], p[1], p[2]};
      affine34(R, x, w);
      val[k][0] = __float_as_uint(w[0]); val[k][1] = __float_as_uint(w[1]); val[k][2] = __float_as_uint(w[2]);
    }
  stage_out<3>(stage, val, m, slot, cnt, (uint32_t*)(points_local + b0 * 3));

  // rgb = img * 0.5 + 0.5 (HWC order from the three planes), colour = w1 rgb + w2 pan_vis
  uint32_t cval[CL_PT][3], pval[CL_PT][1];
#pragma unroll
  for (int k = 0; k < CL_PT; ++k)
    if ((m >> k) & 1) {
      const int p = v.pan[i0 + k];
      pval[k][0] = (uint32_t)p;
      const bool known = p > 0 && p < ncolors;                    // void (0) and ids outside the table are black; the table is never indexed with them
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float g = rn_add(rn_mul(v.img[(int64_t)c * npix + i0 + k], 0.5f), 0.5f);
        const float pv = known ? ctab[p * 3 + c] : 0.f;
        val[k][c] = __float_as_uint(g);
        cval[k][c] = __float_as_uint(rn_add(rn_mul(w1, g), rn_mul(w2, pv)));
      }
    }
  stage_out<3>(stage, val, m, slot, cnt, (uint32_t*)(rgb + b0 * 3));
  stage_out<3>(stage, cval, m, slot, cnt, (uint32_t*)(col_out + b0 * 3));
  stage_out<1>(stage, pval, m, slot, cnt, (uint32_t*)(pan_out + b0));

  uint32_t ival[CL_PT][2];
#pragma unroll
  for (int k = 0; k < CL_PT; ++k) {
    const uint64_t g = (uint64_t)(v.offset + i0 + k);
    ival[k][0] = (uint32_t)g; ival[k][1] = (uint32_t)(g >> 32);
  }
  stage_out<2>(stage, ival, m, slot, cnt, (uint32_t*)(index + b0));
}

// ---------------------------------------------------------------- per-segment median (the select itself: radix_select.h, signed keys, groups of 3)
// grid (point slices, segment blocks).  A workgroup takes MD_SLICE points and the MD_SB segment rows [MD_SB blockIdx.y, ...): it reads pan for every
// point and the coordinates of its own segments' points only, tallies each into the slot of its (segment, axis) and, in pass 0, counts the NaNs.
__global__ __launch_bounds__(CL_T) void median_hist_kernel(const float* __restrict__ pts, const int32_t* __restrict__ pan, const int32_t* __restrict__ m_ptr,
                                                           const int32_t* __restrict__ id2row, int ntab, int S, int pass, const uint32_t* __restrict__ prefix,
                                                           int32_t* __restrict__ hist, int32_t* __restrict__ nan_cnt) {
  __shared__ int h[MD_SB * MD_ROW];
  __shared__ int nn[MD_SB * 3];
  __shared__ uint32_t pre[MD_SB * 6];
  const int M = *m_ptr;
  const int64_t p0 = (int64_t)blockIdx.x * MD_SLICE;
  if (p0 >= M) return;
  const int p1 = (int)min((int64_t)M, p0 + MD_SLICE);
  const int row0 = blockIdx.y * MD_SB, nrow = min(MD_SB, S - row0);
  const int tid = threadIdx.x;
  for (int i = tid; i < MD_SB * MD_ROW; i += CL_T) h[i] = 0;
  if (tid < MD_SB * 3) nn[tid] = 0;
  if (tid < MD_SB * 6) pre[tid] = tid < nrow * 6 ? prefix[row0 * 6 + tid] : 0u;
  __syncthreads();
  for (int i = (int)p0 + tid; i < p1; i += CL_T) {
    const int id = pan[i];
    if (id <= 0 || id >= ntab) continue;                           // void, or an id outside the table: never used as an index
    const int r = id2row[id] - row0;
    if (r < 0 || r >= nrow) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t u = __float_as_uint(pts[(int64_t)i * 3 + a]);
      if (pass == 0) {                                             // the NaN count shares the tally's (uniform) branch on the pass
        select_tally(h, pre, r * 3 + a, select_key<true>(u), 0);
        if ((u & 0x7fffffffu) > 0x7f800000u) atomicAdd(&nn[r * 3 + a], 1);
      } else select_tally(h, pre, r * 3 + a, select_key<true>(u), pass);
    }
  }
  __syncthreads();
  select_flush<CL_T>(h, nrow * MD_ROW, hist + (int64_t)row0 * MD_ROW);
  if (pass == 0 && tid < nrow * 3 && nn[tid]) atomicAdd(&nan_cnt[row0 * 3 + tid], nn[tid]);
}

}  // namespace pst

static int cloud_views_ok(const char* what, const void* views, int nviews, int nwg) {
  using namespace pst;
  if (!views || nviews <= 0 || nwg <= 0) { set_error("%s: bad shape / null operand", what); return PST_EINVAL; }
  return 0;
}

extern "C" int pst_cloud_count(const pst_cloud_view* views, int nviews, int nwg, float thr, int32_t* counts, void* stream) {
  using namespace pst;
  if (cloud_views_ok("cloud_count", views, nviews, nwg) || !counts) { set_error("cloud_count: bad shape / null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(cloud_count_kernel, dim3((unsigned)nwg), dim3(CL_T), 0, (hipStream_t)stream, views, nviews, thr, counts);
  return check_launch("cloud_count");
}

extern "C" int pst_cloud_scan(const int32_t* counts, int n, int32_t* base, void* stream) {
  using namespace pst;
  if (!counts || !base || n <= 0) { set_error("cloud_scan: bad shape / null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, n, base);
  return check_launch("cloud_scan");
}

extern "C" int pst_cloud_compact(const pst_cloud_view* views, int nviews, int nwg, float thr, const int32_t* base, const float* colors, int ncolors, float w1,
                                 float w2, float* points, float* points_local, float* rgb, int32_t* pan, float* colors_out, int64_t* index, void* stream) {
  using namespace pst;
  if (cloud_views_ok("cloud_compact", views, nviews, nwg) || !base || !colors || !points || !points_local || !rgb || !pan || !colors_out || !index) {
    set_error("cloud_compact: bad shape / null operand"); return PST_EINVAL;
  }
  if (ncolors < 1 || ncolors > CL_MAX_COLORS) { set_error("cloud_compact: colour table of %d rows outside [1, %d]", ncolors, CL_MAX_COLORS); return PST_EINVAL; }
  hipLaunchKernelGGL(cloud_compact_kernel, dim3((unsigned)nwg), dim3(CL_T), (size_t)ncolors * 12, (hipStream_t)stream, views, nviews, thr, base, colors, ncolors,
                     w1, w2, points, points_local, rgb, pan, colors_out, index);
  return check_launch("cloud_compact");
}

extern "C" int pst_cloud_segment_median(const float* points_local, const int32_t* pan, const int32_t* m_ptr, int64_t max_points, const int32_t* id2row, int ntab,
                                        int nseg, int32_t* hist, uint32_t* prefix, int32_t* rank, int32_t* nan_cnt, int32_t* count, float* median,
                                        void* stream) {
  using namespace pst;
  if (!points_local || !pan || !m_ptr || !id2row || !hist || !prefix || !rank || !nan_cnt || !count || !median) {
    set_error("cloud_segment_median: null operand"); return PST_EINVAL;
  }
  if (max_points <= 0 || max_points > 0x7fffffffLL || ntab < 1 || nseg < 1 || nseg > 65535 * MD_SB) {
    set_error("cloud_segment_median: bad shape (max_points=%lld, ntab=%d, nseg=%d)", (long long)max_points, ntab, nseg); return PST_EINVAL;
  }
  if (((uintptr_t)hist) & 15) { set_error("cloud_segment_median: the histogram workspace must be 16-byte aligned"); return PST_EINVAL; }
  const dim3 grid((unsigned)((max_points + MD_SLICE - 1) / MD_SLICE), (unsigned)((nseg + MD_SB - 1) / MD_SB));
  hipStream_t st = (hipStream_t)stream;
  return select_passes<true, 3>("cloud_segment_median (histogram)", "cloud_segment_median (narrow)", [&](int pass) {
    hipLaunchKernelGGL(median_hist_kernel, grid, dim3(CL_T), 0, st, points_local, pan, m_ptr, id2row, ntab, nseg, pass, prefix, hist, nan_cnt);
  }, nseg, hist, prefix, rank, nan_cnt, count, median, st);
}
