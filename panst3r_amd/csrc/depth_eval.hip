// Predicted depth maps scored against ground-truth depth maps (the depth-evaluation section of include/panst3r_hip.h; restated in
// tests/depth_eval_ref.py, [restated, parity unpinned]).  Three stages over one table of views, so that a mixed-shape scene is one launch per stage:
//   moments   n, sum p, sum g, sum pp, sum pg over the valid pixels of every slab: what a least-squares scale (and shift) is solved from on the host
//   median    the exact fp32 medians of p and of g per slab by radix select on the float's bits, most significant byte first, four passes: LDS
//             histograms flushed with INTEGER atomics (order-independent), then a one-wave kernel that narrows the two ranks (radix_select.h, shared with csrc/cloud.hip)
//   errors    with p' = s p + b in fp64: n, sum |d|/g, sum dd/g, sum dd, sum |d| and the inlier counts of up to four thresholds
// The fp64 sums are added in the fixed order of icp_sum.h: a block of 256 lanes per 4096 pixels of ONE view, lane l its pixels l, l + 256, ...; the
// butterfly, the four waves in order, one row of partials per block; then one reducer block per slab over the slab's rows.  No float atomics.
// Every operation is part of the contract: contraction is off for the whole file.
#include "icp_sum.h"             // icp_block_sum, ICP_T, ICP_ROWS; and through pinhole.h: common.h, wave_ops.h (last_le), include/panst3r_hip.h
#include "radix_select.h"        // the medians' select: keys, tally, flush, the narrow kernel and the loop over the four passes

#pragma clang fp contract(off)

namespace pst {

struct DepthView {                                                 // a row of the view table: PST_DEPTH_VIEW_WORDS int64 words
  const float* pred; int64_t stride; const float* gt; const float* conf; int64_t npix, first_block, slab, reserved;
};
static_assert(sizeof(DepthView) == 8 * PST_DEPTH_VIEW_WORDS, "the row the header writes out");
struct DepthThresholds { double t[4]; int K; };
constexpr int DE_MOMENTS = PST_DEPTH_MOMENTS, DE_ALIGN = 5, DE_ERR = 9;   // doubles per row; live moments of the two sum kernels
constexpr int DE_HIST = 2 * RS_SLOT;                               // counters per slab: one select slot for p, one for g

__device__ __forceinline__ const DepthView& depth_view_of(const DepthView* __restrict__ views, int nviews, int blk) {
  return views[last_le(nviews, (int64_t)blk, [&](int v) { return views[v].first_block; })];
}

// step 1.  finite: fabsf(x) <= PST_FMAX, so that a NaN fails it; every comparison is false for a NaN
__device__ __forceinline__ bool depth_valid(const DepthView& v, int64_t i, float lo, float hi, float thr, float& p, float& g) {
  g = v.gt[i];
  p = v.pred[i * v.stride];
  bool ok = fabsf(g) <= PST_FMAX && g > lo && g <= hi && fabsf(p) <= PST_FMAX && p > 0.f;
  if (v.conf) ok = ok && v.conf[i] >= thr;
  return ok;
}

// ERRORS = false: the moments of the alignment; true: the error sums under the slab's (s, b)
template <bool ERRORS>
__global__ __launch_bounds__(ICP_T) void depth_sum_kernel(const DepthView* __restrict__ views, int nviews, float lo, float hi, float thr,
                                                          const double* __restrict__ align, DepthThresholds th, double* __restrict__ partials) {
  constexpr int LIVE = ERRORS ? DE_ERR : DE_ALIGN;
  const int blk = blockIdx.x;
  const DepthView v = depth_view_of(views, nviews, blk);
  double s = 1.0, b = 0.0;
  if constexpr (ERRORS) { s = align[2 * v.slab]; b = align[2 * v.slab + 1]; }
  double acc[LIVE];
#pragma unroll
  for (int k = 0; k < LIVE; ++k) acc[k] = 0.0;
  const int64_t i0 = ((int64_t)blk - v.first_block) * PST_ICP_CHUNK + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < ICP_ROWS; ++j) {
    const int64_t i = i0 + (int64_t)j * ICP_T;
    float pf, gf;
    if (i >= v.npix || !depth_valid(v, i, lo, hi, thr, pf, gf)) continue;
    const double p = (double)pf, g = (double)gf;
    acc[0] += 1.0;
    if constexpr (!ERRORS) {
      acc[1] += p;
      acc[2] += g;
      acc[3] += p * p;
      acc[4] += p * g;
    } else {
      double pa = s * p;
      pa = pa + b;
      const double d = pa - g, ad = fabs(d), dd = d * d;
      acc[1] += ad / g;
      acc[2] += dd / g;
      acc[3] += dd;
      acc[4] += ad;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < th.K && pa < th.t[k] * g && g < th.t[k] * pa) acc[5 + k] += 1.0;
    }
  }
  icp_block_sum<LIVE, DE_MOMENTS>(acc, partials + (int64_t)blk * DE_MOMENTS);
}

// one block per slab; lane l adds the rows r0 + l, r0 + l + 256, ... of the slab's partials in ascending order, then the same butterfly and wave order
template <int LIVE>
__global__ __launch_bounds__(ICP_T) void depth_reduce_kernel(const double* __restrict__ partials, const int32_t* __restrict__ slab_rows, int nblocks,
                                                             double* __restrict__ out) {
  const int s = blockIdx.x;
  const int r0 = max(slab_rows[s], 0), r1 = min(slab_rows[s + 1], nblocks);
  double acc[LIVE];
#pragma unroll
  for (int k = 0; k < LIVE; ++k) acc[k] = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += ICP_T)
#pragma unroll
    for (int k = 0; k < LIVE; ++k) acc[k] += partials[(int64_t)r * DE_MOMENTS + k];
  icp_block_sum<LIVE, DE_MOMENTS>(acc, out + (int64_t)s * DE_MOMENTS);
}

// ---------------------------------------------------------------- medians (the select itself: radix_select.h, the raw bits as keys, groups of 2)
// One block per PST_ICP_CHUNK pixels of a view (the grid of the sums): tallies the bits of p and of g of every valid pixel into the slab's two slots.
__global__ __launch_bounds__(ICP_T) void depth_hist_kernel(const DepthView* __restrict__ views, int nviews, float lo, float hi, float thr, int pass,
                                                           const uint32_t* __restrict__ prefix, int32_t* __restrict__ hist) {
  __shared__ int h[DE_HIST];
  __shared__ uint32_t pre[4];
  const int blk = blockIdx.x, tid = threadIdx.x;
  const DepthView v = depth_view_of(views, nviews, blk);
  for (int i = tid; i < DE_HIST; i += ICP_T) h[i] = 0;
  if (tid < 4) pre[tid] = prefix[v.slab * 4 + tid];
  __syncthreads();
  const int64_t i0 = ((int64_t)blk - v.first_block) * PST_ICP_CHUNK + tid;
  for (int j = 0; j < ICP_ROWS; ++j) {
    const int64_t i = i0 + (int64_t)j * ICP_T;
    float pf, gf;
    if (i >= v.npix || !depth_valid(v, i, lo, hi, thr, pf, gf)) continue;
    const uint32_t u[2] = {__float_as_uint(pf), __float_as_uint(gf)};
#pragma unroll
    for (int q = 0; q < 2; ++q) select_tally(h, pre, q, select_key<false>(u[q]), pass);
  }
  __syncthreads();
  select_flush<ICP_T>(h, DE_HIST, hist + v.slab * DE_HIST);
}

}  // namespace pst

// the refusals that the host copy of the table decides (step 3 of the header's section)
static int depth_table_ok(const char* what, const int64_t* views, const int64_t* host, int nviews, int nblocks, int nslabs) {
  using namespace pst;
  if (!views || !host) { set_error("%s: null view table", what); return PST_EINVAL; }
  if (nviews < 1 || nslabs < 1 || nblocks < 1) { set_error("%s: bad shape (nviews=%d, nslabs=%d, nblocks=%d)", what, nviews, nslabs, nblocks); return PST_EINVAL; }
  int64_t blocks = 0, total = 0, slab = 0;
  for (int v = 0; v < nviews; ++v) {
    const int64_t* r = host + (int64_t)v * PST_DEPTH_VIEW_WORDS;
    if (!r[0] || !r[2]) { set_error("%s: view %d has a null pred or gt", what, v); return PST_EINVAL; }
    if (r[1] < 1) { set_error("%s: view %d has the stride %lld < 1", what, v, (long long)r[1]); return PST_EINVAL; }
    if (r[4] < 1 || r[4] > 0x7fffffffLL) { set_error("%s: view %d has %lld pixels", what, v, (long long)r[4]); return PST_EINVAL; }
    if (r[5] != blocks) { set_error("%s: view %d starts at block %lld, not %lld", what, v, (long long)r[5], (long long)blocks); return PST_EINVAL; }
    if (r[6] != slab && r[6] != slab + (v > 0 ? 1 : 0)) { set_error("%s: view %d is in slab %lld after slab %lld", what, v, (long long)r[6], (long long)slab); return PST_EINVAL; }
    slab = r[6];
    blocks += (r[4] + PST_ICP_CHUNK - 1) / PST_ICP_CHUNK;
    total += r[4];
  }
  if (slab != nslabs - 1) { set_error("%s: the table ends in slab %lld of %d", what, (long long)slab, nslabs); return PST_EINVAL; }
  if (total > 0x7fffffffLL) { set_error("%s: %lld pixels; one call takes at most 2^31 - 1", what, (long long)total); return PST_EINVAL; }
  if (blocks != nblocks) { set_error("%s: the table holds %lld blocks, not %d", what, (long long)blocks, nblocks); return PST_EINVAL; }
  return 0;
}

// the bit pattern of a valid g orders as its value only while g > 0: a negative (or NaN) lower bound would let negative depths through step 1
static int depth_bounds_ok(const char* what, float min_depth) {
  if (!(min_depth >= 0.f)) { pst::set_error("%s: min_depth %g; the lower bound is >= 0 (and no NaN)", what, (double)min_depth); return PST_EINVAL; }
  return 0;
}

extern "C" int pst_depth_median(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, int nslabs, float min_depth, float max_depth,
                                float conf_thr, int32_t* hist, uint32_t* prefix, int32_t* rank, int32_t* count, float* median, void* stream) {
  using namespace pst;
  if (depth_table_ok("depth_median", views, views_host, nviews, nblocks, nslabs)) return PST_EINVAL;
  if (depth_bounds_ok("depth_median", min_depth)) return PST_EINVAL;
  if (!hist || !prefix || !rank || !count || !median) { set_error("depth_median: null operand"); return PST_EINVAL; }
  if (((uintptr_t)hist) & 15) { set_error("depth_median: the histogram workspace must be 16-byte aligned"); return PST_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  return select_passes<false, 2>("depth_median (histogram)", "depth_median (narrow)", [&](int pass) {
    hipLaunchKernelGGL(depth_hist_kernel, dim3((unsigned)nblocks), dim3(ICP_T), 0, st, (const DepthView*)views, nviews, min_depth, max_depth, conf_thr, pass,
                       prefix, hist);
  }, nslabs, hist, prefix, rank, nullptr, count, median, st);
}

extern "C" int pst_depth_moments(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, const int32_t* slab_rows, int nslabs,
                                 float min_depth, float max_depth, float conf_thr, double* partials, double* out, void* stream) {
  using namespace pst;
  if (depth_table_ok("depth_moments", views, views_host, nviews, nblocks, nslabs)) return PST_EINVAL;
  if (depth_bounds_ok("depth_moments", min_depth)) return PST_EINVAL;
  if (!slab_rows || !partials || !out) { set_error("depth_moments: null operand"); return PST_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_sum_kernel<false>, dim3((unsigned)nblocks), dim3(ICP_T), 0, st, (const DepthView*)views, nviews, min_depth, max_depth, conf_thr,
                     (const double*)nullptr, DepthThresholds{}, partials);
  const int rc = check_launch("depth_moments");
  if (rc) return rc;
  hipLaunchKernelGGL(depth_reduce_kernel<DE_ALIGN>, dim3((unsigned)nslabs), dim3(ICP_T), 0, st, partials, slab_rows, nblocks, out);
  return check_launch("depth_moments (reduce)");
}

extern "C" int pst_depth_errors(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, const int32_t* slab_rows, int nslabs,
                                float min_depth, float max_depth, float conf_thr, const double* align, int K, double t0, double t1, double t2, double t3,
                                double* partials, double* out, void* stream) {
  using namespace pst;
  if (depth_table_ok("depth_errors", views, views_host, nviews, nblocks, nslabs)) return PST_EINVAL;
  if (depth_bounds_ok("depth_errors", min_depth)) return PST_EINVAL;
  if (!slab_rows || !align || !partials || !out) { set_error("depth_errors: null operand"); return PST_EINVAL; }
  if (K < 0 || K > 4) { set_error("depth_errors: %d thresholds; one call takes 0 .. 4", K); return PST_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  const DepthThresholds th = {{t0, t1, t2, t3}, K};
  hipLaunchKernelGGL(depth_sum_kernel<true>, dim3((unsigned)nblocks), dim3(ICP_T), 0, st, (const DepthView*)views, nviews, min_depth, max_depth, conf_thr, align,
                     th, partials);
  const int rc = check_launch("depth_errors");
  if (rc) return rc;
  hipLaunchKernelGGL(depth_reduce_kernel<DE_ERR>, dim3((unsigned)nslabs), dim3(ICP_T), 0, st, partials, slab_rows, nblocks, out);
  return check_launch("depth_errors (reduce)");
}
