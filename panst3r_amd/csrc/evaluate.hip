// Panoptic evaluation of predicted maps against ground truth (no counterpart in the reference; the rules of COCO panopticapi's
// pq_compute_single_core without iscrowd; restated in tests/eval_ref.py, [restated, parity unpinned]).  With P predicted and G ground-truth segments:
//   rows     a predicted id i -> row id2row_p[i] if 0 < i < ntab_p and that entry is in [0, P), else the void row P; ground truth likewise -> a column,
//            or the void column G.
//   slabs    S slabs of consecutive pixels of the flat maps (scope 'scene': one; scope 'view': one per view), given by S + 1 offsets; equal offsets: an empty slab.
//   count    counts int32 [S, P+1, G+1] = pixels of slab s with (row p, column g): int32 atomicAdd only, independent of order.
//   areas    pa[s,p] = sum_g counts[s,p,g], ga[s,g] = sum_p counts[s,p,g], void included; area 0 = the segment is not in the slab.
//   match    g with ga > 0 and p with pa > 0 of one category: inter = counts[s,p,g], union = pa + ga - inter - counts[s,p,G]; a match iff
//            2 inter > union in int64 (equality is none); match[s,g] = p or -1, iou[s,g] = (double)inter / (double)union or 0.
//   misses   an existing p without a match: ignored (3) if 2 counts[s,p,G] > pa, else an FP (2); matched 1, absent 0.
// The contract (include/panst3r_hip.h) is integer arithmetic plus one fp64 division: contraction is off for the whole file, no float atomics, every
// result but `counts` is written with plain vector stores by one thread - two calls return identical bytes.
// `merge`: segmentation maps are piecewise constant, and same-address atomics serialise.  A lane loads four pixels; a lane whose four keys agree joins
// the run of adjacent such lanes with that key, and the run's first lane adds 4 x the run's length (ballot, as wave_ops.h's vx_run); any other lane adds
// its own in-lane runs.  A wave inside one (p, g) region issues ONE atomic.  Same results.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "wave_ops.h"            // last_le, id_row

#pragma clang fp contract(off)

namespace pst {

constexpr int EV_T = 256, EV_PT = 4, EV_WG = EV_T * EV_PT;         // threads, pixels per lane (one 16-byte load per map), pixels per workgroup
constexpr uint32_t EV_NONE = 0xffffffffu;                          // no key: a pixel beyond N (a table has fewer than 2^31 entries)

// the slab that owns pixel i: the last one whose offset is <= i (uniform per workgroup: scalar loads)
__device__ __forceinline__ int ev_slab_of(const int64_t* __restrict__ off, int S, int64_t i) {
  return last_le(S, i, [&](int s) { return off[s]; });
}

template <bool MERGE>
__global__ __launch_bounds__(EV_T) void pq_count_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt, int64_t N,
                                                        const int64_t* __restrict__ slab_off, int S, const int32_t* __restrict__ id2row_p, int ntab_p,
                                                        const int32_t* __restrict__ id2row_g, int ntab_g, int P, int G, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * EV_WG, i0 = w0 + threadIdx.x * EV_PT;
  int a[EV_PT] = {0, 0, 0, 0}, b[EV_PT] = {0, 0, 0, 0};
  if (i0 + EV_PT <= N) {                                            // both maps are 16-byte aligned (checked by the host entry point)
    const int4 va = *reinterpret_cast<const int4*>(pred + i0), vb = *reinterpret_cast<const int4*>(gt + i0);
    a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
    b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
  } else {
#pragma unroll
    for (int k = 0; k < EV_PT; ++k)
      if (i0 + k < N) { a[k] = pred[i0 + k]; b[k] = gt[i0 + k]; }
  }
  int s = S > 1 ? ev_slab_of(slab_off, S, w0) : 0;                  // the workgroup's first slab; a pixel further on walks up from it
  uint32_t key[EV_PT];
#pragma unroll
  for (int k = 0; k < EV_PT; ++k) {
    const int64_t i = i0 + k;
    while (s + 1 < S && i >= slab_off[s + 1]) ++s;
    const uint32_t p = (uint32_t)id_row(a[k], id2row_p, ntab_p, P, P), g = (uint32_t)id_row(b[k], id2row_g, ntab_g, G, G);      // none: the void row / column
    key[k] = i < N ? ((uint32_t)s * (uint32_t)(P + 1) + p) * (uint32_t)(G + 1) + g : EV_NONE;
  }
  if constexpr (MERGE) {
    const bool uniform = key[0] == key[1] && key[0] == key[2] && key[0] == key[3];
    // every lane of the wave takes part in the shuffle and the ballot
    const uint32_t prev = __shfl_up(key[0], 1);
    const bool prev_uniform = __shfl_up((int)uniform, 1) != 0;
    const uint64_t heads = __ballot(lane == 0 || !uniform || !prev_uniform || prev != key[0]);
    if (uniform) {
      if ((heads >> lane) & 1) {
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = above ? 1 + (int)__builtin_ctzll(above) : 64 - lane;
        if (key[0] != EV_NONE) atomicAdd(&counts[key[0]], EV_PT * len);
      }
    } else {
      int run = 1;
#pragma unroll
      for (int k = 1; k <= EV_PT; ++k) {
        if (k < EV_PT && key[k] == key[k - 1]) { ++run; continue; }
        if (key[k - 1] != EV_NONE) atomicAdd(&counts[key[k - 1]], run);
        run = 1;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < EV_PT; ++k)
      if (key[k] != EV_NONE) atomicAdd(&counts[key[k]], 1);
  }
}

// pa[s,p]: one wave per row of counts, lanes stride the columns
__global__ __launch_bounds__(EV_T) void pq_pred_area_kernel(const int32_t* __restrict__ counts, int64_t rows, int P, int G, int32_t* __restrict__ pa) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (EV_T / 64) + (threadIdx.x >> 6);      // r = s * P + p
  if (r >= rows) return;                                            // uniform per wave
  const int64_t s = r / P, p = r % P;
  const int32_t* row = counts + (s * (P + 1) + p) * (int64_t)(G + 1);
  int v = 0;
  for (int g = lane; g <= G; g += 64) v += row[g];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) pa[r] = v;
}

// ga[s,g]: one thread per column, adjacent threads read adjacent columns
__global__ __launch_bounds__(EV_T) void pq_gt_area_kernel(const int32_t* __restrict__ counts, int64_t cols, int P, int G, int32_t* __restrict__ ga) {
  const int64_t c = (int64_t)blockIdx.x * EV_T + threadIdx.x;      // c = s * G + g
  if (c >= cols) return;
  const int64_t s = c / G, g = c % G;
  const int32_t* col = counts + s * (int64_t)(P + 1) * (G + 1) + g;
  int v = 0;
  for (int p = 0; p <= P; ++p) v += col[(int64_t)p * (G + 1)];
  ga[c] = v;
}

__global__ __launch_bounds__(EV_T) void pq_match_kernel(const int32_t* __restrict__ counts, int64_t cols, int P, int G, const int32_t* __restrict__ cat_p,
                                                        const int32_t* __restrict__ cat_g, const int32_t* __restrict__ pa, const int32_t* __restrict__ ga,
                                                        int32_t* __restrict__ match, double* __restrict__ iou) {
  const int64_t c = (int64_t)blockIdx.x * EV_T + threadIdx.x;
  if (c >= cols) return;
  const int64_t s = c / G, g = c % G;
  const int32_t* tab = counts + s * (int64_t)(P + 1) * (G + 1);
  const int64_t area_g = ga[c];
  const int cat = cat_g[g];
  int m = -1;
  double q = 0.0;
  if (area_g > 0)
    for (int p = 0; p < P; ++p) {
      const int64_t area_p = pa[s * P + p];
      if (area_p == 0 || cat_p[p] != cat) continue;
      const int64_t inter = tab[(int64_t)p * (G + 1) + g];
      const int64_t uni = area_p + area_g - inter - (int64_t)tab[(int64_t)p * (G + 1) + G];
      if (2 * inter > uni && m < 0) { m = p; q = (double)inter / (double)uni; }
    }
  match[c] = m;
  iou[c] = q;
}

__global__ __launch_bounds__(EV_T) void pq_state_kernel(const int32_t* __restrict__ counts, int64_t rows, int P, int G, const int32_t* __restrict__ pa,
                                                        const int32_t* __restrict__ match, int32_t* __restrict__ state) {
  const int64_t r = (int64_t)blockIdx.x * EV_T + threadIdx.x;      // r = s * P + p
  if (r >= rows) return;
  const int64_t s = r / P;
  const int p = (int)(r % P);
  const int64_t area = pa[r];
  int st = 0;
  if (area > 0) {
    bool matched = false;
    for (int g = 0; g < G; ++g) matched = matched || match[s * G + g] == p;
    const int64_t on_void = counts[(s * (P + 1) + p) * (int64_t)(G + 1) + G];
    st = matched ? 1 : (2 * on_void > area ? 3 : 2);
  }
  state[r] = st;
}

static bool ev_shape_ok(int S, int P, int G) {
  return S >= 1 && P >= 0 && G >= 0 && P < (1 << 30) && G < (1 << 30) && (int64_t)S * (P + 1) * (G + 1) <= 0x7fffffffLL;
}

}  // namespace pst

extern "C" int pst_pq_count(const int32_t* pred, const int32_t* gt, int64_t N, const int64_t* slab_off, int nslabs, const int32_t* id2row_p, int ntab_p,
                            const int32_t* id2row_g, int ntab_g, int P, int G, int32_t* counts, int merge, void* stream) {
  using namespace pst;
  if (!pred || !gt || !slab_off || !id2row_p || !id2row_g || !counts) { set_error("pq_count: null operand"); return PST_EINVAL; }
  if (N <= 0 || N > 0x7fffffffLL || !ev_shape_ok(nslabs, P, G) || ntab_p < 1 || ntab_g < 1) {
    set_error("pq_count: bad shape (N=%lld, slabs=%d, P=%d, G=%d, ntab=%d / %d)", (long long)N, nslabs, P, G, ntab_p, ntab_g); return PST_EINVAL;
  }
  if ((((uintptr_t)pred) | ((uintptr_t)gt)) & 15) { set_error("pq_count: the maps must be 16-byte aligned"); return PST_EINVAL; }
  const dim3 grid = blocks_for(N, EV_WG);
  if (merge) hipLaunchKernelGGL(pq_count_kernel<true>, grid, dim3(EV_T), 0, (hipStream_t)stream, pred, gt, N, slab_off, nslabs, id2row_p, ntab_p, id2row_g, ntab_g,
                                P, G, counts);
  else hipLaunchKernelGGL(pq_count_kernel<false>, grid, dim3(EV_T), 0, (hipStream_t)stream, pred, gt, N, slab_off, nslabs, id2row_p, ntab_p, id2row_g, ntab_g, P, G,
                          counts);
  return check_launch("pq_count");
}

extern "C" int pst_pq_match(const int32_t* counts, int nslabs, int P, int G, const int32_t* cat_p, const int32_t* cat_g, int32_t* pred_area, int32_t* gt_area,
                            int32_t* match, double* iou, int32_t* pred_state, void* stream) {
  using namespace pst;
  if (!counts || !ev_shape_ok(nslabs, P, G)) { set_error("pq_match: bad shape (slabs=%d, P=%d, G=%d) / null operand", nslabs, P, G); return PST_EINVAL; }
  if ((P > 0 && (!cat_p || !pred_area || !pred_state)) || (G > 0 && (!cat_g || !gt_area || !match || !iou))) { set_error("pq_match: null operand"); return PST_EINVAL; }
  const int64_t rows = (int64_t)nslabs * P, cols = (int64_t)nslabs * G;
  hipStream_t st = (hipStream_t)stream;
  if (P > 0) hipLaunchKernelGGL(pq_pred_area_kernel, blocks_for(rows, EV_T / 64), dim3(EV_T), 0, st, counts, rows, P, G, pred_area);
  if (G > 0) {
    const dim3 grid = blocks_for(cols, EV_T);
    hipLaunchKernelGGL(pq_gt_area_kernel, grid, dim3(EV_T), 0, st, counts, cols, P, G, gt_area);
    hipLaunchKernelGGL(pq_match_kernel, grid, dim3(EV_T), 0, st, counts, cols, P, G, cat_p, cat_g, pred_area, gt_area, match, iou);
  }
  if (P > 0) hipLaunchKernelGGL(pq_state_kernel, blocks_for(rows, EV_T), dim3(EV_T), 0, st, counts, rows, P, G, pred_area, match, pred_state);
  return check_launch("pq_match");
}
