// The exact fp32 median by radix select, written once for its two users: the per-segment, per-axis median of csrc/cloud.hip (group of 3 slots = the
// axes of a segment, signed keys, NaN counts) and the medians of p and g per slab of csrc/depth_eval.hip (group of 2 slots, raw bits, no NaN reaches it).
// A select SLOT is one multiset of fp32 values with one median; a GROUP is the G consecutive slots that share one count (every value of a group is
// tallied into all G slots, so slot 0's total is the group's).  The contract of the passes:
//   workspace  int32, zeroed by the caller before the first pass: hist [slots, 2, 256] (16-byte aligned), prefix [slots, 2], rank [slots, 2]; index 0 / 1
//              of the middle dimension = the two order statistics (n - 1) / 2 and n / 2 of the slot's n values
//   key        an unsigned order of the values: the order-preserving transform of the bits (SIGNED) or the bits themselves (values > 0 only)
//   pass p     (p = 0 .. 3, most significant byte first, shift = 24 - 8 p) is two launches.  The user's histogram kernel tallies byte 3 - p of every key
//              in LDS - pass 0: every key into the first 256 counters of its slot, shared by both ranks; later: into the rank's 256 counters the keys
//              whose bytes above equal the rank's prefix - and flushes the block's non-zero counters with INTEGER atomics: no order, two calls give
//              equal bytes.  select_narrow_kernel, one wave per slot, then finds per rank the first bin whose inclusive count exceeds the rank, ors
//              the bin into the prefix, makes the rank relative to that bin (no value: bin 0, rank 0), clears the slot's 512 counters for the next
//              pass and, in pass 0, stores the group's count
//   result     after pass 3 the two prefixes are the keys a, b of the two order statistics: median = a for an odd count, rn_mul(rn_add(a, b), 0.5f)
//              for an even one, the NaN 0x7fc00000 for a count of 0 or a slot whose NaN count is positive; hist, prefix and rank are left zeroed
// Integer code but for that one sum and product, which are rn_*: rounded on their own whoever includes this header, and with whatever flags.
#pragma once
#include "wave_ops.h"            // wave_scan, rn_add, rn_mul; and through it common.h: check_launch

namespace pst {

constexpr int RS_SLOT = 2 * 256;                                   // counters per slot: two ranks x 256 bins

// ---------------------------------------------------------------- the key pair
// SIGNED: a < b as floats <=> key(a) < key(b) as unsigned (-0.0 sorts just below +0.0; NaNs sort to the two ends and are counted apart); else the bits
__device__ __forceinline__ uint32_t fkey(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t funkey(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }
template <bool SIGNED>
__device__ __forceinline__ uint32_t select_key(uint32_t u) { return SIGNED ? fkey(u) : u; }
template <bool SIGNED>
__device__ __forceinline__ float select_value(uint32_t k) { return __uint_as_float(SIGNED ? funkey(k) : k); }

// ---------------------------------------------------------------- the histogram pass: what a user's kernel calls between its own barriers
// one key of the block's slot `slot`; h = the block's LDS counters, RS_SLOT per slot, pre = its prefixes, two per slot (read in the passes after 0 only)
__device__ __forceinline__ void select_tally(int* h, const uint32_t* pre, int slot, uint32_t key, int pass) {
  const int shift = 24 - 8 * pass;
  if (pass == 0) atomicAdd(&h[slot * RS_SLOT + (key >> 24)], 1);
  else {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if ((key >> (shift + 8)) == (pre[slot * 2 + j] >> (shift + 8))) atomicAdd(&h[(slot * 2 + j) * 256 + ((key >> shift) & 255)], 1);
  }
}

// the non-zero ones of the block's n LDS counters onto the global counters of the block's first slot; T = threads of the block, all of which call it
template <int T>
__device__ __forceinline__ void select_flush(const int* h, int n, int32_t* __restrict__ hist) {
  for (int i = threadIdx.x; i < n; i += T) {
    const int c = h[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// ---------------------------------------------------------------- the narrowing pass
// one wave on one slot (hist, prefix, rank at the slot): the slot's total -> n (pass 0), the new prefixes -> key and, by lane 0, prefix; rank likewise
__device__ __forceinline__ void select_narrow(const int32_t* hist, uint32_t* prefix, int32_t* rank, int pass, int lane, int& n, uint32_t (&key)[2]) {
  const int shift = 24 - 8 * pass;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int4 c = ((const int4*)(hist + (pass == 0 ? 0 : j) * 256))[lane];
    const int own = c.x + c.y + c.z + c.w;
    const int s = wave_scan(own, lane);
    const int tot = __shfl(s, 63);
    int k;
    if (pass == 0) { n = tot; k = j == 0 ? (tot - 1) / 2 : tot / 2; } else k = rank[j];
    // the bin that holds rank k: the first bin whose inclusive count exceeds k
    int below = s - own, bin = -1;
    const int cc[4] = {c.x, c.y, c.z, c.w};
    if (tot > 0 && k >= below && k < s) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (bin < 0) {
          if (k < below + cc[q]) bin = 4 * lane + q; else below += cc[q];
        }
    }
    const uint64_t who = __ballot(bin >= 0);
    const int src = who ? __builtin_ctzll(who) : 0;
    bin = __shfl(bin, src); below = __shfl(below, src);
    key[j] = (pass == 0 ? 0u : prefix[j]) | ((uint32_t)max(bin, 0) << shift);
    if (lane == 0) { prefix[j] = key[j]; rank[j] = who ? k - below : 0; }
  }
}

// the median of a slot from the keys of its two order statistics after pass 3
template <bool SIGNED>
__device__ __forceinline__ float select_median(const uint32_t (&key)[2], int cnt, int nans) {
  const float a = select_value<SIGNED>(key[0]), b = select_value<SIGNED>(key[1]);
  if (nans > 0 || cnt == 0) return __uint_as_float(0x7fc00000u);
  return (cnt & 1) ? a : rn_mul(rn_add(a, b), 0.5f);
}

// grid = slots, one wave each; G = slots per group; nan_cnt [slots] or null for none.  count [slots / G] is written by pass 0 and read by pass 3.
template <bool SIGNED, int G>
__global__ __launch_bounds__(64) void select_narrow_kernel(int32_t* __restrict__ hist, uint32_t* __restrict__ prefix, int32_t* __restrict__ rank, int pass,
                                                           const int32_t* __restrict__ nan_cnt, int32_t* __restrict__ count, float* __restrict__ median) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  int n = 0;
  uint32_t key[2];
  hist += (int64_t)slot * RS_SLOT; prefix += slot * 2; rank += slot * 2;
  select_narrow(hist, prefix, rank, pass, lane, n, key);
  __syncthreads();                                                 // (one wave: both ranks have read the shared pass-0 histogram)
  const int4 z = {0, 0, 0, 0};
  ((int4*)hist)[lane] = z;
  ((int4*)hist)[lane + 64] = z;
  if (pass == 0 && lane == 0 && slot % G == 0) count[slot / G] = n;
  if (pass == 3 && lane == 0) {
    median[slot] = select_median<SIGNED>(key, count[slot / G], nan_cnt ? nan_cnt[slot] : 0);
    prefix[0] = 0u; prefix[1] = 0u;                                // the workspaces are left as they came: zeroed
    rank[0] = 0; rank[1] = 0;
  }
}

// ---------------------------------------------------------------- the host side: the four passes of one select over `groups` groups
// hist_launch(pass) launches the user's histogram kernel on st; the refusals and the workspace's alignment test stay with the entry point
template <bool SIGNED, int G, typename HistLaunch>
static int select_passes(const char* hist_what, const char* narrow_what, HistLaunch hist_launch, int groups, int32_t* hist, uint32_t* prefix, int32_t* rank,
                         const int32_t* nan_cnt, int32_t* count, float* median, hipStream_t st) {
  for (int pass = 0; pass < 4; ++pass) {
    hist_launch(pass);
    int rc = check_launch(hist_what);
    if (rc) return rc;
    hipLaunchKernelGGL((select_narrow_kernel<SIGNED, G>), dim3((unsigned)groups * G), dim3(64), 0, st, hist, prefix, rank, pass, nan_cnt, count, median);
    rc = check_launch(narrow_what);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace pst
