// ASMK image retrieval of the PanSt3R checkpoint's retriever (reference src/panst3r/engine/retrieval.py:12-47, panst3r.py:88-125; the
// algorithm is restated in panst3r_amd/model/retrieval.py, [3P-recalled, parity unpinned]).  The retrieval head itself runs on pst_gemm /
// pst_layernorm in fp32 mode; these are the four steps after it:
//   select     per view: row norms of the head output, top-nfeat rows (ties to the lower token), L2-normalised gather
//   assign     fused nearest-centroid top-m on split-f16 MFMA distance tiles (the n x k distance matrix never exists), centroid range split
//              over workgroups + a fixed-order merge of the partial lists
//   aggregate  per (view, word) group: fp32 residual sums in ascending descriptor order, packed sign bits
//   scores     V x V ASMK similarity, binary kernel: per query view its sorted word list in LDS, binary search per database word,
//              XOR popcount, kappa, fp32 accumulation in ascending word order
// Every result is deterministic (fixed-order reductions, no atomics) and written with plain vector stores.
#include "common.h"
#include "../../include/panst3r_hip.h"

namespace pst {

// (d, id) lexicographic order: distance ties go to the lower centroid index, whatever order the candidates arrive in
__device__ __forceinline__ bool lexless(float a, int ia, float b, int ib) { return a < b || (a == b && ia < ib); }

template <int M>
__device__ __forceinline__ void topm_insert(float (&d)[M], int (&id)[M], float v, int c) {
  if (!lexless(v, c, d[M - 1], id[M - 1])) return;
  d[M - 1] = v; id[M - 1] = c;
#pragma unroll
  for (int j = M - 1; j > 0; --j) {
    if (lexless(d[j], id[j], d[j - 1], id[j - 1])) {
      const float td = d[j]; d[j] = d[j - 1]; d[j - 1] = td;
      const int ti = id[j]; id[j] = id[j - 1]; id[j - 1] = ti;
    }
  }
}

// ---------------------------------------------------------------- select
// One block per view.  Ranking key = fp32 sum of squares (monotone in the norm, no sqrt ties); out row out_off[v] + rank, rank = number of rows
// with a larger key or an equal key and a lower token index.  Dynamic LDS: maxT keys + nsel token indices.
__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ in_off,
                                                     const int32_t* __restrict__ out_off, int D, float* __restrict__ out, int64_t ldo,
                                                     int32_t* __restrict__ sel_idx) {
  extern __shared__ float smem[];
  const int v = blockIdx.x;
  const int t0 = in_off[v], T = in_off[v + 1] - t0;
  const int o0 = out_off[v], nsel = out_off[v + 1] - o0;
  float* key = smem;
  int* dst = (int*)(smem + T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = wave; t < T; t += 4) {
    const float* r = x + (int64_t)(t0 + t) * ldx;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s = fmaf(r[c], r[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) key[t] = s;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const float q = key[t];
    int rank = 0;
    for (int j = 0; j < T; ++j) {
      const float p = key[j];
      rank += (p > q || (p == q && j < t)) ? 1 : 0;
    }
    if (rank < nsel) dst[rank] = t;
  }
  __syncthreads();
  for (int r = wave; r < nsel; r += 4) {
    const int t = dst[r];
    const float nrm = fmaxf(sqrtf(key[t]), 1e-12f);
    const float* src = x + (int64_t)(t0 + t) * ldx;
    float* o = out + (int64_t)(o0 + r) * ldo;
    for (int c = lane; c < D; c += 64) o[c] = src[c] / nrm;
    if (lane == 0 && sel_idx) sel_idx[o0 + r] = t;
  }
}

// ---------------------------------------------------------------- assign
// Block = 4 waves, 128 descriptor rows x 64-centroid tiles over the block's centroid range [c_begin, c_end).  K3 = 3 Dpad split columns
// (descriptors [hi | hi | lo], centroids [hi | lo | hi]: x.c to 2^-22 on the 16-bit MFMA).  MFMA operand A = a centroid fragment, B = a
// descriptor fragment, so D[centroid][row]: lane l owns descriptor row (l & 15) of each 16-row subtile and centroids 4 (l >> 4) + reg of each
// 16-centroid subtile - it walks its centroids in ascending order and keeps a running top-M per row subtile in registers; the four lanes of a
// row merge their lists by shuffles at the end.  dist = ||c||^2 - 2 x.c (fp32, one fma).
constexpr int AS_BM = 128, AS_BN = 64, AS_BK = 64, AS_LD = AS_BK + 8;      // +8 halves per LDS row: 144-byte stride, conflict-free b128 reads

template <int M>
__global__ __launch_bounds__(256) void assign_kernel(const uint16_t* __restrict__ x3, int64_t ldx, const uint16_t* __restrict__ c3, int64_t ldc,
                                                     const float* __restrict__ cnorm, int n, int k, int K3, int chunk,
                                                     float* __restrict__ out_d, int32_t* __restrict__ out_i) {
  __shared__ __attribute__((aligned(16))) uint16_t As[AS_BM * AS_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[AS_BN * AS_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * AS_BM;
  const int split = blockIdx.y;
  const int c_begin = split * chunk, c_end = min(k, c_begin + chunk);
  float bd[2][M];
  int bi[2][M];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) { bd[i][j] = __builtin_huge_valf(); bi[i][j] = -1; }

  for (int c0 = c_begin; c0 < c_end; c0 += AS_BN) {
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < K3; kk += AS_BK) {
      uint4 ra[4], rb[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, row = i >> 3, ch = i & 7;
        ra[j] = *(const uint4*)(x3 + (int64_t)min(r0 + row, n - 1) * ldx + kk + ch * 8);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j, row = i >> 3, ch = i & 7;
        rb[j] = *(const uint4*)(c3 + (int64_t)min(c0 + row, k - 1) * ldc + kk + ch * 8);
      }
      __syncthreads();                       // the previous K step's fragment reads are done
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j;
        *(uint4*)(As + (i >> 3) * AS_LD + (i & 7) * 8) = ra[j];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j;
        *(uint4*)(Bs + (i >> 3) * AS_LD + (i & 7) * 8) = rb[j];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < AS_BK; ks += 32) {
        const int col = ks + 8 * (lane >> 4);
        bf16x8 af[2], bfr[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *(const bf16x8*)(As + (wave * 32 + i * 16 + (lane & 15)) * AS_LD + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = *(const bf16x8*)(Bs + (j * 16 + (lane & 15)) * AS_LD + col);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = H16<true>::mfma(bfr[j], af[i], acc[i][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = c0 + j * 16 + 4 * (lane >> 4) + r;
        if (c < c_end) {
          const float cn = cnorm[c];
#pragma unroll
          for (int i = 0; i < 2; ++i) topm_insert<M>(bd[i], bi[i], fmaf(-2.f, acc[i][j][r], cn), c);
        }
      }
  }
  // merge the four lanes (l & 15) + 16 g of each row into the g = 0 lane
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int g = 1; g < 4; ++g) {
      float od[M];
      int oi[M];
#pragma unroll
      for (int j = 0; j < M; ++j) { od[j] = __shfl(bd[i][j], (lane & 15) + 16 * g); oi[j] = __shfl(bi[i][j], (lane & 15) + 16 * g); }
      if (lane < 16)
#pragma unroll
        for (int j = 0; j < M; ++j) topm_insert<M>(bd[i], bi[i], od[j], oi[j]);
    }
    const int row = r0 + wave * 32 + i * 16 + lane;
    if (lane < 16 && row < n) {
      const int64_t o = ((int64_t)split * n + row) * M;
#pragma unroll
      for (int j = 0; j < M; ++j) { out_d[o + j] = bd[i][j]; out_i[o + j] = bi[i][j]; }
    }
  }
}

// partial lists [nsplit][n][M] -> [n][M], merged in split order (the lexicographic order makes the result independent of the split count)
template <int M>
__global__ __launch_bounds__(256) void assign_merge_kernel(const float* __restrict__ ws_d, const int32_t* __restrict__ ws_i, int n, int nsplit,
                                                           float* __restrict__ dist, int32_t* __restrict__ ids) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float d[M];
  int id[M];
#pragma unroll
  for (int j = 0; j < M; ++j) { d[j] = __builtin_huge_valf(); id[j] = -1; }
  for (int s = 0; s < nsplit; ++s) {
    const int64_t o = ((int64_t)s * n + row) * M;
#pragma unroll
    for (int j = 0; j < M; ++j) topm_insert<M>(d, id, ws_d[o + j], ws_i[o + j]);
  }
#pragma unroll
  for (int j = 0; j < M; ++j) { dist[(int64_t)row * M + j] = d[j]; ids[(int64_t)row * M + j] = id[j]; }
}

template <int M>
static int assign_launch(const uint16_t* x3, int64_t ldx, const uint16_t* c3, int64_t ldc, const float* cnorm, int n, int k, int K3, int nsplit,
                         float* ws_d, int32_t* ws_i, int32_t* ids, float* dist, hipStream_t st) {
  const int tiles = (k + AS_BN - 1) / AS_BN;
  const int chunk = (tiles + nsplit - 1) / nsplit * AS_BN;
  const dim3 grid((unsigned)((n + AS_BM - 1) / AS_BM), (unsigned)nsplit);
  if (nsplit == 1) {
    hipLaunchKernelGGL(assign_kernel<M>, grid, dim3(256), 0, st, x3, ldx, c3, ldc, cnorm, n, k, K3, chunk, dist, ids);
    return check_launch("retrieval_assign");
  }
  hipLaunchKernelGGL(assign_kernel<M>, grid, dim3(256), 0, st, x3, ldx, c3, ldc, cnorm, n, k, K3, chunk, ws_d, ws_i);
  int rc = check_launch("retrieval_assign");
  if (rc) return rc;
  hipLaunchKernelGGL(assign_merge_kernel<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws_d, ws_i, n, nsplit, dist, ids);
  return check_launch("retrieval_assign (merge)");
}

// ---------------------------------------------------------------- aggregate
// One block per (view, word) group; a wave covers 64 consecutive components, so one ballot packs two bit words (bit j of word w = component 32 w + j).
__global__ __launch_bounds__(256) void aggregate_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ cent, int64_t ldc,
                                                        const int32_t* __restrict__ member, const int32_t* __restrict__ gstart,
                                                        const int32_t* __restrict__ gword, int D, float* __restrict__ sums,
                                                        uint32_t* __restrict__ bits) {
  const int g = blockIdx.x;
  const int b = gstart[g], e = gstart[g + 1];
  const float* c = cent + (int64_t)gword[g] * ldc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = D / 32;
  for (int base = wave * 64; base < D; base += 256) {
    const int col = base + lane;
    float s = 0.f;
    if (col < D) {
      const float cc = c[col];
      for (int m = b; m < e; ++m) s += x[(int64_t)member[m] * ldx + col] - cc;
      if (sums) sums[(int64_t)g * D + col] = s;
    }
    const uint64_t mask = __ballot(col < D && s > 0.f);
    if (lane == 0) {
      bits[(int64_t)g * W + base / 32] = (uint32_t)mask;
      if (base + 32 < D) bits[(int64_t)g * W + base / 32 + 1] = (uint32_t)(mask >> 32);
    }
  }
}

// ---------------------------------------------------------------- scores
// One block per query view i; wave w takes database views j = w, w + 4, ...  Per 64 database groups of view j (sorted by word): lane -> one group,
// binary search of its word in the query's LDS word list, kappa of the match (0 without one); the 64 contributions are then added in group order
// by every lane (shuffles), so S[i, j] is the fp32 sum in ascending word order.
__device__ __forceinline__ float kappa(int h, int D, float alpha, int ialpha, float tau) {
  const float s = 1.0f - (float)(2 * h) / (float)D;
  if (!(s >= tau)) return 0.f;
  if (ialpha > 0) {
    float p = s;
    for (int a = 1; a < ialpha; ++a) p = p * s;
    return p;
  }
  return powf(s, alpha);
}

__global__ __launch_bounds__(256) void scores_kernel(const int32_t* __restrict__ q_off, const int32_t* __restrict__ q_word,
                                                     const uint32_t* __restrict__ q_bits, const int32_t* __restrict__ db_off,
                                                     const int32_t* __restrict__ db_word, const uint32_t* __restrict__ db_bits, int Vdb, int D,
                                                     float alpha, int ialpha, float tau, float* __restrict__ S) {
  extern __shared__ int qw[];
  const int i = blockIdx.x;
  const int q0 = q_off[i], nq = q_off[i + 1] - q0;
  for (int t = threadIdx.x; t < nq; t += blockDim.x) qw[t] = q_word[q0 + t];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = D / 32;
  for (int j = wave; j < Vdb; j += 4) {
    const int b = db_off[j], e = db_off[j + 1];
    float acc = 0.f;
    for (int base = b; base < e; base += 64) {
      const int g = base + lane;
      float c = 0.f;
      if (g < e) {
        const int w = db_word[g];
        int lo = 0, hi = nq;                     // first query word >= w
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (qw[mid] < w) lo = mid + 1; else hi = mid;
        }
        if (lo < nq && qw[lo] == w) {
          const uint32_t* a = q_bits + (int64_t)(q0 + lo) * W;
          const uint32_t* d = db_bits + (int64_t)g * W;
          int h = 0;
          for (int t = 0; t < W; ++t) h += __popc(a[t] ^ d[t]);
          c = kappa(h, D, alpha, ialpha, tau);
        }
      }
      const int cnt = min(64, e - base);
      for (int t = 0; t < cnt; ++t) acc += __shfl(c, t);
    }
    if (lane == 0) S[(int64_t)i * Vdb + j] = acc;
  }
}

}  // namespace pst

extern "C" int pst_retrieval_select(const float* x, int64_t ldx, const int32_t* in_off, const int32_t* out_off, int nviews, int maxT, int D,
                                    float* out, int64_t ldo, int32_t* sel_idx, void* stream) {
  using namespace pst;
  if (!x || !in_off || !out_off || !out || nviews <= 0 || maxT <= 0 || D <= 0) { set_error("retrieval_select: bad shape / null operand"); return PST_EINVAL; }
  if (ldx < D || ldo < D) { set_error("retrieval_select: leading dimensions must be >= D"); return PST_EINVAL; }
  if (maxT > 16384) { set_error("retrieval_select: %d tokens per view exceed the LDS ranking buffer (16384)", maxT); return PST_EINVAL; }
  const size_t lds = (size_t)maxT * 8;
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)nviews), dim3(256), lds, (hipStream_t)stream, x, ldx, in_off, out_off, D, out, ldo, sel_idx);
  return check_launch("retrieval_select");
}

extern "C" int pst_retrieval_assign(const void* x3, int64_t ldx, const void* c3, int64_t ldc, const float* cnorm, int n, int k, int K3, int m,
                                    int nsplit, float* ws_dist, int32_t* ws_ids, int32_t* ids, float* dist, int dtype16, void* stream) {
  using namespace pst;
  if (!x3 || !c3 || !cnorm || !ids || !dist || n <= 0 || k <= 0) { set_error("retrieval_assign: bad shape / null operand"); return PST_EINVAL; }
  if (dtype16 != PST_F16) { set_error("retrieval_assign: the split operands must be f16 (PST_F16)"); return PST_EINVAL; }
  if (m < 1 || m > 8 || m > k) { set_error("retrieval_assign: need 1 <= m <= 8 and m <= k (m=%d, k=%d)", m, k); return PST_EINVAL; }
  if (K3 <= 0 || K3 % AS_BK || ldx < K3 || ldc < K3 || ldx % 8 || ldc % 8 || (((uintptr_t)x3 | (uintptr_t)c3) & 15)) {
    set_error("retrieval_assign: need K3 %% 64 == 0, leading dimensions >= K3 and multiples of 8, 16-byte aligned operands"); return PST_EINVAL;
  }
  const int tiles = (k + AS_BN - 1) / AS_BN;
  if (nsplit < 1 || nsplit > tiles || nsplit > 65535) { set_error("retrieval_assign: nsplit %d outside [1, %d]", nsplit, tiles); return PST_EINVAL; }
  if (nsplit > 1 && (!ws_dist || !ws_ids)) { set_error("retrieval_assign: nsplit > 1 needs the workspace (nsplit x n x m floats and ints)"); return PST_EINVAL; }
  const uint16_t* a = (const uint16_t*)x3;
  const uint16_t* c = (const uint16_t*)c3;
  hipStream_t st = (hipStream_t)stream;
  switch (m) {
    case 1: return assign_launch<1>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 2: return assign_launch<2>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 3: return assign_launch<3>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 4: return assign_launch<4>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 5: return assign_launch<5>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 6: return assign_launch<6>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    case 7: return assign_launch<7>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
    default: return assign_launch<8>(a, ldx, c, ldc, cnorm, n, k, K3, nsplit, ws_dist, ws_ids, ids, dist, st);
  }
}

extern "C" int pst_retrieval_aggregate(const float* x, int64_t ldx, const float* cent, int64_t ldc, const int32_t* member, const int32_t* gstart,
                                       const int32_t* gword, int ngroups, int D, float* sums, uint32_t* bits, void* stream) {
  using namespace pst;
  if (!x || !cent || !member || !gstart || !gword || !bits || ngroups <= 0 || D <= 0) { set_error("retrieval_aggregate: bad shape / null operand"); return PST_EINVAL; }
  if (D % 32 || ldx < D || ldc < D) { set_error("retrieval_aggregate: need D %% 32 == 0 and leading dimensions >= D (D=%d)", D); return PST_EINVAL; }
  hipLaunchKernelGGL(aggregate_kernel, dim3((unsigned)ngroups), dim3(256), 0, (hipStream_t)stream, x, ldx, cent, ldc, member, gstart, gword, D, sums, bits);
  return check_launch("retrieval_aggregate");
}

extern "C" int pst_retrieval_scores(const int32_t* q_off, const int32_t* q_word, const uint32_t* q_bits, const int32_t* db_off, const int32_t* db_word,
                                    const uint32_t* db_bits, int nq_views, int ndb_views, int max_q, int D, float alpha, float tau, float* S, void* stream) {
  using namespace pst;
  if (!q_off || !q_word || !q_bits || !db_off || !db_word || !db_bits || !S || nq_views <= 0 || ndb_views <= 0 || max_q < 1 || D <= 0) {
    set_error("retrieval_scores: bad shape / null operand"); return PST_EINVAL;
  }
  if (D % 32) { set_error("retrieval_scores: D %% 32 != 0 (D=%d)", D); return PST_EINVAL; }
  if (max_q > 16384) { set_error("retrieval_scores: %d words per query view exceed the LDS word list (16384)", max_q); return PST_EINVAL; }
  if (!(tau >= 0.f) || !(alpha > 0.f)) { set_error("retrieval_scores: need tau >= 0 and alpha > 0"); return PST_EINVAL; }
  const int ialpha = (alpha == floorf(alpha) && alpha <= 8.f) ? (int)alpha : 0;       // integer exponents by repeated products (exactly reproducible)
  hipLaunchKernelGGL(scores_kernel, dim3((unsigned)nq_views), dim3(256), (size_t)max_q * 4, (hipStream_t)stream, q_off, q_word, q_bits, db_off, db_word,
                     db_bits, ndb_views, D, alpha, ialpha, tau, S);
  return check_launch("retrieval_scores");
}
