// QUBO mask selection by many-replica simulated annealing (reference engine/postprocess.py:262-336: 20 sequential restarts in numpy on the host).
// Minimises E(x) = x^T W x + lambda * mean(x), x in {0,1}^N, with the reference's moves (single bit flips), acceptance rule (Metropolis) and
// schedule (geometric cooling), but as `replicas` independent anneals at once, and with a counter-based generator instead of np.random: the result is
// a pure function of (W, N, replicas, num_iters, T0, T_end, lambda_reg, seed), restated bit for bit in tests/qubo_ref.py [restated, own design].
//
// Layout: one wave per replica.  W (N <= 200: 160 000 B) sits in LDS, shared by the 1 .. 16 waves of the workgroup; lane l owns the local fields
// h_k = (W x)_k and the diagonal W_kk of k = l + 64 q, q < 4, in registers; x and the best x are four 64-bit masks, wave-uniform.  The move index, the
// energy change and the decision are wave-uniform (v_readlane of h_j and W_jj); only an ACCEPTED move touches LDS: row j of W, contiguous, added into
// the fields.  The generator carries no state from move to move, so it is off the dependent chain.
//
// The contract, operation by operation (every fp32 product, sum and difference below is rounded on its own: contraction is off for the whole file):
//   host      beta0 = fp32(1 / double(T0));  cinv = fp32(pow(double(T0) / double(T_end), 1 / double(num_iters)));  lamN = fp32(lambda_reg) / fp32(N)
//             (an fp32 division);  key = (seed & 0xffffffff, seed >> 32).  The temperature is carried as its INVERSE, beta <- beta * cinv in fp32 once per
//             move, starting from beta0: no division in the loop and no table.
//   random    Philox4x32-10.  counter (c0, c1, c2, c3) = (block, replica, stream, 0) -> words w0..w3.  stream 1, block b in {0, 1}: the initial x, bit
//             (k mod 32) of word ((k / 32) mod 4) of block (k / 128) is x_k.  stream 0, block i / 2: the draws of move i are the word pair (w0, w1)
//             for even i and (w2, w3) for odd i:  j = mulhi32(first word, N),  u = fp32(second word >> 8) * 2^-24 (exact).
//   evaluate  (x) -> h, e:  h_k = 0, then for j = 0 .. N-1 ascending, if x_j:  h_k = h_k + W[j][k]  (all k);  e = 0, then for k = 0 .. N-1 ascending, if
//             x_k:  e = e + h_k;  finally  e = e + lamN * fp32(popcount(x)).
//   start     h, E = evaluate(x);  best_x = x, best_E = E, beta = beta0.
//   move i    s = 1 - 2 x_j (+-1);  d = ((2 s) * h_j + W[j][j]) + s * lamN;  accept if d < 0, else if u < exp_neg(-(d * beta));  on accept:
//             x_j flips, E = E + d, h_k = h_k + s * W[j][k] for all k (row j; W is expected symmetric), and if E < best_E: best_E = E, best_x = x.
//             Then beta = beta * cinv.
//   exp_neg   (a <= 0; not a library or hardware transcendental)  0 unless a >= -87;  n = rint(a * log2e);  r = (a - n * LN2_HI) - n * LN2_LO;
//             p = Horner of the degree-7 Taylor polynomial of exp in r, p = p * r + c from 1/5040 down to 1, 1;  result = the float whose bits are
//             bits(p) + n * 2^23.  |r| <= 0.3466 + rounding, so the truncation is below 5e-9 and the rounding of 7 Horner steps about 3 ulp: the
//             relative error against exp in double stays below 1e-6 on [-87, 0] (tested), exp_neg(0) = 1 exactly, n >= -126 keeps the result normal.
//   finish    _, e = evaluate(best_x) from scratch (the reported number carries no drift of the incremental E);  x_all[r] = best_x, e_all[r] = e.
//   winner    the replica with the smallest (e, r): e_all[r] < e_all[r'] or equal and r < r' (replica 0 if no energy compares, i.e. all NaN).
// Every result is written with plain vector stores; no atomics of any kind.
#include "common.h"
#include "../../include/panst3r_hip.h"
#include <cmath>

#pragma clang fp contract(off)

namespace pst {

constexpr int QS_NMAX = 200;            // N * N * 4 <= 160 000 B of the CU's 163 840 B of LDS
constexpr int QS_WAVES = 16;            // replicas per workgroup at most
constexpr int QS_CUS = 256;             // an MI355X has 256 CUs: the waves per workgroup are chosen so that the workgroups fill them first.  Up to 256 replicas
                                        // every replica is a workgroup of its own and pays N * N * 4 B of global -> LDS traffic for one wave (not measured)

struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

__device__ __forceinline__ float exp_neg(float a) {
  if (!(a >= -87.0f)) return 0.0f;
  const float n = rintf(a * 1.44269502e+00f);                       // v_rndne_f32: exact
  const float r = (a - n * 6.93145752e-01f) - n * 1.42860677e-06f;      // LN2_HI = 0x3f317200 (n * LN2_HI is exact), LN2_LO = ln 2 - LN2_HI
  float p = 1.98412698e-04f;                                        // 1 / 5040
  p = p * r + 1.38888889e-03f;                                      // 1 / 720
  p = p * r + 8.33333333e-03f;                                      // 1 / 120
  p = p * r + 4.16666667e-02f;                                      // 1 / 24
  p = p * r + 1.66666667e-01f;                                      // 1 / 6
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  return __int_as_float(__float_as_int(p) + (int)n * (1 << 23));      // n >= -126: the exponent field stays positive
}

__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// `evaluate` of the header comment: the fields of x from scratch and its energy, both in a fixed order
__device__ __forceinline__ float evaluate(const uint64_t (&xm)[4], const float* __restrict__ Wl, int N, int lane, float lamN, float (&h)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) h[q] = 0.0f;
  int cnt = 0;
#pragma unroll
  for (int qj = 0; qj < 4; ++qj)
    for (int l = 0; l < 64 && 64 * qj + l < N; ++l)
      if ((xm[qj] >> l) & 1) {
        const float* row = Wl + (64 * qj + l) * N;
        ++cnt;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (lane + 64 * q < N) h[q] = h[q] + row[lane + 64 * q];
      }
  float e = 0.0f;
#pragma unroll
  for (int qk = 0; qk < 4; ++qk)
    for (int l = 0; l < 64 && 64 * qk + l < N; ++l)
      if ((xm[qk] >> l) & 1) e = e + lane_value(h[qk], l);
  return e + lamN * (float)cnt;
}

__global__ __launch_bounds__(64 * QS_WAVES) void qubo_anneal_kernel(const float* __restrict__ W, int N, int replicas, int num_iters, float beta0, float cinv,
                                                                   float lamN, uint32_t key0, uint32_t key1, uint8_t* __restrict__ x_all,
                                                                   float* __restrict__ e_all) {
  extern __shared__ float Wl[];
  for (int i = threadIdx.x; i < N * N; i += blockDim.x) Wl[i] = W[i];
  __syncthreads();                                                   // the only barrier: a wave without a replica may leave after it
  const int lane = threadIdx.x & 63;
  const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  if (r >= replicas) return;

  uint64_t xm[4], bx[4];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const u32x4 w = philox4x32_10((uint32_t)b, (uint32_t)r, 1u, 0u, key0, key1);
    xm[2 * b] = (uint64_t)w.x | ((uint64_t)w.y << 32);
    xm[2 * b + 1] = (uint64_t)w.z | ((uint64_t)w.w << 32);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int valid = N - 64 * q;                                    // bits of this mask that are variables
    xm[q] = valid >= 64 ? xm[q] : valid <= 0 ? 0ull : xm[q] & ((1ull << valid) - 1ull);
    bx[q] = xm[q];
  }
  float h[4], dg[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) dg[q] = lane + 64 * q < N ? Wl[(lane + 64 * q) * N + lane + 64 * q] : 0.0f;
  float E = evaluate(xm, Wl, N, lane, lamN, h);
  float bestE = E, beta = beta0;
  u32x4 w = {0u, 0u, 0u, 0u};
  for (int i = 0; i < num_iters; ++i) {
    if ((i & 1) == 0) w = philox4x32_10((uint32_t)(i >> 1), (uint32_t)r, 0u, 0u, key0, key1);
    const uint32_t wj = (i & 1) ? w.z : w.x, wu = (i & 1) ? w.w : w.y;
    const int j = __builtin_amdgcn_readfirstlane((int)__umulhi(wj, (uint32_t)N));
    const float u = (float)(wu >> 8) * 5.9604644775390625e-08f;      // 2^-24: exact
    const int jq = j >> 6, jl = j & 63;
    const float h0 = lane_value(h[0], jl), h1 = lane_value(h[1], jl), h2 = lane_value(h[2], jl), h3 = lane_value(h[3], jl);
    const float d0 = lane_value(dg[0], jl), d1 = lane_value(dg[1], jl), d2 = lane_value(dg[2], jl), d3 = lane_value(dg[3], jl);
    const float hj = jq == 0 ? h0 : jq == 1 ? h1 : jq == 2 ? h2 : h3;
    const float wjj = jq == 0 ? d0 : jq == 1 ? d1 : jq == 2 ? d2 : d3;
    const uint64_t xq = jq == 0 ? xm[0] : jq == 1 ? xm[1] : jq == 2 ? xm[2] : xm[3];
    const float s = ((xq >> jl) & 1) ? -1.0f : 1.0f;
    const float d = ((2.0f * s) * hj + wjj) + s * lamN;
    bool acc = d < 0.0f;
    if (!acc) acc = u < exp_neg(-(d * beta));
    if (acc) {
      const float* row = Wl + j * N;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (lane + 64 * q < N) h[q] = h[q] + s * row[lane + 64 * q];
        xm[q] ^= jq == q ? 1ull << jl : 0ull;
      }
      E = E + d;
      if (E < bestE) {
        bestE = E;
#pragma unroll
        for (int q = 0; q < 4; ++q) bx[q] = xm[q];
      }
    }
    beta = beta * cinv;
  }
  const float e = evaluate(bx, Wl, N, lane, lamN, h);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (lane + 64 * q < N) x_all[(int64_t)r * N + lane + 64 * q] = (uint8_t)((bx[q] >> lane) & 1);
  if (lane == 0) e_all[r] = e;
}

// the smallest (energy, replica): one workgroup, strided scan, tree in LDS; then the winner's x and energy are copied out
__global__ __launch_bounds__(256) void qubo_winner_kernel(const float* __restrict__ e_all, const uint8_t* __restrict__ x_all, int N, int replicas,
                                                          uint8_t* __restrict__ best_x, float* __restrict__ best_e) {
  __shared__ float se[256];
  __shared__ int si[256];
  const int tid = threadIdx.x;
  float be = 0.0f;
  int bi = -1;
  for (int i = tid; i < replicas; i += 256) {
    const float e = e_all[i];
    if (e == e && (bi < 0 || e < be)) { be = e; bi = i; }            // ascending i per thread: a tie keeps the lower index
  }
  se[tid] = be; si[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const float e2 = se[tid + o];
      const int i2 = si[tid + o];
      if (i2 >= 0 && (si[tid] < 0 || e2 < se[tid] || (e2 == se[tid] && i2 < si[tid]))) { se[tid] = e2; si[tid] = i2; }
    }
    __syncthreads();
  }
  const int win = si[0] < 0 ? 0 : si[0];
  for (int k = tid; k < N; k += 256) best_x[k] = x_all[(int64_t)win * N + k];
  if (tid == 0) *best_e = e_all[win];
}

}  // namespace pst

extern "C" int pst_qubo_anneal_max_n(void) { return pst::QS_NMAX; }

extern "C" int pst_qubo_anneal(const float* W, int N, int replicas, int num_iters, float T0, float T_end, float lambda_reg, uint64_t seed, uint8_t* x_all,
                               float* e_all, uint8_t* best_x, float* best_e, void* stream) {
  using namespace pst;
  if (!W || !x_all || !e_all || !best_x || !best_e) { set_error("qubo_anneal: null operand"); return PST_EINVAL; }
  if (N < 1 || N > QS_NMAX) {
    set_error("qubo_anneal: N = %d outside [1, %d] (W must fit in the LDS of one CU); solver='host' remains for such a problem", N, QS_NMAX);
    return PST_EINVAL;
  }
  if (replicas < 1 || replicas > (1 << 20) || num_iters < 0 || !(T0 > 0.0f) || !(T_end > 0.0f) || !std::isfinite(T0) || !std::isfinite(T_end) ||
      !std::isfinite(lambda_reg)) {
    set_error("qubo_anneal: bad argument (replicas=%d in [1, 2^20], num_iters=%d >= 0, T0=%g > 0, T_end=%g > 0, lambda_reg=%g finite)", replicas, num_iters,
              (double)T0, (double)T_end, (double)lambda_reg);
    return PST_EINVAL;
  }
  const float beta0 = (float)(1.0 / (double)T0);
  const float cinv = num_iters > 0 ? (float)std::pow((double)T0 / (double)T_end, 1.0 / (double)num_iters) : 1.0f;
  const float lamN = lambda_reg / (float)N;
  int waves = (replicas + QS_CUS - 1) / QS_CUS;
  waves = waves < 1 ? 1 : waves > QS_WAVES ? QS_WAVES : waves;
  const unsigned grid = (unsigned)((replicas + waves - 1) / waves);
  static unsigned long long seen = 0;
  once_per_device(seen, [] { (void)hipFuncSetAttribute((const void*)qubo_anneal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, QS_NMAX * QS_NMAX * 4); });
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(qubo_anneal_kernel, dim3(grid), dim3(64 * waves), (size_t)N * N * sizeof(float), st, W, N, replicas, num_iters, beta0, cinv, lamN,
                     (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), x_all, e_all);
  int rc = check_launch("qubo_anneal");
  if (rc) return rc;
  hipLaunchKernelGGL(qubo_winner_kernel, dim3(1), dim3(256), 0, st, e_all, x_all, N, replicas, best_x, best_e);
  return check_launch("qubo_anneal (winner)");
}
