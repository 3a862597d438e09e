// Area-weighted vertex normals of an indexed triangle mesh (f17), bit-reproducible whatever the order in which the faces arrive: the contract is the
// mesh shading section of include/panst3r_hip.h (steps 1 - 8), restated in tests/mesh_shade_ref.py.  A face's vector e1 x e2 (fp64, every operation
// rounded on its own, as mesh_face.h writes it) is scaled by 2^sh, rounded to an integer of at most 52 bits and added to its three corners as TWO
// 64-bit integer limbs (hi = q >> 26, lo = q & (2^26 - 1)): integer addition is exact and commutes, so the sums do not depend on scheduling.  No float
// atomics.  With fewer than 2^33 additions of magnitude below 2^26 per word nothing overflows for any Nf < 2^31.
//   accumulate  one lane per face, 18 64-bit vector atomics (three corners x three axes x two limbs) into acc int64 [Nv, 3, 2] the caller zeroed
//   finish      one lane per vertex: S_a = fp64(hi) 2^26 + fp64(lo), n_a = fp32(S_a / sqrt_heron((Sx Sx + Sy Sy) + Sz Sz)), (0, 0, 0) for a zero sum
// One lane per face with scattered same-address atomics is the slow shape of an atomic pass; it runs once per mesh, not per camera
// (tests/diag/shade_bench.py, docs/experiments.md 6v).
#include "common.h"
#include "../../include/panst3r_hip.h"
#include "mesh_face.h"
#include "heron.h"

#pragma clang fp contract(off)

namespace pst {

constexpr int MN_T = 256;

__global__ __launch_bounds__(MN_T) void mesh_normals_accumulate_kernel(const float* __restrict__ vertices, int Nv, const int32_t* __restrict__ faces, int64_t Nf, int sh,
                                                                       unsigned long long* __restrict__ acc) {
  const int64_t f = (int64_t)blockIdx.x * MN_T + threadIdx.x;
  if (f >= Nf) return;
  const MeshFace t = mf_load(vertices, Nv, faces, (int)f);
  if (!t.ok) return;
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { e1[a] = (double)t.v[1][a] - (double)t.v[0][a]; e2[a] = (double)t.v[2][a] - (double)t.v[0][a]; }
  const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  long long hi[3], lo[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const long long q = (long long)rint(ldexp(c[a], sh));           // |c 2^sh| < 2^52 for the host's sh; half to even
    hi[a] = q >> 26;                                                // arithmetic: floor
    lo[a] = q & ((1ll << 26) - 1);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t v = faces[f * 3 + k];                             // mf_load checked the three indices
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (hi[a] != 0) atomicAdd(&acc[(v * 3 + a) * 2 + 0], (unsigned long long)hi[a]);      // two's complement: the signed sum
      if (lo[a] != 0) atomicAdd(&acc[(v * 3 + a) * 2 + 1], (unsigned long long)lo[a]);
    }
  }
}

__global__ __launch_bounds__(MN_T) void mesh_normals_finish_kernel(const long long* __restrict__ acc, int64_t Nv, float* __restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * MN_T + threadIdx.x;
  if (v >= Nv) return;
  double S[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) S[a] = (double)acc[(v * 3 + a) * 2 + 0] * 67108864.0 + (double)acc[(v * 3 + a) * 2 + 1];
  const double len2 = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2];
  float n[3] = {0.f, 0.f, 0.f};
  if (len2 != 0.0) {                                                // integers below 2^86: len2 is finite, and 0 only for three zero sums
    const double len = sqrt_heron(len2);
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = (float)(S[a] / len);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) normals[v * 3 + a] = n[a];
}

}  // namespace pst

extern "C" int pst_mesh_normals_accumulate(const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, int sh, int64_t* acc, void* stream) {
  using namespace pst;
  if (Nv <= 0 || Nv > 0x7fffffffLL || Nf <= 0 || Nf > 0x7fffffffLL || sh < -PST_MESH_NORMALS_MAX_SHIFT || sh > PST_MESH_NORMALS_MAX_SHIFT) {
    set_error("mesh_normals_accumulate: bad shape (Nv=%lld, Nf=%lld in [1, 2^31 - 1], |sh=%d| <= %d)", (long long)Nv, (long long)Nf, sh, PST_MESH_NORMALS_MAX_SHIFT);
    return PST_EINVAL;
  }
  if (!vertices || !faces || !acc) { set_error("mesh_normals_accumulate: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(mesh_normals_accumulate_kernel, blocks_for(Nf, MN_T), dim3(MN_T), 0, (hipStream_t)stream, vertices, (int)Nv, faces, Nf, sh, (unsigned long long*)acc);
  return check_launch("mesh_normals_accumulate");
}

extern "C" int pst_mesh_normals_finish(const int64_t* acc, int64_t Nv, float* normals, void* stream) {
  using namespace pst;
  if (Nv <= 0 || Nv > 0x7fffffffLL) { set_error("mesh_normals_finish: bad shape (Nv=%lld in [1, 2^31 - 1])", (long long)Nv); return PST_EINVAL; }
  if (!acc || !normals) { set_error("mesh_normals_finish: null operand"); return PST_EINVAL; }
  hipLaunchKernelGGL(mesh_normals_finish_kernel, blocks_for(Nv, MN_T), dim3(MN_T), 0, (hipStream_t)stream, (const long long*)acc, Nv, normals);
  return check_launch("mesh_normals_finish");
}
