// Token gather of the SigLIP text tower (reference src/panst3r/model/text_encoder.py:65-79, transformers SiglipTextEmbeddings):
//   out[b L + l, :] = tok_emb[ids[b, l], :] + pos_emb[l, :]          fp32, the residual stream the encoder layers start from.
// The rest of the tower runs on the fp32-input-MFMA GEMM / attention kernels (gemm_f32.hip with act 3 = tanh GELU, attn_f32.hip with a key-padding mask)
// and pst_layernorm / pst_l2norm_rows on strided pooled rows: nothing else of it needs a kernel of its own.
#include "common.h"
#include "../../include/panst3r_hip.h"

namespace pst {

// one block per token row, D / 4 float4 lanes.  A token id outside [0, vocab) is never dereferenced: its row becomes zeros and *status = PST_EINVAL
// (the caller validates the ids on the host first; this is the device-side guard, not the error path users see).
__global__ __launch_bounds__(256) void token_embed_kernel(const int32_t* __restrict__ ids, int L, const float* __restrict__ tok, int vocab,
                                                          const float* __restrict__ pos, int D, float* __restrict__ out, int64_t ldo, int32_t* status) {
  const int row = blockIdx.x;
  const int l = row % L;
  const int id = ids[row];
  const bool ok = id >= 0 && id < vocab;
  if (!ok && threadIdx.x == 0 && status) *status = PST_EINVAL;
  const float4* t = (const float4*)(tok + (int64_t)(ok ? id : 0) * D);
  const float4* p = (const float4*)(pos + (int64_t)l * D);
  float4* o = (float4*)(out + (int64_t)row * ldo);
  for (int c = threadIdx.x; c < D / 4; c += blockDim.x) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      const float4 a = t[c], b = p[c];
      v = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    o[c] = v;
  }
}

}  // namespace pst

extern "C" int pst_token_embed(const int32_t* ids, int B, int L, const float* tok, int vocab, const float* pos, int npos, int D, float* out,
                               int64_t ldo, int32_t* status, void* stream) {
  using namespace pst;
  if (!ids || !tok || !pos || !out || B <= 0 || L <= 0 || vocab <= 0 || D <= 0) { set_error("token_embed: bad shape / null operand"); return PST_EINVAL; }
  if (L > npos) { set_error("token_embed: sequence length %d exceeds the %d position embeddings", L, npos); return PST_EINVAL; }
  if (D % 4 || ldo % 4 || ldo < D || (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15) || ((uintptr_t)ids & 3)) {
    set_error("token_embed: need D %% 4 == 0, ldo %% 4 == 0, ldo >= D, 16-byte aligned tables and output"); return PST_EINVAL;
  }
  if ((int64_t)B * L > 0x7fffffff) { set_error("token_embed: too many rows"); return PST_EINVAL; }
  const int threads = D / 4 >= 256 ? 256 : ((D / 4 + 63) / 64) * 64;
  hipLaunchKernelGGL(token_embed_kernel, dim3((unsigned)(B * L)), dim3(threads), 0, (hipStream_t)stream, ids, L, tok, vocab, pos, D, out, ldo, status);
  return check_launch("token_embed");
}
