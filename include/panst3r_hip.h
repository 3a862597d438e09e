/* panst3r_hip.h -- C ABI of libpanst3r_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the PanSt3R inference forward path.  Plain pointers, sizes and a HIP stream only: no
 * torch types, no allocation, no host synchronisation, no global state besides the last-error string.  The caller
 * (PyTorch-ROCm in panst3r_amd/hip.py, via ctypes) owns every buffer; kernels borrow the raw device pointers for
 * the duration of the enqueue.  Every entry point returns 0 on success, <0 on a rejected argument (PST_EINVAL) or
 * a HIP launch error (PST_ELAUNCH); pst_last_error() gives the text.  `stream` is a hipStream_t passed as void*.
 *
 * Each op states the reference (naver/panst3r v0.2.1, /root/reference) call site it replaces.  The reference has
 * no native code of its own: its "FFI" for this path are the torch ops / optional fused extensions listed in
 * SURVEY.md 2.1 (cuRoPE2D, xFormers memory-efficient attention, nn.MultiheadAttention, the einsum).
 *
 * Conventions: "16-bit" tensors are raw uint16 in ONE of two formats chosen per call by `dtype16` (PST_BF16 / PST_F16; all 16-bit
 * operands of a call share it; "bf16" in the text below reads "the 16-bit format"); activations are token-major [rows, channels]
 * row-major with an explicit leading dimension (elements); weights are torch nn.Linear layout [N, K] (K contiguous).
 *
 * fp32 mode (ABI 16; reference amp=False, tools/demo_panst3r.py:88: torch.float32 end to end): `dtype16` = PST_F32 is accepted by pst_gemm,
 * pst_attn_fwd, pst_rope2d, pst_patchify, pst_patch_rows, pst_l2norm_rows, pst_mean4, pst_resize_bilinear, pst_loftup_guidance_gn,
 * pst_groupnorm_apply and pst_loftup_lr_pe: the "16-bit" tensors of that call are then float (leading dimensions / strides still in
 * elements).  GEMM and attention run on the fp32-input MFMA (gemm_f32.hip, attn_f32.hip: exact fp32 products, fp32 accumulation; 1 / 16 of the 16-bit matrix rate) with the same epilogues;
 * rejected in this mode: a 16-bit C / residual, fused RoPE, the LayerNorm-fold arguments, pst_gemm_params.kernel != 0, attention
 * split-K, pst_mask_head, pst_split3, pst_rowstats (16-bit precision devices with nothing to do in fp32).
 */
#ifndef PANST3R_HIP_H
#define PANST3R_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PST_ABI_VERSION 20

/* element type codes: every `*_type` / `dtype16` argument below (and the former `*_fp32` flags: 0 and 1 keep their meaning) */
#define PST_BF16 0   /* bfloat16, raw uint16 */
#define PST_F32  1   /* float */
#define PST_F16  2   /* IEEE half, raw uint16 (amp="fp16": tools/demo_panst3r.py:88, src/panst3r/utils.py:206-215) */
#define PST_X3H  4   /* OUTPUT type of pst_layernorm*, pst_groupnorm_apply and pst_attn_x3 only (ABI 18): the result as the split A operand of a 3 x f16 GEMM - f16 rows of three blocks
                        [hi | hi | lo], each ld / 3 columns wide (the producer writes what pst_split_operand(side 0) would make of its fp32 result: no fp32 round trip) */

int pst_abi_version(void);
const char* pst_last_error(void);

/* ---------------------------------------------------------------- GEMM (+ fused epilogues, implicit 3x3 conv)
 * C[m, n] = epi( sum_k A[m,k] * W[n,k] ),  v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulate.
 *   epi(x) = res + gamma[n] * act(x + bias[n])        (each part optional)
 * Replaces: every nn.Linear / 1x1 conv / patch-embed conv / 3x3 conv on the path -- croco Mlp/Attention/
 * CrossAttention projections (model/blocks.py:18-26, input_mixer.py:13-20, pixel_shuffle.py:17-27), LoftUp convs
 * (loftup.py:122-130), MaskTransformer projections + FFN + MLP heads (mask_transformer.py:222-230,314,372,435-437)
 * and the query x pixel einsum "bqc,bnchw->bnqhw" (mask_transformer.py:280) with mask_feats kept pixel-major.
 * Requirements: K % 64 == 0, N % 4 == 0, lda/ldw multiples of 8, A/W 16-byte aligned; ldc % 4 == 0 with C 16-byte aligned when fp32 and
 * 8-byte aligned when 16-bit (so rows of a 16-bit C may be 8-byte but not 16-byte aligned: the 64 x 64, 128 x 128 and non-persistent 256 x 256
 * kernels store such rows in 8-byte halves; the persistent and row-streaming classes want ldc % 8 == 0 and a 16-byte aligned C and leave any other
 * layout to the tiled kernels, same bits).  A 16-bit residual: ldr % 8 == 0, 16-byte aligned; an fp32 one: ldr % 4 == 0.
 * Held to these layouts by tests/test_hip_gemm_layout.py.
 */
typedef struct pst_gemm_params {
  const void* A;  int64_t lda;       /* bf16 [M, K] (or NHWC image stack in conv mode) */
  const void* W;  int64_t ldw;       /* bf16 [N, K] */
  void* C;        int64_t ldc;       /* bf16 or fp32 [M, N] (or its transpose, see trans_out) */
  int32_t M, N, K;
  const float* bias;                 /* [N] or NULL */
  const float* gamma;                /* [N] LayerScale or NULL */
  const float* res;  int64_t ldr;    /* fp32 residual or NULL; row = res_mod ? m % res_mod : out_row(m) */
  int32_t res_mod;
  int32_t act;                       /* 0 none, 1 GELU(erf), 2 ReLU, 3 GELU(tanh) = 0.5x(1 + tanh(sqrt(2/pi)(x + 0.044715x^3))) (ABI 20; PST_F32 operands only, 16-bit: PST_EINVAL) */
  int32_t out_fp32;                  /* 0: bf16 C, 1: fp32 C */
  int32_t trans_out;                 /* 1: store C^T, i.e. C[n*ldc + m] (bf16 only; feeds attention V^T) */
  /* output row remap: out_row(m) = grp_in ? (m/grp_in)*grp_out + grp_off + m%grp_in : m   (e.g. skip a CLS row) */
  int32_t grp_in, grp_out, grp_off;
  /* pixel-shuffle store (F.pixel_shuffle fused, weight rows pre-permuted to [dy][dx][c]): ps_p > 0 enables.
     token m = (v, y, x) on a ps_h x ps_w grid; n = dy*(ps_p*ps_c) + r  ->  C[v][(ps_p*y+dy)][(ps_p*x)*ps_c + r] */
  int32_t ps_p, ps_c, ps_h, ps_w;
  /* implicit 3x3 conv (pad 1): conv_c > 0 enables.  A = NHWC [M = nimg*conv_h*conv_w, conv_c] bf16,
     K = 9*conv_c (tap-major, channel-minor), conv_c % 64 == 0, `zeros` = >=128 B of zero bytes on the device */
  int32_t conv_c, conv_h, conv_w;
  const void* zeros;
  /* RoPE-2D fused into the store (q,k projections): rope_hd == 64 enables (bf16 output, N % 64 == 0); rope_pos int32
     [rows, 2] (y, x) indexed by the A row m, rope_cs fp32 [npos, 16, 2] as for pst_rope2d_bf16. */
  const int32_t* rope_pos; const float* rope_cs; int32_t rope_hd;
  int32_t rope_npos;                 /* rows of rope_cs (positions); lets a kernel keep the whole table in LDS.  0 = unknown */
  int32_t res_bf16;                  /* 1: `res` points to bf16 (same indexing, ldr in elements) instead of fp32 */
  int32_t kernel;                    /* 0 = auto; 128 / 256 force the 128x128 / 256x256 tile kernel (tests, benchmarks) */
  /* strided batch: batch > 1 runs `batch` independent problems of this shape in ONE launch; problem i uses
     A + i*a_bs, W + i*w_bs, C + i*c_bs (bf16 / output elements) and bias + i*bias_bs.  gamma / res / conv / rope must be
     unused.  (The 12 per-layer K and V^T projections of a MUSt3R memory append are one launch each instead of 12.) */
  int32_t batch;
  int64_t a_bs, w_bs, c_bs, bias_bs;
  int32_t dtype16;                   /* PST_BF16 / PST_F16: format of A, W, a 16-bit C and a 16-bit residual; PST_F32: A, W, C, res all float (fp32 mode, above) */
  /* ---- LayerNorm folded into the GEMMs around it (pre-LN blocks: x += f(LN(x)) ; no stand-alone LayerNorm pass).
     PRODUCER side (the GEMM that writes the residual stream; plain row-major store, N % 64 == 0):
       xcopy      16-bit copy of the stored C values [M, N] with leading dim ldxc (C fp32 only; the consumer's A operand), or NULL
       stats_out  fp32 [M][stats_ld][2]: (sum, sum of squares) of the stored values of row m over the 64 columns [64 g, 64 g + 64),
                  written at [m][g]; stats_ld >= N / 64.  Deterministic (fixed-order lane reduction, no atomics).  NULL = off.
     CONSUMER side (ln_stats != NULL): A holds the RAW rows x (the producer's xcopy), W = W0 diag(ln_gamma) and bias = W0 beta + b0
     were folded at pack time, ln_colsum[n] = sum_k W[n,k] (fp32 sum of the 16-bit-rounded W).  With mean / rstd of row m from the
     ln_groups partials of ln_stats[m] over K elements:   C[m,n] = epi'( rstd (acc[m,n] - mean ln_colsum[n]) + bias[n] ). */
  void* xcopy; int64_t ldxc;
  float* stats_out; int32_t stats_ld;
  const float* ln_stats; int32_t ln_groups; const float* ln_colsum; float ln_eps;
  /* ---- (ABI 18) split store: x3_block > 0 with out_fp32 = 1 stores the fp32 result as the f16 split A operand of the NEXT 3 x f16 GEMM instead (PST_X3H):
     C = f16 [M, 3 x3_block], ldc in f16 elements, row m = [hi | hi | lo] with hi = rn16(v), lo = rn16(v - hi), blocks of x3_block >= N columns
     (x3_block % 4 == 0; the caller zero-fills columns N .. x3_block if any).  Plain row-major store (no ps / trans_out / xcopy / stats_out); dtype16 = PST_F16.
     The MLP's hidden activation GELU(fc1) goes to fc2 this way: no fp32 round trip and no split pass. */
  int32_t x3_block;
} pst_gemm_params;

int pst_gemm(const pst_gemm_params* p, void* stream);
/* name of the kernel variant pst_gemm dispatches `p` to ("gemm_kernel<4,4,false>", "gemm256_kernel", ...), without launching:
 * what a profiler row of this call is called (bench.py attributes its HIP-event timings with it). NULL for a rejected argument. */
const char* pst_gemm_variant(const pst_gemm_params* p);
/* Two INDEPENDENT GEMMs in ONE launch where that pays; any other pair runs as two pst_gemm launches.  Results are bit-identical to two pst_gemm
 * calls either way.  Fused cases:
 *   - `a` with a row-major store and `b` with trans_out (the q|k and V^T projections of an attention layer: croco Attention's qkv Linear, models/blocks.py -
 *     same A operand, different epilogues) when both resolve to the 64 x 64-tile kernel (the 768-row GEMMs of the sequential memory build: launch latency
 *     and the cold first operand fetch are shared);  variant "gemm_pair_kernel<2,2>"
 *   - (ABI 17) two big problems of the SAME persistent-kernel class (both plain 16-bit / both fp32 residual stream / both transposed) - the same layer of
 *     two independent ViTs, e.g. the CroCo encoder of the views that are not keyframes and DINOv2 of all views (panst3r.py:174-175,229-230): the chip's
 *     workgroups are split between the two tile lists so that both finish in the same number of rounds (tile quantisation: 408 + 608 tiles of 256 x 256
 *     cost 2 + 3 rounds of 256 CUs on their own, 4 side by side);  variant "gemm256p2_kernel"
 * pst_gemm_pair_variant: the fused kernel's name, or "" when the pair is not fused. */
int pst_gemm_pair(const pst_gemm_params* a, const pst_gemm_params* b, void* stream);
const char* pst_gemm_pair_variant(const pst_gemm_params* a, const pst_gemm_params* b);
/* Tuning knob of the GEMM dispatch (process-wide; measurement tools and tests only - results never depend on it, every GEMM variant
 * is bit-identical).  Returns the previous value, or -1 for an unknown knob.  (3, 6 and 11 were knobs of retired experiments: unknown now, never reused.) */
#define PST_TUNE_PAIR 4         /* 1 (default): pst_gemm_pair may put two big problems side by side in one persistent launch, 0: never */
#define PST_TUNE_DEEP_RING 8    /* LDS slabs of the 64x64-tile GEMM when a launch has at most one tile per CU: 4 (the ring of every other launch), 6 or 8 */
#define PST_TUNE_PAIR_ATTN 7    /* 1 (default): pst_attn_pair may put two attention problems into one launch, 0: never */
#define PST_TUNE_ATTN_XCD 9     /* 1 (default): attention blocks in XCD-contiguous order (the query blocks of one head share its K / V tiles through ONE L2), 0: plain order */
#define PST_TUNE_CUS 10        /* CUs the launches enqueued from now on may assume (grid of the persistent kernels): set around work enqueued on a CU-masked stream (hipExtStreamCreateWithCUMask); 0 (default) = all CUs of the device */
#define PST_TUNE_PAIR_RES 5     /* 1 (default): ... including fp32 residual-stream problems at K >= 1024 that would run on the 128x128 kernel on their own */
int pst_tune(int knob, int value);

/* ---------------------------------------------------------------- query x pixel mask einsum (HBM-bound streaming form)
 * pred_masks[v][q][p] = sum_c E[q][c] * F[v][p][c]  (reference mask_transformer.py:280 "bqc,bnchw->bnqhw" with pixel-major mask features):
 * E 16-bit [Q, C] (row stride lde), F 16-bit [nviews][P][C] (view stride f_view_stride elements), out fp32 [nviews][Q][P] (view stride
 * out_view_stride elements).  One launch for all views of a shape group: E stays in registers, F is streamed once.  Bit-identical to pst_gemm
 * on the same operands.  Supported: Q <= 256, P % 64 == 0, C in {256, 384} (pst_mask_head_supported); other shapes: pst_gemm. */
int pst_mask_head_supported(int Q, int P, int C);
int pst_mask_head(const void* E, int64_t lde, const void* F, int64_t f_view_stride, float* out, int64_t out_view_stride, int nviews, int Q, int P, int C,
                  int dtype16, void* stream);

/* ---------------------------------------------------------------- fused attention forward (flash style)
 * O[b,h,q,:] = softmax_k( scale * Q[b,h,q,:] . K[b,h,k,:]  (+ -inf where mask[b,q,k]) ) V[b,h,k,:]
 * bf16 in/out, fp32 softmax/accumulate, head dim 64 or 96.  V is given TRANSPOSED: Vt[b,h,d,k] (k contiguous).
 * Replaces: xFormers memory-efficient attention / SDPA inside croco Attention & CrossAttention, HF Dinov2
 * attention, and nn.MultiheadAttention incl. its bool attn_mask (mask_transformer.py:264-272,314,372).
 * Strides are in elements.  mask: uint8 [B, Nq, Nk] (1 = blocked), shared by all heads, or NULL.
 *
 * The operand contract (all formats: 16-bit, fp32 operands, and the split planes of pst_attn_x3; tests/test_hip_attn_layout.py holds every kernel to it):
 *   strides  Batch and head strides of Q, K, Vt, O and m_bs, and the row strides q_rs, o_rs, m_rs, may be negative or zero: they only enter 64-bit
 *            address arithmetic (a zero m_bs shares one mask among the batches, a zero m_rs one row among the queries, a negative k_bs / v_bs walks the
 *            batches backwards).  k_rs and v_ds must be >= 0: the 16-bit kernels add them as 32-bit unsigned offsets, and every format refuses a negative
 *            one with PST_EINVAL.  The strides of O must send distinct (b, h, q) to distinct rows; that is not checked.
 *   read     Q rows [0, Nq) and K rows [0, Nk), hd columns each.  Of every V^T row the columns [0, Nk) and, in the 16-bit formats and in pst_attn_x3 (both
 *            planes), the rest of the last 8-key chunk [Nk, roundup8(Nk)): those values are multiplied by a probability of exactly 0, so they must be
 *            FINITE (any finite value; they do not reach the result).  The fp32-operand kernel does not read them.  Of every mask row the bytes [0, Nk)
 *            and, except in the fp32-operand kernel, [Nk, roundup4(Nk)), whose values are ignored.
 *   never    Q rows >= Nq, K rows >= Nk, V^T columns >= roundup8(Nk), mask bytes >= roundup4(Nk) and the other columns of a shared buffer are not read.
 *            Of O only the hd columns of the B H Nq logical rows are written, of `ws` only its first pst_attn_workspace_bytes; nothing else of either is
 *            read or written.
 */
typedef struct pst_attn_params {
  const void* Q;  int64_t q_bs, q_hs, q_rs;   /* batch / head / row strides */
  const void* K;  int64_t k_bs, k_hs, k_rs;
  const void* Vt; int64_t v_bs, v_hs, v_ds;   /* batch / head / head-dim-row strides (key contiguous) */
  void* O;        int64_t o_bs, o_hs, o_rs;
  const uint8_t* mask; int64_t m_bs, m_rs;
  int32_t B, H, Nq, Nk, hd;
  float scale;
  const void* zeros;                           /* >=128 B of zero bytes on the device */
  /* split-K ("flash-decoding") for few queries x many keys: nsplit > 1 splits the key range over nsplit blocks per
     query block; partial (O, max, sum) go to `ws` (fp32, >= pst_attn_workspace_bytes) and a combine kernel merges. */
  int32_t nsplit;
  void* ws; int64_t ws_bytes;
  int32_t dtype16;                             /* PST_BF16 / PST_F16 / PST_F32 (fp32 mode: hd 64 / 96, nsplit <= 1): format of Q, K, Vt, O */
  /* 1: Q already carries scale * log2(e) (the model path folds it into the q projection's epilogue, pst_gemm_params.gamma, so it is
     applied in fp32 before q is rounded): the kernel computes p = exp2(q.k - m) with no per-score multiply and ignores `scale`. */
  int32_t prescaled;
} pst_attn_params;

int64_t pst_attn_workspace_bytes(int B, int H, int Nq, int hd, int nsplit);

int pst_attn_fwd(const pst_attn_params* p, void* stream);
const char* pst_attn_variant(const pst_attn_params* p);   /* as pst_gemm_variant */
/* (ABI 17) Two INDEPENDENT attention problems in ONE launch when both take the same 128-query kernel variant (same format, head dim, softmax mode, no key
 * split) - the self-attentions of the two ViT towers that run in lock-step (see pst_gemm_pair): one grid over both block lists, so the last partial round of
 * resident blocks is shared; any other pair runs as two pst_attn_fwd launches.  Bit-identical either way.  pst_attn_pair_variant: "attn2_kernel<64,2>" /
 * "attn2_kernel<96,2>", or "" when not fused. */
int pst_attn_pair(const pst_attn_params* a, const pst_attn_params* b, void* stream);
const char* pst_attn_pair_variant(const pst_attn_params* a, const pst_attn_params* b);

/* ---------------------------------------------------------------- LayerNorm
 * y = (x - mean) / sqrt(var + eps) * gamma + beta over the last dim D (D % 4 == 0, D <= 4096), fp32 statistics.
 * in_fp32/out_fp32 are element type codes (PST_BF16 / PST_F32 / PST_F16); input row remap as in GEMM (grp_*), output leading dim ldy.
 * Replaces nn.LayerNorm everywhere on the path (eps 1e-6 backbones, 1e-5 PanSt3R-owned modules).
 */
int pst_layernorm(const void* x, int64_t ldx, int in_fp32, void* y, int64_t ldy, int out_fp32,
                  const float* gamma, const float* beta, int rows, int D, float eps,
                  int grp_in, int grp_out, int grp_off, void* stream);
/* y = LN(x + add): `add` fp32 rows with ld_add, indexed like x (the feedback term of the MUSt3R memory entries:
 * entry_l = h_l + fb, then norm_y -- one launch instead of add_cast + layernorm). */
int pst_layernorm_add(const void* x, int64_t ldx, int in_fp32, const float* add, int64_t ld_add, void* y, int64_t ldy,
                      int out_fp32, const float* gamma, const float* beta, int rows, int D, float eps,
                      int grp_in, int grp_out, int grp_off, void* stream);

/* ---------------------------------------------------------------- SigLIP text tower (ABI 20)
 * token_embed: out[b L + l, :] = tok[ids[b, l], :] + pos[l, :]  (transformers SiglipTextEmbeddings; reference text_encoder.py:65-79 via
 * SiglipTextModel).  ids int32 [B, L] contiguous, tok fp32 [vocab, D], pos fp32 [npos, D] (L <= npos), out fp32 rows with leading dim ldo;
 * D % 4 == 0, 16-byte aligned tables.  An id outside [0, vocab) is never read: its row is written as zeros and, when `status` (int32 on the
 * device) is not NULL, *status = PST_EINVAL - the caller validates ids beforehand and reads `status` afterwards.
 * The rest of the tower needs no entry point of its own: pst_gemm in fp32 mode (act 3 for the MLP), pst_attn_fwd in fp32 mode with the
 * tokenizer's key-padding mask (uint8 [B, Lpad], m_rs = 0, Lpad % 4 == 0, 1 = blocked), pst_layernorm / pst_gemm on the pooled rows
 * (leading dim L D), pst_l2norm_rows. */
int pst_token_embed(const int32_t* ids, int B, int L, const float* tok, int vocab, const float* pos, int npos, int D, float* out, int64_t ldo,
                    int32_t* status, void* stream);

/* rowstats: the producer-side outputs of the LayerNorm fold for a stream that no GEMM produced (first block of a stack): x [rows, D] of
 * element type x_type (PST_F32, or the 16-bit format itself), D % 64 == 0 -> xcopy 16-bit [rows, D] (optional: NULL when x already is
 * the 16-bit stream) and stats fp32 [rows][stats_ld][2] = per-row (sum, sum of squares) over each 64-column group. */
int pst_rowstats(const void* x, int64_t ldx, int x_type, void* xcopy, int64_t ldxc, float* stats, int stats_ld, int rows, int D, int dtype16,
                 void* stream);

/* strided batch of pst_layernorm_add: problem i uses x + i*x_bs, y + i*y_bs, gamma/beta + i*w_bs (elements); `add` (optional) is shared.
 * One launch for the 12 per-layer `norm_y(h_l + feedback)` of a MUSt3R memory append. */
int pst_layernorm_add_batch(const void* x, int64_t ldx, int in_fp32, const float* add, int64_t ld_add, void* y, int64_t ldy,
                            int out_fp32, const float* gamma, const float* beta, int rows, int D, float eps,
                            int grp_in, int grp_out, int grp_off, int nbatch, int64_t x_bs, int64_t y_bs, int64_t w_bs,
                            void* stream);

/* split3: fp32 x [rows, K] -> bf16 [rows, 3K] = [x_hi | x_hi | x_lo] with x_hi = bf16(x), x_lo = bf16(x - x_hi).  Multiplied by
 * weights packed as [W_hi | W_lo | W_hi] (one pst_gemm_bf16 over 3K, fp32 output) this evaluates x W^T with ~16 mantissa bits on
 * the bf16 MFMA path.  Used for the 200-query mask-embedding MLP (mask_transformer.py:230), whose result is one factor of the
 * ill-conditioned query x pixel product. */
int pst_split3(const float* x, int64_t ldx, void* out, int64_t ldo, int rows, int K, int dtype16, void* stream);

/* ---------------------------------------------------------------- fp32-grade contractions at three 16-bit MFMAs per product (ABI 18)
 * The reference's default is fp32 (amp=False, tools/demo_panst3r.py:88), and under --amp it still runs the whole panoptic decoder and the render of the
 * views that are not keyframes in fp32 (src/panst3r/panst3r.py:236-245,268).  With x = x_hi + x_lo (x_hi = rn16(x), x_lo = rn16(x - x_hi): 22 mantissa bits in
 * f16) a product is x_hi y_hi + x_hi y_lo + x_lo y_hi to 2^-22, so a GEMM on fp32 operands is ONE 16-bit pst_gemm over a 3 x longer K and attention
 * takes (hi, lo) planes - the 16-bit matrix rate / 3 instead of the fp32-input MFMA's 1 / 16.
 *   split_operand  x fp32 [rows, K] -> 16-bit [rows, 3 Kpad]: three blocks of Kpad columns (zero beyond K), side 0 (a GEMM's A operand) [hi | hi | lo],
 *                  side 1 (its W operand, nn.Linear layout) [hi | lo | hi]; with an implicit 3x3 conv the pixel rows of the NHWC image are split with
 *                  Kpad = conv_c (conv_c' = 3 conv_c) and the weights per tap.  pst_split3 is side 0 with Kpad = K.
 *   split2         x fp32 [rows, K] -> planes hi, lo 16-bit [rows, ldo], or with transpose != 0 the planes of x^T ([K, ldo], ldo >= rows): the V^T operand
 *   transpose_f32  y[c][r] = x[r][c]
 *   attn_x3        pst_attn_fwd on split operands: p->Q / K / Vt are the hi planes (format p->dtype16), Q_lo / K_lo / Vt_lo the lo planes with the SAME
 *                  strides, p->O is fp32 (out_type PST_F32, strides in floats) or, with out_type PST_X3H, f16 rows [hi | hi | lo] with blocks of out_block
 *                  columns (strides in f16 elements; the A operand of the output projection).  Softmax in fp32; P is split in registers; mask / split-K /
 *                  prescaled as pst_attn_fwd. */
int pst_split_operand(const float* x, int64_t ldx, void* out, int64_t ldo, int rows, int K, int Kpad, int side, int dtype16, void* stream);
int pst_split2(const float* x, int64_t ldx, void* hi, void* lo, int64_t ldo, int rows, int K, int transpose, int dtype16, void* stream);
int pst_transpose_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int cols, void* stream);
/* rope2d_split: pst_rope2d on fp32 rows x [rows, nheads*hd] (leading dimension ld) written as the (hi, lo) planes of the rotated values ([rows, ldo] each): the
 * rotation in front of pst_attn_x3 without an fp32 write-back and a second pass (same arithmetic as pst_rope2d followed by pst_split2) */
int pst_rope2d_split(const float* x, int64_t ld, const int32_t* pos, const float* cs, void* hi, void* lo, int64_t ldo, int rows, int nheads, int hd, int dtype16,
                     void* stream);
int pst_attn_x3(const pst_attn_params* p, const void* Q_lo, const void* K_lo, const void* Vt_lo, int out_type, int64_t out_block, void* stream);
const char* pst_attn_x3_variant(const pst_attn_params* p);   /* as pst_attn_variant: NULL for parameters pst_attn_x3 refuses */

/* ---------------------------------------------------------------- RoPE-2D (in place on bf16 q and k)
 * Replaces cuRoPE2D / RoPE2D 'RoPE100' (README.md:67-71, input_mixer.py:16): per head the first hd/2 channels
 * rotate with pos y, the last hd/2 with pos x.  x: [rows, nheads*hd] slices of a row-major buffer with ld;
 * pos int32 [rows, 2] (y, x); cs: fp32 table [npos, hd/4, 2] (cos, sin).
 */
int pst_rope2d(void* x, int64_t ld, const int32_t* pos, const float* cs, int rows, int nheads, int hd, int dtype16,
               void* stream);

/* ---------------------------------------------------------------- image -> patch rows
 * patchify: img fp32 [nimg, C, H, W] -> bf16 rows [nimg*(H/p)*(W/p), ld] with column (c*p + dy)*p + dx,
 * zero padded up to ld (patch-embed conv as GEMM; Dust3r 16x16 and DINOv2 14x14).
 * dino_preprocess: reference model/dino.py:61-66 -- [-1,1] -> ImageNet normalise -> bilinear resize
 * (align_corners=False) to [nimg, 3, Ho, Wo] fp32.
 */
int pst_patchify(const float* img, void* out, int64_t ld, int nimg, int C, int H, int W, int p, int dtype16, void* stream);
int pst_dino_preprocess(const float* img, float* out, int nimg, int H, int W, int Ho, int Wo, void* stream);

/* ---------------------------------------------------------------- input side
 * image_prepare: the reference's `load_images` transform on the device (tools/demo_panst3r.py:94-114): decoded uint8 RGB [Hs, Ws, 3]
 *   -> ImgNorm (ToTensor + Normalize(0.5, 0.5): [-1, 1]) -> resize to (Hr, Wr), bilinear with antialiasing (what
 *   torchvision.transforms.Resize does to a tensor) -> crop [top, top+H) x [left, left+W) -> fp32 [3, H, W].
 *   (`get_resize_function` itself is un-vendored must3r code: the (Hr, Wr, top, left) recipe is restated on the host, parity unpinned.)
 * patch_rows: fp32 images [nimg, 3, H, W] in [-1, 1] -> the patch-row operands of BOTH patch-embed GEMMs in one launch (either may be
 *   NULL):  enc  16-bit [nimg*T, ld_enc]: p_enc x p_enc patches, column (c*p + dy)*p + dx, zero padded    (== pst_patchify)
 *           dino 16-bit [nimg*T, ld_dino]: p_dino x p_dino patches of the image ImageNet-normalised and bilinearly resized to
 *                (H/p_enc*p_dino, W/p_enc*p_dino), bit-identical to pst_dino_preprocess + pst_patchify without the fp32 intermediate
 *                (model/dino.py:61-66).  dino_transposed: DINOv2 takes the transposed image (portrait views, model/dino.py:15-47). */
int pst_image_prepare(const uint8_t* src, int Hs, int Ws, float* dst, int Hr, int Wr, int top, int left, int H, int W, void* stream);
int pst_patch_rows(const float* img, void* enc, int64_t ld_enc, void* dino, int64_t ld_dino, int nimg, int H, int W, int p_enc, int p_dino,
                   int dino_transposed, int dtype16, void* stream);

/* ---------------------------------------------------------------- elementwise helpers
 * add_cast: y = a + (b ? b[row % b_mod] : 0); a_fp32 / b_fp32 / y_fp32 are element type codes; [rows, D] with leading dims. */
int pst_add_cast(const void* a, int64_t lda, int a_fp32, const void* b, int64_t ldb, int b_fp32, int b_mod,
                 void* y, int64_t ldy, int y_fp32, int rows, int D, void* stream);
/* l2norm_rows: y = x / (||x|| + eps) per row (fp32 in, bf16 out) -- mask_transformer.py:225 */
int pst_l2norm_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int rows, int D, float eps, int dtype16, void* stream);

/* ---------------------------------------------------------------- panoptic query-decoder helpers
 * mean4: Fm[v, t, :] = mean of the central 2x2 pixels of token t's 8x8 block of the pixel-major mask features
 *   F [nimg, Hm, Wm, C] bf16  (== the 8x bilinear down-sampling of mask_transformer.py:283-287, exact).
 * attn_mask_from_logits: mask[q,k] = logits[q,k] < 0, rows that are fully blocked are cleared
 *   (mask_transformer.py:172,272).  logits fp32 [Q, Nk] -> uint8 [Q, Nk]. */
int pst_mean4(const void* F, void* Fm, int nimg, int Hm, int Wm, int C, int dtype16, void* stream);
/* resize_bilinear: F [nimg, Hs, Ws, C] bf16 -> Fd [nimg, Hd, Wd, C] bf16, F.interpolate(mode='bilinear',
 *   align_corners=False) semantics (mask_transformer.py:283-287 when the key grid of a portrait view is the transposed
 *   one, utils.py:47-49, so the resize is anisotropic and mean4 does not apply). */
int pst_resize_bilinear(const void* F, void* Fd, int nimg, int Hs, int Ws, int Hd, int Wd, int C, int dtype16, void* stream);
int pst_attn_mask_from_logits(const float* logits, int64_t ldl, uint8_t* mask, int64_t ldm, int Q, int Nk,
                              void* stream);

/* ---------------------------------------------------------------- LoftUp guidance branch (loftup.py:9-79,117-130,154-156)
 * guidance: img fp32 [nimg,3,H,W] -> 2x2 mean (bilinear /2) -> per-view per-channel min-max scale -> Fourier
 *   features (5 ch x nf freqs, sin & cos, learned biases [2,5,nf] read with the reference's reshape) + rgb
 *   -> fp32 [nimg, H/2*W/2, 10*nf+3] pixel-major, plus per-view sum / sum-of-squares (GroupNorm(1) statistics).
 * groupnorm_apply: y = relu?((x - mean_g) * rstd_g * gamma_c + beta_c) over pixel-major [nimg, P, C] with G groups,
 *   stats fp32 [nimg, G, 2] (sum, sumsq), bf16 output padded with zeros to ldy.
 * groupnorm_stats: accumulate (sum, sumsq) per (view, group) of a pixel-major tensor. */
#define PST_STATS_BLOCKS 128   /* max partial-sum blocks per view of the deterministic two-level reductions */
/* Buffer sizes (floats): feats >= nimg*(P*(10*nf+3) + 3*P + 6) (features, then scratch);
   guidance stats >= nimg*2*(1 + PST_STATS_BLOCKS);  groupnorm stats >= nimg*G*2*(1 + PST_STATS_BLOCKS).
   The result occupies the first nimg*2 / nimg*G*2 floats; the rest holds per-block partial sums (no atomics: the
   statistics are bit-reproducible). */
/* guidance_gn: the same features followed by GroupNorm(1 group, affine) WITHOUT materialising them: a statistics pass and a
 *   normalise-and-store pass both recompute the features per pixel (no fp32 feature round trip through HBM).
 *   y bf16 [nimg*P, ldy], columns [10*nf+3, ldy) zero; scratch >= nimg*(3*P + 6) floats; stats as for pst_loftup_guidance.
 *   ldy: a multiple of 8, 10*nf+3 <= ldy <= 512; a 16-bit y stages 64 rows of ldy + 8 elements in LDS, which fits the 64 KiB a block may ask for up to
 *   ldy = 496: a larger 16-bit ldy is PST_EINVAL (fp32 rows use no tile: up to 512).
 *   (loftup.py:117-124: fourier_feat -> first GroupNorm of first_conv)
 *   mm_ext (ABI 17): NULL = every view is scaled with its OWN per-channel min / max (the demo's max_bs=1 convention, tools/demo_panst3r.py:201); else
 *   fp32 [nimg][3][2] (min, max) per (view, channel) to scale with - the reference's MinMaxScaler takes min / max over the whole chunk of views it is
 *   handed (loftup.py:14-19; panoptic_decoder.py:50-62 chunks by max_bs): pst_loftup_minmax gives the per-view table, pst_minmax_merge pools it
 *   over the views of a chunk (scope[v] = chunk id of view v; out of place). */
int pst_loftup_guidance_gn(const float* img, const float* biases, const float* gamma, const float* beta, float eps,
                           float* scratch, float* stats, void* y, int64_t ldy, int nimg, int H, int W, int nf, int dtype16,
                           const float* mm_ext, void* stream);
int pst_loftup_minmax(const float* img, float* mm, int nimg, int H, int W, void* stream);
int pst_minmax_merge(const float* mm, const int32_t* scope, float* out, int nviews, void* stream);
int pst_groupnorm_stats(const void* x, int64_t ldx, int x_fp32, float* stats, int nimg, int P, int C, int G,
                        void* stream);
int pst_groupnorm_apply(const void* x, int64_t ldx, int x_fp32, const float* stats, const float* gamma,
                        const float* beta, void* y, int64_t ldy, int nimg, int P, int C, int G, float eps, int relu,
                        int dtype16, void* stream);
/* lr_pe: low-res positional features of loftup.py:159-162 (ImplicitFeaturizer(color_feats=False, n_freqs=5)):
 * writes bf16 [h*w, 20] into columns [col0, col0+20) of a row-major buffer with ld (per view identical). */
int pst_loftup_lr_pe(const float* biases, void* out, int64_t ld, int col0, int nimg, int h, int w, int dtype16, void* stream);

/* ---------------------------------------------------------------- panoptic post-processing
 * GPU replacement of `panoptic_inference_v2` (engine/postprocess.py:14-130; called by tools/demo_panst3r.py:242 with
 * device='cpu').  Everything stays on the device; the surviving-query set is a flag array, so a filter round needs no
 * host sync.  Per scene:  pp_scores once;  per round {per view: pp_sigmoid, pp_argmax};  pp_select;  after the last
 * round per view: pp_finalize.  Q <= 1024.
 *   pp_scores   class logits fp32 [Q,Ncls] -> scores = max sigmoid (or softmax(sigmoid/T).max when temperature > 0),
 *               labels = first argmax, keep = max sigmoid > cls_threshold                       (:40-47)
 *   pp_sigmoid  mask logits fp32 [Q,P] of one view -> probabilities [Q,P] for queries with keep != 0  (:20)
 *   pp_argmax   per pixel of the H x W output: bilinear (align_corners=False) taps of the h x w probabilities of every
 *               kept query, best_q = argmax_q score_q * m_q (first maximum; -1 when nothing is kept), best_m = m of the
 *               winner; cnt_orig[q] += #(m_q >= 0.5), cnt_mask[q] += #(best_q == q && m_q >= mask_threshold)
 *               (integer atomics, accumulated over the views of the scene)                      (:21,64,78,86-88)
 *   pp_argmax_logits  the same from the raw logits: one block per 8x32 output tile keeps the sigmoid of the tile's
 *               low-res footprint in LDS (8 queries at a time), so the logits are read once and no probability scratch
 *               exists.  Returns PST_EINVAL when the footprint does not fit (strong down-sampling): use the pair above.
 *   pp_select   keep_out[q] = keep[q] && cnt_mask > 0 && cnt_orig > 0 && !(cnt_mask / cnt_orig < overlap_threshold)
 *               (double division), seg_id[q] = 1-based running count over the selected queries, 0 otherwise; the two
 *               counters are reset to 0                                                          (:89-104)
 *   pp_finalize pan = seg_id[best_q] if best_m >= mask_threshold else 0; conf = best_m or void_confidence (:105-106) */
int pst_pp_scores(const float* logits, int Q, int Ncls, float cls_threshold, float temperature, float* scores,
                  int* labels, int* keep, void* stream);
/* (ABI 19) label_mode='softmax' (engine/postprocess.py:48-51): scores = softmax(logits).max, labels = its column, keep = label != Ncls - 1 (the
 * "no object" column of panoptic_decoder.py:66-67) && score > cls_threshold; the temperature is not read in this mode */
int pst_pp_scores_softmax(const float* logits, int Q, int Ncls, float cls_threshold, float* scores, int* labels, int* keep, void* stream);
int pst_pp_sigmoid(const float* logits, const int* keep, float* probs, int Q, int P, void* stream);
int pst_pp_argmax(const float* probs, const float* scores, const int* keep, int Q, int Hm, int Wm, int H, int W,
                  float mask_threshold, int* best_q, float* best_m, int* cnt_orig, int* cnt_mask, void* stream);
int pst_pp_argmax_logits(const float* logits, const float* scores, const int* keep, int Q, int Hm, int Wm, int H, int W,
                         float mask_threshold, int* best_q, float* best_m, int* cnt_orig, int* cnt_mask, void* stream);
int pst_pp_select(const int* keep, int* cnt_orig, int* cnt_mask, int Q, double overlap_threshold, int* keep_out,
                  int* seg_id, void* stream);
int pst_pp_finalize(const int* best_q, const float* best_m, const int* seg_id, int n, float mask_threshold,
                    float void_confidence, int* pan, float* conf, void* stream);

/* ---------------------------------------------------------------- QUBO post-processing (engine/postprocess.py:135-336)
 * The O(Q^2 x pixels) part of `panoptic_inference_qubo` on the device; the simulated annealing over the Q x Q matrix stays on the
 * host, as in the reference (:176-183 "Optimization done on CPU").
 *   qubo_upsample  mask logits fp32 [Q,hm,wm] of one view -> sigmoid -> bilinear (align_corners=False) to [Q,H,W] probabilities (:138-142)
 *   qubo_overlap   Wacc[Q][Q] (double, accumulated over the views of the scene) += sum_p min(m_i[p], m_j[p]) -- the overlaps AND, on the
 *                  diagonal, the mask areas of `weight_from_masks` (:243-254).  ws: >= pst_qubo_workspace_floats(Q, P) floats.
 *                  Deterministic: per-block partial sums, reduced over pixel chunks in index order.
 *   qubo_argmax    per pixel (max, first arg-max) over the probabilities of the selected queries `sel` (int32, ascending): conf and
 *                  instance index maps (:188). */
int pst_qubo_upsample(const float* logits, float* probs, int Q, int hm, int wm, int H, int W, void* stream);
int64_t pst_qubo_workspace_floats(int Q, int64_t P);
int pst_qubo_overlap(const float* probs, int Q, int64_t P, float* ws, double* Wacc, void* stream);
int pst_qubo_argmax(const float* probs, const int* sel, int nsel, int64_t P, float* conf, int* inst, void* stream);

/* ---------------------------------------------------------------- pointmap post-processing
 * The demo's camera recovery (tools/demo_panst3r.py:220-221,246-277) on the device, per scene instead of per view on the host:
 *   pointmap_activate  raw decoder output fp32 [npix, 7] -> pts3d [npix,3], pts3d_local [npix,3], conf [npix]
 *                      (must3r.engine.inference.postprocess, [3P]: mode 0 = 'norm_exp' xyz expm1(|xyz|)/|xyz|, 1 = linear; conf = 1 + exp(c))
 *   focal_weiszfeld    dust3r.post_process.estimate_focal_knowing_depth(focal_mode='weiszfeld'): pts3d_local [V, H*W, 3], principal points
 *                      pp [V, 2] (x, y) -> focal [V]; closed-form L2 start + `iters` (reference: 10) re-weighted least-squares steps
 *   rigid_moments      the sums roma.rigid_points_registration(x, y, weights=conf-1) needs: per view 16 doubles = sum w, sum w x (3),
 *                      sum w y (3), sum w y x^T (9); x = pts3d_local, y = pts3d, w = conf + weight_offset (reference: -1).  The 3x3
 *                      special-Procrustes SVD of the centred moment matrix is host work on 9 numbers.
 * One block per view, fixed-order double-precision reductions (bit-reproducible). */
int pst_pointmap_activate(const float* raw, float* pts3d, float* pts3d_local, float* conf, int64_t npix, int mode, void* stream);
int pst_focal_weiszfeld(const float* pts3d_local, const float* pp, float* focal, int nviews, int H, int W, int iters, void* stream);
int pst_rigid_moments(const float* x, const float* y, const float* conf, double* out, int nviews, int npix, float weight_offset, void* stream);

/* ---------------------------------------------------------------- ASMK retrieval (reference engine/retrieval.py:12-47, panst3r.py:88-125)
 * The checkpoint's retriever after its head (the head runs on pst_gemm / pst_layernorm in fp32 mode); restated in panst3r_amd/model/retrieval.py
 * [3P-recalled, parity unpinned].  Deterministic: fixed-order reductions, no atomics.
 *   retrieval_select     head output x fp32 [sum T_v, D] (view v = rows [in_off[v], in_off[v+1]), maxT >= every T_v <= 16384): per view the
 *                        out_off[v+1] - out_off[v] (<= T_v) rows of largest L2 norm (ties to the lower token), in that order, L2-normalised
 *                        (x / max(||x||, 1e-12)) -> out fp32 rows [out_off[v], out_off[v+1]); sel_idx (int32, optional) = the token of each out row
 *   retrieval_assign     the m (1..8, <= k) nearest centroids of each descriptor in L2: smallest ||c||^2 - 2 x.c, ties to the lower centroid, ascending.
 *                        x3 = pst_split_operand(descriptors, side 0), c3 = pst_split_operand(centroids, side 1) (f16, K3 = 3 Dpad columns,
 *                        K3 % 64 == 0), cnorm fp32 [k] (||c||^2 taken in double).  The centroid range is split over nsplit (1 .. ceil(k / 64))
 *                        workgroup columns; with nsplit > 1 the partial lists go to ws_dist / ws_ids (nsplit x n x m each) and a merge kernel
 *                        combines them in split order.  -> ids int32 [n, m], dist fp32 [n, m].  The n x k distance matrix is never formed.
 *   retrieval_aggregate  per group g (a (view, word) pair; members member[gstart[g] .. gstart[g+1]) in ascending descriptor order, word gword[g]):
 *                        s = fp32 sum of (x[member] - cent[word]) -> sums fp32 [ngroups, D] (optional) and bits uint32 [ngroups, D / 32]
 *                        (bit j of word w = s[32 w + j] > 0); D % 32 == 0
 *   retrieval_scores     S[i, j] = sum over the words held by query view i and database view j, ascending, of kappa(1 - 2 popcount(bq XOR bdb) / D),
 *                        kappa(s) = s^alpha if s >= tau else 0 (integer alpha <= 8 by repeated fp32 products); a view's groups are
 *                        [*_off[v], *_off[v+1]) sorted by word; max_q >= every query view's group count (<= 16384).  S fp32 [nq_views, ndb_views]. */
int pst_retrieval_select(const float* x, int64_t ldx, const int32_t* in_off, const int32_t* out_off, int nviews, int maxT, int D, float* out, int64_t ldo,
                         int32_t* sel_idx, void* stream);
int pst_retrieval_assign(const void* x3, int64_t ldx, const void* c3, int64_t ldc, const float* cnorm, int n, int k, int K3, int m, int nsplit,
                         float* ws_dist, int32_t* ws_ids, int32_t* ids, float* dist, int dtype16, void* stream);
int pst_retrieval_aggregate(const float* x, int64_t ldx, const float* cent, int64_t ldc, const int32_t* member, const int32_t* gstart, const int32_t* gword,
                            int ngroups, int D, float* sums, uint32_t* bits, void* stream);
int pst_retrieval_scores(const int32_t* q_off, const int32_t* q_word, const uint32_t* q_bits, const int32_t* db_off, const int32_t* db_word,
                         const uint32_t* db_bits, int nq_views, int ndb_views, int max_q, int D, float alpha, float tau, float* S, void* stream);

/* ---------------------------------------------------------------- panoptic point cloud (reference tools/demo_panst3r.py:279-300, 622-687: numpy on the host)
 * The scene's views concatenated in the caller's order, filtered by confidence (stable), coloured and labelled; restated in tests/cloud_ref.py
 * [restated, parity unpinned].  Integer atomics only, so every result is bit-reproducible.  A device table of pst_cloud_view makes a scene of
 * mixed shapes ONE launch: view v owns the ceil(npix / 1024) consecutive workgroups that start at first_wg (first_wg of view 0 is 0), nwg = their sum,
 * offset = the number of points of the views before it (total < 2^31).
 *   cloud_count           counts[wg] = number of the workgroup's 1024 points with conf >= thr (a NaN confidence is not kept)
 *   cloud_scan            base[i] = counts[0] + ... + counts[i-1] for i in [0, n]: base[n] = M, the number of kept points.  One workgroup.
 *   cloud_compact         the kept points in their original order -> rows [0, M) of
 *                           points fp32 [., 3]        pts3d
 *                           points_local fp32 [., 3]  x' = ((R00 x + R01 y) + R02 z) + t0 ... of pts3d_local, c2w = rows of [R | t]; every product and sum rounded on its own
 *                           rgb fp32 [., 3]           img * 0.5f + 0.5f, HWC order
 *                           pan int32 [.]
 *                           colors_out fp32 [., 3]    w1 * rgb + w2 * pan_vis (two rounded products, one rounded sum), pan_vis = colors[pan] for
 *                                                     0 < pan < ncolors (colors fp32 [ncolors, 3], ncolors <= 4096), black otherwise
 *                           index int64 [.]           offset + pixel: the point's position in the concatenated scene
 *                         Every output buffer must hold the scene's total number of points (M is only known on the device).
 *   cloud_segment_median  exact per-axis median of the rows of points_local whose pan id maps to a segment row: row = id2row[id] for 0 < id < ntab
 *                         (int32 [ntab], -1 = none; other ids take part in nothing), nseg rows.  Radix select, four byte passes (csrc/radix_select.h is the one
 *                         text of the passes, for this select and pst_depth_median's: signed keys here, groups of 3 slots).  m_ptr = device
 *                         pointer to M (base + n), max_points >= M sizes the grid.  Workspaces, all ZEROED by the caller: hist int32
 *                         [nseg, 3, 2, 256] (16-byte aligned; left zeroed), prefix uint32 / rank int32 [nseg, 3, 2], nan_cnt int32 [nseg, 3].
 *                         -> count int32 [nseg] (kept points of the segment), median fp32 [nseg, 3]: the middle element for an odd count,
 *                         (a + b) * 0.5f of the two middle ones for an even count (np.median of float32), NaN for an axis with a NaN or a count of 0.
 *                         The order is total: -inf < ... < -0.0 < +0.0 < ... < +inf (the two zeros are told apart, so the middle two of
 *                         {-0, -0, +0, +0} are -0 and +0 and their median is +0).  The sum and the product are plain fp32 operations, rounded
 *                         on their own: subnormal operands and results are kept (nothing is flushed), a sum beyond FLT_MAX is inf and stays inf,
 *                         -inf + inf is NaN.  Ties need no rule: equal keys are equal values. */
typedef struct pst_cloud_view {
  const float* conf;          /* [npix] */
  const float* pts3d;         /* [npix, 3] */
  const float* pts3d_local;   /* [npix, 3] */
  const float* img;           /* [3, npix] planes in [-1, 1] */
  const int32_t* pan;         /* [npix] */
  int64_t offset;
  int32_t npix;
  int32_t first_wg;
  float c2w[12];
} pst_cloud_view;

int pst_cloud_count(const pst_cloud_view* views, int nviews, int nwg, float thr, int32_t* counts, void* stream);
int pst_cloud_scan(const int32_t* counts, int n, int32_t* base, void* stream);
int pst_cloud_compact(const pst_cloud_view* views, int nviews, int nwg, float thr, const int32_t* base, const float* colors, int ncolors, float w1, float w2,
                      float* points, float* points_local, float* rgb, int32_t* pan, float* colors_out, int64_t* index, void* stream);
int pst_cloud_segment_median(const float* points_local, const int32_t* pan, const int32_t* m_ptr, int64_t max_points, const int32_t* id2row, int ntab, int nseg,
                             int32_t* hist, uint32_t* prefix, int32_t* rank, int32_t* nan_cnt, int32_t* count, float* median, void* stream);

/* ---------------------------------------------------------------- voxel fusion of the point cloud with multi-view label votes (no counterpart in the reference)
 * The rows [0, M) of a cloud (points fp32 [M, 3], rgb fp32 [M, 3], pan int32 [M], index int64 [M]) fused on a grid of cubic cells; restated in
 * tests/voxel_ref.py [restated, parity unpinned].  Every step is exact, so the outputs are held to the restatement bit for bit:
 *   1 cell      inv = fp32(1 / fp64(voxel_size)) (host); per axis t = p * inv (fp32, rounded on its own), c = floor(t).  A point with a non-finite
 *               coordinate or |c| >= 2^20 on any axis is left out and counted.
 *   2 position  q = int(floor((t - c) * 65536)) (fp32: the difference is ONE rounded operation - exact for t >= 0, correctly rounded for t < 0, where it
 *               reaches 1, q = 65536, for a tiny negative t - and the product is exact; 0 <= q <= 65536);
 *               per voxel the q of each axis are summed as 64-bit integers;
 *               pos = fp32((fp64(c) + fp64(sum) / fp64(count) * 2^-16) * fp64(voxel_size)), every fp64 operation rounded on its own.
 *   3 colour    u = floor(clamp(rgb, 0, 1) * 255 + 0.5) in fp32 (a NaN counts as 0), summed as integers; mean = fp32(fp64(sum) / fp64(count) / 255.0);
 *               colour = w1 * mean + w2 * colors[pan] (two rounded fp32 products, one rounded sum; black for void and ids >= ncolors).
 *   4 vote      every point votes for its pan id; ids <= 0, ids >= ntab and ids with id2row[id] < 0 are void.  The winner is the non-void id with the
 *               most votes, ties to the smallest id; a voxel with only void votes gets id 0 and votes = its count.
 *   5 order     voxels in increasing order of their smallest member row.
 * Only integer atomics touch shared state: two calls return identical bytes.  M <= 2^30 - 1; capacity = a power of two >= 2 M (<= 2^31), shared by the
 * two open-addressing tables; every probe loop is bounded by it, and a full table sets status[0] instead of spinning (the caller reads it and raises).
 * `merge` != 0 merges runs of adjacent lanes with one key inside a wave before the global atomics (same results).  Workspaces set by the caller:
 *   keys, pair_keys uint64 [capacity] = all ones; first int32 [capacity] = INT32_MAX; pair_cnt int32 [capacity], cnt int32 [M], sums uint64 [M, 6],
 *   best uint64 [M], status int32 [2] = 0.  Not initialised: point_slot int32 [M], slot_rank int32 [capacity], first_row int32 [M].
 *   voxel_insert      -> point_slot[i] = the table slot of point i's cell (-1: left out), first[slot] = the smallest member row, status[1] += left out
 *   voxel_count       counts[wg] = number of first points among the workgroup's 1024 rows; pst_cloud_scan of it gives base, base[n] = Mv
 *   voxel_rank        -> slot_rank[slot] = the voxel's output row, first_row[row] = its first point
 *   voxel_accumulate  -> cnt[row], sums[row] = (sum qx, qy, qz, sum r, g, b), the vote counts of the pairs (row << 32 | id) in pair_keys / pair_cnt,
 *                     point_voxel int32 [M] = the output row of every point (-1: left out)
 *   voxel_vote        -> best[row] = max over the voxel's pairs of (votes << 32) | (0xFFFFFFFF - id); 0 = no non-void vote
 *   voxel_emit        rows [0, *mv_ptr) of points, rgb, colors fp32 [., 3], pan, votes int32 [.], first_index int64 [.] (index of the first point);
 *                     count is cnt itself.  max_voxels >= Mv sizes the grid; every output holds M rows. */
int pst_voxel_insert(const float* points, int64_t M, float inv, uint64_t* keys, int64_t capacity, int32_t* first, int32_t* point_slot, int32_t* status,
                     int merge, void* stream);
int pst_voxel_count(const int32_t* point_slot, const int32_t* first, int64_t M, int32_t* counts, void* stream);
int pst_voxel_rank(const int32_t* point_slot, const int32_t* first, int64_t M, const int32_t* base, int32_t* slot_rank, int32_t* first_row, void* stream);
int pst_voxel_accumulate(const float* points, const float* rgb, const int32_t* pan, int64_t M, float inv, const int32_t* point_slot,
                         const int32_t* slot_rank, const int32_t* id2row, int ntab, int32_t* cnt, uint64_t* sums, uint64_t* pair_keys, int32_t* pair_cnt,
                         int64_t capacity, int32_t* point_voxel, int32_t* status, int merge, void* stream);
int pst_voxel_vote(const uint64_t* pair_keys, const int32_t* pair_cnt, int64_t capacity, uint64_t* best, void* stream);
int pst_voxel_emit(const float* points, const int64_t* index, const int32_t* first_row, const int32_t* mv_ptr, int64_t max_voxels, float inv,
                   double voxel_size, const int32_t* cnt, const uint64_t* sums, const uint64_t* best, const float* colors, int ncolors, float w1, float w2,
                   float* out_points, float* out_rgb, int32_t* out_pan, float* out_colors, int32_t* out_votes, int64_t* out_first, void* stream);

/* ---------------------------------------------------------------- 3-D connected components of the voxels and label despeckling (no counterpart in the reference)
 * The rows [0, Mv) of a voxel cloud (pan, count int32 [Mv], rgb fp32 [Mv, 3]) plus cells int32 [Mv, 3]; restated in tests/vcc_ref.py [restated, parity
 * unpinned].  Everything is integer arithmetic, so the outputs are held to the restatement bit for bit (additive entry points: the ABI version stays).
 *   cell        a voxel's cell is c = floor(fp32(p * inv)) of its first point, as step 1 of the voxel contract computes it (all members share it);
 *               |c| < 2^20 on every axis.
 *   adjacency   two voxels are adjacent under `connectivity` when their cells differ by at most 1 on every axis and the number of axes that differ is
 *               exactly 1 (6), 1 or 2 (18), 1 to 3 (26).  A neighbour cell with a coordinate outside (-2^20, 2^20) does not exist and is never looked
 *               up (its key field would wrap).
 *   component   a maximal set of voxels with one pan > 0 that is connected through adjacent voxels of that id.  A voxel with pan <= 0 (void) belongs to
 *               none: root = component = -1, never linked, never relabelled.  root[v] = the smallest voxel row of v's component (rows are in the order
 *               of first points); component[v] = the rank of root[v] among all roots in increasing order, in [0, C).
 *   table       per component, in that order: root, pan, size (voxels), points (sum of the voxels' count, int64), cell_lo / cell_hi (int32 per-axis min
 *               and max cell).  The host derives the metric box in fp64: lo = cell_lo * voxel_size, hi = (cell_hi + 1) * voxel_size.
 *   despeckle   a component is small when size < min_voxels.  For a small component every ordered pair (v, n) - v in it, n adjacent to v under the same
 *               connectivity, pan[n] > 0, n in a component that is not small - is one vote for pan[n].  The component takes the id with the most votes,
 *               ties to the smallest id (pst_voxel_vote's (votes << 32) | (0xFFFFFFFF - id), and that kernel); without a vote it becomes void, id 0 (a
 *               floater).  One round.  colour = w1 * rgb + w2 * colors[pan] as step 3 of the voxel contract blends it.
 * Integer atomics only; two calls return identical bytes.  Mv <= 2^30 - 1.  capacity = a power of two >= 2 Mv of the cell table (keys uint64 [capacity] =
 * all ones, rows int32 [capacity] not initialised), pair_capacity = a power of two of the vote table (pair_keys = all ones, pair_cnt = 0; min(ids, 26) Mv
 * distinct pairs at the most).  Every probe, find and union loop is bounded by the capacity or Mv; status int32 [4] = 0: status[0] collects the bits below
 * instead of spinning (the caller reads it with the result and raises), status[1] / status[2] = voxels relabelled / turned void by vcc_apply.
 *   vcc_cells    rows [0, *mv_ptr) of cells from the cloud's points and the fusion's first_row (max_voxels sizes the grid)
 *   vcc_build    cell key -> row into keys / rows (compare-and-swap claim, plain store of the row); parent[v] = v, -1 for a void voxel
 *   vcc_link     one voxel per lane, the lexicographically positive half of the neighbourhood (3, 9 or 13 cells); same id: wait-free union in parent
 *                (find with path halving; the larger root hooked under the smaller with atomicMin, retried from the returned value; parent values only
 *                decrease, so the root of a finished component is its smallest row)
 *   vcc_flatten  root[v] = find(v); size int32 [Mv] = 0, points int64 [Mv] = 0, cell_lo int32 [Mv, 3] = INT32_MAX, cell_hi = INT32_MIN, indexed by the
 *                ROOT's row, by atomicAdd / atomicMin / atomicMax.  `merge` != 0 reduces runs of adjacent lanes with one root inside the wave first.
 *   vcc_count    counts[wg] = roots among the workgroup's 1024 rows; pst_cloud_scan of it gives base, base[n] = C
 *   vcc_rank     rank_of[root row] = its rank, the table rows [0, C) (t_*), component int32 [Mv]
 *   vcc_votes    the votes of the voxels of small components into pair_keys / pair_cnt keyed by (root << 32) | id; pst_voxel_vote then gives best[root]
 *   vcc_apply    out_pan int32 [Mv], out_colors fp32 [Mv, 3] */
#define PST_VCC_FULL 1        /* a table ran full */
#define PST_VCC_DUPLICATE 2   /* two voxels share a cell */
#define PST_VCC_RANGE 4       /* a cell outside (-2^20, 2^20) */
#define PST_VCC_LOOP 8        /* a find / union loop reached its bound */
int pst_vcc_cells(const float* points, const int32_t* first_row, const int32_t* mv_ptr, int64_t max_voxels, float inv, int32_t* cells, void* stream);
int pst_vcc_build(const int32_t* cells, const int32_t* pan, int64_t Mv, uint64_t* keys, int32_t* rows, int64_t capacity, int32_t* parent, int32_t* status,
                  void* stream);
int pst_vcc_link(const int32_t* cells, const int32_t* pan, int64_t Mv, const uint64_t* keys, const int32_t* rows, int64_t capacity, int connectivity,
                 int32_t* parent, int32_t* status, void* stream);
int pst_vcc_flatten(const int32_t* parent, const int32_t* count, const int32_t* cells, int64_t Mv, int32_t* root, int32_t* size, int64_t* points,
                    int32_t* cell_lo, int32_t* cell_hi, int32_t* status, int merge, void* stream);
int pst_vcc_count(const int32_t* root, int64_t Mv, int32_t* counts, void* stream);
int pst_vcc_rank(const int32_t* root, const int32_t* pan, int64_t Mv, const int32_t* base, const int32_t* size, const int64_t* points, const int32_t* cell_lo,
                 const int32_t* cell_hi, int32_t* rank_of, int32_t* component, int32_t* t_root, int32_t* t_pan, int32_t* t_size, int64_t* t_points,
                 int32_t* t_lo, int32_t* t_hi, void* stream);
int pst_vcc_votes(const int32_t* cells, const int32_t* pan, const int32_t* root, const int32_t* size, int64_t Mv, const uint64_t* keys, const int32_t* rows,
                  int64_t capacity, int connectivity, int min_voxels, uint64_t* pair_keys, int32_t* pair_cnt, int64_t pair_capacity, int32_t* status,
                  void* stream);
int pst_vcc_apply(const int32_t* pan, const int32_t* root, const int32_t* size, const uint64_t* best, int64_t Mv, int min_voxels, const float* rgb,
                  const float* colors, int ncolors, float w1, float w2, int32_t* out_pan, float* out_colors, int32_t* status, void* stream);

/* ---------------------------------------------------------------- z-buffered point rendering of the cloud from any camera (no counterpart in the reference)
 * The rows [0, M) of a cloud (points fp32 [M, 3] in the world frame, rgb, colors fp32 [M, 3], pan int32 [M]; a panoptic cloud or a voxel cloud) seen
 * from B pinhole cameras at one output shape (H, W) -> per pixel the nearest point.  The reference's demo hands the cloud to an interactive viewer and has
 * no such stage; restated in tests/render_ref.py [restated, parity unpinned].  Every step is exact, so the outputs are held to it bit for bit.  Every
 * fp32 product and sum is rounded on its own, in the order written (contraction off):
 *   1 camera    host, float64: with the camera-to-world matrix [R | t], W = R^T and s_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2), each rounded to fp32.  The
 *               device table is float [B, 16] per camera: W00 W01 W02 s0 W10 W11 W12 s1 W20 W21 W22 s2 f cx cy near (f = the focal length in pixels,
 *               (cx, cy) = the principal point, near > 0).  Device: xc = ((W00 x + W01 y) + W02 z) + s0, likewise yc, zc.
 *   2 cull      a point is left out if xc, yc or zc is not finite, or zc < near.
 *   3 project   u = (f xc) / zc + cx, v = (f yc) / zc + cy; px = floor(u), py = floor(v): pixel (i, j) covers [j, j+1) x [i, i+1).  A point whose u or
 *               v is not finite or beyond +-2^20 is left out.
 *               THE QUOTIENT is taken in fp64 - fp32(fp64(f xc) / fp64(zc)) - and rounded once, like the voxel contract's fp64 operations.  (For fp32
 *               operands that equals the correctly rounded fp32 quotient, which is what numpy's float32 division gives.)
 *   4 footprint the point covers the (2r + 1)^2 pixels around (px, py), clipped to the image: r = min(max_radius, max(radius, floor((f half_size) / zc))),
 *               the same quotient; half_size >= 0 is fp32(point_size / 2) in world units, rounded on the host.
 *               0 <= radius, max_radius <= PST_RENDER_MAX_RADIUS (pst_render_max_radius()).
 *   5 depth     key = (uint64(bits(zc)) << 32) | uint32(row): zc > 0, so its bit pattern orders as an unsigned integer.  64-bit atomicMin of the key
 *               into zbuf uint64 [B, H, W], which the CALLER clears to all ones: the nearest point wins, equal depths go to the smallest row.  Integer
 *               atomics only: the result does not depend on scheduling.  `precheck` != 0 reads the cell first (relaxed) and skips an atomic that
 *               cannot win (same results).
 *   6 resolve   per pixel of zbuf (npix = B H W): an empty cell gives index -1, depth 0, pan 0, rgb = colors = 0; otherwise index int64 = the winning row,
 *               depth fp32 = its zc, and pan int32, rgb, colors fp32 [., 3] are that row's.  Plain vector stores.  A cell counts as EMPTY if it is all
 *               ones or if the row in its key is >= M (no buffer that pst_render_splat filled over the same cloud holds one: nothing is read outside the
 *               cloud).  The depth bits of any other key come back as they are, whatever they spell.
 * 1 <= M <= 2^32 - 1 (the row is 32 bits of the key), 1 <= B <= 65535, B H W <= 2^31 - 1.  Nothing can fail on the device: there is no status word. */
#define PST_RENDER_MAX_RADIUS 16
int pst_render_max_radius(void);
int pst_render_splat(const float* points, int64_t M, const float* cams, int ncams, int H, int W, float half_size, int radius, int max_radius, uint64_t* zbuf,
                     int precheck, void* stream);
int pst_render_resolve(const uint64_t* zbuf, int64_t npix, int64_t M, const float* rgb, const float* colors, const int32_t* pan, int64_t* index, float* depth,
                       int32_t* out_pan, float* out_rgb, float* out_colors, void* stream);

/* ---------------------------------------------------------------- cross-view depth consistency of the pointmaps (ABI 20, additive; no counterpart in the reference)
 * Every pixel of every view projected into every OTHER view and compared with the depth that view measured there -> per pixel of the concatenated
 * scene (N pixels, view v owns [offset_v, offset_v + H_v W_v)) the number of views that agree with it, the number it violates and the number of
 * agreeing views that give it the same panoptic id; restated in tests/consistency_ref.py [restated, parity unpinned], held to it bit for bit.  No
 * atomics; every fp32 product, sum and difference is rounded on its own, in the order written (contraction off); every test is a negated compare, so
 * a NaN fails it.  The scene is the cloud's table of pst_cloud_view (conf, pts3d, pts3d_local, pan - which may be NULL: every id void -, offset, npix,
 * first_wg and c2w are read, img is not: a view owns ceil(npix / 1024) consecutive workgroups from first_wg, nwg = their sum) next to two plain
 * tables: cams float [V, 16] per view W00 W01 W02 s0 W10 W11 W12 s1 W20 W21 W22 s2 f cx cy near, the render section's step 1 of the view's OWN
 * camera, and dims int32 [V, 2] = (H, W) with H W = npix (a view whose H W exceeds its npix is the target of nothing).
 *   world    the pixel's world point P: pts3d; with local != 0 pts3d_local moved by c2w, x' = ((R00 x + R01 y) + R02 z) + t0 ..., as cloud_compact's
 *            points_local.
 *   camera   pc = W2C P of a view: xc = ((W00 X + W01 Y) + W02 Z) + s0, likewise yc, zc (the render section's step 1).
 *   depth    pst_consist_depth, depth fp32 [N]: zc of the pixel's point in its OWN camera if conf >= thr, xc, yc and zc are finite and zc >= near;
 *            else 0 = "this view measured nothing here" (near > 0, so a measured depth is never 0).
 *   count    pst_consist_count, agree / violate / same_label int32 [N] (same_label may be NULL: no panoptic id is read).  A pixel whose own depth is 0
 *            gets zeros.  Any other, for every view j but its own, in this order:
 *              1  pc = W2C_j P; left out if xc, yc or zc is not finite or !(zc >= near_j)
 *              2  u = (f xc) / zc + cx, v = (f yc) / zc + cy, the quotient fp32(fp64(f xc) / fp64(zc)) as the render section's; left out unless
 *                 |u| <= 2^20 and |v| <= 2^20
 *              3  px = floor(u + 0.5f), py = floor(v + 0.5f): THE NEAREST PIXEL CENTRE.  The pointmaps put pixel x at u = x exactly
 *                 (estimate_focal_knowing_depth subtracts pp from integer pixel coordinates); the render section's floor(u), whose pixel j covers
 *                 [j, j + 1), would send half of a view's own points to their left neighbour.  Outside [0, W_j) x [0, H_j): unseen by j.
 *              4  d = depth[offset_j + py W_j + px]; d == 0: unseen by j
 *              5  tol = rel_tol d.  AGREE if |zc - d| <= tol (a tie agrees); else VIOLATE if d - zc > tol: the point lies in front of what j measured
 *                 along that ray, in space j sees through; else the point is occluded in j and counts for nothing.
 *              6  same_label is incremented on an agreeing pair whose source id pan > 0 equals pan_j[py W_j + px].
 *            No read falls outside a view's planes: the index is formed only after the in-image test.
 * Refused with PST_EINVAL before any launch: nviews outside [1, 65535], N outside [1, 2^31 - 1], nwg outside [1, N], rel_tol not a number in [0, 1),
 * a null views / cams / dims / depth / agree / violate.  Nothing can fail on the device: there is no status word.  No bilinear sampling of the
 * target's depth, no weighting by normal or grazing angle, no frustum pre-cull. */
int pst_consist_depth(const pst_cloud_view* views, const float* cams, int nviews, int nwg, int64_t N, float thr, int local, float* depth, void* stream);
int pst_consist_count(const pst_cloud_view* views, const float* cams, const int32_t* dims, int nviews, int nwg, int64_t N, float rel_tol, int local,
                      const float* depth, int32_t* agree, int32_t* violate, int32_t* same_label, void* stream);

/* ---------------------------------------------------------------- one fused TSDF surface out of all views (f15; ABI 20, additive; no counterpart in the reference)
 * A truncated signed distance averaged over the views on the lattice nodes around the occupied voxels, free space carved by the views that see
 * through it, ONE sheet extracted by naive surface nets (no case table); restated in tests/tsdf_ref.py [restated, parity unpinned], held to it bit
 * for bit.  Inputs: cells int32 [Mv, 3], the unique integer cells of a voxel cloud at the voxel size vs (fp32) with its count, pan and colors; the
 * cloud's pst_cloud_view table with the consistency section's cams, dims and depth (pst_consist_depth at the cloud's own threshold); band in
 * [1, PST_TSDF_MAX_BAND]; min_weight >= 1.  No float atomics; every fp32 product, sum and difference is rounded on its own, in the order written
 * (contraction off); every test is written so that a NaN fails it; two calls return identical bytes.
 *   1 nodes     A node is n in Z^3 at p_a = fp32(n_a) vs (one rounded product).  Pair p = row (2 band)^3 + offset, offset = ox + 2 band (oy + 2 band oz),
 *               names the node n_a = c_a - band + 1 + o_a of voxel `row`: per occupied cell the (2 band)^3 nodes c_a - band + 1 <= n_a <= c_a + band are
 *               ACTIVE (band 1: the cell's eight corners).  pst_tsdf_insert: one lane per pair, the node's 3 x 21-bit key claimed in keys uint64 [cap]
 *               (all ones = empty, cap a power of two >= 2 pairs), atomicMin of p into first int32 [cap] (2^31 - 1 before), pair_slot int32 [pairs].
 *               A node outside (-2^20, 2^20) is not inserted and sets PST_TSDF_RANGE in status[0], a table without a free slot PST_TSDF_FULL: no
 *               result then.  THE ORDER: a node's rank is the order of its smallest pair: pst_voxel_count / pst_cloud_scan / pst_voxel_rank on
 *               (pair_slot, first) give slot_rank int32 [cap], first_pair int32 [pairs] and the number of nodes Nn.  pst_tsdf_nodes: nodes int32
 *               [Nn, 3] in rank order, and voxel_row int32 [Nn] (-1 before): the voxel whose cell IS the node, n = c.
 *   2 integrate pst_tsdf_integrate, one lane per node, the views j in ascending order (a view whose H W exceeds its npix takes no part); S = 0, W = 0:
 *               pc = W2C_j p (the consistency section's `camera`); left out if xc, yc or zc is not finite, then if !(zc >= near_j); u, v as its step 2
 *               with the limit 2^20; px = floor(u + 0.5f), py likewise; outside the image: left out; d = depth[offset_j + py W_j + px]; d == 0: left
 *               out; s = d - zc; tau = fp32(band) vs; s < -tau: occluded, the pair counts for nothing; else S = S + min(s, tau), W += 1.
 *               sdf = fp32(fp64(S) / fp64(fp32(W))) if W > 0, else 0 (no quotient is taken); weight = W.  VALID iff W >= min_weight; INSIDE iff
 *               sdf < 0 (sdf == 0 is outside).
 *   3 cells     Cell c has the corner nodes c + {0,1}^3; a SURFACE CELL iff all eight are active and valid and not all on one side.  Its vertex:
 *               the twelve edges in the order axis x, y, z, within axis a (a, b, c cyclic) the (b, c) offsets 00, 10, 01, 11; for an edge whose ends
 *               differ in side, t = fp64(Da) / (fp64(Da) - fp64(Db)) with a the lower node, the crossing = lower corner offset + t e_a in cell units;
 *               the crossings are summed per coordinate in fp64 in that order and divided by their number; vertex_a = fp32((fp64(c_a) + mean_a) fp64(vs)).
 *               Vertices come in the rank order of their cell's node n = c (pst_tsdf_cells: flags and counts per 1024 nodes; pst_cloud_scan;
 *               pst_tsdf_vertices, which leaves cell_vertex int32 [Nn]: the vertex row of the cell at each node, else -1).
 *   4 labels    The vertex takes vertex id pan[w] and colour colors[w] of the voxel w = voxel_row of node c; without one, of the voxel with the largest
 *               count among those of the 26 neighbouring cells (ties to the smaller row); without any, id 0 and colour 0.
 *   5 faces     For the lattice edge from node n along axis a between two valid nodes of different sides, the four cells n + (b, c) offsets q0 = (0,0),
 *               q1 = (-1,0), q2 = (-1,-1), q3 = (0,-1): if all are surface cells, two triangles over their vertices, (q0,q1,q2), (q0,q2,q3) when n is
 *               inside and (q0,q2,q1), (q0,q3,q2) when it is outside: the normal (v1 - v0) x (v2 - v0) points from inside to outside, towards the
 *               cameras.  Face id: the id two of its corners share, else 0 (the surface section's rule).  edge int64 = 3 rank(n) + a.  Faces come in
 *               the order node rank, axis, first triangle before second (pst_tsdf_face_count: face_mask int32 [Nn], bit a, and counts in FACES per
 *               1024 nodes; pst_cloud_scan; pst_tsdf_face_emit).
 * Refused with PST_EINVAL before any launch: a null operand, band outside [1, PST_TSDF_MAX_BAND], min_weight < 1, Mv (2 band)^3 or Nn outside
 * [1, 2^30 - 1], cap no power of two >= twice the pairs (insert) / the nodes (the others), nviews outside [1, 65535], a voxel size that is no
 * positive finite number.  No confidence weighting, no bilinear depth, no marching-cubes table, no vertex normals; cells only where the cloud has
 * points +- band. */
#define PST_TSDF_FULL 1       /* a table ran full */
#define PST_TSDF_RANGE 4      /* a node outside (-2^20, 2^20) */
#define PST_TSDF_MAX_BAND 4
int pst_tsdf_insert(const int32_t* cells, int64_t Mv, int band, uint64_t* keys, int64_t cap, int32_t* first, int32_t* pair_slot, int32_t* status, void* stream);
int pst_tsdf_nodes(const int32_t* cells, int64_t Mv, int band, const int32_t* first_pair, int64_t Nn, const uint64_t* keys, int64_t cap,
                   const int32_t* slot_rank, int32_t* nodes, int32_t* voxel_row, int32_t* status, void* stream);
int pst_tsdf_integrate(const int32_t* nodes, int64_t Nn, float voxel_size, int band, const pst_cloud_view* views, const float* cams, const int32_t* dims,
                       int nviews, const float* depth, float* sdf, int32_t* weight, void* stream);
int pst_tsdf_cells(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf, const int32_t* weight,
                   int min_weight, int32_t* cell_vertex, int32_t* counts, int32_t* status, void* stream);
int pst_tsdf_vertices(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf, const int32_t* weight,
                      int min_weight, const int32_t* voxel_row, const int32_t* vox_count, const int32_t* vox_pan, const float* vox_colors, int64_t Mv,
                      double voxel_size, const int32_t* base, int32_t* cell_vertex, float* vertices, int32_t* vertex_ids, float* colors, int32_t* status,
                      void* stream);
int pst_tsdf_face_count(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf, const int32_t* weight,
                        int min_weight, const int32_t* cell_vertex, int32_t* face_mask, int32_t* counts, int32_t* status, void* stream);
int pst_tsdf_face_emit(const int32_t* nodes, int64_t Nn, const uint64_t* keys, int64_t cap, const int32_t* slot_rank, const float* sdf,
                       const int32_t* cell_vertex, const int32_t* face_mask, const int32_t* vertex_ids, const int32_t* base, int32_t* faces, int32_t* face_ids,
                       int64_t* edge, int32_t* status, void* stream);

/* ---------------------------------------------------------------- z-buffered triangle rasterisation of a labelled mesh: ground-truth depth and panoptic maps
 * A mesh (vertices fp32 [Nv, 3] in the world frame, faces int32 [Nf, 3], one panoptic id per vertex or per face) seen from B pinhole cameras at one shape
 * (H, W) -> per pixel the nearest face's depth, index and id, and after a per-view minimum-area filter the ground-truth maps pst_pq_count scores
 * against.  The reference renders them through pyrender / OpenGL (tools/preprocess_scannetpp.py:395-494: SKIP_CULL_FACES | SEG_VERT, znear 0.05, zfar
 * 20, MIN_INST_AREA 50), which a compute node does not offer; restated in tests/mesh_ref.py [restated, parity unpinned].  Every step is exact, so the
 * outputs are held to it bit for bit.  Contraction is off: every fp32 and fp64 operation is rounded on its own, in the order written:
 *   1 camera    host, float64: the rows of [R^T | -R^T t] computed and rounded as step 1 of the render contract, then fx fy cx cy: float [B, 16] per camera
 *               W00 W01 W02 s0 W10 W11 W12 s1 W20 W21 W22 s2 fx fy cx cy.  near and far are kernel scalars, 0 < near < far, fp32.
 *   2 vertex    xc, yc, zc as step 1 of the render contract.  u = fp32(fp64(fx xc) / fp64(zc)) + cx, v = fp32(fp64(fy yc) / fp64(zc)) + cy (the
 *               quotient rule of render step 3).  A vertex is UNUSABLE if any of xc, yc, zc, u, v is not finite, if zc < near, or if |u| or |v| > 2^14.
 *               Otherwise it is snapped to 1/256 pixel: X = int32(rint(u 256)), Y = int32(rint(v 256)), half to even; the product is exact.
 *   3 face      a face with an unusable vertex, or with an index outside [0, Nv), is left out whole: THERE IS NO NEAR-PLANE CLIPPING (the reference
 *               clips; with centimetre-sized faces at near = 0.05 the difference is a rim of pixels).  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in
 *               int64; A == 0 drops the face; if A < 0 corners 1 and 2 are exchanged (and A = -A).  No face culling.
 *   4 coverage  pixel (i, j) is sampled at P = (256 j + 128, 256 i + 128).  For corner k with the opposite edge a -> b, (a, b) = (1, 2), (2, 0), (0, 1):
 *               E_k = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa) in int64; E0 + E1 + E2 = A.  The pixel is covered iff for every k E_k > 0, or E_k == 0 and
 *               the edge d = (Xb - Xa, Yb - Ya) has dy < 0 or (dy == 0 and dx > 0) - the top-left rule: a pixel centre on an edge two faces share
 *               belongs to exactly one of them.  With the bounds of step 2 |E| < 2^47: exact in int64 and in fp64.
 *               The BOUNDING BOX of a face is the pixels j0 .. j1 x i0 .. i1 whose centres lie in [min X, max X] x [min Y, max Y], clipped to the
 *               image: j0 = max(0, ceil((min X - 128) / 256)), j1 = min(W - 1, floor((max X - 128) / 256)), likewise i0, i1; an empty box drops the
 *               face.  Only its pixels are tested (none outside it can be covered).
 *   5 depth     perspective-correct, fp64: q_k = 1.0 / fp64(zc_k), s = (fp64(E0) q0 + fp64(E1) q1) + fp64(E2) q2, depth = fp32(fp64(A) / s).  A
 *               sample is left out if depth is not finite, < near or > far.
 *   6 z-buffer  key = (uint64(bits(depth)) << 32) | uint32(face); 64-bit atomicMin into zbuf uint64 [B, H, W], which the CALLER clears to all ones:
 *               the nearest face wins, equal depths go to the smallest face index.  Integer atomics only: the result does not depend on scheduling.
 *               `precheck` != 0 reads the cell first (relaxed) and skips an atomic that cannot win (same results).
 *   7 resolve   an empty cell gives face -1, depth 0, id 0; otherwise face int64 and depth fp32 come from the key.  With face_ids int32 [Nf] the id
 *               is face_ids[face].  With vertex_ids int32 [Nv] the E_k of that face at that pixel are recomputed and the id is vertex_ids[corner] of
 *               the corner with the largest E_k (the nearest corner), ties to the lowest position as listed in `faces`; ids are never blended.
 *               With neither the id is 0.  Plain vector stores.  A cell counts as EMPTY if it is all ones or if the face in its key is >= Nf.  With
 *               vertex_ids, a key whose face is left out or has an empty bounding box in that cell's camera (steps 3 and 4: it cannot have won a pixel
 *               there) gives id 0, with face and depth from the key.  Neither arises from a buffer pst_mesh_raster filled over the same mesh and cameras.
 *   8 area      an id i is LISTED with row id2row[i] if 0 < i < ntab and that entry is in [0, S) (as pst_pq_count maps ids).  counts int32 [B, S],
 *               cleared by the CALLER: the pixels of every (camera, listed id), int32 atomicAdd only.  pst_mesh_area_apply: out = the id if it is
 *               listed and its count in that camera is >= min_area, else 0 (min_area = 0 only removes unlisted ids).  out is not pan.
 * pst_mesh_raster runs two paths with one result (the minimum is order-free): a lane per (camera, face) loops over a bounding box of at most
 * PST_MESH_LANE_PIXELS pixels; a larger face goes to the list big uint64 [big_capacity] ((camera << 32) | face; big_count uint64 [1], cleared by the
 * CALLER, counts the appends) and a second launch walks the list one wave per face, the lanes striding over the box.  A full list is no error: the face
 * is then rasterised by its lane.  big_capacity = 0 (big may be null) keeps everything in the lane path.
 * 1 <= Nf, Nv <= 2^31 - 1, 1 <= B <= 65535, B H W <= 2^31 - 1, B S <= 2^31 - 1.  Nothing can fail on the device: there is no status word. */
#define PST_MESH_LANE_PIXELS 64
int pst_mesh_lane_pixels(void);
int pst_mesh_raster(const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams, int ncams, int H, int W, float near_z, float far_z,
                    uint64_t* zbuf, uint64_t* big, uint64_t* big_count, int64_t big_capacity, int precheck, void* stream);
int pst_mesh_resolve(const uint64_t* zbuf, int ncams, int H, int W, const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams,
                     float near_z, const int32_t* vertex_ids, const int32_t* face_ids, int64_t* face, float* depth, int32_t* pan, void* stream);
int pst_mesh_area_count(const int32_t* pan, int ncams, int64_t hw, const int32_t* id2row, int ntab, int S, int32_t* counts, void* stream);
int pst_mesh_area_apply(const int32_t* pan, int ncams, int64_t hw, const int32_t* id2row, int ntab, int S, const int32_t* counts, int min_area, int32_t* out,
                        void* stream);

/* ---------------------------------------------------------------- mesh shading: vertex normals, interpolated attributes and a headlight shade (f17; ABI 20, additive; no counterpart in the reference)
 * What turns a face map of the section above into a picture: area-weighted vertex normals of the mesh, any per-vertex quantity interpolated
 * perspective-correctly over the rendered pixels, and a two-sided headlight shade term.  Restated in tests/mesh_shade_ref.py [restated, parity unpinned]
 * and held to it bit for bit.  Contraction is off: every fp64 operation is rounded on its own, in the order written.  No float atomics.
 * VERTEX NORMALS  vertices fp32 [Nv, 3], faces int32 [Nf, 3], sh int, acc int64 [Nv, 3, 2] cleared by the CALLER, normals fp32 [Nv, 3]:
 *   1 valid     face f takes part iff its three indices are inside [0, Nv) and its nine coordinates are finite; any other face adds nothing.
 *   2 vector    e1 = v1 - v0, e2 = v2 - v0 in fp64 from the fp32 coordinates; c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), every product
 *               and every difference rounded on its own.  |c| is twice the face's area: the weighting is by AREA, not by angle.
 *   3 scale     sh is chosen by the host: D = the largest axis extent (max - min) over the finite vertex coordinates, formed in fp64 from the fp32 extrema;
 *               ex = the frexp exponent of D (D = m 2^ex, 0.5 <= m < 1); sh = 51 - 2 ex, or 0 when D == 0 or no coordinate is finite.  Then
 *               |c_a 2^sh| < 2^52 for every valid face.  |sh| <= PST_MESH_NORMALS_MAX_SHIFT.
 *   4 quantise  q = int64(rint(ldexp(c_a, sh))), half to even; hi = q >> 26 (arithmetic: floor), lo = q & (2^26 - 1), so q = hi 2^26 + lo, 0 <= lo < 2^26.
 *   5 sum       for each of the face's three corners v and each axis a: acc[v][a][0] += hi, acc[v][a][1] += lo, 64-bit integer atomics, one lane per
 *               face.  Integer sums are exact and commute: the result does not depend on the order of the faces or on scheduling.
 *   6 bounds    fewer than 2^33 additions of magnitude below 2^26 per word: nothing overflows for any Nf <= 2^31 - 1.
 *   7 finish    pst_mesh_normals_finish, one lane per vertex: S_a = fp64(acc[v][a][0]) 67108864.0 + fp64(acc[v][a][1]); len2 = (Sx Sx + Sy Sy) + Sz Sz;
 *               len2 == 0 gives the normal (0, 0, 0) (a vertex on no valid face, or whose faces cancel); otherwise n_a = fp32(S_a / sqrt_heron(len2)).
 *   8 sqrt_heron(x) for finite x > 0: (., e) = frexp(x), e2 = e - (e & 1), r = ldexp(x, -e2) in [0.5, 2); s = 1.0, then six times s = 0.5 (s + r / s);
 *               the result is ldexp(s, e2 / 2).  Only IEEE add, multiply and divide: within 1 ulp of the correctly rounded root on [0.5, 2).
 * INTERPOLATION AND SHADE  pst_mesh_interp, one lane per pixel of face int64 [B, H, W] (as pst_mesh_resolve writes it; ANY values are legal), with
 *   vertices, faces, cams fp32 [B, 16] and near as pst_mesh_resolve takes them.  Optional: attr fp32 [Nv, C], 1 <= C <= PST_MESH_INTERP_MAX_CHANNELS, with
 *   fill (finite) and out_attr fp32 [B, H, W, C] (both pointers or neither); shade_mode PST_MESH_SHADE_NONE / _FLAT / _SMOOTH with out_shade fp32
 *   [B, H, W] (given iff the mode is not NONE) and normals fp32 [Nv, 3] (given iff the mode is SMOOTH).  At least one output.
 *   9 hit       the pixel (i, j) of camera b with f = face[b][i][j] is a HIT iff 0 <= f < Nf, face f is rasterised in camera b (mesh steps 2 and 3 and a
 *               bounding box that is not empty) and the pixel passes the coverage test of mesh step 4.  Anything else - -1, an index >= Nf, a face that
 *               is not drawn in that camera or does not cover the pixel - is a MISS: `fill` in every channel, shade 0.  So s below is never 0.
 *  10 weights   w_k = fp64(E_k) q_k with E_k and q_k of mesh steps 4 and 5, s = (w0 + w1) + w2: the depth's own sum.  SET-UP corner k is listed position
 *               k of the face, with positions 1 and 2 exchanged when mesh step 3 exchanged them.
 *  11 attribute out[c] = fp32(((w0 a0 + w1 a1) + w2 a2) / s), a_k = fp64(attr[vertex at set-up corner k][c]).
 *  12 shade     N, world frame: SMOOTH (w0 n0 + w1 n1) + w2 n2 per axis of the three corners' normals (no division by s: only the direction counts);
 *               FLAT the c of step 2 of the corners AS LISTED (no exchange).  Camera frame: n_r = (fp64(W_r0) N_x + fp64(W_r1) N_y) + fp64(W_r2) N_z for
 *               the rows r of the camera's world-to-camera rotation.  View ray d = (((j + 0.5) - cx) / fx, ((i + 0.5) - cy) / fy, 1) in fp64.
 *               dot = (n0 d0 + n1 d1) + n2, nn = (n0 n0 + n1 n1) + n2 n2, dd = (d0 d0 + d1 d1) + 1, x = nn dd;
 *               shade = fp32(|dot| / sqrt_heron(x)), or 0 when x is zero or not finite.  Two-sided (the rasteriser sees both sides of a face): a
 *               headlight at the camera, in [0, 1] up to rounding; no shadows, no textures.
 * 1 <= Nf, Nv <= 2^31 - 1, 1 <= B <= 65535, B H W <= 2^31 - 1, 0 < near finite.  Nothing can fail on the device: there is no status word.  A refusal
 * (PST_EINVAL) comes before any launch and leaves every output untouched. */
#define PST_MESH_INTERP_MAX_CHANNELS 16
#define PST_MESH_NORMALS_MAX_SHIFT 1100
#define PST_MESH_SHADE_NONE 0
#define PST_MESH_SHADE_FLAT 1
#define PST_MESH_SHADE_SMOOTH 2
int pst_mesh_normals_accumulate(const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, int sh, int64_t* acc, void* stream);
int pst_mesh_normals_finish(const int64_t* acc, int64_t Nv, float* normals, void* stream);
int pst_mesh_interp(const int64_t* face, int ncams, int H, int W, const float* vertices, int64_t Nv, const int32_t* faces, int64_t Nf, const float* cams,
                    float near_z, const float* attr, int C, float fill, float* out_attr, int shade_mode, const float* normals, float* out_shade, void* stream);

/* ---------------------------------------------------------------- surface: the pointmap grids triangulated into one labelled mesh (no counterpart in the reference)
 * Every view's pointmap is a grid, so pixel neighbours are surface neighbours.  The mesh's vertices ARE the rows of the panoptic cloud (points, pan
 * and colors of pst_cloud_compact: nothing is copied or compacted, a vertex that no face uses is allowed); these entry points only make the faces.
 * Restated in tests/surface_ref.py [restated, parity unpinned]; integer work and fp32 compares only, so the outputs are held to the restatement bit
 * for bit.  View v is an H x W grid of npix = H W pixels, pixel (y, x) is scene pixel p = offset + y W + x; N = the scene's pixels, 1 <= N <= 2^30.
 *   1 rows      row int32 [N]: row[p] = the cloud row i with index[i] == p, or -1 if the confidence filter dropped the pixel (index int64 [M] as
 *               pst_cloud_compact wrote it: ascending, distinct).
 *   2 quads     for every view and every (y, x) with 0 <= y < H - 1, 0 <= x < W - 1, corners a = (y, x), b = (y, x + 1), c = (y + 1, x),
 *               d = (y + 1, x + 1).  The z of a present corner is the THIRD COMPONENT OF pts3d_local AT ITS PIXEL, the depth in the source camera
 *               (not of the cloud's points_local, which pst_cloud_compact moved to the world frame).
 *               Four corners present: two candidate triangles, split along the diagonal with the smaller |dz| - diagonal b-c iff
 *               |z_b - z_c| < |z_a - z_d| (one fp32 subtraction each), so a tie or a NaN takes a-d.
 *                 a-d: T0 = (a, c, d), T1 = (a, d, b)        b-c: T0 = (a, c, b), T1 = (b, c, d)
 *               Exactly three present: the one triangle of them, as T0 - missing d: (a, c, b), a: (b, c, d), b: (a, c, d), c: (a, d, b).
 *               Fewer: nothing.  Every winding faces the source camera: (v1 - v0) x (v2 - v0) has negative z in its frame (x right, y down, z forward).
 *   3 cut       a candidate is kept iff zmin > 0 && zmax <= zmin * k over its three corners: one fp32 product, NaN fails, equality keeps.
 *               k = float32(1 + max_depth_ratio) >= 1; k = +inf is "no cut" (zmin > 0 still applies: the product is +inf, never 0 * inf).
 *   4 face id   the id that at least two of the corners' vertex_ids share, 0 (void) if all three differ.
 *   5 order     by view, then by quad in raster order (y, then x), then T0 before T1 -> rows [0, F) of faces int32 [., 3] (cloud rows), face_ids int32
 *               [.], quad int64 [.] (the scene pixel of the face's corner a).  F is only known on the device: every output holds the bound, two
 *               faces per quad.  A workgroup of PST_SURFACE_WG threads takes that many consecutive quads of one view, one per thread; dims int32
 *               [nviews, 4] on the device = (H, W, first_wg, 0) per view, where view v owns the ceil((H - 1)(W - 1) / PST_SURFACE_WG) workgroups from
 *               first_wg on (none for a view without quads) and nwg = their sum.  `views` is the cloud's table (offset, pts3d_local, npix = H W).
 *               surface_count -> counts int32 [nwg]; pst_cloud_scan -> base int32 [nwg + 1], base[nwg] = F; surface_emit evaluates every quad
 *               again and stores at base[wg] + the wave's ballots.  No atomics: the order holds by construction.
 *   6 islands   two faces are connected when they share a vertex row; components are the transitive closure (views never share a vertex).
 *               surface_link: parent int32 [M] and size int32 [M] are initialised here (parent[v] = v, size = 0), then unite(v0, v1), unite(v0, v2) per
 *               face (wait-free union-find: the root is the component's smallest vertex row).  surface_components: component int32 [F] = that root,
 *               size[root] += 1 per face (int32 atomicAdd: a sum of integers).  surface_keep_count / pst_cloud_scan / surface_keep_emit: the faces
 *               with size[component] >= min_faces (>= 1) in their order, one per thread, PST_SURFACE_WG per workgroup: counts int32 [ceil(F / WG)].
 *               status int32 [1], zeroed by the caller: PST_VCC_RANGE (a face index outside [0, M): that face is united with nothing, its component
 *               is -1 and no size counts it, whichever of its corners it is), PST_VCC_LOOP (a bounded loop ran out: component -1) - never on
 *               the faces of surface_emit.  1 <= F <= 2^31 - 256, 1 <= M <= 2^30. */
#define PST_SURFACE_WG 256
int pst_surface_rows(const int64_t* index, int64_t M, int64_t N, int32_t* row, void* stream);
int pst_surface_count(const pst_cloud_view* views, const int32_t* dims, int nviews, int nwg, const int32_t* row, float k, int32_t* counts, void* stream);
int pst_surface_emit(const pst_cloud_view* views, const int32_t* dims, int nviews, int nwg, const int32_t* row, float k, const int32_t* vertex_ids,
                     const int32_t* base, int32_t* faces, int32_t* face_ids, int64_t* quad, void* stream);
int pst_surface_link(const int32_t* faces, int64_t F, int64_t M, int32_t* parent, int32_t* size, int32_t* status, void* stream);
int pst_surface_components(const int32_t* faces, int64_t F, int64_t M, const int32_t* parent, int32_t* component, int32_t* size, int32_t* status,
                           void* stream);
int pst_surface_keep_count(const int32_t* component, const int32_t* size, int64_t F, int min_faces, int32_t* counts, void* stream);
int pst_surface_keep_emit(const int32_t* faces, const int32_t* face_ids, const int64_t* quad, const int32_t* component, const int32_t* size, int64_t F,
                          int min_faces, const int32_t* base, int32_t* out_faces, int32_t* out_face_ids, int64_t* out_quad, void* stream);

/* ---------------------------------------------------------------- mesh simplification by vertex clustering (f18; ABI 20, additive; no counterpart in the reference)
 * Rossignac-Borrel on the cell grid of the voxel section: the vertices that fall into one cubic cell of edge cell_size become ONE vertex, the faces
 * are rewritten onto the new vertices, those that collapsed are dropped and those that then coincide are removed.  Restated in tests/simplify_ref.py
 * [restated, parity unpinned]; integer work plus the voxel section's separately rounded operations, so every output is held to the restatement bit
 * for bit.  Inputs: vertices fp32 [M, 3], colors fp32 [M, 3], vertex_ids int32 [M], faces int32 [F, 3], quad int64 [F], cell_size > 0 and finite.
 *   1 used      a vertex takes part iff at least one face names it; the others vanish.  A face with a corner outside [0, M) is an error: the
 *               PST_SIMPLIFY_RANGE bit of status[0], raised on the host; nothing is read or written through such a corner.
 *               pst_simplify_used: used int32 [M], ZEROED BY THE CALLER, = 1 for every named vertex.  pst_simplify_mask: masked fp32 [M, 3] = the
 *               vertex where used, NaN where not (the voxel section leaves a non-finite point out: the rows keep their order); status[1] += the used
 *               vertices.
 *   2 cluster   steps 1-5 of the voxel section on the used vertices in increasing row order with voxel_size = cell_size - the pst_voxel_* entry
 *               points themselves, on `masked`, colors and vertex_ids: inv = fp32(1 / fp64(cell_size)), c = floor(fp32(p * inv)) in (-2^20, 2^20);
 *               position = the mean of the 16-bit in-cell offsets summed as integers; colour = the mean of the 8-bit quantised colours (palette
 *               weight 0: w1 = 1, w2 = 0, the mean itself); id = the vote over the listed ids (id2row), ties to the smallest id, void only alone.  New
 *               vertices come in increasing order of their smallest member row.  cluster int32 [M] (the voxel section's point_voxel) = the new row of
 *               vertex v; -1 for an unused vertex and for one left out (non-finite, or a cell out of range).  Mv = the new vertices.
 *   3 remap     face f becomes (cluster[a], cluster[b], cluster[c]).  LEFT OUT if a corner is -1, else DEGENERATE if two new corners are equal:
 *               both are dropped, status[2] and status[3] count them; the others are CANDIDATES, counted in status[4].
 *   4 dedupe    (dedupe != 0) among the candidates with one unordered corner set the one with the smallest f survives, whatever its winding.  An
 *               open-addressing table of the voxel section's kind (keys uint64 [cap] filled with ~0, cap a power of two >= 2 F, linear probing bounded
 *               by cap, PST_SIMPLIFY_FULL if it ran full): key = the sorted corners + 1, 21 bits each, smallest lowest; winner int32 [cap], FILLED
 *               WITH INT32_MAX BY THE CALLER, takes a 32-bit atomicMin of f.  The key needs Mv <= 2^21 - 2: a larger Mv with dedupe is PST_EINVAL.
 *               Without dedupe every candidate survives, keys and winner may be null and Mv has no such limit.
 *               pst_simplify_remap: face_slot int32 [F] = the face's slot (0 without dedupe), -1 left out, -2 degenerate.  merge != 0 lets the first
 *               lane of a run of adjacent lanes with one key probe for the run: same results.
 *   5 emit      survivors in the order of the originals: pst_simplify_count -> counts int32 [ceil(F / PST_SURFACE_WG)], one face per thread;
 *               pst_cloud_scan -> base, base[last] = F'; pst_simplify_emit -> rows [0, F') of out_faces int32 [., 3] (the remapped corners in their
 *               original order), out_quad int64 [.] (the original's), src_face int32 [.] (f) and out_face_ids int32 [.]: the id at least two of the
 *               corners' NEW vertex_ids (int32 [Mv], the vote of step 2) share, else 0 - the surface section's rule.  Every output holds F rows.
 * status int32 [8], zeroed by the caller.  Integer atomics only, no float atomics; every result written with plain vector stores; two calls return
 * equal bytes.  Clustering preserves neither topology nor manifoldness, a collapse can flip a face's winding and nothing corrects it, and the
 * representative is the cell's mean, not a quadric optimum.  1 <= F <= 2^31 - 256, 1 <= Mv <= M <= 2^30. */
#define PST_SIMPLIFY_FULL 1       /* status[0]: the face table ran full (never: cap >= 2 F) */
#define PST_SIMPLIFY_RANGE 4      /* status[0]: a face corner outside [0, M), or a cluster outside [-1, Mv) */
int pst_simplify_used(const int32_t* faces, int64_t F, int64_t M, int32_t* used, int32_t* status, void* stream);
int pst_simplify_mask(const float* vertices, const int32_t* used, int64_t M, float* masked, int32_t* status, void* stream);
int pst_simplify_remap(const int32_t* faces, int64_t F, int64_t M, const int32_t* cluster, int64_t Mv, int dedupe, uint64_t* keys, int64_t cap,
                       int32_t* winner, int32_t* face_slot, int32_t* status, int merge, void* stream);
int pst_simplify_count(const int32_t* face_slot, const int32_t* winner, int64_t F, int dedupe, int32_t* counts, void* stream);
int pst_simplify_emit(const int32_t* faces, const int64_t* quad, const int32_t* cluster, const int32_t* vertex_ids, const int32_t* face_slot,
                      const int32_t* winner, int64_t F, int64_t M, int64_t Mv, int dedupe, const int32_t* base, int32_t* out_faces,
                      int32_t* out_face_ids, int64_t* out_quad, int32_t* src_face, void* stream);

/* ---------------------------------------------------------------- score3d: a mesh's surface as points, and the nearest point within a radius (no counterpart in the reference)
 * The two primitives of engine/score3d.py (F-score, chamfer and a 3-D panoptic quality of a reconstruction against a ground-truth mesh, point to
 * point).  Restated in tests/nearest_ref.py [restated, parity unpinned]: the sampler as written here, the search by brute force over all pairs.  Every
 * step is exact, so the outputs are held to the restatement bit for bit.  Contraction is off: every fp32 and fp64 operation is rounded on its own, in the
 * order written.  Additive to ABI 20.
 * MESH SURFACE SAMPLER  vertices fp32 [Nv, 3], faces int32 [F, 3], spacing > 0 fp32, 1 <= max_subdiv <= PST_MESH_SAMPLE_MAX_SUBDIV:
 *   1 drop      a face gets 0 samples and is counted in status[1] if an index is outside [0, Nv), a coordinate of a corner is not finite, or the
 *               cross product (v1 - v0) x (v2 - v0) is exactly zero in fp64 (corners widened to fp64, then one subtraction, product, subtraction each).
 *   2 n         L2 = the largest of the three squared edge lengths, (dx dx + dy dy) + dz dz in fp64 on the widened corners; s2 = fp64(spacing)
 *               fp64(spacing) (exact).  n = the smallest integer in [1, max_subdiv] with (fp64(n) fp64(n)) s2 >= L2 (n n is exact, one rounding); if
 *               max_subdiv itself fails the compare, n = max_subdiv and the face is counted as CLAMPED in status[2].  The compare decides: no square
 *               root is taken.  The face gets n^2 samples, so the sample density differs between faces by what rounding n up to a whole number (and
 *               the clamp) implies: a CHOICE - a uniform lattice per face instead of an area-weighted draw - that keeps the sampler deterministic.
 *   3 samples   the n^2 congruent sub-triangles of the uniform subdivision, t in [0, n^2): row r = floor(sqrt(t)) (integer compares settle it),
 *               c = t - r^2, k = c >> 1.  Even c is upright, odd c inverted; the centroid's integer weights over 3n for (v0, v1, v2) are
 *                 upright:  3(n - r) - 2,  3(r - k) + 1,  3k + 1            inverted:  3(n - r) - 1,  3(r - k) - 1,  3k + 2
 *               point = fp32(((w0 v0 + w1 v1) + w2 v2) / fp64(3n)) per axis in fp64, each operation rounded once, one cast.
 *   4 outputs   rows in face order, t ascending inside a face: points fp32 [., 3], face int32 [.], ids int32 [.] = face_ids[f], or with vertex_ids the id
 *               of the corner with the largest weight (ties to the lower corner), or 0 with neither (both: PST_EINVAL).
 *   mesh_sample_count: counts int32 [F] = n^2 or 0; total int64 [1] (cleared by the CALLER) = their sum, by integer atomics; status int32 [4] (cleared by
 *   the CALLER).  pst_cloud_scan of counts -> prefix int32 [F + 1].  The caller reads `total` and sizes the outputs; mesh_sample_emit refuses
 *   total > capacity (or > 2^31 - 256: the prefix is int32) with PST_EINVAL before anything is launched, runs one lane per sample, which finds its face
 *   by binary search in the prefix, and writes nothing but status[0] |= PST_MESH_SAMPLE_TOTAL if prefix[F] != total.  1 <= F <= 2^30.
 * FIXED-RADIUS NEAREST NEIGHBOUR  targets fp32 [M, 3], queries fp32 [Nq, 3], radius > 0; inv = fp32(1 / radius), r2 = fp32(radius radius) from the host:
 *   1 cells     the cell of a point is floor(fp32(x inv)) per axis (the voxel contract's rule: vx_cell_of of csrc/voxel_table.h for every stage).
 *               A target with a non-finite coordinate or a cell outside (-2^20, 2^20) is left out and counted in status[1].
 *   2 build     nn_insert: the cell's 3 x 21-bit key into keys uint64 [capacity] (all ones = empty, by the CALLER; capacity a power of two >= 2 M),
 *               cell_count int32 [capacity] (cleared by the CALLER) += 1 on its slot, point_slot int32 [M] = the slot or -1.  The caller turns
 *               cell_count into start int32 [capacity] (exclusive prefix sum).  nn_scatter: rows int32 [M]: the rows of slot s at [start[s], start[s] +
 *               cell_count[s]) in arrival order (fill int32 [capacity], cleared by the CALLER); status[2] = the largest cell_count.
 *   3 query     one lane per query: every target p in the 27 cells around the query's cell, dx = qx - px, d2 = (dx dx + dy dy) + dz dz in fp32;
 *               the minimum of (uint64(bits(d2)) << 32) | p: the nearest target, ties to the smaller row, whatever the order inside the lists.
 *               Accepted iff d2 <= r2: d2 fp32 [Nq], row int32 [Nq]; otherwise row -1 and d2 = +inf.  A query with a non-finite coordinate gets
 *               row -1 and is counted in status[3].  At most max_cell_points candidates of a cell are visited: the CALLER compares status[2] with it
 *               after the build and does not launch the query of a fuller cell (a radius too large for the density makes the search quadratic).
 *               THE SEARCH IS THE 27 CELLS: it equals the search over all targets whenever a pair with d2 <= r2 lies in neighbouring cells.  That
 *               fails only if the fp32 roundings of inv, of x inv and of qx - px put two points two cells apart whose rounded d2 is still <= r2: a
 *               pair at a distance within about 2^-23 (|x| / radius + 1) radius of the radius itself.  The scores are counts over millions of points.
 *   status int32 [4], cleared by the CALLER: [0] = PST_NN_FULL | PST_NN_LISTS, [1] targets left out, [2] largest occupancy, [3] non-finite queries.
 *   1 <= M, Nq <= 2^30. */
#define PST_MESH_SAMPLE_MAX_SUBDIV 32768
#define PST_MESH_SAMPLE_TOTAL 1   /* the prefix handed to mesh_sample_emit does not end in `total` */
#define PST_NN_FULL 1             /* the table ran full */
#define PST_NN_LISTS 2            /* start / cell_count / rows are not those of this build */
int pst_mesh_sample_count(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float spacing, int max_subdiv, int32_t* counts, int64_t* total,
                          int32_t* status, void* stream);
int pst_mesh_sample_emit(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, const int32_t* prefix, int64_t total, int64_t capacity,
                         const int32_t* vertex_ids, const int32_t* face_ids, float* points, int32_t* face, int32_t* ids, int32_t* status, void* stream);
int pst_nn_insert(const float* targets, int64_t M, float inv, uint64_t* keys, int64_t capacity, int32_t* cell_count, int32_t* point_slot, int32_t* status,
                  void* stream);
int pst_nn_scatter(const int32_t* point_slot, int64_t M, const int32_t* start, const int32_t* cell_count, int32_t* fill, int32_t* rows, int32_t* status,
                   void* stream);
int pst_nn_query(const float* queries, int64_t Nq, const float* targets, int64_t M, float inv, float r2, const uint64_t* keys, int64_t capacity,
                 const int32_t* start, const int32_t* cell_count, const int32_t* rows, int max_cell_points, float* d2, int32_t* row, int32_t* status,
                 void* stream);

/* ---------------------------------------------------------------- icp: one fused step of the alignment to the ground truth (no counterpart in the reference)
 * The hot path of engine/score3d.py's `icp` / `refine_alignment`: the source points are moved by the current transform, each finds its nearest target in
 * the search structure of the score3d section, and the moments of the matched pairs that `pointmaps.procrustes_from_moments` needs are summed, in one
 * pass over the sources.  Restated in tests/icp_ref.py [restated, parity unpinned] on the brute-force search of tests/nearest_ref.py; every step is
 * exact or separately rounded in a fixed order, so the 20 moments, d2, row and the status are held to the restatement bit for bit.  Contraction is
 * off: every fp32 and fp64 operation is rounded on its own, in the order written.  Additive to ABI 20.
 *   source fp32 [N, 3]; A = (a00 .. a23) the 3 x 4 fp32 matrix, by value, row-major; targets, inv, keys, capacity, start, cell_count, rows and
 *   max_cell_points are those of a finished build (nn_insert, the prefix sum, nn_scatter) with cell edge 1 / inv; 0 <= r2 finite.
 *   1 move      m_r = ((a_r0 x0 + a_r1 x1) + a_r2 x2) + a_r3 in fp32, r = 0, 1, 2.
 *   2 search    step 3 of the fixed-radius contract with m as the query (the same device function as nn_query): the 27 cells around m's cell, the
 *               minimum of (uint64(bits(d2)) << 32) | p, ties to the smaller row; accepted iff d2 <= r2.  The search equals the one over all targets
 *               only for pairs in neighbouring cells, so r2 MUST NOT exceed the square of the cell edge (the CALLER's duty; a smaller r2 is fine: it
 *               is how the radius shrinks without a rebuild).  A non-finite m is unmatched and counted in status[3].  With d2 fp32 [N] and row int32
 *               [N] given (both or neither) they are written as nn_query writes them: row -1 and d2 = +inf for an unmatched source.
 *   3 moments   over the matched sources, with x the ORIGINAL source point (not m) and y = targets[row], both widened to fp64 - a product of two of
 *               them is exact, only the additions round.  An unmatched source adds nothing.
 *                 [0] the number matched   [1..3] sum x   [4..6] sum y   [7..15] sum y x^T, row-major [y][x]   [16] sum of (x0 x0 + x1 x1) + x2 x2
 *                 [17] sum of fp64(d2)     [18], [19] +0.0, reserved
 *   4 order     block b of PST_ICP_LANES lanes owns the source rows [PST_ICP_CHUNK b, PST_ICP_CHUNK (b + 1)).  Lane l adds its rows PST_ICP_CHUNK b + l +
 *               PST_ICP_LANES j, j = 0 .. PST_ICP_CHUNK / PST_ICP_LANES - 1 ascending, into accumulators that start at +0.0.  Inside a wave of 64
 *               lanes six butterfly steps v += v[lane ^ k], k = 32, 16, 8, 4, 2, 1 (fp addition is commutative: all lanes agree); the four waves
 *               are added as ((w0 + w1) + w2) + w3 -> row b of partials double [ceil(N / PST_ICP_CHUNK), PST_ICP_MOMENTS].  A second launch of one
 *               block inside the same call adds the rows of partials the same way - lane l takes the rows l, l + PST_ICP_LANES, ... ascending, then
 *               the same butterfly and the same wave order - into out double [PST_ICP_MOMENTS].  No float atomics, no counter of finished blocks:
 *               two calls return identical bytes, and d2 / row given or not does not change the moments.
 *   status int32 [4], cleared by the CALLER, as the search's: [0] = PST_NN_FULL | PST_NN_LISTS, [3] non-finite moved points; [1], [2] untouched.
 *   Refused with PST_EINVAL before any launch: a null source / targets / table / partials / out / status, exactly one of d2 and row, N < 1 or
 *   N > 2^30, a table that nn_query would refuse, inv or r2 not finite, max_cell_points < 1.  pst_icp_chunk() returns PST_ICP_CHUNK. */
#define PST_ICP_CHUNK 4096        /* source rows per block */
#define PST_ICP_LANES 256         /* lanes per block */
#define PST_ICP_MOMENTS 20        /* doubles per row of partials and in out */
int pst_icp_chunk(void);
int pst_icp_step(const float* source, int64_t N, float a00, float a01, float a02, float a03, float a10, float a11, float a12, float a13, float a20,
                 float a21, float a22, float a23, const float* targets, int64_t M, float inv, float r2, const uint64_t* keys, int64_t capacity,
                 const int32_t* start, const int32_t* cell_count, const int32_t* rows, int max_cell_points, float* d2, int32_t* row, double* partials,
                 double* out, int32_t* status, void* stream);

/* ---------------------------------------------------------------- meshdist: the exact distance from a point to a triangle mesh within a radius (no counterpart in the reference)
 * The primitive of engine/meshdist.py (`mesh_distance`, `score_reconstruction(metric='surface')`): for every query the nearest point of the mesh's
 * SURFACE within the radius - its squared distance, its face and the point itself - exact against the triangles, where the score3d section measures to
 * samples of them.  Restated in tests/meshdist_ref.py [restated, parity unpinned]: the closest point as written here, the search by brute force over
 * all kept faces, the binning on its own.  Every step is exact or separately rounded in a fixed order, so the per-face counts, d2, face and closest are
 * held to the restatement bit for bit.  Contraction is off: every fp32 and fp64 operation is rounded on its own, in the order written.  Integer
 * atomics only; every loop is bounded by a number known before the launch.  Additive to ABI 20.
 *   vertices fp32 [Nv, 3], faces int32 [F, 3], queries fp32 [Nq, 3], radius > 0; inv = fp32(1 / radius), r2 = fp32(radius radius) from the host.
 *   1 cells     edge `radius`: the cell of a coordinate is floor(fp32(x inv)) (the score3d section's rule), the range (-2^20, 2^20), the keys those of
 *               the voxel table.
 *   2 faces     KEPT iff its three indices are in [0, Nv), its nine coordinates are finite and the cross product (v1 - v0) x (v2 - v0) is not exactly
 *               zero in fp64 (the sampler's rule, step 1 of the score3d section), and its box stays in range.  The box of a face is, per axis,
 *               [cell(min of the three coordinates) - 1, cell(max) + 1], computed in fp32 (whole numbers: exact): the fp32 bounding box in cells,
 *               dilated by one cell; it is in range iff its lowest cell > -2^20 and its highest < 2^20 on every axis.  Every other face is DROPPED and
 *               counted in status[1].
 *   3 binning   a kept face is listed in every cell of its box: ext0 ext1 ext2 (face, cell) pairs, pair t of the face being the cell lo + (t mod ext0,
 *               (t / ext0) mod ext1, t / (ext0 ext1)).  A query reads the list of its OWN cell only, so every candidate face is evaluated once.  The
 *               lists are a superset of what is needed and the result does not depend on them: if |q_a - p_a| <= radius for a point p of the face then
 *               cell(q_a) is within one of cell(p_a), and cell(p_a) lies between the cells of the face's extremes.  That fails only in the rounding
 *               case of the score3d section: a pair within about 2^-23 (|x| / radius + 1) radius of the radius itself.  Cells are not pruned against
 *               the triangle's plane.
 *   4 build     meshdist_count: counts int32 [F] = the face's number of pairs, 0 for a dropped face, saturated at PST_MESHDIST_FACE_CAP; total int64
 *               [1] (cleared by the CALLER) = their sum, by integer atomics; the CALLER reads it, refuses what it will not hold and sizes the
 *               workspaces by it (total <= 2^30).  pst_cloud_scan of counts -> prefix int32 [F + 1].  meshdist_insert: one lane per pair, its face by
 *               binary search in the prefix, its cell from t; the cell's key into keys uint64 [capacity] (all ones = empty, by the CALLER; capacity a
 *               power of two >= 2 total), cell_count int32 [capacity] (cleared by the CALLER) += 1 on its slot, pair_slot int32 [total] = the slot.
 *               The caller turns cell_count into start int32 [capacity] (exclusive prefix sum).  meshdist_scatter: rows int32 [total]: the faces of
 *               slot s at [start[s], start[s] + cell_count[s]) in arrival order (fill int32 [capacity], cleared by the CALLER); status[2] = the
 *               longest list.  Insert and scatter write nothing but status[0] |= PST_MESHDIST_TOTAL if prefix[F] != total.
 *   5 closest   the closest point of triangle (a, b, c) to q, all twelve numbers widened to fp64 once; every line below is fp64, each operation
 *               rounded once, dot(u, v) = (u0 v0 + u1 v1) + u2 v2, clamp(t) = t > 0 ? min(t, 1) : 0 (so a NaN gives 0):
 *                 ab = b - a, ac = c - a, ap = q - a, bp = q - b, cp = q - c
 *                 d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
 *                 vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
 *               the first region that holds, in this order (Ericson, Real-Time Collision Detection, 5.1.5):
 *                 A   d1 <= 0 and d2 <= 0                                  x = a
 *                 B   d3 >= 0 and d4 <= d3                                 x = b
 *                 AB  vc <= 0 and d1 >= 0 and d3 <= 0                      t = clamp(d1 / (d1 - d3)),                       x = a + t ab
 *                 C   d6 >= 0 and d5 <= d6                                 x = c
 *                 AC  vb <= 0 and d2 >= 0 and d6 <= 0                      t = clamp(d2 / (d2 - d6)),                       x = a + t ac
 *                 BC  va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0        t = clamp((d4 - d3) / ((d4 - d3) + (d5 - d6))),  x = b + t (c - b)
 *                 interior  den = 1 / ((va + vb) + vc), v = clamp(vb den), w = clamp(vc den),                               x = (a + v ab) + w ac
 *               e = q - x, D2 = (e0 e0 + e1 e1) + e2 e2: always the distance to an actual point of the triangle, never NaN; no finite fp32 input
 *               overflows fp64 here (the largest intermediate is a product of two dots, about 1e155).  fp64 because scans hold sliver faces and
 *               coordinates metres from the origin; the sampler works in fp64 for the same reason.
 *   6 query     one lane per query: every face f of the list of the query's cell, d2 = fp32(D2) (one cast), the minimum of (uint64(bits(d2)) << 32) |
 *               f: the nearest face, ties to the smaller face, whatever the order inside the list.  Accepted iff d2 <= r2: d2 fp32 [Nq], face int32
 *               [Nq], closest fp32 [Nq, 3] = fp32(x) of the winner, recomputed and cast once (closest may be null: d2 and face do not change);
 *               otherwise d2 = +inf, face -1 and closest = the query itself.  A query with a non-finite coordinate gets no hit and is counted in
 *               status[3]; a finite query whose cell is out of range gets no hit.  At most max_cell_faces candidates are visited: the CALLER compares
 *               status[2] with it after the build and does not launch the query of a longer list.
 *   status int32 [4], cleared by the CALLER: [0] = PST_MESHDIST_FULL | PST_MESHDIST_LISTS | PST_MESHDIST_TOTAL, [1] dropped faces, [2] the longest
 *   list, [3] non-finite queries.
 *   Refused with PST_EINVAL before any launch, every output untouched: a null operand (closest excepted), Nv < 1, F, Nq or total < 1 or > 2^30, a
 *   capacity that is no power of two or below 2 total, inv or r2 not finite (inv not positive, r2 negative), max_cell_faces < 1. */
#define PST_MESHDIST_FULL 1       /* the table ran full */
#define PST_MESHDIST_LISTS 2      /* prefix / start / cell_count / rows are not those of this mesh and this build */
#define PST_MESHDIST_TOTAL 4      /* the prefix handed to insert / scatter does not end in `total` */
#define PST_MESHDIST_FACE_CAP 2147483647   /* a face's pair count saturates here */
int pst_meshdist_count(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, int32_t* counts, int64_t* total, int32_t* status,
                       void* stream);
int pst_meshdist_insert(const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, const int32_t* prefix, int64_t total, uint64_t* keys,
                        int64_t capacity, int32_t* cell_count, int32_t* pair_slot, int32_t* status, void* stream);
int pst_meshdist_scatter(const int32_t* pair_slot, const int32_t* prefix, int64_t F, int64_t total, const int32_t* start, const int32_t* cell_count,
                         int32_t* fill, int32_t* rows, int32_t* status, void* stream);
int pst_meshdist_query(const float* queries, int64_t Nq, const float* vertices, int64_t Nv, const int32_t* faces, int64_t F, float inv, float r2,
                       const uint64_t* keys, int64_t capacity, const int32_t* start, const int32_t* cell_count, const int32_t* rows, int64_t total,
                       int max_cell_faces, float* d2, int32_t* face, float* closest, int32_t* status, void* stream);

/* ---------------------------------------------------------------- icp-plane: one fused point-to-plane step against the triangles (no counterpart in the reference)
 * The hot path of engine/meshdist.py's `icp_to_mesh` / `refine_alignment(target='surface')`: the source points are moved by the current transform, each
 * finds its nearest face in the search structure of the meshdist section, and the normal equations of the LINEARISED POINT-TO-PLANE objective - the
 * squared distance of the moved point to the plane of its face, under a small similarity about a centre c0 - are summed, in one pass over the sources.
 * `pointmaps.plane_step_from_moments` solves them on the host.  Restated in tests/icp_plane_ref.py [restated, parity unpinned] on the brute-force
 * search of tests/meshdist_ref.py and the fixed-order sum of tests/icp_ref.py; every step is separately rounded in a fixed order, so the 40 moments,
 * the partials, d2, face and the status are held to the restatement bit for bit.  Contraction is off: every fp32 and fp64 operation is rounded on its
 * own, in the order written.  Additive to ABI 20.
 *   source fp32 [N, 3]; A = (a00 .. a23) the 3 x 4 fp32 matrix, by value, row-major; c0 = (c0x, c0y, c0z) fp32, by value, finite: the centre the
 *   increment turns and scales about, in the frame of the MOVED points; vertices, faces, inv, keys, capacity, start, cell_count, rows, total and
 *   max_cell_faces are those of a finished build of the meshdist section (count, scan, insert, the prefix sum, scatter) with cell edge 1 / inv;
 *   0 <= r2 finite.
 *   1 move      step 1 of the icp section: m_r = ((a_r0 x0 + a_r1 x1) + a_r2 x2) + a_r3 in fp32.
 *   2 search    step 6 of the meshdist section with m as the query (the same device function as meshdist_query): the list of m's own cell, every
 *               face's fp64 D2 cast to fp32 once, the minimum of (uint64(bits(d2)) << 32) | face, ties to the smaller face; accepted iff d2 <= r2.
 *               The lists hold every face within one cell edge, so r2 MUST NOT exceed the square of the cell edge (the CALLER's duty, as in
 *               icp_step; a smaller r2 is how the radius shrinks without a rebuild).  A non-finite m is unmatched and counted in status[3]; a
 *               finite m whose cell is out of range is unmatched.  A listed face that is out of range or was not kept sets PST_MESHDIST_LISTS.  With
 *               d2 fp32 [N] and face int32 [N] given (both or neither) they are written as meshdist_query writes them: face -1 and d2 = +inf
 *               for an unmatched source.
 *   3 terms     of a matched source, all fp64, a, b, c (the corners of its face), m and c0 widened once; every operation rounded once, in this
 *               order; dot(u, v) = (u0 v0 + u1 v1) + u2 v2 as in the meshdist section:
 *                 e1 = b - a, e2 = c - a
 *                 N = (e1_1 e2_2 - e1_2 e2_1, e1_2 e2_0 - e1_0 e2_2, e1_0 e2_1 - e1_1 e2_0)     the face's UNNORMALISED normal (the kept-face test's)
 *                 w = 1 / ((N0 N0 + N1 N1) + N2 N2)                                             a kept face has N != 0; no square root anywhere
 *                 p = m - c0, u = m - a
 *                 rN = dot(N, u)               |N| times the signed distance to the face's PLANE: the in-plane offset of an edge or corner hit is
 *                                              ignored, which is the point of the objective
 *                 J = (p1 N2 - p2 N1, p2 N0 - p0 N2, p0 N1 - p1 N0, N0, N1, N2, dot(N, p))      = (p x N, N, N . p): the derivative of rN under
 *                                              m -> c0 + (1 + sigma) R(omega) (m - c0) + tau at (omega, tau, sigma) = 0
 *                 g_i = w J_i
 *               moments, an unmatched source adds nothing:
 *                 [0] the number matched       [1..28] sum of g_i J_j for i <= j, row-major (i = 0: j = 0 .. 6, then i = 1: j = 1 .. 6, ...)
 *                 [29..35] sum of g_i rN       [36] sum of (w rN) rN, the squared distance to the plane
 *                 [37] sum of fp64(d2), the squared distance to the triangle                    [38], [39] +0.0, reserved
 *               Unlike the icp section's, these products round: each is one multiplication of the two factors named, then one addition into the sum.
 *   4 order     step 4 of the icp section, verbatim, with PST_ICP_CHUNK and PST_ICP_LANES (csrc/icp_sum.h is the one text of both): partials double
 *               [ceil(N / PST_ICP_CHUNK), PST_ICP_PLANE_MOMENTS], out double [PST_ICP_PLANE_MOMENTS].  One kernel and the one-block reducer.  No
 *               float atomics: two calls return identical bytes, and d2 / face given or not does not change the moments.
 *   status int32 [4], cleared by the CALLER, as the meshdist query's: [0] = PST_MESHDIST_FULL | PST_MESHDIST_LISTS, [3] non-finite moved points; [1],
 *   [2] untouched.
 *   Refused with PST_EINVAL before any launch, every output untouched: a null source / mesh / table / partials / out / status, exactly one of d2 and
 *   face, N < 1 or N > 2^30, a mesh, a table or limits that pst_meshdist_query would refuse, inv, r2 or c0 not finite.
 *   (The entry point is pst_plane_icp_step: the names pst_icp_* and pst_meshdist_* are closed sets.) */
#define PST_ICP_PLANE_MOMENTS 40  /* doubles per row of partials and in out */
int pst_plane_icp_step(const float* source, int64_t N, float a00, float a01, float a02, float a03, float a10, float a11, float a12, float a13, float a20,
                       float a21, float a22, float a23, float c0x, float c0y, float c0z, const float* vertices, int64_t Nv, const int32_t* faces, int64_t F,
                       float inv, float r2, const uint64_t* keys, int64_t capacity, const int32_t* start, const int32_t* cell_count, const int32_t* rows,
                       int64_t total, int max_cell_faces, float* d2, int32_t* face, double* partials, double* out, int32_t* status, void* stream);

/* ---------------------------------------------------------------- panoptic evaluation against ground truth: PQ / SQ / RQ, mIoU (no counterpart in the reference)
 * V predicted maps and V ground-truth maps of the same shapes, flattened and concatenated to pred, gt int32 [N] (1 <= N <= 2^31 - 1, both 16-byte
 * aligned), P predicted and G ground-truth segments (ids unique and > 0 within each list, no crowd regions).  The rules are those of COCO
 * panopticapi's pq_compute_single_core without iscrowd; restated in tests/eval_ref.py [restated, parity unpinned].  Every step is exact, so the
 * outputs are held to the restatement bit for bit:
 *   1 rows      a predicted id i maps to row id2row_p[i] if 0 < i < ntab_p and that entry is in [0, P), else to the VOID ROW P; ground truth maps the
 *               same way to column id2row_g[i], or to the VOID COLUMN G.  Ids <= 0, ids beyond the table and ids not listed are all void (as
 *               pst_voxel_accumulate treats them).
 *   2 slabs     slab s holds the pixels [slab_off[s], slab_off[s + 1]) of the flat maps, slab_off int64 [nslabs + 1] on the device, ascending from 0 to
 *               N: one slab with every pixel of every view (scope 'scene'), or one slab per view (scope 'view').  Equal neighbours are allowed: such
 *               a slab is EMPTY, holds no pixel wherever it lies (first, between two others, last), and its table stays as the caller cleared it.
 *   3 counts    counts int32 [nslabs, P+1, G+1], cleared by the CALLER: the number of pixels of slab s with (row p, column g).  int32 atomicAdd only,
 *               so the result does not depend on scheduling.  nslabs (P+1) (G+1) <= 2^31 - 1.  `merge` != 0 adds runs of equal keys inside a
 *               wave with one atomic (same results).
 *   4 areas     pred_area[s,p] = sum_g counts[s,p,g] over all columns, void included (p < P); gt_area[s,g] = sum_p counts[s,p,g] over all rows, void
 *               included (g < G).  A segment with area 0 in a slab does not exist in that slab.
 *   5 match     for every g with gt_area > 0 and every p with pred_area > 0 and cat_p[p] == cat_g[g]: inter = counts[s,p,g],
 *               union = pred_area + gt_area - inter - counts[s,p,G] (the predicted pixels on void ground truth leave the union); the pair matches iff
 *               2 inter > union, tested in int64 - equality is no match.  Segments of one map are disjoint, so at most one p matches a g and at most
 *               one g a p.  match int32 [nslabs, G] = the row or -1; iou double [nslabs, G] = (double)inter / (double)union, one IEEE division, or 0.
 *   6 misses    an existing g without a match is an FN.  An existing p without a match is IGNORED if 2 counts[s,p,G] > pred_area[s,p] (more than half of
 *               it on void), otherwise an FP.  pred_state int32 [nslabs, P]: 0 absent, 1 matched, 2 FP, 3 ignored.
 *   7, 8        per-category tp / fp / fn / iou_sum, PQ = iou_sum / (tp + fp / 2 + fn / 2), SQ, RQ, their means, and the semantic mIoU / pixel accuracy
 *               of the category-merged table are float64 host arithmetic on the copied tables (panst3r_amd/engine/evaluate.py).
 * Every output of pst_pq_match is written by one thread with plain stores.  cat_p int32 [P], cat_g int32 [G] are device arrays; an operand of P (or G)
 * rows may be null when P (or G) is 0. */
int pst_pq_count(const int32_t* pred, const int32_t* gt, int64_t N, const int64_t* slab_off, int nslabs, const int32_t* id2row_p, int ntab_p,
                 const int32_t* id2row_g, int ntab_g, int P, int G, int32_t* counts, int merge, void* stream);
int pst_pq_match(const int32_t* counts, int nslabs, int P, int G, const int32_t* cat_p, const int32_t* cat_g, int32_t* pred_area, int32_t* gt_area,
                 int32_t* match, double* iou, int32_t* pred_state, void* stream);

/* ---------------------------------------------------------------- depth evaluation against ground truth (f16; ABI 20, additive; no counterpart in the reference)
 * V predicted depth maps against V ground-truth depth maps of the same shapes (0 = no surface, as pst_mesh_resolve writes them): the moments of an
 * alignment p' = s p + b, exact medians, and the error sums behind AbsRel, SqRel, RMSE, MAE and the inlier ratios delta < t.  Restated in numpy in
 * tests/depth_eval_ref.py [restated, parity unpinned]; csrc/depth_eval.hip is held to that bit for bit.  Contraction is off in the kernels: every fp32
 * and fp64 operation is rounded on its own, in the order written here.
 *   1 valid     pixel i of a view is VALID iff g = gt[i] is finite and min_depth < g <= max_depth, p = pred[i * stride] is finite and p > 0, and, where
 *               the view has a confidence plane, conf[i] >= conf_thr (a NaN confidence is invalid: the rule of pst_cloud_count, so a
 *               consistency-filtered source scores only what it kept).  Validity never depends on the alignment.
 *   2 slabs     S = nslabs slabs, each a run of consecutive views: every view its own (scope 'view'), or one slab with all views (scope 'scene').  A
 *               slab is aligned and scored as one.
 *   3 blocks    the view table: row v = PST_DEPTH_VIEW_WORDS int64 words - [0] the address of pred (fp32), [1] its element stride >= 1 (3 reads the z
 *               of a pointmap in place), [2] the address of gt (fp32, stride 1), [3] the address of conf (fp32, stride 1) or 0, [4] npix >= 1, [5]
 *               first_block, [6] slab, [7] 0.  View v owns the ceil(npix / PST_ICP_CHUNK) consecutive blocks from first_block (view 0 starts at 0, the
 *               blocks of all views count to nblocks); slab is 0 for view 0, ascends by 0 or 1 and ends at S - 1.  `views` is the table in DEVICE
 *               memory, `views_host` the same rows in host memory: the entry points read only the host copy for their refusals, the kernels only
 *               the device copy.  slab_rows int32 [S + 1] (device): slab s owns the rows [slab_rows[s], slab_rows[s + 1]) of partials - the blocks
 *               of its views.
 *   4 align     p' = s p + b in fp64 on the widened fp32 p: one rounded product, one rounded sum.  (s, b) per slab in align double [S, 2]:
 *               (1, 0), a given scale, fp64(median g) / fp64(median p), sum pg / sum pp, or the least-squares pair from n, sum p, sum g, sum pp,
 *               sum pg - solved on the host in fp64 from pst_depth_moments / pst_depth_median.
 *               pst_depth_median: the exact fp32 medians of p and of g over the valid pixels of every slab by a four-pass radix select, most
 *               significant byte first (csrc/radix_select.h is the one text of the passes, shared with pst_cloud_segment_median: the raw bits as
 *               keys here, groups of 2 slots).  Valid values are positive and finite, so their bit patterns order as the values do: the key is the bits,
 *               with no rule for NaN or signed zero.  Histograms in LDS, flushed with int32 atomics (order-independent); a one-wave kernel narrows
 *               the two ranks (n - 1) / 2 and n / 2 after every pass.  median fp32 [S, 2] = (of p, of g): the middle element for an odd count,
 *               (a + b) * 0.5f in fp32 for an even one, NaN for n = 0; count int32 [S] = n.  Workspaces int32, ZEROED BY THE CALLER, left zeroed:
 *               hist [S, 2, 2, 256] (16-byte aligned), prefix uint32 [S, 2, 2], rank [S, 2, 2].
 *   5 terms     pst_depth_moments adds per valid pixel, widened to fp64: 1, p, g, p p, p g (products of two widened fp32 are exact) -> moments
 *               [0, 5).  pst_depth_errors, with d = p' - g: 1, |d| / g, (d d) / g, d d, |d| -> moments [0, 5), and for each of K <= 4 thresholds
 *               t_k (fp64): 1.0 iff p' < t_k g and g < t_k p' (two rounded products; strict: equality is no inlier; a non-positive p' fails by
 *               itself) -> moment 5 + k.  The other moments of the PST_DEPTH_MOMENTS are +0.0.
 *   6 order     step 4 of the icp section with PST_ICP_CHUNK and PST_ICP_LANES (csrc/icp_sum.h is the one text): lane l of block b of a view adds
 *               the view's pixels PST_ICP_CHUNK (b - first_block) + l + PST_ICP_LANES j, j ascending, into accumulators that start at +0.0 (an
 *               invalid pixel adds nothing), the block is reduced by the butterfly and the wave order of that step -> row b of partials double
 *               [nblocks, PST_DEPTH_MOMENTS].  A second launch of one block per slab adds the slab's rows of partials the same way - lane l takes its
 *               rows slab_rows[s] + l, + PST_ICP_LANES, ... ascending - into out double [S, PST_DEPTH_MOMENTS].  No float atomics: two calls give
 *               equal bytes.
 *   7 metrics   abs_rel = sum |d|/g / n, sq_rel = sum dd/g / n, rmse = sqrt(sum dd / n), mae = sum |d| / n, delta_k = count_k / n: float64 host
 *               arithmetic on out (panst3r_amd/engine/depth_eval.py).  Log-space metrics are left out: a device log is not bit-identical to numpy's.
 * PST_EINVAL before any launch: a null operand (a null pred or gt address in a row included), nviews < 1, S < 1, K < 0 or K > 4, a stride < 1, npix < 1,
 * a total of pixels >= 2^31, first_block or slab entries that are not the ones step 3 names, a block count that is not nblocks, a hist that is not
 * 16-byte aligned, a min_depth that is negative or NaN (all three entry points: a valid g is then > 0, which step 4's bit order rests on). */
#define PST_DEPTH_VIEW_WORDS 8    /* int64 words per row of the view table */
#define PST_DEPTH_MOMENTS 16      /* doubles per row of partials and per slab in out */
int pst_depth_median(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, int nslabs, float min_depth, float max_depth, float conf_thr,
                     int32_t* hist, uint32_t* prefix, int32_t* rank, int32_t* count, float* median, void* stream);
int pst_depth_moments(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, const int32_t* slab_rows, int nslabs, float min_depth,
                      float max_depth, float conf_thr, double* partials, double* out, void* stream);
int pst_depth_errors(const int64_t* views, const int64_t* views_host, int nviews, int nblocks, const int32_t* slab_rows, int nslabs, float min_depth,
                     float max_depth, float conf_thr, const double* align, int K, double t0, double t1, double t2, double t3, double* partials, double* out,
                     void* stream);

/* ---------------------------------------------------------------- QUBO mask selection on the device (reference engine/postprocess.py:262-336: numpy on the host)
 * Minimises E(x) = x^T W x + lambda_reg * mean(x), x in {0,1}^N, by `replicas` independent simulated anneals run at once (the reference's moves,
 * acceptance rule and geometric schedule; it runs 20 restarts one after the other) and returns the best.  W fp32 [N, N] row-major, symmetric (the -W
 * of weight_from_masks), 1 <= N <= pst_qubo_anneal_max_n() (200: W is held in the LDS of one CU); a larger N is PST_EINVAL, nothing is written, and the
 * host annealer remains for it.  1 <= replicas <= 2^20, num_iters >= 0, T0 > 0, T_end > 0.  One wave per replica.
 * The result is a pure function of the arguments: counter-based random numbers (Philox4x32-10 keyed by `seed`, counter = (move / 2, replica, stream)),
 * incremental local fields, an exponential made of separately rounded fp32 operations, a fixed evaluation order; the inverse temperature is carried as
 * beta <- beta * cinv in fp32 (beta0 = fp32(1 / T0), cinv = fp32((T0 / T_end)^(1 / num_iters)), both taken in double on the host).  The operation order
 * is written out at the top of csrc/qubo_solve.hip and restated bit for bit in tests/qubo_ref.py [restated, own design].
 *   -> x_all uint8 [replicas, N]  every replica's best state;  e_all fp32 [replicas]  its energy, re-evaluated from scratch in a fixed order
 *      best_x uint8 [N], best_e fp32 [1]  those of the replica with the smallest (energy, index).  Plain stores, no atomics. */
int pst_qubo_anneal_max_n(void);
int pst_qubo_anneal(const float* W, int N, int replicas, int num_iters, float T0, float T_end, float lambda_reg, uint64_t seed, uint8_t* x_all, float* e_all,
                    uint8_t* best_x, float* best_e, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PANST3R_HIP_H */
