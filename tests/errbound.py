"""Per-element error bounds of the HIP kernels, derived from their arithmetic (not fitted to observed errors).

check(got, ref64, bound, what) asserts |got - ref| <= bound at EVERY element (and that got is finite) and returns the largest err / bound ratio.  A global
rel-L2 lets one wrong tile, one tail row, one dropped key or an intermediate rounded to the wrong format through when it is small in norm; a per-element bound
derived from the kernel's rounding steps does not.  References are float64 evaluations of the SAME rounded inputs the kernel gets.

Notation: u(f) = unit roundoff of format f (bf16 2^-8, f16 2^-11, fp32 2^-24); tiny(f) = half the smallest subnormal spacing (the absolute error of a rounding
near zero).  tests/test_errbound.py proves on the CPU, for every bound here, that an emulation of the kernel's rounding path stays below half the bound and that
the typical kernel mistakes (accumulator through a 16-bit format, P rounded to the wrong format, a dropped key, a negated fragment, wrong LayerNorm eps, ...)
exceed it; tests/test_smallops_host.py does the same for the small row and pixel operations and tests/test_input_host.py for the image input at the end of
this file.

PST_ERRBOUND_LOG=<path>: every check() appends one JSON line {what, ratio, n} there (the per-family maxima the GPU run reports).
"""
import json
import math
import os

import torch

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
U32 = 2.0 ** -24
LAMBDA = 5.0            # probabilistic factor of the attention P-rounding term (sum of independent roundings: a 5-sigma envelope)
# A round-to-nearest store errs by up to half an ulp, i.e. up to u |y| just above a power of two: every rounding to a storage format is allowed TWO u |y| (one
# ulp), so that a correct rounding sits at <= 0.5 of the bound and the margin is the same at every element.
R = 2.0


def u(fmt):
    """unit roundoff of a storage format (torch dtype or one of 'bf16' / 'f16' / 'fp32')"""
    fmt = _dtype(fmt)
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: U32, torch.float64: 2.0 ** -53}[fmt]


def tiny(fmt):
    """half the subnormal spacing: the absolute error of a rounding to fmt near zero"""
    fmt = _dtype(fmt)
    return {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150, torch.float64: 0.0}[fmt]


def _dtype(fmt):
    if isinstance(fmt, torch.dtype):
        return fmt
    return {'bf16': torch.bfloat16, 'f16': torch.float16, 'fp16': torch.float16, 'fp32': torch.float32}[fmt]


def check(got, ref, bound, what):
    """assert |got - ref| <= bound elementwise (bound broadcasts against ref) and that got is finite; returns max(err / bound)"""
    got = got.detach().double()
    ref = ref.detach().double().to(got.device)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device).expand_as(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(got)
    assert bool(fin.all()), '%s: %d non-finite outputs, first at %s' % (what, int((~fin).sum()), tuple(int(i) for i in (~fin).nonzero()[0]))
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = int(ratio.reshape(-1).argmax())
    r = float(ratio.reshape(-1)[worst])
    if os.environ.get('PST_ERRBOUND_LOG'):
        with open(os.environ['PST_ERRBOUND_LOG'], 'a') as f:
            f.write(json.dumps(dict(what=what, ratio=r, n=ref.numel())) + '\n')
    if r > 1.0:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ref.shape))
        nbad = int((err > bound).sum())
        raise AssertionError('%s: %d of %d elements exceed the error bound; worst at %s: got %.9g ref %.9g |err| %.3g bound %.3g (ratio %.3g)'
                             % (what, nbad, ref.numel(), idx, float(got[idx]), float(ref[idx]), float(err[idx]), float(bound[idx]), r))
    return r


# ------------------------------------------------------------------------------------------------------------------------------------------- GEMM
GELU_LIP = 1.13          # max |d/dx GELU(x)| (x ~ 2.42): the Lipschitz factor an activation applies to the error of its argument
GELU_ERF_ABS = 1.5e-7    # |erf error| of Abramowitz-Stegun 7.1.26 (common.h gelu_erf2): 0.5 |x| of it reaches the output


def gemm_bound(a, w, out_fmt, bias=None, act=None, gamma=None, res=None, mode='mfma16'):
    """Per-element bound of C = epilogue(A W^T) for the HIP GEMMs, A [M, K] and W [N, K] the exact operands (16-bit values, or fp32 for the fp32 modes).

    mode 'mfma16' (gemm.hip, gemm256.hip, rowstream.hip, maskhead.hip): products of 16-bit operands are exact in fp32; v_mfma_f32_16x16x32 adds 32 of them
    into the fp32 accumulator per step, K / 32 steps -> (K/32 + 2) * 2 u32 * sum_k |a_k w_k|.  Epilogue (gemm.hip row_phase / the accumulator-layout
    epilogue): fmaf(acc, 1, bias) in fp32 (one rounding), GELU(erf) (gelu_erf2) or ReLU, x gamma (one rounding), then
      - no residual: one rounding to the output format;
      - fp32 residual, fp32 output: one fp32 add;
      - residual and 16-bit output: the value is rounded to 16 bit into the LDS C tile, the residual is added in fp32, rounded once more (two roundings).
    mode 'x3' (split.hip + the 16-bit kernels over 3K: [hi, hi, lo] x [hi, lo, hi]): x = hi + lo with f16 hi / lo -> each operand carries 2^-22 relative
    (+ 2^-25 absolute, f16 subnormal lo), the dropped lo x lo term 2^-22 |a w|, 3K / 32 accumulation steps.
    mode 'fp32' (gemm_f32.hip, v_mfma_f32_16x16x4_f32): every product rounded once (u32), K / 4 accumulation steps.
    Bound = (output / intermediate roundings) + Lip(act) * |gamma| * (accumulation + bias rounding) + activation approximation."""
    a64, w64 = a.double(), w.double()
    core = a64 @ w64.T
    acc = acc_bound(a64.abs() @ w64.abs().T, a.shape[-1], mode, a64.abs().sum(-1, keepdim=True), w64.abs().sum(-1)[None])
    return gemm_bound_from(core, acc, out_fmt, bias, act, gamma, res)


def acc_bound(absprod, K, mode, sum_a=None, sum_w=None):
    """bound of the fp32 accumulator's error of a K-long dot product (gemm_bound's three modes); absprod = sum_k |a_k w_k|; sum_a / sum_w = sum_k |a_k| /
    sum_k |w_k| (x3 only: the absolute error of an f16-subnormal lo part)"""
    if mode == 'mfma16':
        return 2 * (K / 32 + 2) * U32 * absprod
    if mode == 'x3':
        return 2 * (3 * K / 32 + 2) * U32 * absprod + 3 * 2.0 ** -22 * absprod + 2.0 ** -25 * (sum_a + sum_w)
    if mode == 'fp32':
        return 2 * (K / 4 + 2) * U32 * absprod + U32 * absprod
    raise ValueError(mode)


def ln_fold_bound(xc, wf, cs, bias, x, eps, out_fmt, act=None):
    """LayerNorm folded into the consuming GEMM (gemm.hip, ln_fold_prologue / ln_fold_entry in common.h): the raw 16-bit rows xc times the gamma-folded
    16-bit W (mfma16 accumulator), then out = act(fmaf(acc, rstd, fmaf(-mean rstd, cs, bias))).  mean / rstd come from the fp32 per-64-column (sum, sumsq)
    partials of the fp32 rows x: one-pass statistics, var = E[x^2] - mean^2 (rownorm_bound's one-pass model).  cs = the fp32 column sums of wf, taken as
    given.  Returns (float64 reference of the same inputs, bound): the row-norm errors dm (mean) and dr (relative rstd) reach the output as
    rstd (|acc| dr + |cs| (|mean| dr + dm)), the accumulator's as rstd acc_err, then the GEMM epilogue (gemm_bound_from)."""
    x64, xc64, wf64, cs64 = x.double(), xc.double(), wf.double(), cs.double()
    D = x64.shape[-1]
    nred = D / 16 + 8
    mean = x64.mean(-1, keepdim=True)
    var = (x64 * x64).mean(-1, keepdim=True) - mean * mean
    r = (var + eps).rsqrt()
    dm = nred * U32 * x64.abs().mean(-1, keepdim=True) + U32 * mean.abs()
    dv = 2 * nred * U32 * (x64 * x64).mean(-1, keepdim=True) + 2 * U32 * (var + eps) + 2 * dm * mean.abs()
    dr = dv / (2 * (var + eps)) + 3 * U32
    raw = xc64 @ wf64.T
    core = r * raw - (mean * r) * cs64[None]
    acc = r * (acc_bound(xc64.abs() @ wf64.abs().T, D, 'mfma16') + raw.abs() * dr) + r * cs64.abs()[None] * (mean.abs() * (dr + U32) + dm) \
        + U32 * ((mean * r) * cs64[None]).abs()
    ref = core + bias.double()
    ref = torch.nn.functional.gelu(ref) if act == 'gelu' else ref
    return ref, gemm_bound_from(core, acc, out_fmt, bias, act)


def gemm_bound_from(core, acc, out_fmt, bias=None, act=None, gamma=None, res=None):
    """the epilogue part of gemm_bound: core = exact A W^T (float64), acc = bound of the accumulator's error (same shape)"""
    pre = core + (bias.double() if bias is not None else 0.0)
    err = acc + U32 * pre.abs()                                     # fmaf(acc, 1, bias): one fp32 rounding
    if act == 'gelu':
        y = torch.nn.functional.gelu(pre)
        err = GELU_LIP * err + pre.abs() * (0.5 * GELU_ERF_ABS + 8 * U32)
    elif act == 'gelu_tanh':
        y = torch.nn.functional.gelu(pre, approximate='tanh')
        err = GELU_LIP * err + pre.abs() * 16 * U32
    elif act == 'relu':
        y = torch.relu(pre)
    elif act is None:
        y = pre
    else:
        raise ValueError(act)
    if gamma is not None:
        g = gamma.double()
        y = y * g
        err = err * g.abs() + U32 * y.abs()
    uo = u(out_fmt)
    if res is not None:
        if _dtype(out_fmt) != torch.float32:
            err = err + R * uo * (y.abs() + err) + tiny(out_fmt)            # 16-bit value in the LDS C tile, then the residual add
        y = y + res.double()
        err = err + U32 * y.abs()
    return err + R * uo * (y.abs() + err) + tiny(out_fmt)


# ------------------------------------------------------------------------------------------------------------------------------------------- attention
def attn_ref(q, k, v, mask=None, pre=False):
    """float64 softmax attention of the given (rounded) operands, [B, H, N, hd]; mask [B, Nq, Nk] True = blocked; a row with every key blocked is 0 (the
    kernels' l == 0 guard).  pre: q carries hd^-0.5 log2(e) already (softmax of q.k ln 2)."""
    return attn_bound(q, k, v, mask, pre, 'fp32', 'fp32', _ref_only=True)


def attn_bound(q, k, v, mask, pre, out_fmt, p_fmt, nsplit=1, mode='mfma16', _ref_only=False):
    """Per-element bound of O = softmax(q k^T scale) v for attention.hip (mode 'mfma16'), attn_x3.hip ('x3') and attn_f32.hip ('fp32').

    attention.hip: S - m is one MFMA chain in fp32 on top of -m (hd / 32 steps, :186-197), P = exp2((S - m) c) (v_exp_f32) is rounded to the 16-bit format
    p_fmt (:269-280); the row sum l is the MFMA sum of the SAME rounded P (:300), O accumulates rounded P times V in fp32; lazy rescaling (:236-258) keeps
    1 <= P_max <= 2^8; split-K partials are merged in fp32 (:385-394); one rounding to out_fmt at the store (:333).  Because l sums the rounded P, the P
    rounding moves O by sum_j p_j eps_j (v_j - O) with independent |eps_j| <= u(p_fmt): the probabilistic form LAMBDA * sqrt(sum_j e_j^2 (v_j - O)^2),
    e_j = max(u(p_fmt) p_j, tiny(p_fmt) p_max) (a subnormal P has an absolute error; P_max >= 1 bounds l from below).  The worst case
    u(p_fmt) sum_j p_j |v_j - O| would be about sqrt(Nk) times larger and hide a missing key under a near-uniform softmax.
    Score errors (fp32 accumulation, the scale multiply, exp2) move P_j by the relative eta_j: sum_j p_j eta_j |v_j - O| (worst case, u32-sized).
    The fp32 P V / l accumulation: 2 (Nk/32 + nsplit + 4) u32 (sum_j p_j |v_j| + |O|).
    mode 'x3': P, V, Q and K carry 2^-22 (split hi + lo f16 operands), products 3 2^-22.  mode 'fp32': P in fp32, every product rounded (u32).
    Returns the bound [B, H, Nq, hd] (or with _ref_only the float64 reference)."""
    B, H, Nq, hd = q.shape
    Nk = k.shape[2]
    scale = LN2 if pre else hd ** -0.5
    c_exp = 1.0 if pre else hd ** -0.5 * LOG2E
    up, tp = u(p_fmt), tiny(p_fmt)
    eps_prod = {'mfma16': 0.0, 'x3': 3 * 2.0 ** -22, 'fp32': U32}[mode]
    eps_v = {'mfma16': 0.0, 'x3': 2 * 2.0 ** -22, 'fp32': 0.0}[mode]
    if mode == 'x3':
        up, tp = 2.0 ** -22, 2.0 ** -25
    nacc_s = hd / (4 if mode == 'fp32' else 32) * (3 if mode == 'x3' else 1) + 3
    nacc_o = Nk / (4 if mode == 'fp32' else 32) * (3 if mode == 'x3' else 1) + nsplit + 4
    out = torch.empty(B, H, Nq, hd, dtype=torch.float64, device=q.device)
    for b in range(B):
        for h in range(H):
            q64, k64, v64 = q[b, h].double(), k[b, h].double(), v[b, h].double()
            raw = q64 @ k64.T
            s = raw * scale
            if mask is not None:
                s = s.masked_fill(mask[b].to(q.device), float('-inf'))
            dead = torch.isinf(s).all(-1, keepdim=True)
            p = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
            if mask is not None:
                p = p.masked_fill(mask[b].to(q.device), 0.0)
            ref = p @ v64
            if _ref_only:
                out[b, h] = ref
                continue
            absv = v64.abs()
            # P rounding, probabilistic: sqrt(sum_j e_j^2 (v_j - ref)^2) = sqrt(W v^2 - 2 ref (W v) + ref^2 sum W), W = e^2
            e = torch.maximum(R * up * p, tp * p.amax(-1, keepdim=True)) * (p > 0)
            W = e * e
            var = (W @ (v64 * v64) - 2 * ref * (W @ v64) + ref * ref * W.sum(-1, keepdim=True)).clamp_min(0.0)
            t_p = LAMBDA * var.sqrt()
            # score error -> relative P error eta_j (worst case)
            absqk = q64.abs() @ k64.abs().T
            smax = raw.abs().amax(-1, keepdim=True) + 8.0 / c_exp
            eta = LN2 * (c_exp * (nacc_s * 2 * U32 * (absqk + smax) + eps_prod * absqk) + U32 * (raw.abs() + smax) * c_exp) + 4 * U32
            pe = p * eta
            t_s = pe @ absv + ref.abs() * pe.sum(-1, keepdim=True)
            pv = p @ absv
            t_acc = 2 * nacc_o * U32 * (pv + ref.abs()) + eps_v * pv
            err = t_p + t_s + t_acc
            out[b, h] = err + R * u(out_fmt) * (ref.abs() + err) + tiny(out_fmt)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------- row norms
def rownorm_bound(x, gamma, beta, eps, out_fmt, one_pass=False, relu=False, nred=None):
    """Per-element bound of a LayerNorm-type row normalisation y = (x - mean) rstd gamma + beta over the last axis of x (float64 of the kernel's exact
    input rows; for GroupNorm pass x reshaped so the last axis is one group and gamma / beta broadcast to it).

    Statistics in fp32 (misc.hip layernorm_kernel :96-124 and layernorm384_kernel: per-lane sequential sums then a lane tree; two passes - mean, then
    sum (x - mean)^2; one_pass: GroupNorm's (sum, sumsq) statistics, var = E[x^2] - mean^2 - cancellation relative to E[x^2]), each sum with at most
    nred = D / 16 + 8 rounding steps; rsqrtf; (x - mean) rstd gamma + beta in fp32; one rounding to out_fmt.
      mean error      dm = nred u32 mean|x| + u32 |mean|
      variance error  dv = nred u32 (var, or 2 E[x^2] one-pass) + 2 u32 (var + eps)
      rstd relative   dr = dv / (2 (var + eps)) + 2 u32
      y error         |gamma| rstd (dm + u32 |x - mean| + |x - mean| dr) + 3 u32 |y|, then the output rounding."""
    x64 = x.double()
    D = x64.shape[-1]
    if nred is None:
        nred = D / 16 + 8
    mean = x64.mean(-1, keepdim=True)
    xc = x64 - mean
    var = (xc * xc).mean(-1, keepdim=True)
    r = (var + eps).rsqrt()
    g = gamma.double() if torch.is_tensor(gamma) else torch.tensor(float(gamma), dtype=torch.float64)
    bt = beta.double() if torch.is_tensor(beta) else torch.tensor(float(beta), dtype=torch.float64)
    y = xc * r * g + bt
    dm = nred * U32 * x64.abs().mean(-1, keepdim=True) + U32 * mean.abs()
    dv = nred * U32 * (2 * (x64 * x64).mean(-1, keepdim=True) if one_pass else var) + 2 * U32 * (var + eps) + 2 * dm * xc.abs().mean(-1, keepdim=True)
    dr = dv / (2 * (var + eps)) + 2 * U32
    err = g.abs() * r * (dm + U32 * xc.abs() + xc.abs() * dr) + 3 * U32 * y.abs()
    if relu:
        y = torch.relu(y)
    return err + R * u(out_fmt) * (y.abs() + err) + tiny(out_fmt)


def layernorm_ref(x, gamma, beta, eps):
    x64 = x.double()
    return torch.nn.functional.layer_norm(x64, (x64.shape[-1],), gamma.double(), beta.double(), eps)


# ------------------------------------------------------------------------------------------------------------------------------------------- elementwise
def elementwise_bound(ref, out_fmt, in_abs=None, n_ops=4):
    """An elementwise op evaluated in fp32 and rounded once: u(out) |ref| + n_ops u32 in_abs (in_abs = the magnitude of the fp32 terms that are combined,
    e.g. |x| + |partner| for a rotation; default |ref|)."""
    ref = ref.double()
    in_abs = ref.abs() if in_abs is None else in_abs.double()
    err = n_ops * U32 * in_abs
    return err + R * u(out_fmt) * (ref.abs() + err) + tiny(out_fmt)


def rope2d(x, pos, out_fmt, base=100.0):
    """RoPE-2D (misc.hip / the fused GEMM store, tables of hip.rope_table): x [..., T, hd], integer positions pos [T, 2] (y, x); per head the first hd / 2
    channels rotate with y, the rest with x, each half a 1-D RoPE over D = hd / 2 with rotate_half pairs (i, i + D/2).  Returns (float64 reference, bound).
    The kernel: fp32 table (inv_freq = base^(-2i/D) and angle = pos inv_freq in fp32: |d angle| <= 3 u32 |angle|, cos / sin rounded: + u32), one product
    rounded and one fma: |err| <= (|x| + |partner|) (3 u32 |angle| + 4 u32), then the output rounding."""
    x64 = x.double()
    hd = x64.shape[-1]
    D = hd // 2
    inv = base ** (-torch.arange(0, D, 2, dtype=torch.float64, device=x64.device) / D)
    outs, errs = [], []
    for half in range(2):
        t = x64[..., half * D:(half + 1) * D]
        ang = pos[:, half].to(x64.device).double()[:, None] * inv[None]
        ang = torch.cat([ang, ang], -1)
        partner = torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1)
        outs.append(t * ang.cos() + partner * ang.sin())
        errs.append((t.abs() + partner.abs()) * (3 * U32 * ang.abs() + 4 * U32))
    ref, err = torch.cat(outs, -1), torch.cat(errs, -1)
    return ref, err + R * u(out_fmt) * (ref.abs() + err) + tiny(out_fmt)


def conv3x3(x, wt, bias, out_fmt, mode='mfma16'):
    """the implicit-GEMM 3 x 3 convolution (gemm.hip conv mode, padding 1): x NHWC [V, H, W, Cin], wt [Cout, Cin, 3, 3].  A K = 9 Cin dot product per output
    whose zero-padded taps add nothing: gemm_bound's accumulator model on sum |x| |w| over the taps that exist.  Returns (float64 reference [V H W, Cout],
    bound)."""
    V, H, W, Cin = x.shape
    Cout = wt.shape[0]
    conv = lambda xx, ww: torch.nn.functional.conv2d(xx.permute(0, 3, 1, 2), ww, padding=1).permute(0, 2, 3, 1).reshape(V * H * W, -1)
    x64, w64 = x.double(), wt.double()
    core = conv(x64, w64)
    sum_a = conv(x64.abs(), torch.ones(1, Cin, 3, 3, dtype=torch.float64, device=x64.device))
    acc = acc_bound(conv(x64.abs(), w64.abs()), 9 * Cin, mode, sum_a, w64.abs().sum((1, 2, 3))[None])
    return core + bias.double(), gemm_bound_from(core, acc, out_fmt, bias)


def groupnorm(x, n, P, G, gamma, beta, eps, out_fmt, relu=False):
    """GroupNorm over pixel-major rows x [n P, C] (G groups of C / G channels, per view), statistics of pst_groupnorm_stats: fp32 (sum, sumsq) partials over
    256-element pieces merged per group - one-pass, nred = P C / (256 G) + 64 steps.  Returns (float64 reference [n P, C], bound)."""
    C = x.shape[-1]
    Cg = C // G
    x64 = x.double()
    xg = x64.reshape(n, P, G, Cg).permute(0, 2, 1, 3).reshape(n, G, P * Cg)
    per = lambda t: t.double().to(x64.device).reshape(G, 1, Cg).expand(G, P, Cg).reshape(1, G, P * Cg)
    back = lambda t: t.reshape(n, G, P, Cg).permute(0, 2, 1, 3).reshape(n * P, C)
    ref = torch.nn.functional.group_norm(x64.reshape(n, P, C).permute(0, 2, 1), G, gamma.double().to(x64.device), beta.double().to(x64.device), eps)
    ref = ref.permute(0, 2, 1).reshape(n * P, C)
    ref = torch.relu(ref) if relu else ref
    return ref, back(rownorm_bound(xg, per(gamma), per(beta), eps, out_fmt, one_pass=True, relu=relu, nred=P * Cg / 256 + 64))


# ------------------------------------------------------------------------------------------------------------------------------------------- output stages
# postprocess.hip / pointmap.hip (tests/test_hip_pp_stages.py, tests/test_hip_pointmap_stages.py; soundness and tightness: tests/test_pp_stage_checks.py).
# Division and sqrtf are IEEE-rounded in these builds (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the v_div_scale / v_div_fmas sequence
# in the ISA): one rounding each.  For the device expf and expm1f the installation carries no accuracy table, so their allowance is MEASURED against the
# float64 reference, never against a second run of the kernel: twice the largest error seen on the MI355X (profiles/output_kernel_margins.jsonl, rows
# 'expf_ulp' / 'expm1f_ulp'), a factor of two because the cases sample the argument range rather than cover it.
#   expf:   conf = 1 + expf(c) of pointmap_activate over c in [0, 80] (131072 logarithmically and linearly spaced arguments; the error of conf in ulps of
#           exp(c), which includes the rounding of the addition - up to one ulp of exp(c) for c < ln 2): largest 1.764 ulp.
#   expm1f: x expm1f(d) / d of pointmap_activate on axis-aligned vectors (d = |x| exactly) over d in [1e-12, 88] (the error in ulps of the result, which
#           includes the roundings of the division and of the product): largest 2.185 ulp.
# tests/test_hip_pointmap_stages.py::test_device_math_ulps repeats the measurement and fails if twice the observed error exceeds the allowance.
EXPF_ULP = 3.6           # 2 x 1.764, rounded up
EXPM1F_ULP = 4.4         # 2 x 2.185, rounded up
TINY32 = 2.0 ** -149     # absolute error of an fp32 result in the subnormal range


def sigmoid_bound(s):
    """1.0f / (1.0f + expf(-x)) against s = sigmoid(x) (float64): expf moves e = exp(-x) by EXPF_ULP ulps, which reaches s scaled by e / (1 + e) = 1 - s;
    the addition and the division round once each."""
    s = torch.as_tensor(s, dtype=torch.float64)
    return R * U32 * (2.0 + EXPF_ULP * (1.0 - s)) * s + TINY32


def blend_bound(m, dm_taps):
    """m = hy (hx a + lx b) + ly (hx c + lx d) in fp32 with exact fp32 weights: every tap passes through at most four roundings on its way to m (product,
    sum, product, sum; a contracted fma only removes some), the taps are non-negative: 4 R u32 m, plus the blend of the taps' own errors dm_taps."""
    return dm_taps + 4 * R * U32 * torch.as_tensor(m, dtype=torch.float64).abs() + TINY32


def product_bound(score, m, dm):
    """score * m in fp32, score an exact fp32 input: |score| dm + one rounding"""
    return score.abs() * dm + R * U32 * (score * m).abs() + TINY32


def softmax_score_bound(arg, darg, ncls):
    """score = 1 / sum_c expf(arg_c), arg_c <= 0 with max 0 (float64 [Q, Ncls]), darg the bound of the fp32 argument's error.  expf: EXPF_ULP ulps + its
    argument's error (d exp = exp darg); the sum: ceil(Ncls / 64) sequential adds per lane and 6 tree levels; one division.  Relative to the score the sum's
    relative error carries over unchanged."""
    t = arg.exp()
    dt = t * (EXPF_ULP * R * U32 + darg) + TINY32
    S = t.sum(-1)
    nadd = -(-ncls // 64) + 6
    rel = dt.sum(-1) / S + nadd * R * U32 + R * U32
    return rel / S + TINY32


def chunked_sum_bound(S, nchunk, chunk=256):
    """sum of non-negative fp32 terms: sequential fp32 sums of at most `chunk` terms (every one of the chunk - 1 additions rounds a partial <= the chunk's sum),
    the chunk sums then added in double: (chunk R u32 + nchunk 2^-53) S"""
    return (chunk * R * U32 + nchunk * 2.0 ** -53) * S.abs()


def activate_bound(xyz64, ref):
    """pointmap_activate 'norm_exp': d = sqrtf(x^2 + y^2 + z^2) (each square through <= 3 roundings, the root halves that and rounds once: 2.5 -> 3 R u32
    relative), s = expm1f(d) / max(d, 1e-8f), out = x s.  The error of d reaches s through kappa = |d g'(d) / g(d)| = d e^d / (e^d - 1) - 1 with
    g = expm1(d) / d (in the clipped branch s is proportional to d: kappa = 1, and 1e-8f is one rounding away from 1e-8)."""
    d = xyz64.norm(dim=-1, keepdim=True)
    kap = torch.where(d < 1e-8, torch.ones_like(d), d * d.exp() / torch.expm1(d).clamp_min(1e-300) - 1.0)
    kap = torch.where(d == 0, torch.zeros_like(d), kap).clamp_min(0.0)
    rel = (EXPM1F_ULP + 2.0 + 3.0 * kap + (d < 2e-8).double()) * R * U32
    return rel * ref.abs() + TINY32


def conf_bound(c64):
    """conf = 1.0f + expf(c): EXPF_ULP ulps of exp(c) and the addition's rounding"""
    e = c64.exp()
    return EXPF_ULP * R * U32 * e + R * U32 * (1.0 + e) + TINY32


def select_bound(ref, D):
    """retrieval.hip select_kernel, out = x / max(sqrtf(key), 1e-12f) against ref = x / max(||x||, 1e-12) (float64 of the same fp32 row).  key = the fp32
    sum of the D squares: lane l of 64 chains ceil(D / 64) fmas (one rounding each; the terms are non-negative, so every rounding is relative to a partial
    <= key), a six-step butterfly adds the lanes -> (ceil(D / 64) + 6) u32 relative; the root halves that and rounds once, the division rounds once, and for
    a clamped row 1e-12f is one rounding away from 1e-12.  Each rounding allowed twice (R), like everywhere here."""
    n = -(-D // 64)
    return R * U32 * ((n + 6) / 2.0 + 3.0) * torch.as_tensor(ref, dtype=torch.float64).abs() + TINY32


def moments_bound(abs_terms, nadd, dw_terms):
    """rigid_moments: double sums of nadd additions (+ 3 for the products w y x in double) over terms whose absolute sum is abs_terms, and the single fp32
    rounding of w = conf + weight_offset: dw_terms = the same moments of |fl32(conf + off) - (conf + off)|, which the CPU computes exactly (0 with offset 0);
    allowed twice, like every rounding here"""
    return (nadd + 3) * 2.0 ** -53 * abs_terms + R * dw_terms


# ------------------------------------------------------------------------------------------------------------------------------------------- LoftUp guidance
# loftup.hip's sincos_cw (Cody-Waite reduction by three fma steps, Cephes polynomials) promises 1e-7 absolute for |x| < 6e4.  Like the device expf above its
# allowance is MEASURED against float64 sin / cos of the SAME fp32 argument, never against a second run of the kernel: twice the largest error seen on the
# MI355X (profiles/output_kernel_margins.jsonl, rows 'sincos_cw_abs' over the product's range - coordinates of a 256 x 256 grid times the five lr_pe
# frequencies up to e^10, biases in [-pi, pi] - and 'sincos_cw_abs_limit' over the documented |x| < 6e4), a factor of two because the cases sample the
# range.  Largest seen: 8.54e-8 and 8.73e-8, the rounding of the fp32 result included (a replay of the routine's IEEE operations on the host over 6e7
# random arguments per range finds 9.30e-8 and 9.40e-8: inside the allowance, and inside the routine's promise).  tests/test_hip_guidance.py::test_sincos_cw_error repeats
# the measurement and fails if twice the observed error exceeds the allowance.
# A condition, not a measurement: the allowance must stay below 2^-13, one ulp of the smallest phase (2048 rad) at which a one-ulp phase error still matters -
# otherwise the bound could not tell a correct sine from the sine of a phase that is one ulp off.
SINCOS_ABS = 1.75e-7     # 2 x 8.73e-8, rounded up
SINCOS_ABS_MAX = 2.0 ** -13


def guidance_nred(P, nf):
    """rounding steps on the way of one feature into pst_loftup_guidance_gn's (sum, sumsq) (guidance_px_kernel<false>): a thread walks ceil(tiles / 128)
    tiles; per tile ceil(nf / 4) frequencies x 5 inputs, each step rounding vs + vc (or vs^2 + vc^2 and its two products: counted below) and the
    accumulation, then the 3 colours; block_reduce: 6 shuffle levels + 3 adds over the waves; reduce_partials_kernel: at most 128 / 64 = 2 serial adds and 6
    shuffle levels."""
    ntile = -(-P // 64)
    trips = -(-ntile // 128)
    return trips * (2 * 5 * -(-nf // 4) + 3) + 9 + 8


def guidance_perturbation(z, s, gamma, delta):
    """|change of gamma z| when every input of the normalisation moves by at most delta: |gamma| delta (2 + |z|) / (s - delta), s = sqrt(var + eps)
    (derivation: guidance_bound)"""
    return gamma.abs() * delta * (2.0 + z.abs()) / (s - delta).clamp_min(1e-300)


def guidance_bound(feat64, gamma, beta, eps, nf, out_fmt='fp32', delta=None):
    """Per-element bound of pst_loftup_guidance_gn's output against float64 GroupNorm(1) of feat64 = guidance_ref.features64 (float64 [n, P, CH]: sin / cos
    in float64 of the fp32 phases, the scaled colours).  Returns (ref64 [n P, CH], bound, stats64 [n, 2], stats_bound [n, 2]).

    Two terms.  (a) The kernel's arithmetic on ITS features: one-pass fp32 (sum, sumsq) with guidance_nred rounding steps (+ 2 for the squares), rsqrtf,
    (x - mean) rstd gamma + beta in fp32: rownorm_bound(one_pass=True).  (b) Its features are not feat64 but x + e, |e| <= delta = SINCOS_ABS + u32
    (sincos_cw's measured error, which includes the rounding of its result, and one more fp32 rounding for the colours' last bit).  With mu the mean,
    s = sqrt(var + eps), z = (x - mu) / s and y = gamma z + beta:  mu moves by mean(e), at most delta; the standard deviation is 1-Lipschitz in the rms of
    the perturbation (triangle inequality of the l2 norm of x - mu), so sqrt(var) moves by at most delta and s by no more (d s / d sqrt(var) <= 1).  Then
        z' - z = (e_i - mean e) / s' + (x - mu) (1 / s' - 1 / s),   |z' - z| <= 2 delta / s' + |z| delta / s',   s' >= s - delta,
    i.e. to first order |gamma| rstd delta (2 + |z|); the bound keeps the exact denominators.  Term (a) is evaluated at feat64 instead of the kernel's own
    features: a difference of second order (u32 x delta).
    The statistics: |sum - S| <= nred u32 sum |x| + N delta;  |sumsq - S2| <= (nred + 2) u32 S2 + N (2 mean|x| delta + delta^2) (Cauchy-free worst case:
    sum 2 |x| delta), every fp32 step allowed twice (R) like everywhere here."""
    x = feat64.double()
    n, P, CH = x.shape
    delta = SINCOS_ABS + U32 if delta is None else delta
    nred = guidance_nred(P, nf)
    N = P * CH
    flat = x.reshape(n, 1, N)
    g = gamma.double().to(x.device).reshape(1, 1, CH).expand(n, P, CH).reshape(n, 1, N)
    bt = beta.double().to(x.device).reshape(1, 1, CH).expand(n, P, CH).reshape(n, 1, N)
    mean = flat.mean(-1, keepdim=True)
    var = ((flat - mean) ** 2).mean(-1, keepdim=True)
    s = (var + eps).sqrt()
    z = (flat - mean) / s
    ref = z * g + bt
    arith = rownorm_bound(flat, g, bt, eps, out_fmt, one_pass=True, nred=nred + 2)
    pert = guidance_perturbation(z, s, g, delta)
    bound = arith + pert * (1.0 + R * u(out_fmt))
    S, S2, A = flat.sum(-1), (flat * flat).sum(-1), flat.abs().sum(-1)
    stats = torch.cat([S, S2], -1)
    sb = torch.cat([R * nred * U32 * A + N * delta, R * (nred + 2) * U32 * S2 + 2 * A * delta + N * delta * delta], -1)
    return ref.reshape(n * P, CH), bound.reshape(n * P, CH), stats, sb


def sincos_bound(ref, out_fmt='fp32'):
    """a value written by sin_cw / cos_cw with nothing in between (pst_loftup_lr_pe): the measured allowance + one rounding to the output format"""
    return SINCOS_ABS + R * u(out_fmt) * (torch.as_tensor(ref, dtype=torch.float64).abs() + SINCOS_ABS) + tiny(out_fmt)


# ------------------------------------------------------------------------------------------------------------------------------------------- small row / pixel ops
# misc.hip's l2norm_rows, resize_bilinear and dino_preprocess (tests/test_hip_smallops.py; soundness and tightness: tests/test_smallops_host.py).  mean4,
# add_cast, patchify, token_embed and attn_mask_from_logits have no bound: their fp32 expressions are fixed by the header and the results are compared exactly.
def l2norm_nred(D):
    """fp32 additions on the longest path of l2norm_rows' sum of squares: lane l of 64 adds columns l, l + 64, ... (ceil(D / 64) additions), then the six
    levels of the wave's butterfly"""
    return -(-D // 64) + 6


def l2norm_bound(ref, D, out_fmt):
    """y = x * (1 / (sqrtf(S) + eps)) against ref = x / (||x|| + eps) (float64 of the same fp32 row), S the fp32 sum of the D squares.

    S: every square is rounded once (none when the compiler contracts it into an fma) and every one of the nred = l2norm_nred(D) additions on the longest path
    rounds a partial sum of non-negative terms that is <= S: (nred + 1) u32 relative.  sqrtf halves that and rounds once (IEEE sqrt, see the note on division
    and sqrtf above).  Adding eps >= 0 rounds once and only dilutes the error of the root (n / (n + eps) <= 1); the reciprocal rounds once; the product rounds
    once.  So c = the root, the add of eps, the reciprocal and the product = 4 roundings behind half of (nred + 1):
        |y - ref| <= ((nred + 1) / 2 + 4) u32 |ref|,
    every rounding allowed twice (R) like everywhere here: (nred + 9) u32 |ref| = |ref| (nred + c') 2^-24 with c' = 2 x 4 + 1, then the output rounding
    R u(out) |ref| + tiny(out).  Assumes the squares stay in fp32's normal range (|x| > 2^-63 where it matters, ||x||^2 < 2^128)."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    err = R * U32 * ((l2norm_nred(D) + 1) / 2.0 + 4.0) * ref.abs()
    return err + R * u(out_fmt) * (ref.abs() + err) + tiny(out_fmt)


def resize_bound(ref, tapmax, out_fmt, dtaps=0.0, dcoord=0.0):
    """o = (1 - wy) ((1 - wx) a + wx b) + wy ((1 - wx) d + wx e) in fp32 (misc.hip resize_bilinear_kernel, and dino_pre_kernel with the factors the other way
    round) against the float64 blend of the same taps with the same fp32 source coordinate.  tapmax = max(|a|, |b|, |d|, |e|).  blend_bound does not fit: it
    is relative to the result, which only holds for non-negative taps; features are signed, and the result can cancel.

    wx = fx - floor(fx) is exact; 1 - wx rounds once.  Inner blend: the rounding of 1 - wx and of its product with a (2 (1 - wx) |a|), the product with b
    (wx |b|) and the sum (|top|): at most u32 tapmax (2 (1 - wx) + wx + 1) <= 3 u32 tapmax.  The outer blend does the same to two values <= tapmax and passes
    the inner errors on with weights that sum to one: 3 more.  6 u32 tapmax, every rounding allowed twice (R); an fma only removes roundings.
    dtaps:  the error the taps carry themselves (dino_preprocess normalises them in fp32 first: dino_tap_err); the blend is convex, so it passes on unchanged.
    dcoord: the |change of o| when the compiler contracts (d + 0.5) s - 0.5 into one fma, so that the kernel's coordinate is not the twice-rounded one of the
            reference (resize_coord_term; 0 where contraction is switched off: dino_pre_kernel).
    Then the rounding to the output format."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    err = 6 * R * U32 * torch.as_tensor(tapmax, dtype=torch.float64) + R * torch.as_tensor(dtaps, dtype=torch.float64) + torch.as_tensor(dcoord, dtype=torch.float64)
    return err + R * u(out_fmt) * (ref.abs() + err) + tiny(out_fmt)


def resize_coord_term(fy, fx, gy, gx):
    """resize_bound's dcoord.  fl(fl((d + 0.5) s) - 0.5) and the single rounding of an fma differ by at most the rounding of the product, u32 (f + 0.5), and
    the two roundings of the differences, 2 u32 f - together <= 3 u32 (f + 0.5) per axis.  The bilinear interpolant is continuous and piecewise linear; along
    an axis its slope is a convex combination of differences of neighbouring source pixels, at most g = the largest such difference of the image and channel
    (of the whole plane: a coordinate next to an integer may fall into the neighbouring cell, whose taps are not the reference's four).  So o moves by at most
    3 u32 ((fy + 0.5) gy + (fx + 0.5) gx).  A worst case in its own right (the roundings are bounded by their full size): not doubled again."""
    as64 = lambda t: torch.as_tensor(t, dtype=torch.float64)
    return 3 * U32 * ((as64(fy) + 0.5) * as64(gy) + (as64(fx) + 0.5) * as64(gx))


def dino_tap_err(t, nv, std):
    """resize_bound's dtaps for dino_preprocess: nv = ((v 0.5 + 0.5) - mean) / std in fp32, mean and std the fp32 constants.  v 0.5 is exact; t = v 0.5 + 0.5
    rounds once (u32 |t|), t - mean rounds once (u32 |t - mean|) and the division once (u32 |nv|), the first two divided by std:
    u32 (|t| / std + 2 |nv|) - three roundings per tap."""
    t, nv = torch.as_tensor(t, dtype=torch.float64), torch.as_tensor(nv, dtype=torch.float64)
    return U32 * (t.abs() / torch.as_tensor(std, dtype=torch.float64) + 2 * nv.abs())


# ------------------------------------------------------------------------------------------------------------------------------------------- image input
# image.hip's image_prepare (tests/test_hip_input.py; soundness and tightness: tests/test_input_host.py).  patch_rows has no bound of its own: its encoder
# half is exact and its DINOv2 half is dino_preprocess's expression, held under resize_bound with dino_tap_err.
def aa_axis(n_in, n_out, lo, n):
    """The per-axis terms of aa_resize_bound for the outputs lo .. lo + n - 1 of an antialiased resize of n_in source pixels to n_out.

    Exact rule (float64): raw weight t_j = tri((j + 0.5 - c) / s), c = (i + 0.5) n_in / n_out, s = max(n_in / n_out, 1), w_j = t_j / T, T = sum_j t_j.
    The kernel (aa_window): scale' = fl(n_in / n_out), c' = fl(scale' (i + 0.5)) (no fma can form: the sum is inside the product), inv' = fl(1 / scale') or 1,
    window [max((int)(c' - s' + 0.5f), 0), min((int)(c' + s' + 0.5f), n_in)).  These are evaluated HERE in numpy fp32, operation by operation: they are the
    rule's definition in fp32, not an observation of the kernel, and they make the coordinate term exactly zero where scale', c' and inv' are exact.

    Arithmetic, relative to the window (`arith`, in units of u32 |pixel|max).  x'_j = ((float)j - c' + 0.5f) inv' rounds three times: the two sums are each
    relative to at most |j - c'| <= s |x_j| + 0.5, the product to |x_j|; 1 - |x| rounds once (t_j): a_j = (3 |x_j| + t_j + inv' / 2) u32 per raw weight
    (tri is 1-Lipschitz, so the error of x' is the error of t' also where one of the two is clipped to 0).  The sum T' of the nk window taps: sum_j a_j and
    nk - 1 additions of partial sums <= T.  w'_j = fl(t'_j / T'): a_j / T + w_j ((sum a + (nk - 1) u32 T) / T + u32).  Summed over the window:
        sum_j |w'_j - w_j| <= (2 sum_j a_j / T + nk) u32                                                    [weights]
    and the convex sum over the nk taps itself, product and addition rounded separately (an fma only removes the first): (nk + 1) u32  [accumulation].
    Coordinate (`coord`, in units of the half-range of the pixels under the window: both weight sets sum to 1, so only differences of pixels pass).  With
    dc = |c' - c| and dinv = |inv' - 1 / s|, t_j moves by dt_j <= dc inv' + |j + 0.5 - c| dinv (tri is 1-Lipschitz).  A tap with t_j > 0 that the fp32 window
    leaves out moves by its whole weight, dt_j = t_j (at most the window edge's own error over the support); a tap the window adds beyond the support has
    t_j = 0 and is one of the nk taps above.  |w'_j - w_j| <= dt_j / T~ + t_j |1 / T~ - 1 / T| with T~ >= T - sum dt:
        sum_j |w'_j - w_j| <= 2 sum_j dt_j / (T - sum_j dt_j).
    A worst case in its own right (nothing here is a rounding of unknown sign and size): not doubled.
    -> dict of float64 [n]: arith, coord; int64 [n]: nk (fp32 window's taps), wlo, whi (the union of the fp32 window and the exact support, [wlo, whi))."""
    import numpy as np
    f32 = np.float32
    i = np.arange(lo, lo + n)
    j = np.arange(n_in)
    scale = n_in / n_out
    s = max(scale, 1.0)
    c = (i + 0.5) * scale
    x = (j[None, :] + 0.5 - c[:, None]) / s
    t = np.clip(1.0 - np.abs(x), 0.0, None)
    T = t.sum(1)
    sk = f32(n_in) / f32(n_out)
    ck = (sk * (i.astype(f32) + f32(0.5))).astype(f32)
    supk = sk if sk >= 1 else f32(1.0)
    invk = f32(1.0) / sk if sk >= 1 else f32(1.0)
    klo = np.maximum((ck - supk + f32(0.5)).astype(f32).astype(np.int64), 0)
    khi = np.minimum((ck + supk + f32(0.5)).astype(f32).astype(np.int64), n_in)
    inwin = (j[None, :] >= klo[:, None]) & (j[None, :] < khi[:, None])
    nk = inwin.sum(1)
    a = (3.0 * np.abs(x) + t + 0.5 * float(invk)) * inwin
    arith = 2.0 * a.sum(1) / T + nk + (nk + 1)
    dc = np.abs(ck.astype(np.float64) - c)
    dinv = abs(float(invk) - 1.0 / s)
    dt = np.where(inwin, dc[:, None] * float(invk) + np.abs(j[None, :] + 0.5 - c[:, None]) * dinv, t)
    dt = np.where(inwin | (t > 0), dt, 0.0)
    sdt = dt.sum(1)
    coord = 2.0 * sdt / np.clip(T - sdt, 1e-300, None)
    has = inwin | (t > 0)
    wlo = np.where(has.any(1), has.argmax(1), 0)
    whi = np.where(has.any(1), n_in - has[:, ::-1].argmax(1), 1)
    as64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    return dict(arith=as64(arith), coord=as64(coord), nk=torch.from_numpy(nk), wlo=torch.from_numpy(wlo), whi=torch.from_numpy(whi))


def aa_resize_bound(p, n_out, crop):
    """Per-element bound of image_prepare against input_ref.aa_resize.  p = the ImgNorm pixels in float64 [3, Hs, Ws]; n_out = (Hr, Wr);
    crop = (top, left, H, W).  -> float64 [3, H, W].

    Pixel normalisation: t = fl(v / 255) (IEEE division), fl(t - 0.5), and / 0.5 is exact: 2 u32 (t + |t - 0.5|) = u32 (1 + p + |p|) <= u32 (1 + 2 |p|) per
    pixel; the two nested sums are convex and pass it on unchanged.
    Arithmetic and coordinate: aa_axis per axis.  The inner sum (x) errs by arith_x u32 pmax, the outer (y) by arith_y u32 pmax and passes the inner sum's
    error on unchanged (convex); pmax = the largest |pixel| under the window - not the result, which cancels.  The coordinate terms add likewise, times the
    half-range of the pixels under the window: (coord_y + coord_x) (max - min) / 2, zero on a constant image and wherever the fp32 scale and centres are exact.
        bound = R u32 (pmax (arith_y + arith_x) + 1 + 2 pmax) + (coord_y + coord_x) halfrange + TINY32,
    every rounding allowed twice (R) as everywhere here."""
    p = p.double()
    top, left, H, W = crop
    ay, ax = aa_axis(p.shape[1], n_out[0], top, H), aa_axis(p.shape[2], n_out[1], left, W)
    hi = torch.stack([p[:, int(a):int(b)].amax(1) for a, b in zip(ay['wlo'], ay['whi'])], 1)                 # [3, H, Ws]
    lo = torch.stack([p[:, int(a):int(b)].amin(1) for a, b in zip(ay['wlo'], ay['whi'])], 1)
    hi = torch.stack([hi[:, :, int(a):int(b)].amax(2) for a, b in zip(ax['wlo'], ax['whi'])], 2)             # [3, H, W]
    lo = torch.stack([lo[:, :, int(a):int(b)].amin(2) for a, b in zip(ax['wlo'], ax['whi'])], 2)
    pmax = torch.maximum(hi.abs(), lo.abs())
    arith = ay['arith'][None, :, None] + ax['arith'][None, None, :]
    coord = ay['coord'][None, :, None] + ax['coord'][None, None, :]
    return R * U32 * (pmax * arith + 1.0 + 2.0 * pmax) + coord * (hi - lo) / 2.0 + TINY32
