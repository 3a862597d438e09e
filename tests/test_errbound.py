"""The per-element bounds of tests/errbound.py are SOUND and TIGHT (CPU only, no GPU).

Sound: a CPU emulation of the kernel's stated rounding path stays at or below half of each bound.  Tight: the typical kernel mistakes - an fp32 result whose
accumulator passed through a 16-bit format, one negated 16 x 16 output fragment, the bias added after the output rounding, an fp32 residual read as 16 bit,
P rounded to the wrong format, a dropped key (last tile / split boundary / last query row), a wrong LayerNorm eps, the variance over D - 1 - each exceed
the bound (ratio > 1) AND land at least 4x above the emulation on the same inputs.  Inputs are the ones the GPU tests use (same seeds and shapes), cut down
in heads where float64 time on the CPU would be long.
"""
import numpy as np
import pytest
import torch

import errbound as EB

FMTS = {'bf16': torch.bfloat16, 'f16': torch.float16}


def rn(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def ratio(got, ref, bound):
    return float(((got.double() - ref.double()).abs() / bound).max())


# ------------------------------------------------------------------------------------------------------------------------------------------- GEMM
def emu_acc(a, w):
    """fp32 accumulation of exact 16-bit products, one MFMA step (32 products) at a time"""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 32):
        acc = acc + (a[:, k0:k0 + 32].double() @ w[:, k0:k0 + 32].double().T).float()
    return acc


def gemm_case(M, N, K, fmt, seeds=(1, 2, 3)):
    d = FMTS[fmt]
    a, w, b = rn(seeds[0], M, K).to(d), rn(seeds[1], N, K, scale=K ** -0.5).to(d), rn(seeds[2], N, scale=0.1)
    ref = a.double() @ w.double().T + b.double()
    return a, w, b, ref, emu_acc(a, w)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
def test_gemm_bound_fp32_output_rejects_a_16bit_accumulator(fmt):
    """test_gemm_basic's 768 x 1024 x 1024 with fp32 output: emulation <= 0.5; accumulator via bf16 / via f16 > 1 and >= 4x the emulation"""
    a, w, b, ref, acc = gemm_case(768, 1024, 1024, fmt)
    bound = EB.gemm_bound(a, w, torch.float32, bias=b)
    r_ok = ratio(acc + b, ref, bound)
    assert r_ok <= 0.5, r_ok
    for via in (torch.bfloat16, torch.float16):
        r_bad = ratio((acc + b).to(via).float(), ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (via, r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('act', [None, 'gelu', 'relu'])
def test_gemm_bound_16bit_output(fmt, act):
    """16-bit output, the tail shapes of test_gemm_basic: emulation <= 0.5; one negated 16 x 16 fragment and the bias added after the output rounding fail"""
    import torch.nn.functional as F
    d = FMTS[fmt]
    for (M, N, K) in [(4096, 512, 256), (257, 260, 64), (129, 4, 128)]:
        a, w, b, ref, acc = gemm_case(M, N, K, fmt)
        f = {'gelu': F.gelu, 'relu': F.relu, None: lambda x: x}[act]
        ref = f(ref)
        bound = EB.gemm_bound(a, w, d, bias=b, act=act)
        emu = f(acc + b).to(d)
        r_ok = ratio(emu, ref, bound)
        assert r_ok <= 0.5, (M, N, K, r_ok)
        neg = emu.clone()
        if N >= 16:
            neg[16:32, 16:32] *= -1
        else:
            neg[M - 16:M, :] *= -1                              # N = 4: the fragment is the last 16 rows of the only column block
        r_neg = ratio(neg, ref, bound)
        assert r_neg > 1 and r_neg >= 4 * r_ok, ('negated fragment', M, N, K, r_neg, r_ok)
        if act is None:
            late = (acc.to(d).float() + b).to(d)                # bias added after the output rounding: two roundings
            r_late = ratio(late, ref, bound)
            assert r_late > 1 and r_late >= 4 * r_ok, ('bias after rounding', M, N, K, r_late, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
def test_gemm_bound_residual(fmt):
    """test_gemm_residual_gamma_remap (fp32 residual, fp32 output) and test_gemm_bf16_residual (16-bit residual, both outputs): emulations <= 0.5; an fp32
    residual read as 16 bit fails"""
    d = FMTS[fmt]
    M, N, K = 2 * 96, 64, 128
    a, w = rn(4, M, K).to(d), rn(5, N, K, scale=K ** -0.5).to(d)
    bias, gamma, pe = rn(6, N), rn(7, N), rn(9, 96, N).repeat(2, 1)
    acc = emu_acc(a, w)
    ref = (a.double() @ w.double().T + bias.double()) * gamma.double() + pe.double()
    bound = EB.gemm_bound(a, w, torch.float32, bias=bias, gamma=gamma, res=pe)
    r_ok = ratio((acc + bias) * gamma + pe, ref, bound)
    assert r_ok <= 0.5, r_ok
    r_bad = ratio((acc + bias) * gamma + pe.to(d).float(), ref, bound)
    assert r_bad > 1 and r_bad >= 4 * r_ok, (r_bad, r_ok)
    for (M, N, K) in [(300, 384, 384), (200, 104, 64)]:
        a, w, b = rn(100, M, K).to(d), rn(101, N, K, scale=K ** -0.5).to(d), rn(102, N)
        x = rn(103, M, N).to(d)
        acc = emu_acc(a, w)
        ref = a.double() @ w.double().T + b.double() + x.double()
        b16 = EB.gemm_bound(a, w, d, bias=b, res=x)
        assert ratio(((acc + b).to(d).float() + x.float()).to(d), ref, b16) <= 0.5
        b32 = EB.gemm_bound(a, w, torch.float32, bias=b, res=x)
        r_ok = ratio(acc + b + x.float(), ref, b32)
        assert r_ok <= 0.5
        r_bad = ratio((acc + b).to(d).float() + x.float(), ref, b32)           # fp32 output through a 16-bit intermediate
        assert r_bad > 1 and r_bad >= 4 * r_ok, (r_bad, r_ok)


# ------------------------------------------------------------------------------------------------------------------------------------------- attention
def emu_attn(q, k, v, fmt_p, fmt_out, mask=None, pre=False, drop=None, head_room=7.9):
    """attention.hip's rounding path: fp32 scores, P = exp2((s - m) c) with P_max = 2^head_room (lazy rescaling lets it reach 2^8) rounded to fmt_p, l the
    fp32 sum of the SAME rounded P, fp32 P V, one rounding to fmt_out.  drop: (row, key) pairs whose P is zeroed (a dropped key)."""
    hd = q.shape[-1]
    c = 1.0 if pre else hd ** -0.5 * EB.LOG2E
    s = (q.float() @ k.float().transpose(-1, -2))
    if mask is not None:
        s = s.masked_fill(mask[:, None], float('-inf'))
    m = s.amax(-1, keepdim=True) - head_room / c
    P = torch.exp2((s - m) * c).to(fmt_p).float()
    if drop is not None:
        for (row, key) in drop:
            P[..., row, key] = 0.0
    l = P.sum(-1, keepdim=True)
    return ((P @ v.float()) / l).to(fmt_out)


def attn_case(H, Nq, Nk, hd, fmt, seeds, plant=()):
    """q, k, v as test_attention builds them (unit-variance, 16-bit); plant: (row, key) pairs whose logit is made large (the key dominates the row)"""
    d = FMTS[fmt]
    q, k, v = rn(seeds[0], 1, H, Nq, hd), rn(seeds[1], 1, H, Nk, hd), rn(seeds[2], 1, H, Nk, hd).to(d)
    for (row, key) in plant:
        k[0, :, key] = q[0, :, row] * 1.5
    return q.to(d), k.to(d), v


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
def test_attention_bound_rejects_p_in_the_wrong_format(fmt):
    """12 x 768 x 6144 (test_attention_split_k's shape; 2 heads): emulation <= 0.5; P rounded to the other 16-bit format fails in f16 (bf16 P in an f16
    kernel).  bf16 -> f16 P is MORE precise, so it is no mistake for the bf16 kernel; there only the emulation is checked."""
    d = FMTS[fmt]
    q, k, v = attn_case(2, 768, 6144, 64, fmt, (23, 24, 25))
    ref = EB.attn_ref(q, k, v)
    bound = EB.attn_bound(q, k, v, None, False, d, d)
    r_ok = ratio(emu_attn(q, k, v, d, d), ref, bound)
    assert r_ok <= 0.5, r_ok
    if fmt == 'f16':
        r_bad = ratio(emu_attn(q, k, v, torch.bfloat16, d), ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (r_bad, r_ok)


# a dropped unweighted key of Nk moves an output by ~|v - O| / Nk: below bf16's resolution once Nk is large.  These (format, Nk) are exempt from the
# unweighted check; the planted-logit rows (test_attention_bound_rejects_a_dropped_planted_key and the GPU tests' planted shapes) catch the mistake there.
# Computed sizes (max |err| / (u(bf16) |O|) over the last row): 769 keys 0.45, 3000 keys 0.12, 6144 keys 0.06 - all below one output rounding.
EXEMPT_UNWEIGHTED_DROP = {('bf16', 769), ('bf16', 3000), ('bf16', 6144)}


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('Nk', [769, 3000, 6144])
def test_attention_bound_rejects_a_dropped_last_key(fmt, Nk):
    """the last query row loses the last key (one key in the last tile), unit-variance q / k as the GPU tests use"""
    d = FMTS[fmt]
    Nq = 70
    q, k, v = attn_case(1, Nq, Nk, 64, fmt, (20, 21, 22))
    ref = EB.attn_ref(q, k, v)
    bound = EB.attn_bound(q, k, v, None, False, d, d)
    r_ok = ratio(emu_attn(q, k, v, d, d), ref, bound)
    assert r_ok <= 0.5, r_ok
    r_bad = ratio(emu_attn(q, k, v, d, d, drop=[(Nq - 1, Nk - 1)]), ref, bound)
    if (fmt, Nk) in EXEMPT_UNWEIGHTED_DROP:
        assert r_bad < 4 * r_ok + 1                 # (documents the exemption: below resolution)
    else:
        assert r_bad > 1 and r_bad >= 4 * r_ok, (r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('Nk,ns', [(6144, 4), (1025, 8), (513, 8)])
def test_attention_bound_rejects_a_dropped_planted_key(fmt, Nk, ns):
    """the planted-logit rows of the GPU tests: the last key of the last tile and the first / last key of every split carry a large logit in some rows; dropping
    (or double counting) any of them moves those rows by O(|v|) - in both formats, at every Nk"""
    d = FMTS[fmt]
    Nq = 80
    tiles = (Nk + 63) // 64
    tps = (tiles + ns - 1) // ns
    keys = sorted({Nk - 1} | {min(s * tps * 64, Nk - 1) for s in range(ns)} | {min((s + 1) * tps * 64, Nk) - 1 for s in range(ns)})
    plant = [(2 * i + 3, key) for i, key in enumerate(keys)]
    q, k, v = attn_case(1, Nq, Nk, 64, fmt, (40, 41, 42), plant)
    ref = EB.attn_ref(q, k, v)
    bound = EB.attn_bound(q, k, v, None, False, d, d, nsplit=ns)
    r_ok = ratio(emu_attn(q, k, v, d, d), ref, bound)
    assert r_ok <= 0.5, r_ok
    for (row, key) in plant:
        r_bad = ratio(emu_attn(q, k, v, d, d, drop=[(row, key)]), ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (row, key, r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
def test_attention_bound_rejects_a_key_dropped_at_a_split_boundary(fmt):
    """Nk = 6144, 4 splits: one key at the boundary dropped from every row (a split walking one key short) - caught in both formats"""
    d = FMTS[fmt]
    q, k, v = attn_case(1, 200, 6144, 64, fmt, (23, 24, 25))
    ref = EB.attn_ref(q, k, v)
    bound = EB.attn_bound(q, k, v, None, False, d, d, nsplit=4)
    r_ok = ratio(emu_attn(q, k, v, d, d), ref, bound)
    assert r_ok <= 0.5, r_ok
    r_bad = ratio(emu_attn(q, k, v, d, d, drop=[(r, 1536) for r in range(200)]), ref, bound)
    assert r_bad > 1 and r_bad >= 4 * r_ok, (r_bad, r_ok)          # every one of the 200 rows loses the key: some row moves past the bound in bf16 too


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
def test_attention_bound_masked_and_prescaled(fmt):
    """masks (incl. a row whose only open key is the last one) and the prescaled mode: emulation <= 0.5"""
    d = FMTS[fmt]
    hd = 96
    q, k, v = attn_case(2, 65, 577, hd, fmt, (20, 21, 22))
    q = (q.float() * (hd ** -0.5 * EB.LOG2E)).to(d)
    g = np.random.Generator(np.random.PCG64(5))
    mask = torch.from_numpy(g.uniform(size=(1, 65, 577)) < 0.6)
    mask[:, :, 0] = False
    mask[:, 1, :576] = True
    mask[:, 1, 576] = False
    ref = EB.attn_ref(q, k, v, mask, pre=True)
    bound = EB.attn_bound(q, k, v, mask, True, d, d)
    assert ratio(emu_attn(q, k, v, d, d, mask, pre=True), ref, bound) <= 0.5


# ------------------------------------------------------------------------------------------------------------------------------------------- LayerNorm
def emu_ln(x, g, b, eps, out, ddof=0):
    x = x.float()
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    xc = x - mean
    var = (xc * xc).sum(-1, keepdim=True) / (x.shape[-1] - ddof)
    return (xc * torch.rsqrt(var + eps) * g + b).to(out)


def ln_rows(D, seed=40):
    """test_layernorm's rows: 74 rows x * 3 + 1, plus the quiet rows (std 0.01 around 1) where eps matters"""
    x = rn(seed, 2 * 37, D) * 3 + 1
    x[::9] = rn(seed + 7, x[::9].shape[0], D) * 0.01 + 1
    return x


@pytest.mark.parametrize('D,eps', [(1024, 1e-6), (384, 1e-5), (48, 1e-5), (2816, 1e-5)])
def test_layernorm_bound(D, eps):
    """every output format: emulation <= 0.5; wrong eps (1e-5 <-> 1e-6, visible on the quiet rows) and the variance over D - 1 fail"""
    x, g, b = ln_rows(D), 1 + 0.1 * rn(41, D), 0.1 * rn(42, D)
    other = 1e-6 if eps == 1e-5 else 1e-5
    for out in (torch.float32, torch.bfloat16, torch.float16):
        xin = x if out == torch.float32 else x.to(out).float()
        ref = EB.layernorm_ref(xin, g, b, eps)
        bound = EB.rownorm_bound(xin, g, b, eps, out)
        r_ok = ratio(emu_ln(xin, g, b, eps, out), ref, bound)
        assert r_ok <= 0.5, (out, r_ok)
        r_eps = ratio(emu_ln(xin, g, b, other, out), ref, bound)
        assert r_eps > 1 and r_eps >= 4 * r_ok, ('eps', out, r_eps, r_ok)
        r_ddof = ratio(emu_ln(xin, g, b, eps, out, ddof=1), ref, bound)
        assert r_ddof > 1 and r_ddof >= 4 * r_ok, ('D-1', out, r_ddof, r_ok)


# ------------------------------------------------------------------------------------------------------------------------------------------- fp32 modes
def split16(x):
    """x = hi + lo, both f16 (split.hip / pack_split3)"""
    hi = x.half()
    return hi, (x - hi.float()).half()


def emu_acc_fp32(a, w):
    """v_mfma_f32_16x16x4_f32: fp32 products, four per step into the fp32 accumulator"""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 4):
        acc = acc + a[:, k0:k0 + 4].float() @ w[:, k0:k0 + 4].float().T
    return acc


def emu_acc_x3(a, w):
    """three f16 MFMAs on split operands: [hi, hi, lo] x [hi, lo, hi] over 3K, the lo x lo term dropped"""
    ah, al = split16(a)
    wh, wl = split16(w)
    return emu_acc(torch.cat([ah, ah, al], 1), torch.cat([wh, wl, wh], 1))


@pytest.mark.parametrize('act', [None, 'gelu'])
@pytest.mark.parametrize('M,N,K', [(200, 256, 384), (130, 68, 208)])
def test_gemm_bound_fp32_operand_modes(M, N, K, act):
    """test_gemm_f32's inputs: the x3 and fp32-input emulations <= 0.5 of their bounds; the same GEMM on f16 or bf16 operands, or with the lo parts dropped
    (plain f16), fails both"""
    import torch.nn.functional as F
    a, w, b = rn(1, M, K), rn(2, N, K, scale=K ** -0.5), rn(3, N, scale=0.1)
    f = F.gelu if act else (lambda t: t)
    ref = f(a.double() @ w.double().T + b.double())
    mutants = {'f16 operands': emu_acc(a.half(), w.half()), 'bf16 operands': emu_acc(a.bfloat16(), w.bfloat16()),
               'x3 without lo': emu_acc(split16(a)[0], split16(w)[0])}
    for mode, acc in (('x3', emu_acc_x3(a, w)), ('fp32', emu_acc_fp32(a, w))):
        bound = EB.gemm_bound(a, w, torch.float32, bias=b, act=act, mode=mode)
        r_ok = ratio(f(acc + b), ref, bound)
        assert r_ok <= 0.5, (mode, r_ok)
        for name, bad in mutants.items():
            r_bad = ratio(f(bad + b), ref, bound)
            assert r_bad > 1 and r_bad >= 4 * r_ok, (mode, name, r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16', 'fp32'])
@pytest.mark.parametrize('Cin,Cout,H,W', [(64, 128, 12, 20), (128, 64, 9, 7)])
def test_conv3x3_bound(fmt, Cin, Cout, H, W):
    """test_gemm_implicit_conv3x3's inputs (fp32 output; fp32 operands in the fp32 mode's twin): im2col emulation <= 0.5; one missing tap and the
    accumulator through a 16-bit format fail"""
    import torch.nn.functional as F
    V = 2
    x, wt, b = rn(16, V, H, W, Cin), rn(17, Cout, Cin, 3, 3, scale=(9 * Cin) ** -0.5), rn(18, Cout)
    if fmt != 'fp32':
        x, wt = x.to(FMTS[fmt]), wt.to(FMTS[fmt])
    cols = F.unfold(x.float().permute(0, 3, 1, 2), 3, padding=1).permute(0, 2, 1).reshape(V * H * W, 9 * Cin)
    wmat = wt.float().reshape(Cout, 9 * Cin)
    mode = 'x3' if fmt == 'fp32' else 'mfma16'
    ref, bound = EB.conv3x3(x, wt, b, torch.float32, mode)
    acc = emu_acc_x3(cols, wmat) if fmt == 'fp32' else emu_acc(cols.to(x.dtype), wmat.to(x.dtype))
    r_ok = ratio(acc + b, ref, bound)
    assert r_ok <= 0.5, r_ok
    w_miss = wt.float().clone()
    w_miss[:, :, 0, 0] = 0
    miss = emu_acc(cols.to(torch.float16), w_miss.reshape(Cout, 9 * Cin).to(torch.float16)) if fmt == 'fp32' else emu_acc(cols.to(x.dtype), w_miss.reshape(Cout, 9 * Cin).to(x.dtype))
    for name, bad in (('missing tap', miss + b), ('acc via f16', (acc + b).half().float())):
        r_bad = ratio(bad, ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (name, r_bad, r_ok)


def emu_attn_fp32(q, k, v, split=False, p_fmt=None):
    """attn_f32.hip (split=False): fp32 scores, P, l and P V; attn_x3.hip (split=True): q, k, P, v as f16 hi + lo pairs, three MFMAs each, lo x lo dropped.
    p_fmt: a mutant that rounds P to a 16-bit format"""
    hd = q.shape[-1]
    c = hd ** -0.5 * EB.LOG2E
    if split:
        (qh, ql), (kh, kl) = split16(q), split16(k)
        s = qh.float() @ kh.float().transpose(-1, -2) + qh.float() @ kl.float().transpose(-1, -2) + ql.float() @ kh.float().transpose(-1, -2)
    else:
        s = q.float() @ k.float().transpose(-1, -2)
    P = torch.exp2((s - s.amax(-1, keepdim=True)) * c)
    if p_fmt is not None:
        P = P.to(p_fmt).float()
    l = P.sum(-1, keepdim=True)
    if split:
        (Ph, Pl), (vh, vl) = split16(P), split16(v)
        o = Ph.float() @ vh.float() + Ph.float() @ vl.float() + Pl.float() @ vh.float()
    else:
        o = P @ v.float()
    return o / l


@pytest.mark.parametrize('mode', ['x3', 'fp32'])
def test_attention_bound_fp32_operand_modes(mode):
    """test_attention_f32's (2, 3, 200, 333, 64) inputs: emulation <= 0.5; f16 / bf16 operands, or P rounded to f16 (the x3 kernel without P's lo part), fail"""
    q, k, v = rn(20, 2, 3, 200, 64), rn(21, 2, 3, 333, 64), rn(22, 2, 3, 333, 64)
    ref = EB.attn_ref(q, k, v)
    bound = EB.attn_bound(q, k, v, None, False, torch.float32, torch.float32, mode=mode)
    r_ok = ratio(emu_attn_fp32(q, k, v, split=mode == 'x3'), ref, bound)
    assert r_ok <= 0.5, r_ok
    mutants = {'f16 operands': emu_attn(q.half(), k.half(), v.half(), torch.float32, torch.float32, head_room=0),
               'bf16 operands': emu_attn(q.bfloat16(), k.bfloat16(), v.bfloat16(), torch.float32, torch.float32, head_room=0),
               'P in f16': emu_attn_fp32(q, k, v, split=mode == 'x3', p_fmt=torch.float16)}
    for name, bad in mutants.items():
        r_bad = ratio(bad, ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (name, r_bad, r_ok)


# ------------------------------------------------------------------------------------------------------------------------------------------- GroupNorm, RoPE
def gn_input(C, P, n, fmt):
    """test_groupnorm_apply_streaming_16bit's rows: x * 1.7 + 0.4, and a quiet view (zero mean, std 0.003) where eps matters"""
    x = rn(990, n * P, C) * 1.7 + 0.4
    x[P:2 * P] = rn(994, P, C) * 0.003
    return x.to(FMTS[fmt])


def emu_gn(x, n, P, G, g, b, eps, out, relu, ddof=0, shift_gamma=False):
    """one-pass fp32 statistics per (view, group), (x - mean) rstd gamma + beta in fp32, one rounding"""
    C = x.shape[-1]
    xg = x.float().reshape(n, P, G, C // G)
    cnt = P * (C // G)
    s1 = xg.sum((1, 3), keepdim=True)
    s2 = (xg * xg).sum((1, 3), keepdim=True)
    mean = s1 / cnt
    var = (s2 / cnt - mean * mean) * cnt / (cnt - ddof)
    gg = (g.roll(1) if shift_gamma else g).reshape(1, 1, G, C // G)
    y = ((xg - mean) * torch.rsqrt(var + eps) * gg + b.reshape(1, 1, G, C // G)).reshape(n * P, C)
    return (torch.relu(y) if relu else y).to(out)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('C,G,P,relu', [(384, 8, 700, True), (64, 8, 96, False), (384, 8, 33, True)])
def test_groupnorm_bound(fmt, C, G, P, relu):
    """emulation <= 0.5; wrong eps (on the quiet view), gamma of the neighbouring channel and E[x^2] without the mean^2 fail"""
    d = FMTS[fmt]
    n = 3
    x = gn_input(C, P, n, fmt)
    g, b = 1 + 0.1 * rn(991, C), 0.1 * rn(992, C)
    ref, bound = EB.groupnorm(x, n, P, G, g, b, 1e-5, d, relu)
    r_ok = ratio(emu_gn(x, n, P, G, g, b, 1e-5, d, relu), ref, bound)
    assert r_ok <= 0.5, r_ok
    mutants = {'eps': emu_gn(x, n, P, G, g, b, 1e-6, d, relu), 'gamma shifted': emu_gn(x, n, P, G, g, b, 1e-5, d, relu, shift_gamma=True),
               'no mean^2': emu_gn(x, n, P, G, g, b, 1e-5 - 1, d, relu)}
    mutants['no mean^2'] = None
    xs = x.float().reshape(n, P, G, C // G)
    m2 = xs.mean((1, 3), keepdim=True) ** 2
    var_bad = (xs * xs).mean((1, 3), keepdim=True)                            # E[x^2]: the mean^2 term forgotten
    y = ((xs - xs.mean((1, 3), keepdim=True)) * torch.rsqrt(var_bad + 1e-5) * g.reshape(1, 1, G, -1) + b.reshape(1, 1, G, -1)).reshape(n * P, C)
    mutants['no mean^2'] = (torch.relu(y) if relu else y).to(d)
    assert float(m2.max()) > 0.1
    for name, bad in mutants.items():
        r_bad = ratio(bad, ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (name, r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16', 'fp32'])
@pytest.mark.parametrize('hd,H', [(64, 16), (96, 4), (16, 2)])
def test_rope_bound(fmt, hd, H):
    """test_rope2d's inputs (5 x 7 grid): the fp32-table emulation <= 0.5; a position off by one, base 10000 instead of 100 and cos / sin swapped fail"""
    from panst3r_amd import hip
    d = FMTS.get(fmt, torch.float32)
    gh, gw = 5, 7
    ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing='ij')
    pos = torch.stack([ys, xs], -1).reshape(gh * gw, 2)
    x = rn(50, gh * gw, H, hd).to(d).permute(1, 0, 2)                         # [H, T, hd]
    ref, bound = EB.rope2d(x, pos, d)

    def emu(p=pos, base=100.0, swap=False):
        tab = hip.rope_table(max(gh, gw) + 1, hd, base, 'cpu')               # [npos, hd / 4, 2] fp32 (cos, sin)
        D = hd // 2
        outs = []
        for half in range(2):
            t = x[..., half * D:(half + 1) * D].float()
            cs = tab[p[:, half]]
            c, s_ = torch.cat([cs[..., 0]] * 2, -1), torch.cat([cs[..., 1]] * 2, -1)
            if swap:
                c, s_ = s_, c
            partner = torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1)
            outs.append(t * c + partner * s_)
        return torch.cat(outs, -1).to(d)
    r_ok = ratio(emu(), ref, bound)
    assert r_ok <= 0.5, r_ok
    for name, bad in (('pos + 1', emu(p=pos + torch.tensor([1, 0]))), ('base', emu(base=10000.0)), ('cos/sin swapped', emu(swap=True))):
        r_bad = ratio(bad, ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (name, r_bad, r_ok)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('M,N,D', [(300, 256, 128), (200, 192, 192)])
def test_ln_fold_bound(fmt, M, N, D):
    """test_gemm_layernorm_fold_consumer's inputs (fp32 output): emulation of the fold (one-pass fp32 statistics, 16-bit xc x gamma-folded W, fmaf epilogue)
    <= 0.5; the mean correction dropped, the variance over D - 1 and the result through the 16-bit format fail"""
    d = FMTS[fmt]
    x = rn(800, M, D) * 1.7 + 0.4
    x[:, 5] += 6.0
    gamma, beta = 1 + 0.2 * rn(801, D), 0.1 * rn(802, D)
    w, b = rn(803, N, D, scale=D ** -0.5), 0.1 * rn(804, N)
    xc, wf = x.to(d), (w * gamma).to(d)
    cs, bfold = wf.float().sum(1), w @ beta + b
    ref, bound = EB.ln_fold_bound(xc, wf, cs, bfold, x, 1e-6, torch.float32)
    acc = emu_acc(xc, wf)

    def emu(ddof=0, centre=True):
        mean = x.sum(-1, keepdim=True) / D
        var = ((x * x).sum(-1, keepdim=True) / D - mean * mean) * D / (D - ddof)
        r = torch.rsqrt(var + 1e-6)
        return acc * r + ((-mean * r) * cs[None] if centre else 0.0) + bfold
    r_ok = ratio(emu(), ref, bound)
    assert r_ok <= 0.5, r_ok
    for name, bad in (('no mean correction', emu(centre=False)), ('D - 1', emu(ddof=1)), ('via 16 bit', emu().to(d).float())):
        r_bad = ratio(bad, ref, bound)
        assert r_bad > 1 and r_bad >= 4 * r_ok, (name, r_bad, r_ok)
