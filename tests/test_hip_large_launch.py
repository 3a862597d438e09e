"""Device code that only a large launch selects.

1. launch_layernorm (csrc/misc.hip) takes layernorm_kernel<NIT, 4> - four rows per wave, a clamped load row and a `break` on the ragged tail - from
   32768 rows on (D <= 1024).  Its comment promises "results do not depend on RPW": the same rows normalised in two launches below the threshold (one row
   per wave) must give the same bits, for every NIT, type pair, the addend and the row remap; the fp32 result is also held to the float64 reference.
2. Launchers that cap their grid (GRID_CAPS) rely on a grid-stride loop beyond the cap.  Each test here picks the smallest convenient shape whose work-item
   count exceeds cap x 256 threads by a ragged amount (asserted from the table), so some threads run the loop body twice and the last block's second trip
   is partial, and checks the WHOLE output against the plain reference the op's small-shape test uses.
test_grid_caps_match_the_sources (host side) parses the launchers and fails if a cap differs from the table or a capped launcher is missing from it.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import errbound as EB

gpu = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
THREADS = 256
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'panst3r_amd', 'csrc')

# launcher (the function that holds the cap) -> largest grid it launches; 256 threads per block everywhere
GRID_CAPS = {
    # `if (g > N) g = N;`
    'pst_rowstats': 8192, 'pst_image_prepare': 8192, 'pst_pointmap_activate': 8192, 'pst_qubo_argmax': 8192,
    'pst_patch_rows': 16384, 'pst_groupnorm_apply': 16384, 'pst_qubo_upsample': 16384,
    'pst_loftup_lr_pe': 4096, 'launch_attn4': 4096, 'launch_x3': 4096,
    # through grid_for() of misc.hip (8192) / split.hip (16384): the same cap, written as a conditional expression
    'pst_split3': 8192, 'pst_rope2d': 8192, 'pst_patchify': 8192, 'pst_dino_preprocess': 8192, 'pst_add_cast': 8192, 'pst_mean4': 8192,
    'pst_resize_bilinear': 8192, 'pst_split_operand': 16384, 'pst_split2': 16384, 'pst_rope2d_split': 16384,
}


def crosses(op, work_items):
    """the launch of `op` over `work_items` threads' worth of work wraps its grid-stride loop, and not by whole blocks"""
    over = work_items - GRID_CAPS[op] * THREADS
    assert over > 0 and over % THREADS, (op, work_items, over)
    return True


def test_grid_caps_match_the_sources():
    func = re.compile(r'^(?:extern "C" |static (?:inline )?)int (\w+)\(', re.M)
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith('.hip'):
            continue
        src = open(os.path.join(CSRC, name)).read()
        defs = [(m.start(), m.group(1)) for m in func.finditer(src)]
        owner = lambda pos: [f for p, f in defs if p < pos][-1]
        for m in re.finditer(r'if \((\w+) > (\d+)\) (\w+) = (\d+);', src):
            assert m.group(1) == m.group(3) and m.group(2) == m.group(4), (name, m.group(0))
            assert owner(m.start()) not in found, (name, owner(m.start()))
            found[owner(m.start())] = int(m.group(2))
        helper = re.search(r'int grid_for\(.*?\n\}', src, re.S)
        if helper:
            cap = re.search(r'g > (\d+) \? (\d+) : g', helper.group(0))
            assert cap and cap.group(1) == cap.group(2), name
            for m in re.finditer(r'grid_for\(', src):
                if owner(m.start()) != 'grid_for':
                    found[owner(m.start())] = int(cap.group(1))
    assert found == GRID_CAPS, ('caps in the sources that differ from GRID_CAPS', sorted(set(found.items()) ^ set(GRID_CAPS.items())))


# ---------------------------------------------------------------------------------------------------------------- helpers
def rn(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def rel64(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def dn(seed, *shape):
    """standard normal fp32 on the device (large inputs: generated where they are used)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---------------------------------------------------------------------------------------------------------------- layernorm, four rows per wave
LN_THRESHOLD = 32768        # launch_layernorm: `rows >= 32768` (and D <= 1024) selects layernorm_kernel<NIT, 4>
LN_ROWS = [32768, 32769, 32771, 32783]      # full 4-row groups; 1, 3 and 3 rows in the last wave's group, the last block one / four waves wide
LN_GUARD = 4                # rows behind the output that must stay untouched (a wave without the tail `break` would write up to three)
LN_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _ln_input(D):
    x = dn(900 + D, 33700, D) * 3 + 1
    x[::9] = dn(901 + D, x[::9].shape[0], D) * 0.01 + 1            # quiet rows (variance 1e-4)
    return x, (1 + 0.1 * rn(41, D)).to(DEV), (0.1 * rn(42, D)).to(DEV)


def _ln_out(rows, D, kind):
    """(buffer with LN_GUARD sentinel rows behind the output, the output view, split)"""
    if kind == 'x3h':
        buf = torch.full((rows + LN_GUARD, 3 * D), -777.0, dtype=F16, device=DEV)
    else:
        buf = torch.full((rows + LN_GUARD, D), -777.0, dtype=kind, device=DEV)
    return buf, buf[:rows], kind == 'x3h'


def _ln_both(x, g, b, rows, D, kind, grp=None, add=None):
    """one launch over all rows (four rows per wave) and two launches of fewer than LN_THRESHOLD rows each (one row per wave)"""
    from panst3r_amd import hip
    gi, go = (grp[0], grp[1]) if grp else (1, 1)
    h = 16384 // gi * gi                                           # the second launch starts at a group boundary of the remap
    assert h < LN_THRESHOLD and rows - h < LN_THRESHOLD <= rows
    bufa, outa, split = _ln_out(rows, D, kind)
    bufb, outb, _ = _ln_out(rows, D, kind)
    kw = dict(grp=grp)
    if split:
        kw['split'] = True
    hip.layernorm(x, g, b, outa, LN_EPS, add=add, **kw)
    x2 = x[h // gi * go:]
    hip.layernorm(x, g, b, outb[:h], LN_EPS, add=add, **kw)
    hip.layernorm(x2, g, b, outb[h:], LN_EPS, add=(add[h // gi * go:] if add is not None else None), **kw)
    assert same_bits(bufa[rows:], torch.full_like(bufa[rows:], -777.0)), 'layernorm wrote behind its last row'
    assert same_bits(outa, outb), 'four rows per wave and one row per wave give different bits'
    return outa


# (16-bit -> 16-bit rows of 384 take layernorm384_kernel whatever the row count: tests/test_hip_ops.py::test_layernorm_384_wide_16bit_rows)
LN_KINDS = {'f32-f32': F32, 'bf16-bf16': BF16, 'f16-f16': F16, 'f32-x3h': 'x3h'}
LN_CASES = [(D, k) for D in (48, 384, 768, 1024) for k in LN_KINDS if not (D == 384 and LN_KINDS[k] in (BF16, F16))]


@gpu
@pytest.mark.parametrize('D,kind', LN_CASES, ids=['%d-%s' % c for c in LN_CASES])
@pytest.mark.parametrize('rows', LN_ROWS)
def test_layernorm_four_rows_per_wave(rows, D, kind):
    kind = LN_KINDS[kind]
    x, g, b = _ln_input(D)
    x = x[:rows]
    xin = x.to(kind) if kind in (BF16, F16) else x
    out = _ln_both(xin, g, b, rows, D, kind)
    if kind == F32:                                                 # not only kernel against kernel
        EB.check(out, EB.layernorm_ref(x, g, b, LN_EPS), EB.rownorm_bound(x, g, b, LN_EPS, F32), 'layernorm rows=%d D=%d, 4 rows per wave' % (rows, D))


@gpu
def test_layernorm_four_rows_per_wave_addend_and_remap():
    rows, D = 32771, 768
    x, g, b = _ln_input(D)
    add = dn(77, rows, D)
    out = _ln_both(x[:rows], g, b, rows, D, F32, add=add)
    xa = x[:rows] + add                                            # the kernel's fp32 add: one rounding, the same as torch's
    EB.check(out, EB.layernorm_ref(xa, g, b, LN_EPS), EB.rownorm_bound(xa, g, b, LN_EPS, F32), 'layernorm + addend, 4 rows per wave')
    out = _ln_both(x, g, b, rows, D, F32, grp=(37, 38, 1))           # skip a leading row per 38-row group
    ngrp = -(-rows // 37)
    xr = x[:ngrp * 38].reshape(ngrp, 38, D)[:, 1:].reshape(ngrp * 37, D)[:rows]
    EB.check(out, EB.layernorm_ref(xr, g, b, LN_EPS), EB.rownorm_bound(xr, g, b, LN_EPS, F32), 'layernorm row remap, 4 rows per wave')


# ---------------------------------------------------------------------------------------------------------------- grid-stride kernels past their cap
@pytest.fixture(params=[BF16, F16], ids=['bf16', 'f16'])
def fmt16(request):
    return request.param


@gpu
def test_rowstats_past_the_cap(fmt16):
    """16 lanes per (row, 64-column group): the 16-bit copy is the rounding of the stream, every (sum, sumsq) is a 64-term fp32 sum (64 u32 sum |x| resp.
    65 u32 sum x^2 with the squares' roundings), and a producer GEMM's epilogue gives the same bits (tests/test_hip_ops.py, LayerNorm-fold producer)"""
    from panst3r_amd import hip
    M, N, K = 8747, 960, 64
    assert crosses('pst_rowstats', M * (N // 64) * 16)
    a, w, b = dn(810, M, K).to(fmt16), (dn(811, N, K) * K ** -0.5).to(fmt16), dn(812, N)
    y = dn(813, M, N)
    xc = torch.full((M, N), float('nan'), dtype=fmt16, device=DEV)
    st = torch.full((M, N // 64, 2), float('nan'), device=DEV)
    hip.gemm(a, w, y, bias=b, res=y, xcopy=xc, stats_out=st)
    xc2, st2 = torch.full_like(xc, float('nan')), torch.full_like(st, float('nan'))
    hip.rowstats(y, xc2, st2)
    assert same_bits(xc, xc2) and same_bits(st.view(M, -1), st2.view(M, -1))
    assert torch.equal(xc2, y.to(fmt16))
    g64 = y.double().reshape(M, N // 64, 64)
    EB.check(st2[..., 0], g64.sum(-1), 64 * EB.U32 * g64.abs().sum(-1), 'rowstats sums')
    EB.check(st2[..., 1], (g64 * g64).sum(-1), 65 * EB.U32 * (g64 * g64).sum(-1), 'rowstats sums of squares')


@gpu
def test_image_prepare_past_the_cap():
    """a 1451 x 1449 crop of an up-sampled image against torch's antialiased bilinear interpolation on the CPU (tests/test_hip_input.py).  The image is a
    smooth ramp with a few grey levels of noise: an output written from the wrong index is off by the ramp, while the last bit of an fp32 tap weight at
    coordinates beyond 1000 (6e-5) times a neighbour difference of a few levels stays far below the tolerance"""
    from panst3r_amd import hip
    Hs, Ws, Hr, Wr, top, left, H, W = 1000, 1100, 1500, 1600, 20, 70, 1451, 1449
    assert crosses('pst_image_prepare', H * W)
    g = np.random.Generator(np.random.PCG64(7))
    ramp = (np.arange(Hs)[:, None, None] * 110 // Hs + np.arange(Ws)[None, :, None] * 110 // Ws + np.arange(3)[None, None, :] * 10)
    img = (ramp + g.integers(0, 8, size=(Hs, Ws, 3))).astype(np.uint8)
    out = torch.full((3 * H * W + 64,), float('nan'), device=DEV)
    hip.image_prepare(torch.from_numpy(img).to(DEV), out[:3 * H * W].view(3, H, W), (Hr, Wr), (top, left))
    t = (torch.from_numpy(img).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5
    ref = F.interpolate(t[None], size=(Hr, Wr), mode='bilinear', align_corners=False, antialias=True)[0][:, top:top + H, left:left + W]
    got = out.cpu()
    assert bool(torch.isnan(got[3 * H * W:]).all())
    assert float((got[:3 * H * W].view(3, H, W) - ref).abs().max()) < 2e-5


@gpu
def test_patch_rows_patchify_dino_preprocess_past_their_caps(fmt16):
    """many small images: patch_rows bit for bit against the separate kernels (tests/test_hip_input.py), which cross their own cap here and are anchored on
    torch: patchify is F.unfold rounded, dino_preprocess the normalised bilinear resize (rel-L2 <= 1e-5, here held for every image on its own)"""
    from panst3r_amd import hip
    n, H, W = 1901, 64, 96
    T = (H // 16) * (W // 16)
    assert crosses('pst_patch_rows', n * T * (3 * 16 + 1 + 3 * 14 + 1))
    assert crosses('pst_patchify', n * T * (3 * 16 + 1))
    assert crosses('pst_dino_preprocess', n * 3 * (H // 16 * 14) * (W // 16 * 14 // 4))
    g = torch.Generator(device=DEV).manual_seed(H + W)
    img = torch.rand(n, 3, H, W, generator=g, device=DEV) * 2 - 1
    enc = torch.full((n * T, 768), 7.0, dtype=fmt16, device=DEV)
    dino = torch.full((n * T, 640), 7.0, dtype=fmt16, device=DEV)
    hip.patch_rows(img, enc=enc, dino=dino, p_enc=16, p_dino=14)
    ref_e = torch.full((n * T, 768), 7.0, dtype=fmt16, device=DEV)
    hip.patchify(img, ref_e, 16)
    pre = torch.full((n, 3, H // 16 * 14, W // 16 * 14), float('nan'), device=DEV)
    hip.dino_preprocess(img, pre)
    ref_d = torch.full((n * T, 640), 7.0, dtype=fmt16, device=DEV)
    hip.patchify(pre, ref_d, 14)
    assert torch.equal(enc, ref_e) and torch.equal(dino, ref_d)
    assert torch.equal(ref_e, F.unfold(img, kernel_size=16, stride=16).transpose(1, 2).reshape(-1, 768).to(fmt16))
    assert torch.equal(ref_d[:, :588], F.unfold(pre, kernel_size=14, stride=14).transpose(1, 2).reshape(-1, 588).to(fmt16)) and not bool(ref_d[:, 588:].any())
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    ref = F.interpolate(((img.cpu() * 0.5 + 0.5) - mean) / std, size=pre.shape[-2:], mode='bilinear', align_corners=False).double()
    err = (pre.cpu().double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    assert bool((err < 1e-5).all()), float(err.max())


GN_CASES = [(BF16, 64, 8, 72, False), (F16, 64, 8, 72, False), (BF16, 203, 1, 208, False), (F16, 203, 1, 208, False), (F16, 64, 8, 192, True)]


@gpu
@pytest.mark.parametrize('fmt16,C,G,ld,split', GN_CASES, ids=['bf16-vec4', 'f16-vec4', 'bf16-scalar', 'f16-scalar', 'x3h'])
def test_groupnorm_apply_generic_kernels_past_the_cap(fmt16, C, G, ld, split):
    """fp32 rows in, padded 16-bit rows (or the split form) out: gn_apply_kernel<4> / <1>, not the 384-channel streaming kernel"""
    from panst3r_amd import hip
    cols = (ld // 3 if split else ld) // (4 if C % 4 == 0 else 1)
    nimg = 2
    P = (GRID_CAPS['pst_groupnorm_apply'] * THREADS // cols + 50) // nimg
    assert crosses('pst_groupnorm_apply', nimg * P * cols)
    x = dn(84, nimg * P, C) * 2 + 0.3
    g, b = (1 + 0.1 * rn(85, C)).to(DEV), (0.1 * rn(86, C)).to(DEV)
    st = hip.stats_buffer(nimg, G, DEV)
    if C % 4 == 0:
        hip.groupnorm_stats(x, st, nimg, P, C, G)
    else:
        x64 = x.double().reshape(nimg, -1)
        st[:2 * nimg].copy_(torch.stack([x64.sum(1), (x64 * x64).sum(1)], -1).reshape(-1).float())
    out = torch.full((nimg * P + 2, ld), 7.0, dtype=fmt16, device=DEV)
    hip.groupnorm_apply(x, st, g, b, out[:nimg * P], nimg, P, C, G, 1e-5, True, split=split)
    assert bool((out[nimg * P:] == 7.0).all())
    ref, bound = EB.groupnorm(x, nimg, P, G, g, b, 1e-5, F32 if split else fmt16, relu=True)
    if split:
        blk = ld // 3
        v = out[:nimg * P].view(nimg * P, 3, blk)
        assert same_bits(v[:, 0], v[:, 1])
        EB.check(v[:, 0, :C].double() + v[:, 2, :C].double(), ref, bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25, 'groupnorm_apply X3H past the cap')
        assert not bool(v[:, :, C:].any())
    else:
        EB.check(out[:nimg * P, :C], ref, bound, 'groupnorm_apply C=%d past the cap' % C)
        assert not bool(out[:nimg * P, C:].any())


@gpu
@pytest.mark.parametrize('fmt', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
def test_loftup_lr_pe_past_the_cap(fmt):
    """against the oracle's ImplicitFeaturizer with the tolerances of the small-shape tests (fp32 rows 1e-5, 16-bit rows 2e-2 max-abs); both images equal"""
    from panst3r_amd import hip
    from oracle.panoptic import ImplicitFeaturizer
    nimg, h, w = 2, 163, 161
    assert crosses('pst_loftup_lr_pe', nimg * h * w * 20)
    lr = ImplicitFeaturizer(False, n_freqs=5, learn_bias=True)
    with torch.no_grad():
        lr.biases.copy_(rn(87, 2, 2, 5))
        refl = lr(torch.zeros(1, 4, h, w))[0].permute(1, 2, 0).reshape(h * w, 20)
    o = torch.full((nimg * h * w + 1, 32), 3.0, dtype=fmt, device=DEV)
    hip.loftup_lr_pe(lr.biases.detach().to(DEV), o[:nimg * h * w], 8, nimg, h, w)
    oc = o.float().cpu()
    assert float((oc[:h * w, 8:28] - refl).abs().max()) < (1e-5 if fmt == F32 else 2e-2)
    assert torch.equal(oc[:h * w], oc[h * w:2 * h * w])
    assert bool((oc[:, :8] == 3.0).all()) and bool((oc[:, 28:] == 3.0).all()) and bool((oc[-1] == 3.0).all())


def _attn_long_q(fmt, seed):
    H, Nq, Nk, hd = 3, 14567, 256, 96
    D = H * hd
    q, k, v = (dn(seed + i, 1, H, n, hd).to(fmt) for i, n in enumerate((Nq, Nk, Nk)))
    qd = q[0].permute(1, 0, 2).reshape(Nq, D).contiguous()
    kd = k[0].permute(1, 0, 2).reshape(Nk, D).contiguous()
    vt = torch.zeros(D, Nk + 8, dtype=fmt, device=DEV)
    vt[:, :Nk] = v[0].permute(0, 2, 1).reshape(D, Nk)
    return H, Nq, Nk, hd, D, q, k, v, qd, kd, vt


@gpu
def test_attention_split_k_combine_past_the_cap(fmt16):
    """many query rows, two key splits: attn_combine_kernel merges 3 x 14567 rows of 24 four-element groups"""
    from panst3r_amd import hip
    H, Nq, Nk, hd, D, q, k, v, qd, kd, vt = _attn_long_q(fmt16, 23)
    assert crosses('launch_attn4', H * Nq * (hd // 4))
    od = torch.full((Nq + 1, D), float('nan'), dtype=fmt16, device=DEV)
    hip.attention(qd, kd, vt, od[:Nq], 1, H, Nq, Nk, hd, (0, hd, D), (0, hd, D), (0, hd * vt.stride(0), vt.stride(0)), (0, hd, D), nsplit=2)
    assert bool(torch.isnan(od[Nq]).all())
    EB.check(od[:Nq].reshape(1, Nq, H, hd).permute(0, 2, 1, 3), EB.attn_ref(q, k, v), EB.attn_bound(q, k, v, None, False, fmt16, fmt16, nsplit=2),
             'attention split-K combine past the cap')


@gpu
def test_attention_x3_split_k_combine_past_the_cap():
    from panst3r_amd import hip
    H, Nq, Nk, hd, D, q, k, v, qd, kd, vt = _attn_long_q(F32, 26)
    assert crosses('launch_x3', H * Nq * (hd // 4))
    prev, hip.X3 = hip.X3, True
    try:
        od = torch.full((Nq + 1, D), float('nan'), device=DEV)
        hip.attention(qd, kd, vt, od[:Nq], 1, H, Nq, Nk, hd, (0, hd, D), (0, hd, D), (0, hd * vt.stride(0), vt.stride(0)), (0, hd, D), nsplit=2)
    finally:
        hip.X3 = prev
    assert bool(torch.isnan(od[Nq]).all())
    EB.check(od[:Nq].reshape(1, Nq, H, hd).permute(0, 2, 1, 3), EB.attn_ref(q, k, v), EB.attn_bound(q, k, v, None, False, F32, F32, nsplit=2, mode='x3'),
             'attention on split operands, split-K combine past the cap')


@gpu
def test_pointmap_activate_past_the_cap():
    from panst3r_amd import hip
    import pp_stage_cases as C
    npix = 2097152 + 257
    assert crosses('pst_pointmap_activate', npix)
    raw = C.activate_case(npix, 0)
    pts, loc, conf = (torch.full(s, -777.0, device=DEV) for s in ((npix + 1, 3), (npix + 1, 3), (npix + 1,)))
    hip.pointmap_activate(raw.to(DEV), pts[:npix], loc[:npix], conf[:npix], 0)
    assert bool((pts[npix] == -777.0).all()) and bool((loc[npix] == -777.0).all()) and float(conf[npix]) == -777.0
    p, l, c, bp, bl, bc = C.ref_activate(raw)
    for got, ref, bound, what in ((pts, p, bp, 'pts3d'), (loc, l, bl, 'pts3d_local'), (conf, c, bc, 'conf')):
        EB.check(got[:npix].cpu(), ref, bound, 'pointmap_activate %s past the cap' % what)


@gpu
def test_qubo_argmax_past_the_cap():
    from panst3r_amd import hip
    import pp_stage_cases as C
    Q, P = 3, 2097152 + 257
    assert crosses('pst_qubo_argmax', P)
    probs = C.qubo_probs(Q, P, 1)
    probs[:, ::3] = probs[0, ::3].clone()                              # every query equal on a third of the pixels: the first selected one wins
    pd = probs.to(DEV)
    for sel in ([0, 2], [0, 1, 2]):
        conf = torch.full((P + 64,), -777.0, device=DEV)
        inst = torch.full((P + 64,), -12345, dtype=torch.int32, device=DEV)
        hip.qubo_argmax(pd, torch.tensor(sel, dtype=torch.int32, device=DEV), P, conf[:P], inst[:P])
        conf_r, inst_r = C.ref_qubo_argmax(probs, sel)
        assert torch.equal(conf[:P].cpu(), conf_r) and torch.equal(inst[:P].cpu(), inst_r)
        assert bool((conf[P:] == -777.0).all()) and bool((inst[P:] == -12345).all())


@gpu
def test_qubo_upsample_past_the_cap():
    from panst3r_amd import hip
    import pp_stage_cases as C
    Q, hm, wm, H, W = 17, 25, 31, 500, 495
    assert crosses('pst_qubo_upsample', Q * H * W)
    logits = C.blobs(3, Q, hm, wm)
    out = torch.full((Q * H * W + 64,), -777.0, device=DEV)
    hip.qubo_upsample(logits.to(DEV), out[:Q * H * W], Q, hm, wm, H, W)
    got = out.cpu()
    assert bool((got[Q * H * W:] == -777.0).all())
    grid = C.Grid(hm, wm, H, W)
    for q0 in range(0, Q, 8):
        m, dm = C.ref_m(logits[q0:q0 + 8], grid)
        EB.check(got[:Q * H * W].view(Q, H * W)[q0:q0 + 8], m, dm, 'qubo_upsample past the cap')


@gpu
def test_add_cast_and_split3_past_the_cap(fmt16):
    from panst3r_amd import hip
    rows, D = 8193, 1028
    assert crosses('pst_add_cast', rows * D // 4) and crosses('pst_split3', rows * D // 4)
    a, b = dn(70, rows, D), dn(71, 5, D)
    out = torch.full((rows + 1, D), 7.0, dtype=fmt16, device=DEV)
    hip.add_cast(a, out[:rows], b=b, b_mod=5)
    assert torch.equal(out[:rows], (a + b.repeat(rows // 5 + 1, 1)[:rows]).to(fmt16)) and bool((out[rows] == 7.0).all())
    s3 = torch.full((rows + 1, 3 * D), 7.0, dtype=fmt16, device=DEV)
    hip.split3(a, s3[:rows])
    hi = a.to(fmt16)
    lo = (a - hi.float()).to(fmt16)
    assert same_bits(s3[:rows], torch.cat([hi, hi, lo], 1)) and bool((s3[rows] == 7.0).all())


@gpu
def test_split_operand_and_split2_past_the_cap(fmt16):
    """the definition, as tests/test_hip_x3.py: hi = rn16(x), lo = rn16(x - hi); a K that is no multiple of 4 (scalar tail loads) and zero pad columns"""
    from panst3r_amd import hip
    rows, K, kpad = 16400, 1025, 1028
    assert crosses('pst_split_operand', rows * kpad // 4) and crosses('pst_split2', rows * kpad // 4)
    x = dn(1, rows, kpad + 4)
    for side in (0, 1):
        xs = x[:, :K]
        hi = xs.to(fmt16)
        lo = (xs - hi.float()).to(fmt16)
        ref = torch.zeros(rows, 3, kpad, dtype=fmt16, device=DEV)
        for blk, t in enumerate((hi, lo, hi) if side else (hi, hi, lo)):
            ref[:, blk, :K] = t
        got = torch.full((rows + 1, 3 * kpad), 7.0, dtype=fmt16, device=DEV)
        hip.split_operand(xs, side, kpad=kpad, out=got[:rows])
        assert same_bits(got[:rows], ref.view(rows, 3 * kpad)) and bool((got[rows] == 7.0).all())
    xs = x[:, :kpad]
    h2, l2 = hip.split2(xs, fmt=fmt16)
    hi = xs.to(fmt16)
    assert same_bits(h2, hi) and same_bits(l2, (xs - hi.float()).to(fmt16))


@gpu
@pytest.mark.parametrize('fmt', [F32, BF16, F16], ids=['f32', 'bf16', 'f16'])
def test_rope2d_past_the_cap(fmt):
    """thread = (row, head, half, four frequencies); against the float64 rotation under errbound.rope2d's bound, the untouched v third bit for bit"""
    from panst3r_amd import hip
    H, hd, rows = 2, 64, 65551
    assert crosses('pst_rope2d', rows * 2 * H * 2 * (hd // 16))
    g = torch.Generator(device=DEV).manual_seed(3)
    pos = torch.randint(0, 32, (rows, 2), generator=g, device=DEV, dtype=torch.int32)
    x = dn(50, rows, 3 * H * hd).to(fmt)
    y = x.clone()
    hip.rope2d_(y, pos, hip.rope_table(32, hd, 100.0, DEV), 2 * H, hd)
    got = y.reshape(rows, 3, H, hd)
    x4 = x.reshape(rows, 3, H, hd)
    for i in range(2):
        ref, bound = EB.rope2d(x4[:, i].permute(1, 0, 2), pos, fmt)
        EB.check(got[:, i].permute(1, 0, 2), ref, bound, 'rope2d past the cap')
    assert same_bits(got[:, 2], x4[:, 2])


@gpu
def test_rope2d_split_past_the_cap():
    """rope2d_split is rope2d_ followed by split2 bit for bit (tests/test_hip_x3.py), and hi + lo holds the float64 rotation to the fp32 bound plus the
    split's own 2^-22 |ref| + 2^-25"""
    from panst3r_amd import hip
    H, hd, rows = 4, 64, 65551
    assert crosses('pst_rope2d_split', rows * 2 * H * 2 * (hd // 16))
    g = torch.Generator(device=DEV).manual_seed(3)
    pos = torch.randint(0, 32, (rows, 2), generator=g, device=DEV, dtype=torch.int32)
    D = 2 * H * hd
    x = dn(21, rows, D + 8)[:, :D]
    keep = x.clone()
    table = hip.rope_table(32, hd, 100.0, DEV)
    pl = hip.rope2d_split(x, pos, table, 2 * H, hd)
    assert torch.equal(x, keep)
    y = x.clone().contiguous()
    hip.rope2d_(y, pos, table, 2 * H, hd)
    hi, lo = hip.split2(y)
    assert same_bits(pl.hi, hi) and same_bits(pl.lo, lo)
    ref, bound = EB.rope2d(x.reshape(rows, 2 * H, hd).permute(1, 0, 2), pos, F32)
    EB.check((pl.hi.double() + pl.lo.double()).reshape(rows, 2 * H, hd).permute(1, 0, 2), ref, bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25, 'rope2d_split past the cap')


@gpu
def test_mean4_past_the_cap(fmt16):
    """the mean of the central 2 x 2 pixels of every 8 x 8 block, 0.25 (((a + b) + c) + d) in fp32 rounded once: the same expression in torch, bit for bit"""
    from panst3r_amd import hip
    nimg, th, tw, C = 1, 91, 91, 1020
    assert crosses('pst_mean4', nimg * th * tw * (C // 4))
    Fm = dn(73, nimg, th * 8, tw * 8, C // 2).to(fmt16).repeat(1, 1, 1, 2)        # (half of the channels drawn, repeated: the values do not matter to the indexing)
    Fm[..., C // 2:] += 1
    out = torch.full((nimg * th * tw + 1, C), 7.0, dtype=fmt16, device=DEV)
    hip.mean4(Fm, out[:nimg * th * tw], nimg, th * 8, tw * 8, C)
    f = lambda dy, dx: Fm[:, 3 + dy::8, 3 + dx::8].float()
    ref = (0.25 * (((f(0, 0) + f(0, 1)) + f(1, 0)) + f(1, 1))).to(fmt16).reshape(nimg * th * tw, C)
    assert same_bits(out[:nimg * th * tw], ref) and bool((out[-1] == 7.0).all())


@gpu
def test_resize_bilinear_past_the_cap():
    """fp32 rows against F.interpolate on the CPU, max-abs 1e-5 (tests/test_hip_fp32.py)"""
    from panst3r_amd import hip
    n, Hs, Ws, Hd, Wd, C = 3, 75, 73, 300, 292, 32
    assert crosses('pst_resize_bilinear', n * Hd * Wd * (C // 4))
    xx = rn(74, n, Hs, Ws, C)
    ref = F.interpolate(xx.permute(0, 3, 1, 2), size=(Hd, Wd), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    out = torch.full((n * Hd * Wd + 1, C), float('nan'), device=DEV)
    hip.resize_bilinear(xx.to(DEV), out[:n * Hd * Wd], n, Hs, Ws, Hd, Wd, C)
    oc = out.cpu()
    assert float((oc[:n * Hd * Wd].reshape(n, Hd, Wd, C) - ref).abs().max()) < 1e-5 and bool(torch.isnan(oc[-1]).all())
