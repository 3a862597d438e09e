"""The bounds and exact references of the small row and pixel kernels (tests/smallops_ref.py, errbound.l2norm_bound / resize_bound) are SOUND and TIGHT
(CPU only): at the shapes and data of tests/test_hip_smallops.py an fp32 emulation of the correct kernel - the same order of operations in torch fp32 - meets
each bound, and each planted wrong kernel fails it (or, for the exact operations, differs from the reference).

Where a planted kernel computes the same thing as the right one at a shape (an identity resize cannot tell two scale factors apart), the test says so and
asserts the failure at every other shape.
"""
import numpy as np
import pytest
import torch

import errbound as EB
import smallops_ref as SR

F32 = np.float32
FMTS = {'bf16': torch.bfloat16, 'f16': torch.float16, 'fp32': torch.float32}


def ratio(got, ref, bound, keep=None):
    r = (got.double() - ref.double()).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float((r if keep is None else r[keep]).max())


# ------------------------------------------------------------------------------------------------------------------------------------------- l2norm_rows
def emu_l2norm(x, eps, fmt, ncols=None, eps_inside=False, no_eps=False):
    """one wave per row: lane l sums the squares of columns l, l + 64, ... in fp32, a pairwise tree (the xor butterfly) adds the lanes; 1 / (sqrt + eps); the
    product; one rounding to the storage format.  ncols / eps_inside / no_eps plant the mistakes."""
    rows, D = x.shape
    n = -(-D // 64)
    xp = torch.zeros(rows, n * 64)
    xp[:, :D] = x
    if ncols is not None:
        xp[:, ncols:] = 0.0
    s = torch.zeros(rows, 64)
    for i in range(n):
        v = xp[:, i * 64:(i + 1) * 64]
        s = s + v * v
    w = 64
    while w > 1:
        w //= 2
        s = s[:, :w] + s[:, w:2 * w]
    e = torch.tensor(eps, dtype=torch.float32)
    nrm = torch.sqrt(s + e) if eps_inside else (torch.sqrt(s) if no_eps else torch.sqrt(s) + e)
    return (x * (1.0 / nrm)).to(fmt)


@pytest.mark.parametrize('fmt', list(FMTS))
@pytest.mark.parametrize('D', SR.L2_D)
def test_l2norm_bound(D, fmt):
    """every (rows, eps) of the GPU test: the emulation <= 0.5 of the bound; columns >= 64 dropped (D > 64), eps inside the root, eps left out (eps = 1e-7,
    which the quiet rows tell) all exceed it"""
    f = FMTS[fmt]
    for rows in SR.L2_ROWS:
        x = SR.l2norm_case(rows, D)
        for eps in (1e-7, 0.0):
            ref = SR.l2norm(x, eps)
            keep = torch.isfinite(ref)                       # the all-zero row is 0 / 0 with eps = 0: the GPU test holds that row to NaN on its own
            assert bool(keep.all()) == (eps > 0 or rows < 5)
            ref = torch.where(keep, ref, torch.zeros_like(ref))
            bound = EB.l2norm_bound(ref, D, f)
            got = emu_l2norm(x, eps, f)
            normal = ref.abs() >= torch.finfo(f).tiny          # a rounding into the subnormal range errs by up to tiny(fmt), which the bounds do not double
            r_ok, r_sub = ratio(got, ref, bound, keep & normal), ratio(got, ref, bound, keep)
            assert r_ok <= 0.5 and r_sub <= 1.0, (rows, eps, r_ok, r_sub)
            if D > 64:
                assert ratio(emu_l2norm(x, eps, f, ncols=64), ref, bound, keep) > 1, (rows, eps)
            if eps > 0:
                assert ratio(emu_l2norm(x, eps, f, eps_inside=True), ref, bound, keep) > 1, rows
                assert ratio(emu_l2norm(x, eps, f, no_eps=True), ref, bound, keep) > 1, rows


# ------------------------------------------------------------------------------------------------------------------------------------------- bilinear resize
def emu_coords(S, Dn, half=True, exchange=False, fused=False, clamp1=True):
    """the kernel's fp32 coordinate -> (i0, i1, w fp32).  half=False: no half-pixel offset; exchange: D / S as the scale; fused: (d + 0.5) s - 0.5 rounded
    once (an fma: the product is exact in float64); clamp1=False: i1 = i0 + 1 even behind the last pixel"""
    s = F32(Dn) / F32(S) if exchange else F32(S) / F32(Dn)
    d = np.arange(Dn, dtype=F32)
    if not half:
        f = d * s
    elif fused:
        f = ((d.astype(np.float64) + 0.5) * np.float64(s) - 0.5).astype(F32)
    else:
        f = (d + F32(0.5)) * s - F32(0.5)
    f = np.maximum(f, F32(0)).astype(F32)
    i0 = np.minimum(f.astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1) if clamp1 else i0 + 1
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy((f - i0.astype(F32)).astype(F32))


def emu_blend(src, Hd, Wd, fmt, swap=False, clamp_x1=True, dino_order=False, **kw):
    """the 4-tap blend in torch fp32, one rounding per operation, of src [n, C, H, W] fp32.  An unclamped x1 reads the next pixel in memory: the first of the
    next row, or of the next image (only the last image's last row has nothing behind it: clipped here)"""
    n, C, H, W = src.shape
    y0, y1, wy = emu_coords(H, Hd, **kw)
    x0, x1, wx = emu_coords(W, Wd, clamp1=clamp_x1, **kw)
    flat = src.permute(1, 0, 2, 3).reshape(C, n * H * W)
    base = (torch.arange(n) * H * W)[:, None, None]
    tap = lambda yy, xx: flat[:, (base + yy[None, :, None] * W + xx[None, None, :]).clamp_max(n * H * W - 1)].permute(1, 0, 2, 3)
    a, b, d, e = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    wy = wy[:, None]
    hx, lx = (wx, 1.0 - wx) if swap else (1.0 - wx, wx)
    if dino_order:
        o = (a * hx + b * lx) * (1.0 - wy) + (d * hx + e * lx) * wy
    else:
        o = (1.0 - wy) * (hx * a + lx * b) + wy * (hx * d + lx * e)
    return o.to(fmt)


def emu_resize(x, Hd, Wd, fmt, **kw):
    return emu_blend(x.float().permute(0, 3, 1, 2), Hd, Wd, fmt, **kw).permute(0, 2, 3, 1)


# the planted resize kernels and the shapes (Hs, Ws, Hd, Wd) at which they compute something else than the right kernel
RESIZE_PLANTS = {
    'no half-pixel offset': (dict(half=False), lambda Hs, Ws, Hd, Wd: (Hs > 1 and Hs != Hd) or (Ws > 1 and Ws != Wd)),     # scale 1 or a single pixel: the same taps
    'x1 = x0 + 1 unclamped': (dict(clamp_x1=False), lambda Hs, Ws, Hd, Wd: Wd > Ws),                         # only an up-scaling samples behind the last pixel centre
    'wx and 1 - wx swapped': (dict(swap=True), lambda Hs, Ws, Hd, Wd: Ws > 1 and Ws % (2 * Wd) != 0),              # one column: the same pixel twice; an even ratio: wx = 1 / 2
    'Hs / Hd and Ws / Wd exchanged': (dict(exchange=True), lambda Hs, Ws, Hd, Wd: (Hs > 1 and Hs != Hd) or (Ws > 1 and Ws != Wd)),
}


@pytest.mark.parametrize('fmt', list(FMTS))
@pytest.mark.parametrize('shape', SR.RESIZE_SHAPES)
def test_resize_bound(shape, fmt):
    """the emulation with either rounding of the coordinate (two roundings, or one fma) <= 0.5 of the bound (and bit-exact at the identity shape); every
    planted kernel exceeds it wherever it is a different computation"""
    Hs, Ws, Hd, Wd = shape
    f = FMTS[fmt]
    x = SR.resize_case(Hs, Ws, 4, f)
    r = SR.resize(x, Hd, Wd)
    bound = SR.resize_bound(r, f)
    for fused in (False, True):
        got = emu_resize(x, Hd, Wd, f, fused=fused)
        r_ok = ratio(got, r['ref'], bound)
        assert r_ok <= 0.5, (fused, r_ok)
        if (Hs, Ws) == (Hd, Wd):
            assert torch.equal(got, x)
    assert (Hs, Ws) != (Hd, Wd) or torch.equal(r['ref'], x.double())
    for name, (kw, differs) in RESIZE_PLANTS.items():
        r_bad = ratio(emu_resize(x, Hd, Wd, f, **kw), r['ref'], bound)
        assert (r_bad > 1) == differs(*shape), (name, r_bad)


def emu_dino(img, Ho, Wo, one_channel=False):
    mean = torch.tensor(SR.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(SR.IMAGENET_STD).view(3, 1, 1)
    if one_channel:
        mean, std = mean[:1].expand(3, 1, 1), std[:1].expand(3, 1, 1)
    nv = ((img * 0.5 + 0.5) - mean) / std
    return emu_blend(nv, Ho, Wo, torch.float32, dino_order=True)


@pytest.mark.parametrize('shape', SR.DINO_SHAPES)
def test_dino_preprocess_bound(shape):
    """the emulation <= 0.5 of the bound; channel 0's mean and std on every channel, and the planted resize kernels, exceed it"""
    H, W, Ho, Wo = shape
    img = SR.dino_case(H, W)
    ref, tapmax, emax = SR.dino_preprocess(img, Ho, Wo)
    bound = EB.resize_bound(ref, tapmax, torch.float32, dtaps=emax)
    r_ok = ratio(emu_dino(img, Ho, Wo), ref, bound)
    assert r_ok <= 0.5, r_ok
    r_bad = (emu_dino(img, Ho, Wo, one_channel=True).double() - ref).abs() / bound
    assert float(r_bad[:, 0].max()) <= 0.5 and float(r_bad[:, 1].min()) > 1 and float(r_bad[:, 2].min()) > 1
    mean = torch.tensor(SR.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(SR.IMAGENET_STD).view(3, 1, 1)
    nv = ((img * 0.5 + 0.5) - mean) / std
    for name, (kw, differs) in RESIZE_PLANTS.items():
        r_bad = ratio(emu_blend(nv, Ho, Wo, torch.float32, dino_order=True, **kw), ref, bound)
        assert (r_bad > 1) == differs(H, W, Ho, Wo), (name, r_bad)


def test_resize_reference_is_interpolate():
    """the float64 references against torch's own bilinear resize in float64 (a different implementation of the same rule) at every shape: 1e-6 of the data's
    range, which leaves room for a coordinate that differs in its last fp32 bit and for nothing else"""
    import torch.nn.functional as F
    for (Hs, Ws, Hd, Wd) in SR.RESIZE_SHAPES:
        x = SR.resize_case(Hs, Ws, 4, torch.float32)
        ours = SR.resize(x, Hd, Wd)['ref']
        theirs = F.interpolate(x.double().permute(0, 3, 1, 2), size=(Hd, Wd), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
        assert float((ours - theirs).abs().max()) <= 1e-6 * float(x.abs().max()), (Hs, Ws, Hd, Wd)
    m, s = SR.dino_constants()
    for (H, W, Ho, Wo) in SR.DINO_SHAPES:
        img = SR.dino_case(H, W)
        theirs = F.interpolate(((img.double() * 0.5 + 0.5) - m) / s, size=(Ho, Wo), mode='bilinear', align_corners=False)
        assert float((SR.dino_preprocess(img, Ho, Wo)[0] - theirs).abs().max()) <= 1e-5, (H, W, Ho, Wo)


# ------------------------------------------------------------------------------------------------------------------------------------------- exact operations
@pytest.mark.parametrize('Nk', SR.MASK_NK)
def test_attn_mask_reference_rejects_the_planted_kernels(Nk):
    lg = SR.mask_case(Nk, SR.MASK_KINDS)
    ref = SR.attn_mask(lg)
    kinds = {k: i for i, k in enumerate(SR.MASK_KINDS)}
    # what the rows are for
    assert not ref[kinds['blocked']].any() and not ref[kinds['open']].any() and not ref[kinds['minus_zero']].any() and not ref[kinds['blocked_specials']].any()
    if Nk > 1:
        assert int(ref[kinds['last']].sum()) == Nk - 1 and ref[kinds['last'], Nk - 1] == 0
        assert int(ref[kinds['nan_only']].sum()) == Nk - 1
        assert int(ref[kinds['second_trip']].sum()) == Nk - 1 and ref[kinds['second_trip'], (300 if Nk > 300 else Nk - 1) if Nk > 256 else 0] == 0
    # `<= 0`: -0.0 and 0.0 become blocked.  (With a single key every row is open or cleared: the mask is zero whatever the rule.)
    m = lg <= 0
    m[m.all(-1)] = False
    assert torch.equal(m.to(torch.uint8), ref) == (Nk == 1)
    # a row is cleared when its first 256 columns are blocked: the same for Nk <= 256
    m = lg < 0
    m[m[:, :256].all(-1)] = False
    assert torch.equal(m.to(torch.uint8), ref) == (Nk <= 256)
    # NaN written as 1
    m = ~(lg >= 0)
    m[m.all(-1)] = False
    assert torch.equal(m.to(torch.uint8), ref) == (Nk == 1)


def test_add_cast_reference_rejects_row_indexing():
    """b[row] (clamped to b's rows) instead of b[row % b_mod] differs for b_mod = 1 and 5; b_mod = 0 and b_mod = rows ARE b[row]"""
    for D in SR.ADD_D:
        a, b = SR.add_cast_case(D, torch.float32, torch.float32)
        for b_mod in SR.ADD_BMOD:
            ref = SR.add_cast(a, b, b_mod, torch.bfloat16)
            bad = (a + b[torch.arange(SR.ADD_ROWS).clamp_max(b.shape[0] - 1)]).to(torch.bfloat16)
            assert torch.equal(bad, ref) == (b_mod in (0, SR.ADD_ROWS)), (D, b_mod)


def test_token_embed_reference_rejects_row_positions():
    """pos[row] (clamped) instead of pos[row % L] differs as soon as there is a second sequence"""
    for (B, L) in SR.TOK_BL:
        ids, tok, pos = SR.token_case(B, L, 8)
        assert int(ids.min()) == 0 or B * L == 1
        assert int(ids.max()) == SR.TOK_VOCAB - 1
        ref, status = SR.token_embed(ids, tok, pos)
        assert status == 0
        bad = tok[ids.long().view(-1)] + pos[torch.arange(B * L).clamp_max(SR.TOK_NPOS - 1)]
        assert torch.equal(bad, ref) == (B == 1)
        ids[-1, -1] = SR.TOK_VOCAB
        ref2, status = SR.token_embed(ids, tok, pos)
        assert status == -1 and not ref2[-1].any() and torch.equal(ref2[:-1], ref[:-1])


def test_mean4_reference_is_the_8x_downsampling():
    """the exact expression is the 8x bilinear down-sampling (align_corners=False) to fp32 rounding"""
    import torch.nn.functional as F
    Fm = SR.rn(73, 2, 16, 24, 8)
    ref = F.interpolate(Fm.double().permute(0, 3, 1, 2), size=(2, 3), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    assert float((SR.mean4(Fm).double() - ref).abs().max()) <= 4 * EB.U32 * float(Fm.abs().max())
