"""Stage-level parity of csrc/loftup.hip's guidance front end where its loops repeat and its branches turn: pst_loftup_guidance_gn, pst_loftup_minmax,
pst_minmax_merge, pst_loftup_lr_pe and pst_groupnorm_stats called directly and held, element by element, to float64 references of the restatement
tests/guidance_ref.py under errbound.guidance_bound / sincos_bound (derived from the kernel's arithmetic and the MEASURED error of its sincos_cw;
tests/test_guidance_host.py shows on the CPU that the restatement is torch's arithmetic bit for bit and that the bound catches a fused phase, an unmirrored
linspace and a serially summed 2x2 mean).

Shapes (guidance_ref.SHAPES): 132 x 250 x 3 views (8250 pixels = 129 tiles: the stats pass, capped at 128 blocks, strides once and its second trip is the
ragged tile of 58 pixels; down2_minmax_kernel loops 9 times with a partial last trip; 128 partials: the second trip of reduce_partials_kernel; odd W2),
2 x 250 (H2 = 1: linspace's n = 1 branch), 2 x 6 (3 pixels: 61 idle lanes clamped to the last pixel), 384 x 4 and 4 x 512 (linspace at the product's n = 192
and n = 256), 16 x 24 (the case of tests/test_hip_ops.py).  The inputs (guidance_ref.make_case) put every plane's minimum at its last pixel and its maximum
into the last partial trip, and carry a constant plane, one whose range is exactly the scaler's 1e-4 clamp and one a float32 below it.

Per shape: fp32 rows at ldy = 208 and 256 - every element under the bound, exact zeros in the padding columns, sentinel rows behind the output untouched,
the (sum, sumsq) statistics under their bound, the down-sampled image and the min / max table in the scratch buffer bit-equal to the restatement; 16-bit
rows bit-equal to the rounding of the fp32 rows; two calls give the same bytes; swapped views give swapped outputs; a scale table pooled over scopes.
test_sincos_cw_error is the measurement behind errbound.SINCOS_ABS.

Measured on the MI355X (profiles/output_kernel_margins.jsonl): see docs/experiments.md."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import errbound as EB
import guidance_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5
SENTINEL = -768.0                 # representable in bf16 and f16
TAIL = 5                          # sentinel rows behind the output


def _log(**kw):
    if os.environ.get('PST_STAGE_LOG'):
        with open(os.environ['PST_STAGE_LOG'], 'a') as f:
            f.write(json.dumps(kw) + '\n')


def _hip():
    from panst3r_amd import hip
    return hip


@functools.lru_cache(maxsize=None)
def _case(shape, pooled=False):
    """the case, its restatement and the float64 reference with its bounds - computed once per shape, shared by the tests, never modified"""
    H, W, n = shape
    case = G.make_case(H, W, n)
    own = G.guidance_inputs(case['img'], case['biases'], G.NF)
    G.assert_case(case, own)
    r = G.guidance_inputs(case['img'], case['biases'], G.NF, mm=G.pooled(own['mm'], case['scope'])) if pooled else own
    feat = G.features64(r['s_in'], r['c_in'], r['col'])
    if torch.cuda.is_available():
        feat = feat.to(DEV)                                     # the float64 bound of the 8250-pixel shape: 5 M elements, quicker there
    ref, bound, stats, sb = EB.guidance_bound(feat, case['gamma'], case['beta'], EPS, G.NF)
    return case, r, ref, bound, stats, sb


def _run(hip, case, dtype, ldy, mm=None, nf=G.NF):
    img = case['img'].to(DEV)
    n, _, H, W = img.shape
    P = (H // 2) * (W // 2)
    buf = torch.full((n * P + TAIL, ldy), SENTINEL, dtype=dtype, device=DEV)
    scratch = torch.zeros(n * (3 * P + 6), device=DEV)
    st = torch.full_like(hip.stats_buffer(n, 1, DEV), SENTINEL)
    hip.loftup_guidance_gn(img, case['biases'].to(DEV), case['gamma'].to(DEV), case['beta'].to(DEV), EPS, scratch, st, buf[:n * P], nf, mm=mm)
    torch.cuda.synchronize()
    return buf, st, scratch


def _check_layout(buf, n, P, CH):
    assert float(buf[:n * P, CH:].float().abs().max()) == 0.0, 'padding columns must be exact zeros'
    assert bool((buf[n * P:].float() == SENTINEL).all()), 'rows behind the output were written'


@pytest.mark.parametrize('ldy', [208, 256])
@pytest.mark.parametrize('shape', G.SHAPES, ids=G.shape_id)
def test_guidance_fp32(shape, ldy):
    hip = _hip()
    H, W, n = shape
    P, CH = (H // 2) * (W // 2), 10 * G.NF + 3
    case, r, ref, bound, stats, sb = _case(shape)
    buf, st, scratch = _run(hip, case, torch.float32, ldy)
    # stage by stage: the 2x2 mean and the min / max table the kernel left in its scratch buffer are the restatement's, bit for bit
    assert torch.equal(scratch[:n * 3 * P].cpu(), torch.from_numpy(r['img2']).reshape(-1)), '2x2 mean'
    assert torch.equal(scratch[n * 3 * P:].cpu(), torch.from_numpy(r['mm']).reshape(-1)), 'min / max'
    _check_layout(buf, n, P, CH)
    ratio = EB.check(buf[:n * P, :CH], ref, bound, 'guidance_gn fp32 %s ldy=%d' % (G.shape_id(shape), ldy))
    rs = EB.check(st[:2 * n].view(n, 2), stats, sb, 'guidance_gn statistics %s' % G.shape_id(shape))
    gx = min(-(-P // 64), hip.STATS_BLOCKS)
    assert bool((st[2 * n * (1 + gx):] == SENTINEL).all()), 'statistics buffer written beyond its partials'
    # a fixed order and no atomics: a second call gives the same bytes, statistics and partials included
    buf2, st2, scratch2 = _run(hip, case, torch.float32, ldy)
    assert torch.equal(buf, buf2) and torch.equal(st, st2) and torch.equal(scratch, scratch2)
    print('%s ldy=%d: err / bound %.3f (output), %.3g (statistics)' % (G.shape_id(shape), ldy, ratio, rs))
    _log(stage='guidance_gn', shape=G.shape_id(shape), ldy=ldy, ratio=ratio, ratio_stats=rs)


@pytest.mark.parametrize('dtype,ldy', [(torch.bfloat16, 208), (torch.bfloat16, 256), (torch.float16, 208), (torch.float16, 256)], ids=['bf16-208', 'bf16-256', 'f16-208', 'f16-256'])
@pytest.mark.parametrize('shape', G.SHAPES, ids=G.shape_id)
def test_guidance_16bit_rows_are_the_rounded_fp32_rows(shape, dtype, ldy):
    hip = _hip()
    H, W, n = shape
    P, CH = (H // 2) * (W // 2), 10 * G.NF + 3
    case = _case(shape)[0]
    b32, st32, _ = _run(hip, case, torch.float32, ldy)
    b16, st16, _ = _run(hip, case, dtype, ldy)
    _check_layout(b16, n, P, CH)
    assert torch.equal(b16[:n * P].view(torch.int16), b32[:n * P].to(dtype).view(torch.int16))
    assert torch.equal(st16, st32)
    b16b, st16b, _ = _run(hip, case, dtype, ldy)
    assert torch.equal(b16.view(torch.int16), b16b.view(torch.int16)) and torch.equal(st16, st16b)


@pytest.mark.parametrize('shape', [s for s in G.SHAPES if s[2] >= 2], ids=G.shape_id)
def test_swapped_views_swap_their_outputs(shape):
    """the partials are indexed view * gridDim.x + block: two views exchanged exchange their rows and their statistics and nothing else"""
    hip = _hip()
    H, W, n = shape
    P = (H // 2) * (W // 2)
    case = _case(shape)[0]
    perm = [1, 0] + list(range(2, n))
    assert not torch.equal(case['img'][0], case['img'][1])
    swapped = dict(case, img=case['img'][perm].contiguous())
    a, sa, _ = _run(hip, case, torch.float32, 208)
    b, sb_, _ = _run(hip, swapped, torch.float32, 208)
    assert torch.equal(b[:n * P].view(n, P, 208), a[:n * P].view(n, P, 208)[perm])
    assert torch.equal(sb_[:2 * n].view(n, 2), sa[:2 * n].view(n, 2)[perm])
    assert not torch.equal(a[:P], a[P:2 * P])


@pytest.mark.parametrize('shape', G.SHAPES, ids=G.shape_id)
def test_minmax_and_pooled_table(shape):
    """pst_loftup_minmax == amin / amax of the 2x2 mean exactly (minimum at the plane's last pixel, maximum in the last partial trip of the 1024-thread
    loop); pst_minmax_merge pools exactly; the guidance kernel scaled with a pooled table that is strictly wider than view 0's own range is held to the
    bound of the restatement with that table, which test_guidance_host.py shows to be the oracle's scaler over the chunk"""
    hip = _hip()
    H, W, n = shape
    P, CH = (H // 2) * (W // 2), 10 * G.NF + 3
    case, r = _case(shape)[:2]
    mm = torch.full((n, 3, 2), SENTINEL, device=DEV)
    hip.loftup_minmax(case['img'].to(DEV), mm)
    small = torch.from_numpy(G.half_mean(case['img']))
    assert torch.equal(mm[..., 0].cpu(), small.amin(dim=(2, 3))) and torch.equal(mm[..., 1].cpu(), small.amax(dim=(2, 3)))
    if n < 2:
        return
    tab = hip.minmax_merge(mm, torch.tensor(case['scope'], dtype=torch.int32, device=DEV), torch.full_like(mm, SENTINEL))
    want = G.pooled(r['mm'], case['scope'])
    assert torch.equal(tab.cpu(), torch.from_numpy(want))
    assert ((want[0, :, 0] < r['mm'][0, :, 0]) | (want[0, :, 1] > r['mm'][0, :, 1])).all()
    _, rp, ref, bound, stats, sb = _case(shape, True)
    buf, st, _ = _run(hip, case, torch.float32, 208, mm=tab)
    _check_layout(buf, n, P, CH)
    ratio = EB.check(buf[:n * P, :CH], ref, bound, 'guidance_gn pooled table %s' % G.shape_id(shape))
    EB.check(st[:2 * n].view(n, 2), stats, sb, 'guidance_gn statistics, pooled table %s' % G.shape_id(shape))
    _log(stage='guidance_gn_pooled', shape=G.shape_id(shape), ratio=ratio)


@pytest.mark.parametrize('n,C,G_', [(70, 64, 8), (3, 1024, 8)], ids=['C64', 'C1024-67-partials'])
def test_groupnorm_stats_130x130(n, C, G_):
    """pst_groupnorm_stats on 4225 rows.  With C = 64 a block takes 16 rows at a time and 5 blocks cover the map; with C = 1024 a block is one row wide, 67
    blocks leave 67 partials per (view, group) and reduce_partials_kernel makes its `lane + 64` trip (the 132 x 250 guidance case reaches it with 128).
    (sum, sumsq) against float64 sums of the same fp32 input; rounding steps on one element's way: 4 channels x its thread's rows, the rpb x chunks-per-group
    walk through LDS, ceil(nb / 64) serial adds and 6 shuffle levels, every one allowed twice (R)."""
    hip = _hip()
    P = 65 * 65
    g = torch.Generator().manual_seed(130)
    x = (torch.randn(n * P, C, generator=g) * 2 + 0.3).to(DEV)
    st = torch.full_like(hip.stats_buffer(n, G_, DEV), SENTINEL)
    hip.groupnorm_stats(x, st, n, P, C, G_)
    c4 = C // 4
    rpb = 1 if c4 >= 256 else 256 // c4
    nb = min(-(-P // (64 * rpb)), hip.STATS_BLOCKS)
    assert nb == (67 if C == 1024 else 5)
    rows = -(-(-(-P // nb)) // rpb)
    nred = 4 * rows + rpb * (C // G_ // 4) + -(-nb // 64) + 6
    xg = x.double().view(n, P, G_, C // G_).permute(0, 2, 1, 3).reshape(n, G_, -1)
    ref = torch.stack([xg.sum(-1), (xg * xg).sum(-1)], -1)
    bound = torch.stack([EB.R * nred * EB.U32 * xg.abs().sum(-1), EB.R * (nred + 2) * EB.U32 * (xg * xg).sum(-1)], -1)
    ratio = EB.check(st[:n * G_ * 2].view(n, G_, 2), ref, bound, 'groupnorm_stats C=%d' % C)
    assert bool((st[n * G_ * 2 * (1 + nb):] == SENTINEL).all())
    st2 = torch.full_like(st, SENTINEL)
    hip.groupnorm_stats(x, st2, n, P, C, G_)
    assert torch.equal(st, st2)
    _log(stage='groupnorm_stats', C=C, nb=nb, ratio=ratio)


def _lr_pe(hip, biases, n, h, w):
    out = torch.full((n * h * w + TAIL, 20), SENTINEL, device=DEV)
    hip.loftup_lr_pe(biases.to(DEV), out[:n * h * w], 0, n, h, w)
    torch.cuda.synchronize()
    assert bool((out[n * h * w:] == SENTINEL).all())
    return out[:n * h * w].view(n, h * w, 20)


def test_sincos_cw_error():
    """The measurement behind errbound.SINCOS_ABS.  pst_loftup_lr_pe with fp32 output writes sin_cw / cos_cw of a phase the test controls completely through
    h, w and the ten biases per function, with no other arithmetic in between; the phase itself is the restatement's fp32 number (if the kernel's differed
    by an ulp the error would be 1e-3, not 1e-7), the reference float64 sin / cos of it.
    Product range: a 256 x 256 grid, coordinates in [-1, 1] times the five frequencies e^-2 .. e^10, biases in [-pi, pi] (every quadrant), 4 draws.
    Documented limit |x| < 6e4: the same grid with biases up to +-3.79e4, 8 draws (|phase| <= 22027 + 37900).
    Fails if twice the observed error exceeds the allowance, or if the allowance could not tell a phase that is one ulp off (2^-13)."""
    hip = _hip()
    g = torch.Generator().manual_seed(314)
    h = w = 256
    seen = {}
    for name, amp, draws in (('sincos_cw_abs', float(np.pi), 4), ('sincos_cw_abs_limit', 3.79e4, 8)):
        worst, top = 0.0, 0.0
        for _ in range(draws):
            biases = ((torch.rand(2, 2, 5, generator=g) * 2 - 1) * amp).float()
            s_in, c_in = G.lr_pe_inputs(biases, 1, h, w)
            top = max(top, float(np.abs(s_in).max()), float(np.abs(c_in).max()))
            err = (_lr_pe(hip, biases, 1, h, w).double().cpu() - G.features64(s_in, c_in)).abs()
            worst = max(worst, float(err.max()))
        assert top < 6e4 and (top > 5.5e4 or name == 'sincos_cw_abs'), top
        seen[name] = worst
        _log(stage=name, observed=worst, allowance=EB.SINCOS_ABS, max_abs_phase=top)
    print('sincos_cw: %.3g over the product range, %.3g over |x| < 6e4; allowance %.3g' % (seen['sincos_cw_abs'], seen['sincos_cw_abs_limit'], EB.SINCOS_ABS))
    assert EB.SINCOS_ABS < EB.SINCOS_ABS_MAX
    assert 2 * max(seen.values()) <= EB.SINCOS_ABS, seen


@pytest.mark.parametrize('h,w', [(1, 7), (5, 3), (256, 3)])
def test_lr_pe(h, w):
    hip = _hip()
    n = 3
    biases = torch.randn(2, 2, 5, generator=torch.Generator().manual_seed(h))
    s_in, c_in = G.lr_pe_inputs(biases, 1, h, w)
    ref = G.features64(s_in, c_in)[0]
    got = _lr_pe(hip, biases, n, h, w)
    ratio = EB.check(got[0], ref, EB.sincos_bound(ref), 'lr_pe %dx%d' % (h, w))
    for k in range(1, n):
        assert torch.equal(got[0], got[k])
    _log(stage='lr_pe', h=h, w=w, ratio=ratio)


def test_ldy_limit():
    """The apply pass stages 64 x (ldy + 8) 16-bit elements in dynamic LDS behind the frequency table and no function attribute raises the kernel's
    limit, so the launcher refuses what exceeds the default 64 KiB per block: 16-bit ldy = 504 and 512.  The largest that fits (496) and fp32 rows at 512
    (no tile) run through the bound.  Only requests within the device's own per-block limit are launched."""
    hip = _hip()
    shape = (16, 24, 2)
    H, W, n = shape
    P, CH = (H // 2) * (W // 2), 10 * G.NF + 3
    case, r, ref, bound, stats, sb = _case(shape)
    for ldy in (504, 512):
        with pytest.raises(RuntimeError, match=r'ldy=%d needs \d+ bytes of LDS, over the limit of 65536' % ldy):
            _run(hip, case, torch.bfloat16, ldy)
    with pytest.raises(RuntimeError, match='bad argument'):
        _run(hip, case, torch.float32, 520)
    request = ((G.NF + 4 + 3) & ~3) * 4 + 64 * (496 + 8) * 2
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    assert request <= 65536 <= limit, (request, limit)
    feat = G.features64(r['s_in'], r['c_in'], r['col'])
    for dtype in (torch.bfloat16, torch.float16):
        buf, st, _ = _run(hip, case, dtype, 496)
        _check_layout(buf, n, P, CH)
        ref16, bound16 = EB.guidance_bound(feat, case['gamma'], case['beta'], EPS, G.NF, out_fmt=dtype)[:2]
        EB.check(buf[:n * P, :CH].float(), ref16, bound16, 'guidance_gn %s ldy=496' % dtype)
    buf, st, _ = _run(hip, case, torch.float32, 512)
    _check_layout(buf, n, P, CH)
    EB.check(buf[:n * P, :CH], ref, bound, 'guidance_gn fp32 ldy=512')
    b496, _, _ = _run(hip, case, torch.float16, 496)
    assert torch.equal(b496[:n * P].view(torch.int16), buf[:n * P, :496].half().view(torch.int16))
