"""attention.hip's range check by tile sums (DESIGN s4) where it can go wrong: planted keys that trip a tile's sum, overflow the 16-bit P, move the reference
tile after tile, arrive behind a masked tile or inside the second key split - every output element held to tests/errbound.py, and the bits of a row held
independent of what another row of its wave did.

Shapes: H = 2, Nq = 40, Nk = 256 (four full tiles) and 193 (three full tiles and a one-key tail), head dim 64 and 96, prescaled or not, both 16-bit formats.
`big`: the same problem 128 times in one launch (batch stride 0 on the operands), which makes the dispatch rule pick the 128-query kernel with two query
fragments per wave (rows 0-15 | 16-31 in wave 0, rows 32-39 | none in wave 1, two waves without rows); every batch must then repeat batch 0 bit for bit.
"""
import numpy as np
import pytest
import torch

import test_hip_ops as T
from test_hip_ops import check_attention, dev, rn

pytestmark = pytest.mark.gpu

H, NQ = 2, 40


@pytest.fixture(autouse=True, params=['bf16', 'f16'])
def fmt(request):
    """check_attention takes the 16-bit format from test_hip_ops.d16(): set it as that module's own fixture does"""
    T._D16[0] = torch.bfloat16 if request.param == 'bf16' else torch.float16
    yield request.param
    T._D16[0] = torch.bfloat16


def c_exp(hd, pre):
    """score units -> exp2 domain (a prescaled q carries the factor already)"""
    from panst3r_amd import hip
    return 1.0 if pre else hd ** -0.5 * hip.LOG2E


def operands(seed, Nk, hd, pre):
    from panst3r_amd import hip
    q = T.bf(rn(seed, 1, H, NQ, hd) * (hd ** -0.5 * hip.LOG2E if pre else 1.0))
    return q, T.bf(rn(seed + 1, 1, H, Nk, hd)), T.bf(rn(seed + 2, 1, H, Nk, hd))


def scores2(q, k, h, row, hd, pre):
    """the row's scores in the exp2 domain, float64, of the rounded operands"""
    return (k[0, h].double() @ q[0, h, row].double()) * c_exp(hd, pre)


def plant(q, k, h, row, keys, target, hd, pre):
    """k[key] = q[row] * gain (as test_hip_ops.plant_keys does), the gain chosen so that the row scores `target` (exp2 domain) on the key"""
    qr = q[0, h, row].double()
    gain = target / (float(qr @ qr) * c_exp(hd, pre))
    k[0, h, keys] = (qr * gain).to(k.dtype)


def tile_max(q, k, h, row, tile, hd, pre, Nk):
    return float(scores2(q, k, h, row, hd, pre)[tile * 64:min(tile * 64 + 64, Nk)].max())


def launch(q, k, v, Nk, hd, pre, big, mask=None, nsplit=None):
    """-> O [B, H, Nq, hd] on the device; B = 128 launches of the same operands when big"""
    from panst3r_amd import hip
    B, D = (128 if big else 1), H * hd
    qd = q[0].permute(1, 0, 2).reshape(NQ, D).contiguous().to(dev())
    kd = k[0].permute(1, 0, 2).reshape(Nk, D).contiguous().to(dev())
    vt = torch.zeros(D, (Nk + 7) // 8 * 8 + 8, dtype=T.d16())
    vt[:, :Nk] = v[0].permute(0, 2, 1).reshape(D, Nk)
    vt = vt.to(dev())
    md, ms = None, (0, 0)
    if mask is not None:
        Nkm = (Nk + 3) // 4 * 4
        mm = torch.zeros(NQ, Nkm, dtype=torch.uint8)
        mm[:, :Nk] = mask[0].to(torch.uint8)
        md, ms = mm.to(dev()), (0, Nkm)
    od = torch.full((B, NQ, D), float('nan'), dtype=T.d16(), device=dev())
    args = (qd, kd, vt, od, B, H, NQ, Nk, hd, (0, hd, D), (0, hd, D), (0, hd * vt.stride(0), vt.stride(0)), (NQ * D, hd, D))
    kw = dict(mask=md, mask_strides=ms, nsplit=nsplit, prescaled=pre)
    hip.attention(*args, **kw)
    if big and nsplit is None:
        assert hip._variant('pst_attn_variant', '', hip._attn_params(*args, **kw)[0]).endswith(',2>')        # two query fragments per wave
    return od.reshape(B, NQ, H, hd).permute(0, 2, 1, 3), (args, kw)


def check(o, q, k, v, mask, pre, nsplit, what):
    """batch 0 within the bound; every other batch (the same operands) equal to it bit for bit"""
    r = check_attention(o[:1], q, k, v, mask, pre, nsplit, what)
    assert torch.equal(o, o[:1].expand_as(o)), what + ': batches of identical operands differ'
    return r


SHAPES = pytest.mark.parametrize('Nk,hd,pre,big', [(Nk, hd, pre, big) for Nk in (256, 193) for hd in (64, 96) for pre in (False, True) for big in (False, True)])


def planted_problem(Nk, hd, pre, spike=20.0):
    """Head 0: rows 3 / 5 / 7 / 9 / 35 meet one key in tile 2 at reference + 7.5 / 8.5 / 20 / 60 / 20 and row 11 all 64 keys of tile 1 at reference + 3.
    Head 1: row 7's first tile scores about -60; row 13 climbs 10 per tile; rows 2 and 18 (one wave, two query fragments) trip in tiles 1 and 2.
    The reference of a row is the maximum of its first tile: the planted keys all lie in later tiles and leave it alone.
    -> q, k, v and {(head, row): [(key, offset above the reference)]} for the setup's own check."""
    q, k, v = operands(5000 + Nk + hd, Nk, hd, pre)
    want = {}
    # head 1 first: the -60 tile changes tile 0 itself
    qr = q[0, 1, 7].double()
    k[0, 1, :64] = (k[0, 1, :64].double() - qr * (60.0 / (float(qr @ qr) * c_exp(hd, pre)))).to(k.dtype)
    ref = lambda h, row: tile_max(q, k, h, row, 0, hd, pre, Nk)
    for row, key, off in ((3, 133, 7.5), (5, 130, 8.5), (7, 140, spike), (9, 150, 60.0), (35, 160, 20.0)):
        plant(q, k, 0, row, key, ref(0, row) + off, hd, pre)
        want[(0, row)] = [(key, off)]
    plant(q, k, 0, 11, slice(64, 128), ref(0, 11) + 3.0, hd, pre)
    want[(0, 11)] = [(key, 3.0) for key in range(64, 128)]
    stairs = [(min(64 * t + 7, Nk - 1), 10.0 * t) for t in range(1, (Nk + 63) // 64)]
    for key, off in stairs:
        plant(q, k, 1, 13, key, ref(1, 13) + off, hd, pre)
    want[(1, 13)] = stairs
    plant(q, k, 1, 2, 84, ref(1, 2) + 20.0, hd, pre)
    plant(q, k, 1, 18, 148, ref(1, 18) + 20.0, hd, pre)
    want[(1, 2)], want[(1, 18)] = [(84, 20.0)], [(148, 20.0)]
    # the setup did what it says (16-bit rounding of the planted keys moves a score by a few hundredths)
    for (h, row), lst in want.items():
        s = scores2(q, k, h, row, hd, pre)
        r0 = float(s[:64].max())
        for key, off in lst:
            assert abs(float(s[key]) - r0 - off) < 0.4, (h, row, key, float(s[key]) - r0, off)
    s = scores2(q, k, 1, 7, hd, pre)
    assert float(s[:64].max()) < -40.0 and float(s[64:].max()) > -5.0
    return q, k, v


@SHAPES
def test_planted_rows_meet_the_bound(Nk, hd, pre, big):
    """cases 1 - 5 and 8 in one launch: + 7.5 (no P above 2^8), + 8.5 / + 20 / + 60 (a 16-bit P of the old reference overflows: outputs stay finite), the
    plateau whose sum trips although no P does, the staircase that recomputes every tile, the first tile at -60, two rows of one wave tripping in different
    tiles"""
    q, k, v = planted_problem(Nk, hd, pre)
    o, _ = launch(q, k, v, Nk, hd, pre, big)
    r = check(o, q, k, v, None, pre, 1, 'attention tile-sum planted Nk=%d hd=%d' % (Nk, hd))
    print('err / bound = %.3f' % r)


@SHAPES
def test_masked_first_tile_then_spike(Nk, hd, pre, big):
    """case 6: row 4's first tile is fully masked and a later tile carries a + 20 key; row 6 is fully masked (zeros); row 8 keeps one key"""
    q, k, v = operands(5100 + Nk + hd, Nk, hd, pre)
    mask = torch.zeros(1, NQ, Nk, dtype=torch.bool)
    mask[0, 4, :64] = True
    mask[0, 6] = True
    mask[0, 8] = True
    mask[0, 8, Nk - 1] = False
    plant(q, k, 0, 4, 135, tile_max(q, k, 0, 4, 1, hd, pre, Nk) + 20.0, hd, pre)
    plant(q, k, 1, 4, 135, tile_max(q, k, 1, 4, 1, hd, pre, Nk) + 20.0, hd, pre)
    o, _ = launch(q, k, v, Nk, hd, pre, big, mask=mask)
    check(o, q, k, v, mask, pre, 1, 'attention tile-sum masked')
    assert float(o[:, :, 6].float().abs().max()) == 0.0


@pytest.mark.parametrize('hd,pre,big', [(hd, pre, big) for hd in (64, 96) for pre in (False, True) for big in (False, True)])
def test_spike_inside_the_second_split(hd, pre, big):
    """case 7: nsplit = 2 at Nk = 256 (tiles 0 1 | 2 3); row 5's + 20 key (above the maximum of tile 2, its split's first) lies in tile 3, row 9's + 60 key in
    tile 1: each split trips on its own and the combine merges the (reference, sum) pairs the splits really used"""
    Nk = 256
    q, k, v = operands(5200 + hd, Nk, hd, pre)
    for h in range(H):
        plant(q, k, h, 5, 200, tile_max(q, k, h, 5, 2, hd, pre, Nk) + 20.0, hd, pre)
        plant(q, k, h, 9, 100, tile_max(q, k, h, 9, 0, hd, pre, Nk) + 60.0, hd, pre)
    o, _ = launch(q, k, v, Nk, hd, pre, big, nsplit=2)
    check(o, q, k, v, None, pre, 2, 'attention tile-sum split-K')
    o1, _ = launch(q, k, v, Nk, hd, pre, big)
    check(o1, q, k, v, None, pre, 1, 'attention tile-sum unsplit')


@SHAPES
@pytest.mark.parametrize('spike', [8.5, 20.0, 60.0])
def test_rows_do_not_depend_on_their_wave(Nk, hd, pre, big, spike):
    """case 9, bitwise: row 7 of head 0 trips tile 2 (and rows 3, 5, 9, 11 their own tiles), so its whole wave computes those tiles twice.  The second launch
    differs in the QUERY of the tripping rows only - K and V are the same, so no other row's scores change (taking the planted key out of K instead would
    change every row's scores and, rightly, its output) - and every other row must come out bit for bit the same, whichever path its wave took."""
    q, k, v = planted_problem(Nk, hd, pre, spike)
    o, _ = launch(q, k, v, Nk, hd, pre, big)
    check(o, q, k, v, None, pre, 1, 'attention tile-sum independence')
    q2 = q.clone()
    moved = [3, 5, 7, 9, 11, 35]
    q2[0, 0, moved] = operands(5300, Nk, hd, pre)[0][0, 0, moved]
    o2, _ = launch(q2, k, v, Nk, hd, pre, big)
    keep = [r for r in range(NQ) if r not in moved]
    assert torch.equal(o[:, 0, keep], o2[:, 0, keep])
    assert torch.equal(o[:, 1], o2[:, 1])
    assert not torch.equal(o[:, 0, moved], o2[:, 0, moved])


@pytest.mark.parametrize('hd', [64, 96])
def test_pair_of_tripping_problems_equals_two_launches(hd):
    """case 10: two planted problems (256 and 193 keys) in ONE launch of the two-problem kernel: bit for bit the two single launches"""
    from panst3r_amd import hip
    single, calls = [], []
    for Nk in (256, 193):
        q, k, v = planted_problem(Nk, hd, True)
        o, call = launch(q, k, v, Nk, hd, True, True)
        check(o, q, k, v, None, True, 1, 'attention tile-sum pair (single launch)')
        single.append(o)
        calls.append(call)
    outs = [torch.full_like(calls[i][0][3], float('nan')) for i in range(2)]
    pair = [((a[:3] + (outs[i],) + a[4:]), kw) for i, (a, kw) in enumerate(calls)]
    hip.TIMER = hip.KernelTimer()
    try:
        hip.attention_pair(*pair)
        names = [r[0] for r in hip.TIMER.records]
    finally:
        hip.TIMER = None
    assert len(names) == 1 and names[0].startswith('attn2_kernel'), names
    for i in range(2):
        got = outs[i].reshape(128, NQ, H, hd).permute(0, 2, 1, 3)
        assert torch.equal(got, single[i])
