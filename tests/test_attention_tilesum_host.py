"""A numpy model of attention.hip's range check by tile sums (DESIGN s4), one query row at a time, held to tests/errbound.py on the CPU.

The rule: the first tile of a key range and a ragged last tile are "checked" (row maximum; the reference moves when the row is virgin or the maximum lies
more than 2^8 above it).  Every other tile is "fast": P = exp2(S - m) rounded to 16 bit with the OLD reference, the tile's sum of the rounded P is compared
with 2^8, and the tile is committed as it is unless the sum trips (> 2^8, inf, NaN).  A tripped tile is computed again on the checked path, where the row
also takes the tile's maximum as its reference whenever that maximum lies above the old one.

Scores are exact here: q is the first unit vector and the operands are prescaled, so S_j = k[j, 0] (an f16 value, exp2 domain) - the model and the float64
reference see the same scores and every deviation is the rule's.
"""
import numpy as np
import pytest
import torch

import errbound as EB

KT, HD = 64, 64


def model_row(s, v, fmt=np.float16):
    """s [Nk] float32 scores (exp2 domain), v [Nk, hd] float32 -> (O [hd] float32, recomputed tiles, largest committed P, smallest running P_max)"""
    m, virgin = np.float32(0), True
    l, o = np.float32(0), np.zeros(v.shape[1], np.float32)
    recomputed, p_hi, p_max_run, p_max_lo = 0, 0.0, 0.0, np.inf
    ntiles = (len(s) + KT - 1) // KT
    for t in range(ntiles):
        st, vt = s[t * KT:(t + 1) * KT], v[t * KT:(t + 1) * KT]
        fast = t > 0 and len(st) == KT
        trip = False
        if fast:
            with np.errstate(over='ignore'):
                p = np.exp2(st - m).astype(np.float32).astype(fmt).astype(np.float32)
                tsum = np.float32(p.sum(dtype=np.float32))
            if tsum <= 256.0:
                l, o = np.float32(l + tsum), o + p @ vt
                p_hi, p_max_run = max(p_hi, float(p.max())), max(p_max_run, float(p.max()))
                p_max_lo = min(p_max_lo, p_max_run)
                continue
            trip, recomputed = True, recomputed + 1
        mx = np.float32((st - m).max())
        need = True if virgin else bool(mx > 8.0 or (trip and mx > 0.0))
        if need:
            alpha = np.float32(1) if virgin else np.exp2(-mx).astype(np.float32)
            m, virgin = np.float32(m + mx), False
            l, o = np.float32(l * alpha), o * alpha
            p_hi, p_max_run = p_hi * float(alpha), p_max_run * float(alpha)
        p = np.exp2(st - m).astype(np.float32).astype(fmt).astype(np.float32)
        l, o = np.float32(l + p.sum(dtype=np.float32)), o + p @ vt
        p_hi, p_max_run = max(p_hi, float(p.max())), max(p_max_run, float(p.max()))
        p_max_lo = min(p_max_lo, p_max_run)
    return (o / l).astype(np.float32), recomputed, p_hi, p_max_lo


def rows():
    """the seven score rows: name -> (scores, expected recomputed tiles or None where it depends on the draw)"""
    g = np.random.Generator(np.random.PCG64(77))
    base = lambda n, sd=1.4: g.standard_normal(n) * sd           # ~ unit-variance logits in the exp2 domain
    out = {}
    out['near-uniform'] = (base(512, 0.3), 0)
    s = base(512); s[0] = 4.0; s[1:64] = np.minimum(s[1:64], 3.5); s[150] = 4.0 + 7.5           # reference 4 (tile 0's maximum)
    out['spike +7.5'] = (s, None)                                    # 2^7.5 = 181 plus the rest of its tile: either route is correct
    s = base(512); s[0] = 4.0; s[1:64] = np.minimum(s[1:64], 3.5); s[150] = 64.0
    out['spike +60'] = (s, 1)
    s = base(256); s[0] = 4.0; s[1:64] = np.minimum(s[1:64], 3.5); s[64:128] = 7.0
    out['plateau +3'] = (s, 1)                                       # 64 x 2^3 = 512 > 2^8 although no P exceeds 2^8
    s = base(384, 0.5)
    for t in range(6):
        s[t * KT + 9] = 3.0 + 10.0 * t
    out['staircase +10'] = (s, 5)                                    # every tile after the first is recomputed: twice the tile work, still correct
    s = base(768); s[:64] -= 60.0
    out['first tile -60'] = (s, 1)
    out['sigma 12'] = (base(768, 12.0), None)
    return out


ROWS = rows()


@pytest.mark.parametrize('name', list(ROWS))
def test_tilesum_rule_meets_the_attention_bound(name):
    s64, expect = ROWS[name]
    g = np.random.Generator(np.random.PCG64(78))
    Nk = len(s64)
    k = torch.zeros(1, 1, Nk, HD, dtype=torch.float16)
    k[0, 0, :, 0] = torch.from_numpy(s64).to(torch.float16)
    q = torch.zeros(1, 1, 1, HD, dtype=torch.float16)
    q[0, 0, 0, 0] = 1.0
    v = torch.from_numpy(g.standard_normal((1, 1, Nk, HD))).to(torch.float16)
    out, recomputed, p_hi, p_max_lo = model_row(k[0, 0, :, 0].float().numpy(), v[0, 0].float().numpy())
    print('%s: recomputed %d of %d tiles, largest P %.4g, smallest running P_max %.4g' % (name, recomputed, (Nk + KT - 1) // KT, p_hi, p_max_lo))
    if expect is not None:
        assert recomputed == expect
    # the invariants errbound.attn_bound relies on: the largest P of the row so far is >= 1 (the reference is always a score of the row), every P <= 2^8
    assert p_hi <= 256.0 and p_max_lo >= 1.0
    ref = EB.attn_ref(q, k, v, None, True)
    bound = EB.attn_bound(q, k, v, None, True, torch.float16, torch.float16)
    got = torch.from_numpy(out).to(torch.float16).reshape(1, 1, 1, HD)
    r = EB.check(got, ref, bound, 'tile-sum model: ' + name)
    print('  err / bound = %.3f' % r)


def test_reference_without_the_tripped_rule_keeps_tripping():
    """why a tripped row re-references below the 2^8 threshold: on the plateau row the lazy rule alone (maximum + 3: no move) would leave the reference where
    it is; with the rule the plateau tile is the only one computed twice even when the plateau goes on for three tiles"""
    g = np.random.Generator(np.random.PCG64(79))
    s = (g.standard_normal(320) * 1.4).astype(np.float32)
    s[0] = 4.0; s[1:64] = np.minimum(s[1:64], 3.5); s[64:256] = 7.0
    s = s.astype(np.float16).astype(np.float32)
    v = g.standard_normal((320, HD)).astype(np.float32)
    _, recomputed, p_hi, _ = model_row(s, v)
    assert recomputed == 1 and p_hi <= 256.0
