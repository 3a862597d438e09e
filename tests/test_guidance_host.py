"""The checker of tests/test_hip_guidance.py is checked here, on the CPU (no GPU), as tests/test_pp_stage_checks.py does for the output stages.

(a) tests/guidance_ref.py IS torch's arithmetic: its linspace equals torch.linspace bit for bit for every n up to 256 (odd n, n = 1 and the branch at
    i < n / 2 included), its features equal oracle.panoptic.ImplicitFeaturizer after MinMaxScaler on half_bilinear bit for bit at every shape of the GPU module,
    with and without colour features, with a scale table per view and with one pooled over a chunk of views.
(b) the cases have the properties they were built for (guidance_ref.assert_case).
(c) the comparison bites: against float64 GroupNorm(1) of features64, each of three deliberate mutants of the restatement - the phase with one fused
    rounding, a linspace without the mirrored upper half, the 2x2 mean summed serially - violates errbound.guidance_bound at every shape with P >= 96, while
    the unmutated fp32 features stay inside it.
(d) the perturbation term of the bound is sound: float64 GroupNorm of features moved by +-delta never moves by more than it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import errbound as EB
import guidance_ref as G

EPS = 1e-5


@pytest.mark.parametrize('a,b,ns', [(-1, 1, range(1, 257)), (-2, 10, range(2, 65))], ids=['grid', 'freq'])
def test_linspace_bit_for_bit(a, b, ns):
    for n in ns:
        ref = torch.linspace(a, b, n).numpy()
        got = G.linspace32(a, b, n)
        assert got.dtype == np.float32 and np.array_equal(got, ref), (n, int((got != ref).sum()))
    if a == -1:                                                              # the mirrored half is not decoration: a + i step differs somewhere above the middle
        assert any(not np.array_equal(G.linspace32(a, b, n, mirrored=False), torch.linspace(a, b, n).numpy()) for n in (125, 192, 256))


def _oracle(small, biases, nf, colour):
    from oracle.panoptic import ImplicitFeaturizer
    feat = ImplicitFeaturizer(colour, n_freqs=nf, learn_bias=True)
    with torch.no_grad():
        feat.biases.copy_(biases)
        out = feat(small)
    return out.permute(0, 2, 3, 1).reshape(small.shape[0], -1, out.shape[1])


@pytest.mark.parametrize('shape', G.SHAPES, ids=G.shape_id)
def test_features_equal_oracle(shape):
    """features32 == the oracle's modules, bit for bit: torch.sin / torch.cos of equal fp32 phases are equal whatever the layout (torch's CPU kernels apply
    one vector routine to every element, the tail included), so no fall-back to comparing the phases was needed at any shape."""
    from oracle.panoptic import MinMaxScaler, half_bilinear
    H, W, n = shape
    case = G.make_case(H, W, n)
    small = half_bilinear(case['img'])
    r = G.guidance_inputs(case['img'], case['biases'], G.NF)
    assert np.array_equal(r['img2'], small.numpy())
    G.assert_case(case, r)
    ref = torch.cat([_oracle(MinMaxScaler()(small[i:i + 1]), case['biases'], G.NF, True) for i in range(n)])
    assert torch.equal(G.features32(r['s_in'], r['c_in'], r['col']), ref)
    # a table pooled over the views of a scope == the oracle's scaler over that chunk; a view's own range lies strictly inside the table's
    if n >= 2:
        tab = G.pooled(r['mm'], case['scope'])
        assert ((tab[0, :, 0] < r['mm'][0, :, 0]) | (tab[0, :, 1] > r['mm'][0, :, 1])).all()
        rp = G.guidance_inputs(case['img'], case['biases'], G.NF, mm=tab)
        got = G.features32(rp['s_in'], rp['c_in'], rp['col'])
        for s in set(case['scope']):
            grp = [v for v in range(n) if case['scope'][v] == s]
            assert torch.equal(got[grp], _oracle(MinMaxScaler()(small[grp]), case['biases'], G.NF, True))
    # no colour features: the positional features of an (H2, W2) token grid
    b2 = case['biases'][:, :2, :5].contiguous()
    s_in, c_in = G.lr_pe_inputs(b2, 1, H // 2, W // 2)
    assert torch.equal(G.features32(s_in, c_in), _oracle(torch.zeros(1, 4, H // 2, W // 2), b2, 5, False))


def _gn64(feat, gamma, beta):
    x = feat.double()
    n, P, CH = x.shape
    return F.group_norm(x.permute(0, 2, 1), 1, gamma.double(), beta.double(), EPS).permute(0, 2, 1).reshape(n * P, CH)


BIG = [s for s in G.SHAPES if (s[0] // 2) * (s[1] // 2) >= 96]


@pytest.mark.parametrize('shape', BIG, ids=G.shape_id)
def test_mutants_violate_the_bound(shape):
    H, W, n = shape
    case = G.make_case(H, W, n)
    r = G.guidance_inputs(case['img'], case['biases'], G.NF)
    ref, bound, stats, sb = EB.guidance_bound(G.features64(r['s_in'], r['c_in'], r['col']), case['gamma'], case['beta'], EPS, G.NF)
    assert torch.allclose(ref, _gn64(G.features64(r['s_in'], r['c_in'], r['col']), case['gamma'], case['beta']), rtol=0, atol=1e-12)
    # the restatement itself: torch's fp32 sin / cos of the same phases (<= 1 ulp), GroupNorm in float64
    ok = EB.check(_gn64(G.features32(r['s_in'], r['c_in'], r['col']), case['gamma'], case['beta']), ref, bound, 'restatement %s' % G.shape_id(shape))
    assert ok <= 0.5, ok
    for mutant in ('fused', 'mirrored', 'serial'):
        m = G.guidance_inputs(case['img'], case['biases'], G.NF, **{mutant: mutant != 'mirrored'})
        got = _gn64(G.features64(m['s_in'], m['c_in'], m['col']), case['gamma'], case['beta'])
        nbad = int(((got - ref).abs() > bound).sum())
        print('%s %s: %d of %d elements beyond the bound' % (G.shape_id(shape), mutant, nbad, ref.numel()))
        assert nbad > 0, '%s: the %s mutant stays inside the bound at every one of %d elements' % (G.shape_id(shape), mutant, ref.numel())
        with pytest.raises(AssertionError, match='exceed the error bound'):
            EB.check(got, ref, bound, mutant)


def test_allowance_can_tell_a_phase_ulp():
    assert EB.SINCOS_ABS < EB.SINCOS_ABS_MAX == 2.0 ** -13


@pytest.mark.parametrize('delta', [EB.SINCOS_ABS + EB.U32, 1e-4, 1e-2])
def test_perturbation_term_is_sound(delta):
    """float64 GroupNorm(1) of x + e, |e| <= delta, against that of x: never beyond guidance_perturbation - random signs, random magnitudes, the common
    shift (moves the mean by delta) and the pattern that stretches sigma most (e = delta sign(x - mean))"""
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for P, CH in ((3, 203), (96, 203), (125, 23)):
        for trial in range(6):
            x = torch.cat([torch.sin(40 * torch.randn(1, P, CH - 3, generator=g, dtype=torch.float64)), torch.rand(1, P, 3, generator=g, dtype=torch.float64) - 0.5], -1)
            if trial == 5:
                x = x * 1e-3                                                  # a nearly flat map: sigma comparable with sqrt(eps)
            gamma, beta = 1 + 0.1 * torch.randn(CH, generator=g, dtype=torch.float64), 0.1 * torch.randn(CH, generator=g, dtype=torch.float64)
            mean = x.mean()
            s = (x.var(unbiased=False) + EPS).sqrt()
            term = EB.guidance_perturbation((x - mean) / s, s, gamma.reshape(1, 1, CH), delta).reshape(P, CH)
            ref = _gn64(x, gamma, beta)
            sign = torch.where(torch.rand(x.shape, generator=g) < 0.5, -1.0, 1.0).double()
            for e in (sign * delta, sign * delta * torch.rand(x.shape, generator=g, dtype=torch.float64), torch.full_like(x, delta), -torch.full_like(x, delta),
                      delta * torch.sign(x - mean), -delta * torch.sign(x - mean)):
                d = (_gn64(x + e, gamma, beta) - ref).abs()
                assert bool((d <= term).all()), (P, CH, trial, float((d / term).max()))
                worst = max(worst, float((d / term).max()))
    assert worst > 0.3, worst                                                # and the term is no more than a small factor above what happens
