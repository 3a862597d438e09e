"""The stage checkers of tests/pp_stage_cases.py BITE (CPU only, no GPU), as tests/test_errbound.py shows for the arithmetic bounds.

For every stage of csrc/postprocess.hip and csrc/pointmap.hip: (a) a float32 numpy emulation of the kernel's arithmetic passes its checker at or below half
of every derived bound; (b) the same emulation with ONE planted mistake fails it.  The mistakes: LDS footprint one row / one column short with the clamp in
place, >= for > in the winner rule, kept list walked in reverse, last query of an odd chunk dropped, the valid mask missing from the 0.5 count on a ragged
tile, counters overwritten instead of accumulated, cm / co < thr in fp32, seg_id numbered over all queries, align_corners=True coordinates, the source
coordinate contracted into one fma, a grid-stride loop that stops after one pass, expf(d) - 1 for expm1f(d), Weiszfeld weights 1 / max(d^2, eps), the y x^T
moments transposed.  The module also asserts the decidedness caps (pp_stage_cases.CAP_WINNER / CAP_BAND) for every shape, seed and keep pattern the GPU module
uses, on the float64 reference alone, so the caps are verified where there is no GPU."""
import numpy as np
import pytest
import torch

import errbound as EB
import pp_stage_cases as C

SMALL = [s for s in C.ARGMAX_SHAPES if s[3] * s[4] < 100000]
RAGGED = C.ARGMAX_SHAPES[2]                     # 257 x (40 x 56 -> 75 x 93): ragged tiles, non-dyadic ratio, nk % CH odd with everything kept


def _run(shape, keep, variant=None, seed=0):
    logits, scores = C.make_case(shape, seed)
    return logits, scores, C.emulate_argmax(logits, scores, keep, shape[3], shape[4], variant=variant)


@pytest.mark.parametrize('shape', C.ARGMAX_SHAPES + [C.DOWN4_SHAPE], ids=C.shape_id)
def test_caps_and_emulation_every_pattern(shape):
    """every keep pattern of every shape: the caps hold on the reference; the emulation passes best_q / best_m / counters with best_m at <= half its bound"""
    Q, Hm, Wm, H, W = shape
    logits, scores = C.make_case(shape)
    CH = max(C.fused_geometry(Hm, Wm, H, W)[2], 1)
    for name, keep in C.keep_patterns(Q, CH).items():
        r = C.ref_argmax(logits, scores, keep, H, W)
        C.assert_caps(r, C.shape_id(shape) + ' ' + name)
        if shape == C.DOWN4_SHAPE:
            continue                                            # pp_argmax only: no tile footprint to emulate
        bq, bm, do, dm = C.emulate_argmax(logits, scores, keep, H, W)
        ratio = C.check_best(r, bq, bm, name)
        assert ratio <= 0.5, (name, ratio)
        C.check_counts([r], do, dm, np.zeros(Q), np.zeros(Q), name)
        if name == 'none':
            assert (bq == -1).all() and (bm == 0).all() and not do.any() and not dm.any()


@pytest.mark.parametrize('variant', ['rows_short', 'cols_short', 'drop_odd_last', 'align_corners', 'fma'])
def test_planted_mistake_fails_best(variant):
    # the footprint rule ceil(8 s) + 2 is tight (= floor(7 s) + 3 rows used) at the dyadic ratios, one row generous at 40 -> 75: the 2 x shape for those
    shape = C.ARGMAX_SHAPES[5] if variant in ('rows_short', 'cols_short') else RAGGED
    keep = np.ones(shape[0], np.int32)
    logits, scores, (bq, bm, do, dm) = _run(shape, keep, variant)
    r = C.ref_argmax(logits, scores, keep, shape[3], shape[4])
    with pytest.raises(AssertionError):
        C.check_best(r, bq, bm, variant)


def test_planted_mistake_missing_valid_mask_fails_counts():
    shape = RAGGED
    keep = np.ones(shape[0], np.int32)
    logits, scores, (bq, bm, do, dm) = _run(shape, keep, 'no_valid')
    r = C.ref_argmax(logits, scores, keep, shape[3], shape[4])
    C.check_best(r, bq, bm, 'no_valid')                       # the maps are right: only the 0.5 count sees the pixels beyond the image
    with pytest.raises(AssertionError, match='cnt_orig'):
        C.check_counts([r], do, dm, np.zeros(shape[0]), np.zeros(shape[0]), 'no_valid')


@pytest.mark.parametrize('shape', [C.ARGMAX_SHAPES[0], C.ARGMAX_SHAPES[1]], ids=C.shape_id)
def test_counters_accumulate_over_two_views_and_overwriting_fails(shape):
    """both two-view shapes of the GPU module, seeds 0 and 1: caps, accumulated counters pass, overwritten counters fail"""
    Q, Hm, Wm, H, W = shape
    keep = np.ones(Q, np.int32)
    g = np.random.Generator(np.random.PCG64(5))
    o0, m0 = g.integers(1, 1000, Q), g.integers(1, 1000, Q)
    views = [C.make_case(shape, s) for s in (0, 1)]
    refs = [C.ref_argmax(lg, sc, keep, H, W) for lg, sc in views]
    for r in refs:
        C.assert_caps(r, C.shape_id(shape))
    emu = [C.emulate_argmax(lg, sc, keep, H, W) for lg, sc in views]
    C.check_counts(refs, o0 + emu[0][2] + emu[1][2], m0 + emu[0][3] + emu[1][3], o0, m0, 'accumulated')
    with pytest.raises(AssertionError):
        C.check_counts(refs, emu[1][2], emu[1][3], o0, m0, 'overwritten')


@pytest.mark.parametrize('variant', ['ge', 'reverse'])
@pytest.mark.parametrize('bump', [False, True])
def test_tie_rule(variant, bump):
    """identical planes: the lower id owns an exact tie; one ulp more score hands every pixel to the higher id.  >= and the reversed walk break the exact tie."""
    shape = C.ARGMAX_SHAPES[3]
    Q, Hm, Wm, H, W = shape
    logits, scores, lo, hi = C.tie_case(shape, 0, bump)
    keep = np.ones(Q, np.int32)
    alone = keep.copy(); alone[hi] = 0
    ref_run = C.emulate_argmax(logits, scores, alone, H, W)
    C.check_tie(C.emulate_argmax(logits, scores, keep, H, W), ref_run, lo, hi, bump, 'emulation')
    if not bump:
        with pytest.raises(AssertionError):
            C.check_tie(C.emulate_argmax(logits, scores, keep, H, W, variant=variant), ref_run, lo, hi, bump, variant)


@pytest.mark.parametrize('ncls', C.SCORE_NCLS)
def test_scores_emulation(ncls):
    for Q in C.SCORE_Q:
        x = C.scores_case(Q, ncls, 0)
        for temp in (None, 0.1, 1.0):
            r, nexact = C.check_scores(x, 'sigmoid', 0.5, temp, *C.emulate_scores(x, 'sigmoid', 0.5, temp), 'sigmoid T=%s' % temp)
            assert r <= 0.5 and nexact >= (temp is None), (Q, ncls, temp, r)
        r, _ = C.check_scores(x, 'softmax', 0.3, None, *C.emulate_scores(x, 'softmax', 0.3, None), 'softmax')
        assert r <= 0.5, (Q, ncls, r)
    if ncls <= 7:
        return
    sc, lb, kp = C.emulate_scores(x, 'sigmoid', 0.5, 0.1)
    lb2 = lb.copy(); lb2[1] = 7                              # the higher of two exactly equal maxima
    with pytest.raises(AssertionError):
        C.check_scores(x, 'sigmoid', 0.5, 0.1, sc, lb2, kp, 'higher tie')
    with pytest.raises(AssertionError):
        C.check_scores(x, 'sigmoid', 0.5, 0.1, sc * np.float32(1 + 2e-5), lb, kp, 'temperature applied twice-size error')


@pytest.mark.parametrize('Q', C.SELECT_Q)
@pytest.mark.parametrize('thr', [0.5, 0.8])
def test_select(Q, thr):
    keep, co, cm, plants = C.select_case(Q, thr, 0)
    sel, seg = C.ref_select(keep, co, cm, thr)
    assert [int(s) for s in sel[:len(plants)]] == [p[3] for p in plants]
    C.check_select(keep, co, cm, thr, *C.emulate_select(keep, co, cm, thr), 'emulation')
    if Q >= 255:
        with pytest.raises(AssertionError, match='seg_id'):
            C.check_select(keep, co, cm, thr, *C.emulate_select(keep, co, cm, thr, 'seg_all'), 'seg_all')
        if thr == 0.8:
            with pytest.raises(AssertionError, match='keep_out'):
                C.check_select(keep, co, cm, thr, *C.emulate_select(keep, co, cm, thr, 'fp32_ratio'), 'fp32_ratio')


def test_finalize_reference_edges():
    bq, bm, seg = C.finalize_case(257, 40, 0.25, 0)
    pan, conf = C.ref_finalize(bq, bm, seg, 0.25, 0.1)
    at, below = np.arange(257)[::5], np.arange(257)[1::5]
    assert (pan[below] == 0).all() and (conf[below] == np.float32(0.1)).all()
    ok = bq[at] >= 0
    assert np.array_equal(pan[at][ok], seg[bq[at][ok]]) and (pan[bq == -1] == 0).all()
    assert ((pan == 0) == (conf == np.float32(0.1))).all()


@pytest.mark.parametrize('Q,P', [(17, 257), (16, 384 * 512 // 64), (1, 1)])
def test_overlap_bound(Q, P):
    probs = C.qubo_probs(Q, P, 0)
    S, bound = C.ref_overlap(probs)
    emu = torch.from_numpy(C.emulate_overlap(probs))
    assert EB.check(emu, S, bound, 'overlap') <= 0.5
    if P > 256:
        bad = emu.clone(); bad -= torch.minimum(probs[:, None, -1], probs[None, :, -1]).double()      # the last pixel dropped
        with pytest.raises(AssertionError):
            EB.check(bad, S, bound, 'last pixel dropped')


@pytest.mark.parametrize('npix', [257, 384 * 512, 12 * 384 * 512])
def test_activate_bound(npix):
    raw = C.activate_case(npix, 0)
    p, l, c, bp, bl, bc = C.ref_activate(raw)
    ep, el, ec = C.emulate_activate(raw)
    for got, ref, b, what in ((ep, p, bp, 'pts3d'), (el, l, bl, 'pts3d_local'), (ec, c, bc, 'conf')):
        assert EB.check(torch.from_numpy(got), ref, b, what) <= 0.5, what
    ep, el, ec = C.emulate_activate(raw, 'expf_minus_1')
    with pytest.raises(AssertionError):
        EB.check(torch.from_numpy(ep), p, bp, 'expf(d) - 1')
    if npix > 8192 * 256:
        ep, el, ec = C.emulate_activate(raw, 'one_pass')
        with pytest.raises(AssertionError):
            EB.check(torch.from_numpy(ec), c, bc, 'one pass')


@pytest.mark.parametrize('H,W', C.FOCAL_HW)
def test_focal_bound(H, W):
    loc, pp = C.focal_case(H, W, 2, 0)
    for iters in C.FOCAL_ITERS:
        f, b, L = C.ref_focal(loc, pp, H, W, iters)
        r = EB.check(torch.from_numpy(C.emulate_focal(loc, pp, H, W, iters)), f, b, 'focal iters=%d' % iters)
        assert r <= 0.5, (iters, r)
        if iters:
            with pytest.raises(AssertionError):
                EB.check(torch.from_numpy(C.emulate_focal(loc, pp, H, W, iters, 'weights_sq')), f, b, 'weights 1 / d^2')


@pytest.mark.parametrize('off', [0.0, -1.0])
@pytest.mark.parametrize('V,P', [(1, 1), (1, 35), (50, 35), (1, 1025), (1, 384 * 512)])
def test_moments_bound(V, P, off):
    x, y, conf = C.moments_case(V, P, 0)
    ref, bound = C.ref_moments(x, y, conf, off)
    assert EB.check(torch.from_numpy(C.emulate_moments(x, y, conf, off)), ref, bound, 'moments') <= 0.5
    if P > 1:
        with pytest.raises(AssertionError):
            EB.check(torch.from_numpy(C.emulate_moments(x, y, conf, off, 'transposed')), ref, bound, 'transposed')
    if off == 0.0:                                              # conf + 0 is exact: only the double arithmetic is allowed for
        with pytest.raises(AssertionError):
            EB.check(torch.from_numpy(C.emulate_moments(x, y, conf, off, 'fp32_acc')), ref, bound, 'fp32 products and sums')
