"""The numpy restatement of the depth evaluation (tests/depth_eval_ref.py) held to closed forms: the yardstick of tests/test_hip_depth_eval.py must itself
be right.  No GPU."""
import math

import numpy as np
import pytest

import depth_eval_ref as D

F32 = np.float32
TH = (1.03, 1.25, 1.25 ** 2, 1.25 ** 3)


def dyadic(shape, seed):
    """depths k / 8 in [1, 9): every sum and product below is exact in float64"""
    r = np.random.Generator(np.random.PCG64(seed))
    return (r.integers(8, 72, shape) / 8.0).astype(F32)


def test_half_scale_is_recovered_exactly_by_the_median():
    gt = [dyadic((7, 9), 1), dyadic((5, 12), 2)]
    pred = [g / F32(2) for g in gt]
    for scope in ('view', 'scene'):
        out = D.depth_quality(pred, gt, align='median', scope=scope, thresholds=TH)
        for row in out['slabs']:
            assert row['scale'] == 2.0 and row['shift'] == 0.0 and row['median_gt'] == 2.0 * row['median_pred']
            assert row['abs_rel'] == row['sq_rel'] == row['rmse'] == row['mae'] == 0.0 and row['delta'] == (1.0,) * 4
        assert out['abs_rel'] == 0.0 and out['delta'] == (1.0,) * 4 and out['n_valid'] == 63 + 60
    assert D.depth_quality(pred, gt, align='median', scope='view')['pooled']['n_valid'] == 123


def test_abs_rel_of_a_known_factor():
    gt = [dyadic((6, 11), 3)]
    out = D.depth_quality([gt[0] * F32(1.5)], gt, align='none', scope='scene', thresholds=TH)
    assert out['abs_rel'] == 0.5
    assert out['slabs'][0]['scale'] == 1.0 and out['delta'] == (0.0, 0.0, 1.0, 1.0)             # 1.5 is between 1.25 and 1.25^2
    assert out['mae'] == float(np.mean(gt[0].astype(np.float64) * 0.5))
    out = D.depth_quality([gt[0] * F32(1.5)], gt, align=1.0 / 1.5, scope='scene')
    assert out['abs_rel'] < 1e-15
    out = D.depth_quality([gt[0] * F32(1.5)], gt, align='scale', scope='scene')
    assert out['slabs'][0]['scale'] == pytest.approx(1 / 1.5, rel=1e-15) and out['abs_rel'] < 1e-15


def test_scale_and_shift_are_recovered_exactly():
    gt = [dyadic((9, 8), 4)]
    pred = [(gt[0] - F32(0.5)) / F32(2)]
    out = D.depth_quality(pred, gt, align='scale_shift', scope='view', thresholds=TH)
    row = out['slabs'][0]
    assert (row['scale'], row['shift']) == (2.0, 0.5) and row['rmse'] == 0.0 and row['delta'] == (1.0,) * 4
    assert out['align_moments'][0, 0] == 72 and out['align_moments'][0, 2] == float(gt[0].astype(np.float64).sum())
    # a constant prediction has no least-squares line: None, not an exception
    out = D.depth_quality([np.full((9, 8), 2, dtype=F32)], gt, align='scale_shift', scope='view')
    assert out['slabs'][0]['abs_rel'] is None and out['slabs'][0]['n_valid'] == 72 and out['abs_rel'] is None


def test_median_of_odd_and_even_counts():
    assert D.median32([3, 1, 2]) == 2 and D.median32([4, 1, 3, 2]) == F32(2.5) and np.isnan(D.median32([]))
    a, b = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    assert D.median32([a, b]) in (a, b)                                          # (a + b) * 0.5f rounds to one of them in fp32
    gt = [np.array([[1, 2, 4, 8, 0]], dtype=F32)]
    pred = [np.array([[1, 1, 1, 1, 1]], dtype=F32)]
    row = D.depth_quality(pred, gt, align='median', scope='view')['slabs'][0]     # the hole leaves an even count
    assert row['n_valid'] == 4 and row['median_gt'] == 3.0 and row['median_pred'] == 1.0 and row['scale'] == 3.0
    gt[0][0, 4] = 16
    row = D.depth_quality(pred, gt, align='median', scope='view')['slabs'][0]
    assert row['n_valid'] == 5 and row['median_gt'] == 4.0


def test_a_pixel_on_the_threshold_is_no_inlier():
    below = np.nextafter(F32(1.25), F32(0))
    gt = [np.ones((1, 4), dtype=F32)]
    pred = [np.array([[1.25, below, 1 / 1.25, 1.0]], dtype=F32)]
    out = D.depth_quality(pred, gt, align='none', scope='view', thresholds=(1.25,))
    assert out['moments'][0, 5] == 2.0 + (1.0 if 1.25 * float(F32(1 / 1.25)) > 1.0 else 0.0) and out['slabs'][0]['n_valid'] == 4
    flags = D.error_terms(pred[0].reshape(-1), gt[0].reshape(-1), np.ones(4, bool), 1.0, 0.0, (1.25,))[5]
    assert flags[0] == 0.0 and flags[1] == 1.0 and flags[3] == 1.0
    # a non-positive aligned depth fails by itself
    f = D.error_terms(np.array([1.0], dtype=F32), np.array([1.0], dtype=F32), np.ones(1, bool), 1.0, -1.5, (1e30,))
    assert f[5, 0] == 0.0 and f[1, 0] == 1.5


def test_validity():
    g = np.array([1, 0, -1, np.inf, np.nan, 5, 5.0000005, 2, 2, 2, 2, 2, 2, 2], dtype=F32)
    p = np.array([1, 1, 1, 1, 1, 1, 1, np.nan, np.inf, -np.inf, 0, -2, 1, 1], dtype=F32)
    c = np.array([3] * 12 + [np.nan, 2.9999], dtype=F32)
    ok = D.valid(p, g, c, 3.0, 0.0, 5.0)
    assert ok.tolist() == [True] + [False] * 4 + [True] + [False] * 8
    assert D.valid(p, g, c, None, 0.0, 5.0).tolist() == [True] + [False] * 4 + [True] + [False] * 6 + [True, True]
    assert not D.valid(p[:1], g[:1], None, None, 1.0, 5.0)[0]                    # min_depth itself is outside


@pytest.mark.parametrize('n', [1, 255, 4097, 256 * 4096 + 4097])
def test_the_fixed_order_is_a_sum(n):
    r = np.random.Generator(np.random.PCG64(n))
    v = r.uniform(0.0, 3.0, n) * 10.0 ** r.integers(-3, 4, n)
    got, want = D.slab_sum([v]), math.fsum(v)
    assert abs(got - want) <= n * 2.0 ** -53 * math.fsum(np.abs(v))
    if n == 4097:                                                                # two views in a slab are not one view of their pixels: blocks do not straddle views
        assert len(D.view_partials(v)) == 2 and len(np.concatenate([D.view_partials(v[:5]), D.view_partials(v[5:])])) == 2
        parts = D.slab_sum([v[:5], v[5:]])
        assert abs(parts - want) <= n * 2.0 ** -53 * math.fsum(np.abs(v))


def test_an_all_invalid_slab_is_none_and_left_out():
    pred, gt, conf = D.random_views([(9, 13), (8, 8), (11, 7)], seed=5)
    gt[1][:] = 0
    for align in D.ALIGNS + (2.5,):
        out = D.depth_quality(pred, gt, conf=conf, min_conf_thr=1.0, align=align, scope='view', thresholds=TH)
        empty, rest = out['slabs'][1], [out['slabs'][0], out['slabs'][2]]
        assert empty['n_valid'] == 0 and all(empty[k] is None for k in D.METRICS + ('delta', 'scale', 'shift', 'median_pred'))
        assert all(r['n_valid'] > 20 and r['abs_rel'] is not None for r in rest)
        assert out['abs_rel'] == (rest[0]['abs_rel'] + rest[1]['abs_rel']) / 2 and out['pooled']['n_valid'] == out['n_valid']
        scene = D.depth_quality(pred, gt, conf=conf, min_conf_thr=1.0, align=align, scope='scene', thresholds=TH)
        assert scene['n_valid'] == out['n_valid'] and scene['abs_rel'] is not None
    gt[0][:], gt[2][:] = 0, 0
    out = D.depth_quality(pred, gt, align='median', scope='scene')
    assert out['abs_rel'] is None and out['n_valid'] == 0
    out = D.depth_quality(pred, gt, align='none', scope='view')
    assert out['abs_rel'] is None and out['delta'] is None and out['pooled']['abs_rel'] is None


def test_scene_scope_pools_the_views():
    """two views at different scales: per view the median alignment is exact, for the scene it cannot be"""
    gt = [dyadic((8, 8), 6), dyadic((8, 8), 7)]
    pred = [gt[0] / F32(2), gt[1] / F32(4)]
    view = D.depth_quality(pred, gt, align='median', scope='view')
    scene = D.depth_quality(pred, gt, align='median', scope='scene')
    assert view['abs_rel'] == 0.0 and [r['scale'] for r in view['slabs']] == [2.0, 4.0]
    assert scene['abs_rel'] > 0.1 and len(scene['slabs']) == 1 and scene['n_valid'] == 128
    assert scene['slabs'][0]['median_gt'] == float(D.median32(np.concatenate([g.reshape(-1) for g in gt])))


def test_the_engine_refuses_before_it_touches_a_device():
    import torch
    from panst3r_amd.engine import depth_quality
    p, g = [torch.ones(4, 5)], [torch.ones(4, 5)]
    for bad in (dict(align='mean'), dict(scope='slab'), dict(thresholds=(1.0,)), dict(min_depth=-1.0), dict(max_depth=0.0)):
        with pytest.raises(ValueError):
            depth_quality(p, g, **bad)
    with pytest.raises(ValueError):
        depth_quality(p, g + g)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        depth_quality(p, g)


def test_the_library_refuses_a_bad_table_without_a_device():
    """the refusals are decided on the host copy of the view table, before any launch: they need no GPU"""
    from panst3r_amd import hip
    from panst3r_amd.build import build
    build(verbose=False)
    L = hip.lib()
    fake = 4096                                                                  # an address that is never read
    good = np.array([[fake, 1, fake, 0, 4097, 0, 0, 0], [fake, 3, fake, fake, 5, 2, 1, 0]], dtype=np.int64)

    def moments(h, nviews=2, nblocks=3, nslabs=2, views=fake, out=fake):
        return L.pst_depth_moments(views, h.ctypes.data, nviews, nblocks, fake, nslabs, 0.0, 9.0, 1.0, fake, out, None)

    def changed(v, word, val):
        h = good.copy()
        h[v, word] = val
        return h
    bad = [changed(0, 0, 0), changed(1, 2, 0), changed(0, 1, 0), changed(1, 1, -3), changed(1, 4, 0), changed(1, 5, 1), changed(1, 6, 0), changed(0, 6, 1),
           changed(1, 6, 2), changed(1, 4, 2 ** 31)]
    assert [moments(h) for h in bad] == [-1] * len(bad)
    assert moments(good, nblocks=2) == moments(good, nblocks=4) == moments(good, nslabs=0) == moments(good, nviews=0) == -1
    assert moments(good, views=None) == moments(good, out=None) == -1
    big = np.array([[fake, 1, fake, 0, 2 ** 30, 0, 0, 0], [fake, 1, fake, 0, 2 ** 30, 2 ** 18, 1, 0]], dtype=np.int64)
    assert moments(big, nblocks=2 ** 19) == -1 and b'2^31' in L.pst_last_error()
    assert L.pst_depth_errors(fake, good.ctypes.data, 2, 3, fake, 2, 0.0, 9.0, 1.0, fake, 5, 1.1, 1.2, 1.3, 1.4, fake, fake, None) == -1
    assert b'thresholds' in L.pst_last_error()
    assert L.pst_depth_median(fake, good.ctypes.data, 2, 3, 2, 0.0, 9.0, 1.0, fake + 4, fake, fake, fake, fake, None) == -1


def test_the_library_refuses_a_negative_or_nan_lower_bound_without_a_device():
    """a valid g is > min_depth; the median's bit order needs g > 0, so the three entry points refuse min_depth < 0 and NaN themselves, not only
    the Python entry point; -0.0 is 0 and is accepted as far as the next refusal (a null output)"""
    from panst3r_amd import hip
    from panst3r_amd.build import build
    build(verbose=False)
    L = hip.lib()
    fake = 4096
    good = np.array([[fake, 1, fake, 0, 4097, 0, 0, 0], [fake, 3, fake, fake, 5, 2, 1, 0]], dtype=np.int64)
    h = good.ctypes.data
    for lo in (-1.0, -1e-45, float('-inf'), float('nan')):
        for rc in (L.pst_depth_moments(fake, h, 2, 3, fake, 2, lo, 9.0, 1.0, fake, fake, None),
                   L.pst_depth_errors(fake, h, 2, 3, fake, 2, lo, 9.0, 1.0, fake, 2, 1.1, 1.2, 1.3, 1.4, fake, fake, None),
                   L.pst_depth_median(fake, h, 2, 3, 2, lo, 9.0, 1.0, fake, fake, fake, fake, fake, None)):
            assert rc == -1 and b'min_depth' in L.pst_last_error(), lo
    assert L.pst_depth_moments(fake, h, 2, 3, fake, 2, -0.0, 9.0, 1.0, fake, None, None) == -1 and b'null operand' in L.pst_last_error()
