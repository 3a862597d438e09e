"""The depth evaluation on the GPU (csrc/depth_eval.hip, panst3r_amd/engine/depth_eval.py) against the numpy restatement of tests/depth_eval_ref.py:
moments, medians, scales and every reported float BIT FOR BIT - fp64 sums in a fixed order, exact medians and separately rounded operations leave no
tolerance to choose.  The restatement is held to closed forms by tests/test_depth_eval_host.py.  Every case asserts the restatement's count of valid
pixels, so that none passes by scoring nothing."""
import numpy as np
import pytest
import torch

import depth_eval_ref as D
from panst3r_amd import hip
from panst3r_amd.engine import depth_quality
from panst3r_amd.engine.depth_eval import _depth_plane

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
TH = (1.03, 1.25, 1.25 ** 2, 1.25 ** 3)
ALIGNS = D.ALIGNS + (2.4375,)
# 1, 255, 256, 257, 4095, 4096 and 4097 pixels: a lane, a wave short of a row, a row, a row and one, a pixel short of a chunk, a chunk, a chunk and one
EDGES = [(1, 1), (5, 51), (16, 16), (1, 257), (45, 91), (64, 64), (17, 241)]
assert [h * w for h, w in EDGES] == [1, 255, 256, 257, 4095, 4096, 4097]


def dev(maps):
    return None if maps is None else [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in maps]


def raw(x):
    return None if x is None else np.ascontiguousarray(x).view(np.uint8).tobytes()


def assert_same(got, want):
    """every entry of the result, floats by value and type (equal float64 numbers are equal bits: no NaN, no -0 is reported), the moments by bytes"""
    assert set(got) == set(want)
    assert raw(got['moments']) == raw(want['moments']) and raw(got['align_moments']) == raw(want['align_moments'])
    assert len(got['slabs']) == len(want['slabs'])
    for g, w in zip(got['slabs'], want['slabs']):
        assert g == w and all(type(g[k]) is type(w[k]) for k in w), (g, w)
    for k, w in want.items():
        if k not in ('moments', 'align_moments', 'slabs'):
            assert got[k] == w and type(got[k]) is type(w), k


def run_case(case, *, aligns=ALIGNS, scopes=('view', 'scene'), thr=1.0, share=0.5, **kw):
    pred, gt, conf = case
    pd, gd, cd = dev(pred), dev(gt), dev(conf)
    pixels = sum(g.size for g in gt)
    out = []
    for align in aligns:
        for scope in scopes:
            want = D.depth_quality(pred, gt, conf=conf, min_conf_thr=thr if conf is not None else None, align=align, scope=scope, thresholds=TH, **kw)
            assert want['n_valid'] > share * pixels, (want['n_valid'], pixels)
            got = depth_quality(pd, gd, conf=cd, min_conf_thr=thr if conf is not None else None, align=align, scope=scope, thresholds=TH, **kw)
            assert_same(got, want)
            out.append(got)
    return out


@pytest.mark.parametrize('align', ALIGNS, ids=[str(a) for a in ALIGNS])
def test_chunk_edges_in_a_mixed_shape_scene(align):
    """seven views of 1 .. 4097 pixels in one launch per stage, per view and pooled into one slab"""
    case = D.random_views(EDGES, seed=11, holes=0.1, bad=0.05)
    view, scene = run_case(case, aligns=(align,), thr=0.5)
    assert len(view['slabs']) == 7 and len(scene['slabs']) == 1 and scene['n_valid'] == view['n_valid'] == view['pooled']['n_valid']
    if align == 'median':                                                        # 'scene' pools the views into ONE median and one sum
        allp = np.concatenate([p.reshape(-1)[D.valid(p, g, c, 0.5, 0.0, np.inf)] for p, g, c in zip(*case)])
        assert scene['slabs'][0]['median_pred'] == float(D.median32(allp)) and scene['slabs'][0]['median_pred'] != view['slabs'][6]['median_pred']


def test_a_chunk_edge_inside_a_slab_and_a_tiny_slab():
    """4097 and 5 pixels: per view a slab of two blocks and one of five pixels, for the scene three rows of partials"""
    run_case(D.random_views([(17, 241), (1, 5)], seed=12, holes=0.1, bad=0.02), thr=0.2)
    run_case(D.random_views([(1, 5), (17, 241)], seed=13, holes=0.1, bad=0.02, with_conf=False))


def test_the_reducer_runs_twice_and_ends_on_a_partial_row():
    """one slab of 256 * 4096 + 4097 pixels: 258 rows of partials"""
    n = 256 * 4096 + 4097
    assert n == 3 * 350891 and (n + hip.ICP_CHUNK - 1) // hip.ICP_CHUNK == 258
    got = run_case(D.random_views([(3, 350891)], seed=14, with_conf=False), aligns=('median', 'scale_shift'), scopes=('scene',))
    assert got[0]['n_valid'] > n // 2 and got[0]['moments'].shape == (1, hip.DEPTH_MOMENTS)


def test_validity():
    """NaN, +-inf, 0 and negative predictions; gt == 0 holes, gt at max_depth exactly and just above; NaN and sub-threshold confidences; a view without
    a valid pixel, which reports None and is left out of the mean"""
    pred, gt, conf = D.random_views([(24, 32), (9, 13), (23, 31)], seed=15, holes=0.1, bad=0.1)
    gt[0][0, :8] = [7.0, np.nextafter(F32(7.0), F32(8)), np.nextafter(F32(7.0), F32(0)), 0.25, np.nextafter(F32(0.25), F32(1)), np.inf, np.nan, -3.0]
    pred[0][0, :8] = 1.0
    conf[0][0, :8] = 3.0
    conf[0][1, :4] = [0.5, np.nextafter(F32(0.5), F32(0)), np.nan, np.inf]
    pred[0][1, :4], gt[0][1, :4] = 1.0, 2.0
    gt[1][:] = 0                                                                  # view 1 scores nothing
    assert D.valid(pred[0][0, :8], gt[0][0, :8], conf[0][0, :8], 0.5, 0.25, 7.0).tolist() == [True, False, True, False, True, False, False, False]
    assert D.valid(pred[0][1, :4], gt[0][1, :4], conf[0][1, :4], 0.5, 0.25, 7.0).tolist() == [True, False, False, True]
    for got in run_case((pred, gt, conf), thr=0.5, min_depth=0.25, max_depth=7.0):
        if got['scope'] == 'view':
            assert got['slabs'][1]['n_valid'] == 0 and got['slabs'][1]['abs_rel'] is None and got['slabs'][0]['abs_rel'] is not None
            assert got['abs_rel'] == (got['slabs'][0]['abs_rel'] + got['slabs'][2]['abs_rel']) / 2
    # nothing valid anywhere: None for everything, no exception
    gt[0][:], gt[2][:] = 0, 0
    for align in ALIGNS:
        for scope in ('view', 'scene'):
            want = D.depth_quality(pred, gt, align=align, scope=scope, thresholds=TH)
            got = depth_quality(dev(pred), dev(gt), align=align, scope=scope, thresholds=TH)
            assert want['n_valid'] == 0 and want['abs_rel'] is None
            assert raw(got['moments']) == raw(want['moments']) and got['slabs'] == want['slabs'] and got['abs_rel'] is None and got['delta'] is None


def test_a_degenerate_solve_is_none():
    gt = D.random_views([(9, 13)], seed=16, with_conf=False)[1]
    pred = [np.full((9, 13), 2.0, dtype=F32)]                                     # n sum pp - (sum p)^2 == 0: no least-squares line
    want = D.depth_quality(pred, gt, align='scale_shift', scope='view', thresholds=TH)
    got = depth_quality(dev(pred), dev(gt), align='scale_shift', scope='view', thresholds=TH)
    assert want['slabs'][0]['n_valid'] > 60 and want['slabs'][0]['abs_rel'] is None
    assert raw(got['align_moments']) == raw(want['align_moments']) and got['slabs'] == want['slabs'] and got['abs_rel'] is None


def test_a_pointmap_is_read_in_place():
    """component 2 of [1, H, W, 3] at an element stride of 3, and x_out dicts: the bytes of the contiguous z plane"""
    pred, gt, conf = D.random_views([(23, 31), (32, 24)], seed=17)
    r = np.random.Generator(np.random.PCG64(1))
    pts = []
    for p in pred:
        xyz = r.normal(size=p.shape + (3,)).astype(F32)
        xyz[..., 2] = p
        pts.append(torch.from_numpy(xyz[None]).to(DEV))
    z, stride = _depth_plane(pts[0], (23, 31), 0)
    assert stride == 3 and z.data_ptr() == pts[0].data_ptr() + 8                  # no copy
    gd, cd = dev(gt), dev(conf)
    for align in ('median', 'scale_shift'):
        want = D.depth_quality(pred, gt, conf=conf, min_conf_thr=1.0, align=align, scope='view', thresholds=TH)
        assert want['n_valid'] > 0.5 * sum(g.size for g in gt)
        assert_same(depth_quality(pts, gd, conf=cd, min_conf_thr=1.0, align=align, scope='view', thresholds=TH), want)
        x_out = [{'pts3d_local': p, 'conf': c[None], 'pts3d': p} for p, c in zip(pts, cd)]
        assert_same(depth_quality(x_out, gt, min_conf_thr=1.0, align=align, scope='view', thresholds=TH), want)      # ground truth from the host
        # a transposed depth map is not uniformly strided: it is copied, not misread
        assert_same(depth_quality([p.T.contiguous().T for p in dev(pred)], gd, conf=cd, min_conf_thr=1.0, align=align, scope='view', thresholds=TH), want)


def test_views_at_an_odd_element_offset():
    """pred, gt and conf are views one and three elements into larger buffers: 4-byte aligned only"""
    pred, gt, conf = D.random_views([(23, 31), (17, 241)], seed=18)

    def odd(maps, k):
        out = []
        for m in maps:
            buf = torch.zeros(m.size + 8, dtype=torch.float32, device=DEV)
            buf[k:k + m.size] = torch.from_numpy(m.reshape(-1)).to(DEV)
            out.append(buf[k:k + m.size].view(m.shape))
            assert out[-1].data_ptr() % 8 == 4 and out[-1].is_contiguous()
        return out
    for align in ('median', 'scale', 'none'):
        for scope in ('view', 'scene'):
            want = D.depth_quality(pred, gt, conf=conf, min_conf_thr=1.0, align=align, scope=scope, thresholds=TH)
            assert want['n_valid'] > 0.5 * sum(g.size for g in gt)
            assert_same(depth_quality(odd(pred, 1), odd(gt, 3), conf=odd(conf, 1), min_conf_thr=1.0, align=align, scope=scope, thresholds=TH), want)


def test_threshold_equality_is_no_inlier():
    below = np.nextafter(F32(1.25), F32(0))
    gt, pred = [np.ones((1, 4), dtype=F32)], [np.array([[1.25, below, 0.8, 1.0]], dtype=F32)]
    want = D.depth_quality(pred, gt, align='none', scope='view', thresholds=(1.25,))
    got = depth_quality(dev(pred), dev(gt), align='none', scope='view', thresholds=(1.25,))
    assert_same(got, want)
    assert got['n_valid'] == 4 and got['moments'][0, 5] == 3.0 and got['delta'] == (0.75,)      # fp32(0.8) is above 0.8: 1 < 1.25 fp32(0.8)
    got = depth_quality(dev(pred), dev(gt), align='none', scope='view', thresholds=())
    assert got['delta'] == () and got['n_valid'] == 4


def test_two_calls_give_equal_bytes():
    pred, gt, conf = D.random_views([(96, 128), (128, 96), (37, 51)], seed=19)
    pd, gd, cd = dev(pred), dev(gt), dev(conf)
    for align in ALIGNS:
        for scope in ('view', 'scene'):
            a = depth_quality(pd, gd, conf=cd, min_conf_thr=1.0, align=align, scope=scope)
            b = depth_quality(pd, gd, conf=cd, min_conf_thr=1.0, align=align, scope=scope)
            assert a['n_valid'] > 0.5 * sum(g.size for g in gt)
            assert raw(a['moments']) == raw(b['moments']) and raw(a['align_moments']) == raw(b['align_moments']) and a['slabs'] == b['slabs']


def test_model_evaluate_depth_is_the_direct_call():
    from panst3r_amd.panst3r import PanSt3R
    pred, gt, conf = D.random_views([(48, 64), (37, 51)], seed=20)
    x_out = [{'pts3d_local': torch.stack([p, p, p], -1)[None].contiguous(), 'conf': c[None]} for p, c in zip(dev(pred), dev(conf))]
    kw = dict(min_conf_thr=1.0, align='median', scope='scene', thresholds=TH)
    want = D.depth_quality(pred, gt, conf=conf, **kw)
    assert want['n_valid'] > 0.5 * sum(g.size for g in gt)
    assert_same(PanSt3R.evaluate_depth(None, x_out, dev(gt), **kw), want)
    assert_same(depth_quality(x_out, dev(gt), **kw), want)


def test_python_refusals():
    pred, gt, conf = D.random_views([(8, 9), (7, 5)], seed=21)
    pd, gd, cd = dev(pred), dev(gt), dev(conf)
    for bad in (dict(align='mean'), dict(align=True), dict(align=float('nan')), dict(scope='slab'), dict(thresholds=(1.0,)), dict(thresholds=(1.25, 0.5)),
                dict(thresholds=(1.1,) * 5), dict(min_depth=-1.0), dict(max_depth=0.0), dict(min_depth=2.0, max_depth=2.0)):
        with pytest.raises(ValueError):
            depth_quality(pd, gd, **bad)
    for a, b, c in ((pd, gd[:1], None), (pd[:1], gd, None), (pd, gd, cd[:1]), (pd[::-1], gd, None), ([], [], None), (pd, gd, [cd[0], cd[0]])):
        with pytest.raises(ValueError):
            depth_quality(a, b, conf=c, min_conf_thr=1.0)
    with pytest.raises(ValueError):
        depth_quality([p.double() for p in pd], gd)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        depth_quality([p.cpu() for p in pd], gd)


def test_every_library_refusal_returns_without_a_launch():
    """PST_EINVAL, and the outputs keep their sentinel"""
    pred, gt, conf = D.random_views([(17, 241), (9, 13)], seed=22)
    views = [(p, 1, g, c) for p, g, c in zip(dev(pred), dev(gt), dev(conf))]
    t = hip.depth_table(views, [0, 1], DEV)
    L = hip.lib()
    S, nb = t.nslabs, t.nblocks
    assert (S, nb, t.nviews) == (2, 3, 2)
    f64 = dict(dtype=torch.float64, device=DEV)
    partials, out, align = torch.full((nb, hip.DEPTH_MOMENTS), -7.0, **f64), torch.full((S, hip.DEPTH_MOMENTS), -7.0, **f64), torch.ones(S, 2, **f64)
    ws = torch.zeros(S * 1032, dtype=torch.int32, device=DEV)
    count, median = torch.full((S,), -7, dtype=torch.int32, device=DEV), torch.full((S, 2), -7.0, dtype=torch.float32, device=DEV)
    hist, prefix, rank = ws[:S * 1024], ws[S * 1024:S * 1028], ws[S * 1028:]
    st = hip._stream()

    def table(**change):
        h = t.host.copy()
        for k, (v, val) in change.items():
            h[v, {'pred': 0, 'stride': 1, 'gt': 2, 'npix': 4, 'first_block': 5, 'slab': 6}[k]] = val
        return h

    def call(h=None, *, only=(0, 1, 2), views=True, nviews=2, nblocks=nb, nslabs=S, K=4, rows=True, outp=True):
        """moments, errors, median (those of `only`) on the operands above with one thing changed -> their return codes"""
        h = t.host if h is None else h
        hp, vp = h.ctypes.data, (t.dev.data_ptr() if views else None)
        sr, o = (t.slab_rows.data_ptr() if rows else None), (out.data_ptr() if outp else None)
        fns = (lambda: L.pst_depth_moments(vp, hp, nviews, nblocks, sr, nslabs, 0.0, 9.0, 1.0, partials.data_ptr(), o, st),
               lambda: L.pst_depth_errors(vp, hp, nviews, nblocks, sr, nslabs, 0.0, 9.0, 1.0, align.data_ptr(), K, 1.1, 1.2, 1.3, 1.4, partials.data_ptr(), o, st),
               lambda: L.pst_depth_median(vp, hp, nviews, nblocks, nslabs, 0.0, 9.0, 1.0, hist.data_ptr(), prefix.data_ptr(), rank.data_ptr(), count.data_ptr(),
                                          median.data_ptr() if outp else None, st))
        return tuple(fns[i]() for i in only)
    EINVAL = (-1, -1, -1)
    assert call(views=False) == EINVAL and call(rows=False, only=(0, 1)) == (-1, -1) and call(outp=False) == EINVAL          # null operands
    assert L.pst_depth_moments(t.dev.data_ptr(), None, 2, nb, t.slab_rows.data_ptr(), S, 0.0, 9.0, 1.0, partials.data_ptr(), out.data_ptr(), st) == -1
    assert call(table(pred=(1, 0))) == EINVAL and call(table(gt=(0, 0))) == EINVAL                                 # a null plane in a row
    assert call(nslabs=0) == EINVAL and call(nslabs=3) == EINVAL and call(nviews=0) == EINVAL                       # S < 1, S that the table does not end in
    assert call(K=5, only=(1,)) == (-1,) and call(K=-1, only=(1,)) == (-1,)                                                              # K > 4
    assert call(table(stride=(0, 0))) == EINVAL and call(table(stride=(1, -3))) == EINVAL                           # a stride < 1
    assert call(table(npix=(1, 0))) == EINVAL
    big = table(npix=(0, 2 ** 30), first_block=(1, 2 ** 18))                                                        # 2^30 + 2^30 pixels >= 2^31
    big[1, 4] = 2 ** 30
    assert call(big, nblocks=2 ** 19) == EINVAL
    assert b'2^31' in L.pst_last_error()
    assert call(nblocks=nb + 1) == EINVAL and call(nblocks=nb - 1) == EINVAL                                        # a block count that does not match the table
    assert call(table(first_block=(1, 1))) == EINVAL and call(table(slab=(1, 0))) == EINVAL and call(table(slab=(0, 1))) == EINVAL
    assert L.pst_depth_median(t.dev.data_ptr(), t.host.ctypes.data, 2, nb, S, 0.0, 9.0, 1.0, hist.data_ptr() + 4, prefix.data_ptr(), rank.data_ptr(),
                              count.data_ptr(), median.data_ptr(), st) == -1                                       # a misaligned histogram
    torch.cuda.synchronize()
    assert (partials == -7).all() and (out == -7).all() and (count == -7).all() and (median == -7).all() and (ws == 0).all()
    # and the same operands, unchanged, are accepted
    assert call() == (0, 0, 0)
    torch.cuda.synchronize()
    assert (out[:, 0] > 0).all() and (count > 0).all() and (ws == 0).all()       # the workspaces of the median are left zeroed


def test_a_negative_or_nan_lower_bound_is_refused_without_a_launch():
    """PST_EINVAL from all three entry points for min_depth < 0 and NaN: the outputs keep their sentinel and the workspaces stay zero; 0 and -0.0 run"""
    pred, gt, conf = D.random_views([(9, 13)], seed=24, with_conf=False)
    t = hip.depth_table([(dev(pred)[0], 1, dev(gt)[0], None)], [0], DEV)
    L, st = hip.lib(), hip._stream()
    f64 = dict(dtype=torch.float64, device=DEV)
    partials, out, align = torch.full((1, hip.DEPTH_MOMENTS), -7.0, **f64), torch.full((1, hip.DEPTH_MOMENTS), -7.0, **f64), torch.ones(1, 2, **f64)
    ws = torch.zeros(1032, dtype=torch.int32, device=DEV)
    count, median = torch.full((1,), -7, dtype=torch.int32, device=DEV), torch.full((1, 2), -7.0, dtype=torch.float32, device=DEV)

    def call(lo):
        a = (t.dev.data_ptr(), t.host.ctypes.data, 1, 1)
        return (L.pst_depth_moments(*a, t.slab_rows.data_ptr(), 1, lo, 9.0, 1.0, partials.data_ptr(), out.data_ptr(), st),
                L.pst_depth_errors(*a, t.slab_rows.data_ptr(), 1, lo, 9.0, 1.0, align.data_ptr(), 1, 1.25, 0.0, 0.0, 0.0, partials.data_ptr(), out.data_ptr(), st),
                L.pst_depth_median(*a, 1, lo, 9.0, 1.0, ws[:1024].data_ptr(), ws[1024:1028].data_ptr(), ws[1028:].data_ptr(), count.data_ptr(), median.data_ptr(), st))
    for lo in (-1.0, -1e-45, float('-inf'), float('nan')):
        assert call(lo) == (-1, -1, -1) and b'min_depth' in L.pst_last_error(), lo
    torch.cuda.synchronize()
    assert (partials == -7).all() and (out == -7).all() and (count == -7).all() and (median == -7).all() and (ws == 0).all()
    with pytest.raises(RuntimeError, match='min_depth'):
        hip.depth_median(t, -0.5, 9.0, 1.0, count, median)
    want = int(D.valid(pred[0], gt[0], None, None, 0.0, 9.0).sum())
    for lo in (0.0, -0.0):
        assert call(lo) == (0, 0, 0)
        torch.cuda.synchronize()
        assert int(count[0]) == want > 60 and float(out[0, 0]) == want and (ws == 0).all()


def test_the_call_copies_back_twice_at_most(monkeypatch):
    """one copy to the host after the alignment stage (none for 'none' or a given scale), one at the end: the call's only host syncs"""
    pred, gt, conf = D.random_views([(37, 51), (48, 64)], seed=23)
    pd, gd, cd = dev(pred), dev(gt), dev(conf)
    copies, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(self.numel()), cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, 'item', lambda self: pytest.fail('an .item() in depth_quality'))
    for align, want in (('none', 1), (2.5, 1), ('median', 2), ('scale', 2), ('scale_shift', 2)):
        for scope in ('view', 'scene'):
            del copies[:]
            r = depth_quality(pd, gd, conf=cd, min_conf_thr=1.0, align=align, scope=scope)
            assert len(copies) == want and r['n_valid'] > 0.5 * sum(g.size for g in gt), (align, scope, copies)
