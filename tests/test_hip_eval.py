"""The panoptic evaluation on the GPU (csrc/evaluate.hip, panst3r_amd/engine/evaluate.py) against the numpy restatement of tests/eval_ref.py: every table
and every number of the result BIT FOR BIT - integer atomics, integer comparisons and one float64 division leave no tolerance to choose.  Before a
comparison the restatement is asked whether the case exercises what it is for."""
import numpy as np
import pytest
import torch

import cloud_ref as C
import eval_ref as E
import voxel_ref as R
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_quality, panoptic_point_cloud, default_colors
from test_hip_cloud import to_dev, bits, thresholds

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ALL = ('tp', 'fp', 'fn', 'ignored', 'void_row', 'void_col')
THINGS = [0, 2]


def dev(maps):
    return [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in maps]


def exercised(ref, need=ALL):
    """what the restatement says the case holds"""
    tp, fp, fn, ign = E.totals(ref)
    c = ref['tables']['counts']
    have = {'tp': tp, 'fp': fp, 'fn': fn, 'ignored': ign, 'void_row': int(c[:, -1, :].sum()), 'void_col': int(c[:, :, -1].sum())}
    print('   restatement: %s, pq %.4f, miou %.4f' % (have, ref['pq'], ref['miou']))
    assert all(have[k] >= 1 for k in need), have
    return have


def assert_same(got, want):
    assert set(got) == set(want) and set(got['tables']) == set(want['tables'])
    for k, w in want['tables'].items():
        g = got['tables'][k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        assert np.array_equal(bits(g), bits(w)), k
    for k, w in want.items():
        if k != 'tables':
            assert got[k] == w and type(got[k]) is type(w), k                  # floats compare by value: equal float64 numbers are equal bits (no NaN, no -0)


def run_case(case, need=ALL, scopes=('scene', 'view'), things=THINGS):
    pred, info, gt, gseg = case
    out = []
    for scope in scopes:
        want = E.panoptic_quality(pred, info, gt, gseg, scope=scope, things=things)
        exercised(want, need)
        got = panoptic_quality(dev(pred), info, dev(gt), gseg, scope=scope, things=things)
        assert_same(got, want)
        out.append(got)
    return out


def scored_scene(scene):
    """an overlapping_scene as an evaluation case: the noisy maps against the clean ones, with the floor (5) not annotated - void in the ground truth, so the
    predicted floor is ignored -, box 7 not predicted (void row, an FN) and surface 1 predicted with a foreign category (an FP and an FN)"""
    x, im, pan, info, cams, clean = scene
    pinfo = [dict(s, category_id=s['category_id'] + 1 if s['id'] == 1 else s['category_id']) for s in info if s['id'] != 7]
    return pan, pinfo, clean, [s for s in info if s['id'] != 5]


@pytest.mark.parametrize('shapes', [[(24, 32), (24, 32)], [(24, 32), (32, 24), (23, 31)]], ids=['two_views', 'mixed_odd'])
def test_mixed_shapes(shapes):
    """23 x 31 makes N odd and puts a slab boundary inside a 16-byte load and inside a wave"""
    case = E.random_segments(shapes, 6, 5, seed=1)
    assert len(shapes) == 2 or (sum(h * w for h, w in shapes) % 4 and sum(h * w for h, w in shapes[:2]) % 1024)
    run_case(case)
    run_case(scored_scene(R.overlapping_scene(shapes, seed=2)))


def test_one_segment_each():
    """P = G = 1 in three views: a match, a miss on both sides, a prediction on void"""
    gt = [np.ones((8, 40), dtype=np.int32), np.ones((8, 40), dtype=np.int32), np.zeros((9, 37), dtype=np.int32)]
    gt[0][:, 30:], gt[1][:, 20:] = 0, 4                                          # (4 is not listed: void)
    pred = [np.full((8, 40), 3, dtype=np.int32), np.zeros((8, 40), dtype=np.int32), np.full((9, 37), 3, dtype=np.int32)]
    pred[1][:, 15:25] = 3                                                       # half of it on void: 2 x 40 == 80, an FP
    seg = lambda i: [{'id': i, 'category_id': 2}]
    run_case((pred, seg(3), gt, seg(1)), scopes=('view',))
    run_case((pred, seg(3), gt, seg(1)), need=('tp', 'void_row', 'void_col'), scopes=('scene',))


def test_no_segments_at_all():
    pred, info, gt, gseg = E.random_segments([(24, 32), (23, 31)], 0, 0, seed=2)
    assert info == [] and gseg == []
    for got in run_case((pred, info, gt, gseg), need=('void_row', 'void_col')):
        assert got['pq'] == 0.0 and got['n_pixels'] == got['void_pixels'] == 24 * 32 + 23 * 31 and got['tables']['counts'].shape[1:] == (1, 1)
    # ... and on one side only
    pred, info, gt, gseg = E.random_segments([(24, 32), (23, 31)], 6, 5, seed=2)
    run_case((pred, [], gt, gseg), need=('fn', 'void_row'))
    run_case((pred, info, gt, []), need=('ignored', 'void_col'))


def test_every_lane_its_own_key():
    """P = 200, G = 300 with independent labels per pixel: no two neighbouring lanes share a key, and the table (201 x 301 counters) is larger than any LDS tile"""
    case = E.random_segments([(64, 96)], 200, 300, seed=3, coherent=False)
    pr, gr = np.asarray(case[0][0]).reshape(-1)[4 * 96:], np.asarray(case[2][0]).reshape(-1)[4 * 96:]
    assert np.mean((pr[1:] == pr[:-1]) & (gr[1:] == gr[:-1])) < 0.01
    got, _ = run_case(case)
    assert (got['tables']['counts'] > 0).sum() > 4000


def test_one_pair():
    """every pixel of 4 views of 96 x 128 is the same (p, g) pair: maximum contention, runs across every wave and workgroup boundary"""
    pred, gt = [np.full((96, 128), 9, dtype=np.int32)] * 4, [np.full((96, 128), 2, dtype=np.int32)] * 4
    info, gseg = [{'id': 4, 'category_id': 1}, {'id': 9, 'category_id': 3}], [{'id': 2, 'category_id': 3}]
    for got in run_case((pred, info, gt, gseg), need=('tp',)):
        assert got['pq'] == 1.0 and got['tables']['counts'].max() == (4 * 96 * 128 if got['tables']['counts'].shape[0] == 1 else 96 * 128)


def test_id_handling():
    """sparse ids (largest 1000), negative ids, ids beyond the table, ids listed on one side only"""
    g = np.random.Generator(np.random.PCG64(5))
    gt = np.repeat(np.array([[1, 1, 40, 40, 999, 0, -7, 2 ** 30, 17, 17]], dtype=np.int32), 30, axis=0).repeat(5, axis=1)
    pred = np.roll(gt, 2, axis=1).copy()
    pred[gt == 999], pred[gt == 17] = 1000, -2 ** 31
    pred[:20][gt[:20] == 40] = 333                                              # unlisted; what is left of pred 40 is a third of gt 40: an FP and an FN
    pred[:, :3] = 2 ** 31 - 1
    pred[20:, 25:40] = 6                                                        # pred 6 on void ground truth
    info = [{'id': 1000, 'category_id': 0}, {'id': 1, 'category_id': 0}, {'id': 40, 'category_id': 1}, {'id': 6, 'category_id': 0}]
    gseg = [{'id': 999, 'category_id': 0}, {'id': 40, 'category_id': 1}, {'id': 1, 'category_id': 0}, {'id': 17, 'category_id': 1}]
    run_case(([pred, pred[:, ::-1].copy()], info, [gt, gt[:, ::-1].copy()], gseg))


def test_calls_repeat_and_the_merge_changes_nothing():
    pred, info, gt, gseg = E.random_segments([(96, 128), (128, 96), (37, 51)], 9, 12, seed=7)
    pd, gd = dev(pred), dev(gt)

    def raw(scope):
        r = panoptic_quality(pd, info, gd, gseg, scope=scope, things=THINGS)
        return r, b''.join(bits(r['tables'][k]).tobytes() for k in sorted(r['tables']))
    for scope in ('scene', 'view'):
        (a, ba), (b, bb) = raw(scope), raw(scope)
        assert ba == bb and {k: v for k, v in a.items() if k != 'tables'} == {k: v for k, v in b.items() if k != 'tables'}
        old = hip.EVAL_MERGE
        try:
            hip.EVAL_MERGE = 1 - old
            c, bc = raw(scope)
        finally:
            hip.EVAL_MERGE = old
        assert bc == ba and c['pq'] == a['pq']
    # a stacked [V, H, W] tensor, ground truth from the host, int64 maps: the same result as the list of device maps
    p3 = E.random_segments([(24, 32)] * 3, 6, 5, seed=8)
    want = E.panoptic_quality(*p3, scope='view', things=THINGS)
    assert_same(panoptic_quality(torch.from_numpy(np.stack(p3[0])).to(DEV), p3[1], np.stack(p3[2]).astype(np.int64), p3[3], scope='view', things=THINGS), want)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        panoptic_quality([torch.from_numpy(m) for m in p3[0]], p3[1], p3[2], p3[3])


def test_model_evaluate_on_post_processing_shaped_input():
    """`PanSt3R.evaluate` on a pan_preds-shaped result (maps and segments_info as the post-processings leave them: device int32 maps, ids with query_id)"""
    from panst3r_amd.panst3r import PanSt3R
    pred, info, gt, gseg = scored_scene(R.overlapping_scene([(48, 64), (64, 48), (37, 51)], seed=3))
    pan_preds = [{'pan': dev(pred), 'segments_info': info, 'conf': None}]
    for scope in ('scene', 'view'):
        want = E.panoptic_quality(pred, info, gt, gseg, scope=scope, things=THINGS)
        exercised(want)
        assert_same(PanSt3R.evaluate(None, pan_preds, dev(gt), gseg, scope=scope, things=THINGS), want)


def test_consistent_maps_of_the_voxel_vote():
    """the device's `consistent_maps()` scored as they are (views into one flat buffer, the second one not 16-byte aligned) = the restatement's figure
    for the restatement's maps"""
    scene = R.overlapping_scene([(37, 51), (48, 64), (64, 48)], seed=3)
    x, im, pan, info, cams, clean = scene
    thr, colors = thresholds(scene[:5])['half'], default_colors(len(info) + 1)
    rc = C.cloud(x, im, pan, info, cams, min_conf_thr=thr, colors=colors)
    rv = R.voxelize(rc['points'], rc['rgb'], rc['pan'], rc['index'], [s['id'] for s in rc['segments']], 0.25, colors)
    maps = R.consistent_maps(rv, rc, pan)
    xd, imd, pand, _, camd = to_dev(scene[:5])
    vox = panoptic_point_cloud(xd, imd, None, pand, info, camd, min_conf_thr=thr, colors=colors).voxelize(0.25)
    _, pinfo, _, gseg = scored_scene(scene)
    for scope in ('scene', 'view'):
        want = E.panoptic_quality(maps, pinfo, clean, gseg, scope=scope, things=THINGS)
        exercised(want)
        assert_same(panoptic_quality(vox.consistent_maps(), pinfo, dev(clean), gseg, scope=scope, things=THINGS), want)
    assert_same(panoptic_quality(vox.consistent_maps()[1:2], pinfo, dev(clean[1:2]), gseg), E.panoptic_quality(maps[1:2], pinfo, clean[1:2], gseg))


@pytest.fixture(scope='module')
def bench_case():
    case = scored_scene(R.overlapping_scene([(384, 512)] * 50, seed=4))
    return case, dev(case[0]), dev(case[2])


@pytest.mark.parametrize('scope', ['scene', 'view'])
def test_large_launch(bench_case, scope):
    """50 views of 384 x 512: 9.8 M pixels, 9600 workgroups"""
    (pred, info, gt, gseg), pd, gd = bench_case
    want = E.panoptic_quality(pred, info, gt, gseg, scope=scope, things=THINGS)
    assert want['n_pixels'] == 50 * 384 * 512
    exercised(want)
    assert_same(panoptic_quality(pd, info, gd, gseg, scope=scope, things=THINGS), want)
