"""Known answers for the numpy restatement of the panoptic evaluation (tests/eval_ref.py), the interface's refusals and the ABI's two new entry points.
No GPU: the device kernels are held to the restatement in test_hip_eval.py."""
import numpy as np
import pytest
import torch

import abi_header
import cloud_ref
import eval_ref as E
import voxel_ref

I = np.int32
SEG = lambda *pairs: [{'id': i, 'category_id': c} for i, c in pairs]

# the hand-computed case: two views of 4 x 6.  Ground truth 1 (category 0), 2 and 3 (category 1); predictions 5, 8, 9 (category 0), 6, 7 (category 1)
GT = [np.array([[1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 2], [1, 1, 1, 2, 2, 0], [1, 1, 1, 2, 2, 0]], dtype=I),
      np.array([[1, 1, 1, 1, 3, 3], [1, 1, 1, 1, 3, 3], [0, 0, 0, 0, 3, 3], [0, 0, 0, 0, 3, 3]], dtype=I)]
PRED = [np.array([[5, 5, 5, 5, 6, 6], [5, 5, 5, 6, 6, 6], [5, 5, 5, 6, 6, 6], [5, 5, 5, 6, 6, 7]], dtype=I),
        np.array([[5, 5, 8, 8, 6, 6], [5, 5, 8, 8, 6, 6], [7, 7, 7, 0, 6, 6], [7, 7, 0, 0, 9, 9]], dtype=I)]
GT_SEG, PRED_SEG = SEG((1, 0), (2, 1), (3, 1)), SEG((5, 0), (6, 1), (7, 1), (8, 0), (9, 0))


def test_hand_computed_two_views_scene_scope():
    r = E.panoptic_quality(PRED, PRED_SEG, GT, GT_SEG, scope='scene', things=[0])
    t = r['tables']
    #                                  gt 1  2  3 void
    assert t['counts'].tolist() == [[[16, 1, 0, 0],      # 5
                                     [0, 9, 6, 1],       # 6
                                     [0, 0, 0, 6],       # 7
                                     [4, 0, 0, 0],       # 8
                                     [0, 0, 2, 0],       # 9
                                     [0, 0, 0, 3]]]      # void
    assert t['pred_area'].tolist() == [[17, 16, 6, 4, 2]] and t['gt_area'].tolist() == [[20, 10, 8]]
    # gt 1 - pred 5: 2 x 16 > 17 + 20 - 16 = 21; gt 2 - pred 6: 2 x 9 > 16 + 10 - 9 - 1 = 16; gt 3 - pred 6: 2 x 6 < 16 + 8 - 6 - 1 = 17
    assert t['match'].tolist() == [[0, 1, -1]] and t['iou'].tolist() == [[16 / 21, 9 / 16, 0.0]]
    assert t['pred_state'].tolist() == [[E.MATCHED, E.MATCHED, E.IGNORED, E.FP, E.FP]]
    assert r['matches'] == [(0, 5, 1, 16 / 21), (0, 6, 2, 9 / 16)] and r['ignored'] == [(0, 7)]
    c0, c1 = r['per_class'][0], r['per_class'][1]
    assert (c0['tp'], c0['fp'], c0['fn'], c0['iou_sum']) == (1, 2, 0, 16 / 21) and (c1['tp'], c1['fp'], c1['fn'], c1['iou_sum']) == (1, 0, 1, 9 / 16)
    assert (c0['pq'], c0['sq'], c0['rq']) == ((16 / 21) / 2.0, 16 / 21, 0.5) and (c1['pq'], c1['sq'], c1['rq']) == ((9 / 16) / 1.5, 9 / 16, 1 / 1.5)
    assert r['pq'] == (c0['pq'] + c1['pq']) / 2 and r['sq'] == (16 / 21 + 9 / 16) / 2 and r['rq'] == (0.5 + 1 / 1.5) / 2
    assert (r['pq_things'], r['sq_things'], r['rq_things']) == (c0['pq'], c0['sq'], c0['rq'])
    assert (r['pq_stuff'], r['sq_stuff'], r['rq_stuff']) == (c1['pq'], c1['sq'], c1['rq'])
    # semantic: category 0 = pred {5, 8, 9} on gt {1}: inter 20, pred 23, gt 20; category 1 = pred {6, 7} on gt {2, 3}: inter 15, pred 22 (7 on void), gt 18
    assert c0['iou'] == 20 / 23 and c1['iou'] == 15 / 18 and r['miou'] == (20 / 23 + 15 / 18) / 2
    assert r['n_pixels'] == 48 and r['void_pixels'] == 10 and r['pixel_acc'] == 35 / 38
    assert E.panoptic_quality(PRED, PRED_SEG, GT, GT_SEG)['pq_things'] is None


def test_hand_computed_two_views_view_scope():
    r = E.panoptic_quality(PRED, PRED_SEG, GT, GT_SEG, scope='view')
    t = r['tables']
    assert t['pred_area'].tolist() == [[13, 10, 1, 0, 0], [4, 6, 5, 4, 2]] and t['gt_area'].tolist() == [[12, 10, 0], [8, 0, 8]]
    # view 1, gt 1: pred 5 and pred 8 both have 2 x 4 == 4 + 8 - 4: equality is no match
    assert t['match'].tolist() == [[0, 1, -1], [-1, -1, 1]] and t['iou'].tolist() == [[12 / 13, 9 / 10, 0.0], [0.0, 0.0, 6 / 8]]
    assert t['pred_state'].tolist() == [[E.MATCHED, E.MATCHED, E.IGNORED, E.ABSENT, E.ABSENT], [E.FP, E.MATCHED, E.IGNORED, E.FP, E.FP]]
    c0, c1 = r['per_class'][0], r['per_class'][1]
    assert (c0['tp'], c0['fp'], c0['fn']) == (1, 3, 1) and (c1['tp'], c1['fp'], c1['fn']) == (2, 0, 0)
    assert c0['pq'] == (12 / 13) / 3.0 and c1['pq'] == (9 / 10 + 6 / 8) / 2.0 and r['pq'] == (c0['pq'] + c1['pq']) / 2
    assert r['ignored'] == [(0, 7), (1, 7)] and r['miou'] == (20 / 23 + 15 / 18) / 2          # the semantic reading does not depend on the scope


def test_identical_maps_score_one_and_ids_do_not_matter():
    pred, info, gt, gseg = E.random_segments([(24, 32), (23, 31)], 6, 5, seed=3)
    for scope in ('scene', 'view'):
        r = E.panoptic_quality(gt, gseg, gt, gseg, scope=scope)
        tp, fp, fn, ign = E.totals(r)
        assert (r['pq'], r['sq'], r['rq'], r['miou'], r['pixel_acc']) == (1.0, 1.0, 1.0, 1.0, 1.0) and fp == fn == ign == 0
        assert tp == int((r['tables']['gt_area'] > 0).sum()) > 0 and all(m[3] == 1.0 for m in r['matches'])
        # permuted predicted ids: another table order, other ids in the maps, the same scores
        base = E.panoptic_quality(pred, info, gt, gseg, scope=scope, things=[0, 1])
        perm = {s['id']: 100 + 7 * ((k + 2) % len(info)) for k, s in enumerate(info)}
        pred2 = [np.vectorize(lambda i: perm.get(i, i))(m).astype(I) for m in pred]
        info2 = [{'id': perm[s['id']], 'category_id': s['category_id']} for s in reversed(info)]
        other = E.panoptic_quality(pred2, info2, gt, gseg, scope=scope, things=[0, 1])
        assert E.totals(base) == E.totals(other) and min(E.totals(base)[:3]) > 0
        for k in ('pq', 'sq', 'rq', 'pq_things', 'pq_stuff', 'miou', 'pixel_acc', 'n_pixels', 'void_pixels'):
            assert base[k] == other[k], k
        assert sorted((s, perm[p], g, q) for s, p, g, q in base['matches']) == sorted(other['matches'])


def test_equality_is_no_match_and_one_pixel_more_is():
    gt = [np.array([[1, 1, 1, 1, 1, 1, 1, 1]], dtype=I)]
    half = [np.array([[4, 4, 4, 4, 0, 0, 0, 0]], dtype=I)]                      # inter 4, union 8: 2 x 4 == 8
    r = E.panoptic_quality(half, SEG((4, 0)), gt, SEG((1, 0)))
    assert E.totals(r) == (0, 1, 1, 0) and r['pq'] == 0.0 and r['tables']['match'].tolist() == [[-1]]
    more = [np.array([[4, 4, 4, 4, 4, 0, 0, 0]], dtype=I)]                      # inter 5, union 8
    r = E.panoptic_quality(more, SEG((4, 0)), gt, SEG((1, 0)))
    assert E.totals(r) == (1, 0, 0, 0) and r['pq'] == 5 / 8 and r['matches'] == [(0, 4, 1, 5 / 8)]


def test_half_on_void_is_a_false_positive_and_one_pixel_more_is_ignored():
    gt = [np.array([[1, 1, 1, 1, 0, 0, 0, 0, 0, 2]], dtype=I)]
    gseg = SEG((1, 0), (2, 0))
    r = E.panoptic_quality([np.array([[0, 0, 3, 3, 3, 3, 0, 0, 0, 0]], dtype=I)], SEG((3, 0)), gt, gseg)      # 2 of 4 on void: 2 x 2 == 4
    assert E.totals(r) == (0, 1, 2, 0) and r['tables']['pred_state'].tolist() == [[E.FP]]
    r = E.panoptic_quality([np.array([[0, 0, 3, 3, 3, 3, 3, 0, 0, 0]], dtype=I)], SEG((3, 0)), gt, gseg)      # 3 of 5 on void
    assert E.totals(r) == (0, 0, 2, 1) and r['tables']['pred_state'].tolist() == [[E.IGNORED]] and r['ignored'] == [(0, 3)]
    # the pixels on void leave the union: pred 3 covers gt 1 and three void pixels -> iou 1
    r = E.panoptic_quality([np.array([[3, 3, 3, 3, 3, 3, 3, 0, 0, 0]], dtype=I)], SEG((3, 0)), gt, gseg)
    assert r['matches'] == [(0, 3, 1, 1.0)] and E.totals(r) == (1, 0, 1, 0)


def test_category_mismatch_is_one_fp_plus_one_fn():
    m = [np.array([[1, 1, 2, 2]], dtype=I)]
    r = E.panoptic_quality(m, SEG((1, 0), (2, 5)), m, SEG((1, 0), (2, 6)))
    assert E.totals(r) == (1, 1, 1, 0) and r['per_class'][5]['fp'] == 1 and r['per_class'][6]['fn'] == 1 and r['per_class'][0]['pq'] == 1.0
    assert r['pq'] == 1 / 3 and r['per_class'][5]['iou'] is None and r['per_class'][6]['iou'] == 0.0 and r['miou'] == 0.5 and r['pixel_acc'] == 0.5


def test_void_ids_unlisted_negative_and_beyond_the_table():
    gt = [np.array([[1, 1, 1, 1, 7, -2, 0, 2 ** 30]], dtype=I)]               # 7 is not listed, 2^30 is beyond the table
    pred = [np.array([[1000, 1000, 1000, 1000, 1000, 5, -1, 2000]], dtype=I)]
    r = E.panoptic_quality(pred, SEG((3, 0), (1000, 0), (17, 0)), gt, SEG((1, 0), (9, 0)))
    assert r['tables']['counts'].tolist() == [[[0, 0, 0], [4, 0, 1], [0, 0, 0], [0, 0, 3]]] and r['void_pixels'] == 4
    assert r['matches'] == [(0, 1000, 1, 1.0)] and E.totals(r) == (1, 0, 0, 0)


def test_a_segment_absent_from_a_view_counts_in_the_scene_only():
    gt = [np.array([[1, 1, 2, 2]], dtype=I), np.array([[1, 1, 1, 1]], dtype=I)]
    seg = SEG((1, 0), (2, 0))
    r = E.panoptic_quality(gt, seg, gt, seg, scope='view')
    assert r['tables']['gt_area'].tolist() == [[2, 2], [4, 0]] and r['tables']['match'].tolist() == [[0, 1], [0, -1]]
    assert r['tables']['pred_state'].tolist() == [[1, 1], [1, 0]] and E.totals(r) == (3, 0, 0, 0)
    assert E.totals(E.panoptic_quality(gt, seg, gt, seg, scope='scene')) == (2, 0, 0, 0)


def test_ids_swapped_between_views_cost_scene_pq_and_not_view_pq():
    """the property the scene scope exists for: every view on its own is perfect, but the two instances trade ids from one view to the next"""
    gt = [np.array([[1, 1, 1, 2, 2, 2]] * 3, dtype=I)] * 2
    pred = [gt[0], np.array([[2, 2, 2, 1, 1, 1]] * 3, dtype=I)]
    seg = SEG((1, 4), (2, 4))
    view, scene = E.panoptic_quality(pred, seg, gt, seg, scope='view'), E.panoptic_quality(pred, seg, gt, seg, scope='scene')
    assert view['pq'] == 1.0 and E.totals(view) == (4, 0, 0, 0)
    assert scene['pq'] == 0.0 and E.totals(scene) == (0, 2, 2, 0)             # 2 x 9 == 18 + 18 - 9 - 9: not even a half match
    assert view['miou'] == scene['miou'] == 1.0                                  # same category: the semantic reading cannot see it
    stable = E.panoptic_quality([gt[0], gt[0]], seg, gt, seg, scope='scene')
    assert stable['pq'] == 1.0 > scene['pq']


def test_overlapping_scene_counts():
    """the figures a sketch of the rules gives on voxel_ref.overlapping_scene; the device tests rely on TP, FP and FN all being there"""
    def run(flip, scope):
        sc = voxel_ref.overlapping_scene([(24, 32)] * 2, seed=2, flip=flip)
        return E.totals(E.panoptic_quality(sc[2], sc[3], sc[5], sc[3], scope=scope))[:3]
    assert run(0.2, 'scene') == (9, 1, 0)
    assert run(0.45, 'scene') == (1, 9, 8)
    assert run(0.2, 'view') == (15, 5, 1)
    assert min(run(0.45, 'scene')) > 0 and min(run(0.2, 'view')) > 0


def test_the_voxel_vote_raises_scene_pq():
    """usefulness, on the restatements: 8 views of 96 x 128 with a fifth of the pixels relabelled; the maps after the voxel vote at 0.1 score a strictly
    higher scene-scope PQ against the clean labels than the input maps"""
    x, im, pan, info, cams, clean = voxel_ref.overlapping_scene([(96, 128)] * 8, seed=7, flip=0.2)
    conf = np.concatenate([v['conf'].reshape(-1) for v in x])
    colors = np.zeros((len(info) + 1, 3), dtype=np.float32)
    c = cloud_ref.cloud(x, im, pan, info, cams, min_conf_thr=float(np.sort(conf)[len(conf) // 2]), colors=colors)
    vox = voxel_ref.voxelize(c['points'], c['rgb'], c['pan'], c['index'], [s['id'] for s in c['segments']], 0.1, colors)
    maps = voxel_ref.consistent_maps(vox, c, pan)
    before, after = E.panoptic_quality(pan, info, clean, info), E.panoptic_quality(maps, info, clean, info)
    print('scene PQ %.4f -> %.4f, SQ %.4f -> %.4f, RQ %.4f -> %.4f, mIoU %.4f -> %.4f' % tuple(v[k] for k in ('pq', 'sq', 'rq', 'miou') for v in (before, after)))
    assert after['pq'] > before['pq']


def test_product_summary_equals_the_restatement():
    """steps 7 and 8 of the product (float64 host arithmetic) on the restatement's tables: every number of the dict, exactly"""
    from panst3r_amd.engine import evaluate as ev
    for P, G, coherent in ((6, 5, True), (9, 12, True), (20, 30, False), (1, 1, True), (0, 0, True)):
        pred, info, gt, gseg = E.random_segments([(24, 32), (32, 24), (23, 31)], P, G, seed=5, coherent=coherent)
        for scope in ('scene', 'view'):
            tab = E.tables(pred, info, gt, gseg, scope)
            want = E.summarize(tab, info, gseg, things=[0, 2])
            got = ev._summarize(tab, [s['id'] for s in info], [s['category_id'] for s in info], [s['id'] for s in gseg], [s['category_id'] for s in gseg], [0, 2])
            assert set(got) == set(want)
            for k in want:
                if k != 'tables':
                    assert got[k] == want[k], k


def test_every_refusal_comes_before_the_device():
    from panst3r_amd import hip
    from panst3r_amd.engine import panoptic_quality
    m = torch.zeros(4, 6, dtype=torch.int32)
    seg = SEG((1, 0), (2, 1))
    with pytest.raises(ValueError, match='scope'):
        panoptic_quality([m], seg, [m], seg, scope='image')
    with pytest.raises(ValueError, match='V >= 1'):
        panoptic_quality([], seg, [], seg)
    with pytest.raises(ValueError, match='as many'):
        panoptic_quality([m, m], seg, [m], seg)
    with pytest.raises(ValueError, match='view 1: the predicted map is'):
        panoptic_quality([m, m], seg, [m, torch.zeros(6, 4, dtype=torch.int32)], seg)
    with pytest.raises(ValueError, match=r'\[V, H, W\]'):
        panoptic_quality(torch.zeros(4, 6, dtype=torch.int32), seg, [m], seg)
    huge = torch.zeros(1, dtype=torch.int32).expand(1 << 16, 1 << 15)          # 2^31 pixels, one element of memory
    with pytest.raises(ValueError, match='2\\^31'):
        panoptic_quality([huge], seg, [huge], seg)
    for segs in (SEG((1, 0), (1, 1)), SEG((0, 0)), SEG((-4, 0)), SEG((hip.EVAL_MAX_ID, 0))):
        with pytest.raises(ValueError, match='unique and in'):
            panoptic_quality([m], segs, [m], seg)
        with pytest.raises(ValueError, match='unique and in'):
            panoptic_quality([m], seg, [m], segs)
    with pytest.raises(ValueError, match='iscrowd'):
        panoptic_quality([m], seg, [m], [{'id': 1, 'category_id': 0, 'iscrowd': 1}])
    many = SEG(*[(i + 1, 0) for i in range(8192)])
    assert 4 * 8193 * 8193 > hip.EVAL_MAX_TABLE_BYTES
    with pytest.raises(ValueError, match='EVAL_MAX_TABLE_BYTES'):
        panoptic_quality([m], many, [m], many)
    with pytest.raises(ValueError, match='integer ids'):
        panoptic_quality([m.float()], seg, [m], seg)
    with pytest.raises(ValueError, match='integer ids'):
        panoptic_quality([m], seg, [np.zeros((4, 6), dtype=bool)], seg)
    # ... and maps on the host are refused, not scored with torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        panoptic_quality([m], seg, [m], seg)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.pq_count(m.reshape(-1), m.reshape(-1), torch.zeros(2, dtype=torch.int64), m.reshape(-1), m.reshape(-1), 2, 2, torch.zeros(1, 3, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        z = torch.zeros(1, 2, dtype=torch.int32)
        hip.pq_match(torch.zeros(1, 3, 3, dtype=torch.int32), z[0], z[0], z, z, z, z.double(), z)


def test_abi_has_the_two_entry_points_and_keeps_its_version():
    from panst3r_amd import hip
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']
    protos = {p[0]: p for p in abi_header.prototypes()}
    for name in ('pst_pq_count', 'pst_pq_match'):
        assert name in hip.SIGNATURES and name in protos and protos[name][1] == 'int'
        assert len(hip.SIGNATURES[name].split(':')[1]) == len(protos[name][2]) and protos[name][2][-1] == 'void*'
        assert all(t.endswith('*') or t in abi_header.SCALARS for t in protos[name][2])
    assert hip.EVAL_MERGE == 1 and hip.EVAL_MAX_TABLE_BYTES > 0


def test_model_evaluate_only_composes():
    from panst3r_amd.panst3r import PanSt3R
    from panst3r_amd import engine
    seen = {}
    orig = engine.panoptic_quality
    try:
        engine.panoptic_quality = lambda *a, **k: seen.update(a=a, k=k) or 'result'
        out = PanSt3R.evaluate(None, [{'pan': 'maps', 'segments_info': 'info'}], 'gt', 'gseg', scope='view', things=[1])
    finally:
        engine.panoptic_quality = orig
    assert out == 'result' and seen['a'] == ('maps', 'info', 'gt', 'gseg') and seen['k'] == {'scope': 'view', 'things': [1]}
