"""The panoptic point cloud on the GPU (csrc/cloud.hip, panst3r_amd/engine/cloud.py) against the numpy restatement of tests/cloud_ref.py: every
output BIT FOR BIT - the stage is compares, integer work and separately rounded fp32 operations, so there is no tolerance to choose.  The one cap:
the "about half" threshold (the median of the generated confidences) must keep a share in [0.3, 0.7] of the points."""
import numpy as np
import pytest
import torch

import cloud_ref as R
import tiny
from panst3r_amd.engine import panoptic_point_cloud, default_colors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32


def to_dev(scene):
    x, im, pan, info, cams = scene
    xd = [{k: torch.from_numpy(v).to(DEV) for k, v in d.items()} for d in x]
    return xd, [torch.from_numpy(i).to(DEV) for i in im], [torch.from_numpy(p).to(DEV) for p in pan], info, [torch.from_numpy(c) for c in cams]


def shapes_of(scene):
    return [v['conf'].shape for v in scene[0]]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(cloud, ref):
    assert len(cloud) == len(ref['index'])
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        got, want = getattr(cloud, k), ref[k]
        assert tuple(got.shape) == want.shape and got.cpu().numpy().dtype == want.dtype, k
        assert np.array_equal(bits(got), bits(want)), k
    assert [s['id'] for s in cloud.segments] == [s['id'] for s in ref['segments']]
    for a, b in zip(cloud.segments, ref['segments']):
        assert a['count'] == b['count'] and (a['query_id'], a['category_id']) == (b['query_id'], b['category_id'])
        assert np.array_equal(bits(a['median']), bits(b['median'].astype(F))), (a['id'], a['median'], b['median'])


def assert_equal_clouds(a, b):
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert len(a.segments) == len(b.segments)
    for s, t in zip(a.segments, b.segments):
        assert (s['id'], s['count']) == (t['id'], t['count']) and np.array_equal(bits(s['median']), bits(t['median']))


def thresholds(scene):
    """keep nothing, about half (the median confidence: a value that occurs in the input), everything (the smallest confidence: equality keeps it)"""
    conf = np.concatenate([v['conf'].reshape(-1) for v in scene[0]])
    return {'none': float(conf.max()) * 2, 'half': float(np.sort(conf)[len(conf) // 2]), 'all': float(conf.min())}


def run_case(scene, which, local_pointmaps, opacity=0.5):
    thr = thresholds(scene)[which]
    x, im, pan, info, cams = scene
    colors = default_colors(len(info) + 1)
    ref = R.cloud(x, im, pan, info, cams, min_conf_thr=thr, opacity=opacity, colors=colors, local_pointmaps=local_pointmaps)
    N = sum(h * w for h, w in shapes_of(scene))
    share = len(ref['index']) / N
    print('%s: kept %d of %d (%.3f), %d segments' % (which, len(ref['index']), N, share, len(ref['segments'])))
    if which == 'half':
        assert 0.3 <= share <= 0.7
        conf = np.concatenate([v['conf'].reshape(-1) for v in x])
        assert np.any(conf == F(thr))                       # a confidence exactly at the threshold is in the input (and is kept)
    elif which == 'none':
        assert share == 0 and ref['segments'] == []
    else:
        assert share == 1
    xd, imd, pand, _, camd = to_dev(scene)
    cloud = panoptic_point_cloud(xd, imd, [list(s) for s in shapes_of(scene)], pand, info, camd, min_conf_thr=thr, opacity=opacity, colors=colors,
                                 local_pointmaps=local_pointmaps)
    assert_same(cloud, ref)
    return cloud


@pytest.mark.parametrize('which', ['none', 'half', 'all'])
@pytest.mark.parametrize('local_pointmaps', [False, True])
def test_tiny_two_view_scene(which, local_pointmaps):
    run_case(R.synthetic_scene([(24, 32), (24, 32)], seed=2, nseg=12), which, local_pointmaps)


@pytest.mark.parametrize('which', ['none', 'half', 'all'])
@pytest.mark.parametrize('local_pointmaps', [False, True])
def test_mixed_landscape_and_portrait_scene(which, local_pointmaps):
    """views of different shapes, pixel counts that are not multiples of the 1024-point workgroup or of 4"""
    run_case(R.synthetic_scene([(48, 64), (64, 48), (37, 51), (48, 64), (30, 43)], seed=3, nseg=25), which, local_pointmaps, opacity=0.3)


@pytest.fixture(scope='module')
def bench_scene():
    return R.synthetic_scene([(384, 512)] * 50, seed=4, nseg=60)


@pytest.mark.parametrize('which,local_pointmaps', [('none', False), ('half', False), ('half', True), ('all', False)])
def test_benchmark_shape(bench_scene, which, local_pointmaps):
    """50 views of 384 x 512, about 60 segments of very unequal size: one of a single point, one of an even count, one wholly below the threshold"""
    cloud = run_case(bench_scene, which, local_pointmaps)
    if which != 'none':
        seg = {s['id']: s['count'] for s in cloud.segments}
        assert seg[1] == 1 and seg[2] == 6 and (which == 'all' or 3 not in seg) and len(seg) >= 50


def test_rethreshold_and_recolor_equal_a_fresh_call_and_calls_repeat():
    scene = R.synthetic_scene([(96, 128), (128, 96), (96, 128)], seed=5, nseg=30)
    xd, imd, pand, info, camd = to_dev(scene)
    t = thresholds(scene)
    call = lambda **kw: panoptic_point_cloud(xd, imd, None, pand, info, camd, **kw)
    a = call(min_conf_thr=t['half'], opacity=0.5)
    assert_equal_clouds(a, call(min_conf_thr=t['half'], opacity=0.5))                    # two identical calls: identical bits
    thr2 = float(np.sort(np.concatenate([v['conf'].reshape(-1) for v in scene[0]]))[1000])
    assert_equal_clouds(a.rethreshold(thr2), call(min_conf_thr=thr2, opacity=0.5))
    assert len(a.rethreshold(t['none'])) == 0 and a.rethreshold(t['none']).segments == []
    assert_equal_clouds(a.recolor(opacity=0.8), call(min_conf_thr=t['half'], opacity=0.8))
    table = default_colors(len(info) + 1)[::-1].copy()
    b = a.recolor(colors=table)
    assert_equal_clouds(b, call(min_conf_thr=t['half'], opacity=0.5, colors=table))
    assert not np.array_equal(bits(a.colors), bits(b.colors)) and np.array_equal(bits(a.points), bits(b.points))
    c = a.cpu()
    assert c.points.device.type == 'cpu' and np.array_equal(bits(c.points), bits(a.points))
    with pytest.raises(RuntimeError):
        c.rethreshold(1.0)


def test_nan_coordinates_make_the_axis_nan_and_nan_confidences_are_dropped():
    scene = R.synthetic_scene([(32, 32), (32, 32)], seed=6, nseg=10)
    x, im, pan, info, cams = scene
    ids, cnt = np.unique(pan[1], return_counts=True)
    big = int(ids[ids > 3][np.argmax(cnt[ids > 3])])
    ys, xs = np.nonzero(pan[1] == big)
    x[1]['pts3d_local'][ys[0], xs[0], 1] = np.nan
    x[1]['conf'][ys[0], xs[0]] = 100.0
    x[0]['conf'][5, 5] = np.nan
    thr = thresholds(([{'conf': np.nan_to_num(v['conf'], nan=2.0)} for v in x],))['half']
    colors = default_colors(len(info) + 1)
    ref = R.cloud(x, im, pan, info, cams, min_conf_thr=thr, colors=colors)
    xd, imd, pand, _, camd = to_dev(scene)
    cloud = panoptic_point_cloud(xd, imd, None, pand, info, camd, min_conf_thr=thr, colors=colors)
    assert len(cloud) == len(ref['index']) and np.array_equal(cloud.index.cpu().numpy(), ref['index'])
    got = {s['id']: s for s in cloud.segments}
    want = {s['id']: s for s in ref['segments']}
    assert sorted(got) == sorted(want)
    assert np.isnan(want[big]['median']).any()
    for i in got:
        assert got[i]['count'] == want[i]['count']
        assert np.array_equal(np.isnan(got[i]['median']), np.isnan(want[i]['median']))
        ok = ~np.isnan(want[i]['median'])
        assert np.array_equal(bits(got[i]['median'][ok]), bits(want[i]['median'][ok].astype(F)))


def test_a_segment_id_outside_the_table_raises_before_any_launch():
    scene = R.synthetic_scene([(24, 32), (24, 32)], seed=2, nseg=12)
    xd, imd, pand, info, camd = to_dev(scene)
    with pytest.raises(ValueError, match='does not fit the colour table'):
        panoptic_point_cloud(xd, imd, None, pand, info, camd, colors=default_colors(5))
    with pytest.raises(ValueError):
        panoptic_point_cloud(xd, imd, None, pand, info + [{'id': 100000}], camd)
    with pytest.raises(ValueError):
        panoptic_point_cloud(xd, imd, None, pand, [{'id': 0}], camd)
    with pytest.raises(ValueError):
        panoptic_point_cloud(xd, imd, None, pand, [{'id': -3}], camd)


def test_reconstruct_equals_the_four_stages_called_by_hand():
    from panst3r_amd.engine import panoptic_inference_v2
    from panst3r_amd.engine.pointmaps import cameras_from_pointmaps
    V, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    thr = 1.5
    ppkw = dict(cls_threshold=0.0, mask_threshold=0.0, overlap_threshold=0.0)      # seeded random weights: thresholds under which segments survive
    cloud, cameras, pan_preds = h.reconstruct(imgs, ts, tiny.NAMES, min_conf_thr=thr, opacity=0.4, postprocess_kwargs=ppkw, num_keyframes=K, amp='fp16')
    pms, panout = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, amp='fp16')
    pp = panoptic_inference_v2(panout['pred_logits'], panout['pred_masks'], ts, label_mode=h.panoptic_decoder.label_mode, multi_ar=True, **ppkw)
    x_out, focals, cams = cameras_from_pointmaps(pms, ts)
    want = panoptic_point_cloud(x_out, imgs, ts, pp[0]['pan'], pp[0]['segments_info'], cams, focals, min_conf_thr=thr, opacity=0.4)
    assert_equal_clouds(cloud, want)
    assert pan_preds[0]['segments_info'] == pp[0]['segments_info'] and all(torch.equal(a, b) for a, b in zip(pan_preds[0]['pan'], pp[0]['pan']))
    assert len(cameras) == V and all(c['focal'] == f and torch.equal(c['cam2world'], m) for c, f, m in zip(cameras, focals, cams))
    assert cameras[0]['aspect'] == W / H and cloud.view_offsets == [H * W * i for i in range(V + 1)]
    # ... and against the restatement, on what the model produced
    ref = R.cloud([{k: v.cpu().numpy() for k, v in d.items()} for d in x_out], [i.cpu().numpy() for i in imgs], [p.cpu().numpy() for p in pp[0]['pan']],
                  pp[0]['segments_info'], [c.numpy() for c in cams], min_conf_thr=thr, opacity=0.4,
                  colors=default_colors(max([s['id'] for s in pp[0]['segments_info']] + [1]) + 1))
    print('reconstruct: kept %d of %d points, %d segments' % (len(cloud), V * H * W, len(cloud.segments)))
    assert_same(cloud, ref)
    assert len(cloud) > 0 and len(cloud.segments) > 0                  # the comparison is not an empty one
    with pytest.raises(ValueError):
        h.reconstruct(imgs, ts, tiny.NAMES, postprocess='nope', num_keyframes=K)
