"""The voxel fusion of the point cloud on the GPU (csrc/voxel.hip, panst3r_amd/engine/voxels.py) against the numpy restatement of tests/voxel_ref.py:
every output BIT FOR BIT - integer sums, separately rounded fp32 / fp64 operations and integer atomics leave no tolerance to choose.  The device
cloud under test is the product's (`panoptic_point_cloud`, itself held to tests/cloud_ref.py by test_hip_cloud.py); the restatement runs on
cloud_ref's cloud of the same scene."""
import numpy as np
import pytest
import torch

import cloud_ref as C
import tiny
import voxel_ref as R
from panst3r_amd.engine import panoptic_point_cloud, default_colors, voxelize_cloud
from test_hip_cloud import to_dev, bits, thresholds

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
# all points in one voxel (maximum contention) / in between (per scene: a few pixel spacings of its resolution) / every point alone; the scenes live in
# [1, 9]^2 x [1, 5]
SIZES = {'one': 1024.0, 'mid': None, 'alone': 1e-5}
FIELDS = ('points', 'rgb', 'pan', 'colors', 'count', 'votes', 'first_index', 'point_voxel')


def assert_same(vox, ref, ref_segments):
    assert len(vox) == len(ref['pan']) and vox.dropped == ref['dropped']
    for k in FIELDS:
        got, want = getattr(vox, k), ref[k]
        assert tuple(got.shape) == want.shape and got.cpu().numpy().dtype == want.dtype, k
        assert np.array_equal(bits(got), bits(want)), k
    assert [s['id'] for s in vox.segments] == [s['id'] for s in ref_segments]
    for a, b in zip(vox.segments, ref_segments):
        assert a['count'] == b['count'] and (a['query_id'], a['category_id']) == (b['query_id'], b['category_id'])
        assert np.array_equal(bits(a['median']), bits(b['median'].astype(F))), (a['id'], a['median'], b['median'])


def assert_equal_voxels(a, b):
    assert a.dropped == b.dropped and a.voxel_size == b.voxel_size
    for k in FIELDS:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert len(a.segments) == len(b.segments)
    for s, t in zip(a.segments, b.segments):
        assert (s['id'], s['count']) == (t['id'], t['count']) and np.array_equal(bits(s['median']), bits(t['median']))


def device_cloud(scene, thr, opacity, colors):
    xd, imd, pand, info, camd = to_dev(scene[:5])
    return panoptic_point_cloud(xd, imd, None, pand, info, camd, min_conf_thr=thr, opacity=opacity, colors=colors)


def run_case(scene, which, size, opacity=0.5, mid=0.05):
    x, im, pan, info, cams, clean = scene
    thr = thresholds(scene)[which]
    colors = default_colors(len(info) + 1)
    ref_cloud = C.cloud(x, im, pan, info, cams, min_conf_thr=thr, opacity=opacity, colors=colors)
    vs = mid if size == 'mid' else SIZES.get(size, size)                       # a named size, or a number
    ref = R.voxelize(ref_cloud['points'], ref_cloud['rgb'], ref_cloud['pan'], ref_cloud['index'], [s['id'] for s in ref_cloud['segments']], vs, colors, opacity)
    M, Mv = len(ref_cloud['index']), len(ref['pan'])
    print('%s / %s: %d points -> %d voxels, %d dropped, largest voxel %d' % (which, size, M, Mv, ref['dropped'], ref['count'].max() if Mv else 0))
    if which == 'none':
        assert M == 0 and Mv == 0
    else:
        assert ref['dropped'] == 0
        if size == 'one':
            assert Mv == 1 and ref['count'][0] == M
        elif size == 'alone':
            assert Mv == M
        elif size == 'mid':
            assert 1 < Mv < M
    cloud = device_cloud(scene, thr, opacity, colors)
    assert len(cloud) == M
    vox = cloud.voxelize(vs)
    assert_same(vox, ref, R.segments(ref, info))
    assert np.array_equal(vox.point_labels().cpu().numpy(), R.point_labels(ref, ref_cloud['pan']))
    got, want = vox.consistent_maps(), R.consistent_maps(ref, ref_cloud, pan)
    assert len(got) == len(want) and all(g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    return cloud, vox, ref, want


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
def test_tiny_two_view_scene(which, size):
    run_case(R.overlapping_scene([(24, 32), (24, 32)], seed=2), which, size, mid=0.5)


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
def test_mixed_landscape_and_portrait_scene(which, size):
    run_case(R.overlapping_scene([(48, 64), (64, 48), (37, 51), (48, 64), (30, 43)], seed=3), which, size, opacity=0.3, mid=0.25)


@pytest.fixture(scope='module')
def bench_scene():
    return R.overlapping_scene([(384, 512)] * 50, seed=4)


@pytest.mark.parametrize('size', list(SIZES))
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
def test_benchmark_shape(bench_scene, which, size):
    """50 views of 384 x 512 of one room: up to 9.8 M points"""
    run_case(bench_scene, which, size)


def test_the_vote_cleans_the_per_view_maps():
    """the behavioural claim: with a fifth of every view's pixels relabelled at random, the share of kept pixels that carry the clean label is higher
    in consistent_maps than in the input maps.  Shown on the restatement; the device result equals the restatement's maps exactly (run_case)."""
    scene = R.overlapping_scene([(96, 128)] * 8, seed=7, flip=0.2)
    x, im, pan, info, cams, clean = scene
    cloud, vox, ref, maps = run_case(scene, 'half', 0.1)
    kept = np.zeros(sum(p.size for p in pan), dtype=bool)
    kept[cloud.index.cpu().numpy()] = True
    flat = lambda ms: np.concatenate([np.asarray(m).reshape(-1) for m in ms])
    before, after = np.mean(flat(pan)[kept] == flat(clean)[kept]), np.mean(flat(maps)[kept] == flat(clean)[kept])
    print('share of kept pixels with the clean label: %.4f in the input maps, %.4f after the vote' % (before, after))
    assert 0.78 < before < 0.86 and after > before + 0.05
    assert np.array_equal(flat(maps)[~kept], flat(pan)[~kept])                 # a pixel below the threshold keeps its 2-D id


def test_nan_infinite_and_far_points_are_left_out():
    scene = R.overlapping_scene([(32, 40), (40, 32)], seed=6)
    x = scene[0]
    x[0]['pts3d'][3, 4, 1] = np.nan
    x[0]['pts3d'][3, 5, 0] = np.inf
    x[1]['pts3d'][7, 7, 2] = -np.inf
    x[1]['pts3d'][8, 8] = [3e38, 1e30, -2e25]
    x[1]['pts3d'][9, 9, 0] = 0.05 * 2 ** 20 + 1.0                              # just beyond the last cell
    x[0]['pts3d'][0, 0] = [-0.05 * (2 ** 20 - 2), -1e-12, 0.0]                 # the farthest cell that is kept, a tiny negative, zero
    info, colors = scene[3], default_colors(len(scene[3]) + 1)
    ref_cloud = C.cloud(*scene[:5], min_conf_thr=0.0, colors=colors)
    ref = R.voxelize(ref_cloud['points'], ref_cloud['rgb'], ref_cloud['pan'], ref_cloud['index'], [s['id'] for s in ref_cloud['segments']], 0.05, colors)
    assert ref['dropped'] == 5 and ref['point_voxel'][0] == 0
    vox = device_cloud(scene, 0.0, 0.5, colors).voxelize(0.05)
    assert vox.dropped == 5
    for k in FIELDS:
        assert np.array_equal(bits(getattr(vox, k)), bits(ref[k])), k
    assert np.array_equal(vox.point_labels().cpu().numpy(), R.point_labels(ref, ref_cloud['pan']))


def test_calls_repeat_and_options_and_refusals():
    scene = R.overlapping_scene([(96, 128), (128, 96), (96, 128)], seed=5)
    x, im, pan, info, cams, clean = scene
    colors = default_colors(len(info) + 1)
    thr = thresholds(scene)['half']
    cloud = device_cloud(scene, thr, 0.5, colors)
    a, b = voxelize_cloud(cloud, 0.07), voxelize_cloud(cloud, 0.07)
    assert_equal_voxels(a, b)                                                  # two calls: identical bytes
    assert all(torch.equal(p, q) for p, q in zip(a.consistent_maps(), b.consistent_maps()))
    # merged and unmerged atomics give the same result
    from panst3r_amd import hip
    old = hip.VOXEL_MERGE
    try:
        hip.VOXEL_MERGE = 1 - old
        assert_equal_voxels(a, voxelize_cloud(cloud, 0.07))
    finally:
        hip.VOXEL_MERGE = old
    # another opacity and table: only `colors` changes, and equals the restatement's
    table = colors[::-1].copy()
    c = cloud.voxelize(0.07, opacity=0.8, colors=table)
    ref_cloud = C.cloud(x, im, pan, info, cams, min_conf_thr=thr, colors=colors)
    ref = R.voxelize(ref_cloud['points'], ref_cloud['rgb'], ref_cloud['pan'], ref_cloud['index'], [s['id'] for s in ref_cloud['segments']], 0.07, table, 0.8)
    assert np.array_equal(bits(c.colors), bits(ref['colors'])) and np.array_equal(bits(c.points), bits(a.points)) and not np.array_equal(bits(c.colors), bits(a.colors))
    # the CPU copy keeps the data and loses the device inputs
    h = a.cpu()
    assert h.points.device.type == 'cpu' and np.array_equal(bits(h.points), bits(a.points)) and torch.equal(h.point_labels(), a.point_labels().cpu())
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        h.consistent_maps()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        voxelize_cloud(cloud.cpu(), 0.07)
    for bad in (0.0, -0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='voxel_size'):
            cloud.voxelize(bad)
    with pytest.raises(ValueError, match='does not fit the colour table'):
        cloud.voxelize(0.07, colors=default_colors(3))


def test_reconstruct_with_a_voxel_size_equals_reconstruct_then_voxelize():
    V, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    kw = dict(min_conf_thr=1.5, opacity=0.4, postprocess_kwargs=dict(cls_threshold=0.0, mask_threshold=0.0, overlap_threshold=0.0), num_keyframes=K, amp='fp16')
    plain = h.reconstruct(imgs, ts, tiny.NAMES, **kw)
    assert isinstance(plain, tuple) and len(plain) == 3                        # without the keyword: the 3-tuple, as before
    cloud, cameras, pan_preds = plain
    pts = cloud.points.float().cpu().numpy()
    s = float(np.abs(pts[np.isfinite(pts).all(axis=1)]).max()) / 40 if len(cloud) else 1.0
    out = h.reconstruct(imgs, ts, tiny.NAMES, voxel_size=s, **kw)
    assert len(out) == 4
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        assert np.array_equal(bits(getattr(out[0], k)), bits(getattr(cloud, k))), k
    assert all(torch.equal(a, b) for a, b in zip(out[2][0]['pan'], pan_preds[0]['pan'])) and len(out[1]) == len(cameras)
    want = cloud.voxelize(s)
    assert_equal_voxels(out[3], want)
    print('reconstruct: %d points -> %d voxels at voxel_size %.4g' % (len(cloud), len(want), s))
    assert 0 < len(want) < len(cloud)                                          # the comparison is not an empty one
    # ... and against the restatement, on what the model produced
    ref = R.voxelize(cloud.points.cpu().numpy(), cloud.rgb.cpu().numpy(), cloud.pan.cpu().numpy(), cloud.index.cpu().numpy(), [x['id'] for x in cloud.segments], s,
                     default_colors(max([x['id'] for x in pan_preds[0]['segments_info']] + [1]) + 1), 0.4)
    assert_same(want, ref, R.segments(ref, cloud.segments))
