"""The z-buffered rendering of a cloud on the GPU (csrc/render.hip, panst3r_amd/engine/render.py) against the numpy restatement of tests/render_ref.py:
every field of `CloudRender` BIT FOR BIT - separately rounded fp32 operations, a quotient rounded once and a minimum of integers leave no tolerance to
choose.  The device cloud under test is the product's (`panoptic_point_cloud`, itself held to tests/cloud_ref.py by test_hip_cloud.py); the restatement
runs on cloud_ref's cloud of the same scene.

A condition, not a measurement: for every non-empty case the test first asserts ON THE RESTATEMENT that some pixel is hit and that some pixel received
at least two candidate points - the depth test decides something - and, for the cameras placed outside the room, that some pixels stay empty."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref as C
import render_ref as R
import voxel_ref as V
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_point_cloud, default_colors, render_cloud, render_cameras, orbit_cameras, CloudRender
from panst3r_amd.engine import render as render_mod
from test_hip_cloud import to_dev, bits, thresholds

pytestmark = pytest.mark.gpu
F = np.float32
FIELDS = ('depth', 'pan', 'rgb', 'colors', 'index')
# the scenes of test_hip_voxel.py: (shapes, seed, opacity, a voxel size of a few pixel spacings)
SCENES = {'two': ([(24, 32), (24, 32)], 2, 0.5, 0.5), 'mixed': ([(48, 64), (64, 48), (37, 51), (48, 64), (30, 43)], 3, 0.3, 0.25)}
NOVEL = (37, 51)                                                               # an odd size that no input view has in the two-view scene


@functools.lru_cache(maxsize=None)
def scene_of(name):
    shapes, seed = SCENES[name][:2]
    return V.overlapping_scene(shapes, seed=seed)


def focal_of(shape):
    return 0.55 * max(shape)                                                   # overlapping_scene's


def novel_cameras():
    """four cameras of a turntable outside the room (it fills part of the image: empty pixels around it) and one inside it, under the ceiling, with
    most of the room behind it"""
    return orbit_cameras((5.0, 5.0, 2.5), 14.0, 4, 4.0) + orbit_cameras((5.0, 5.0, 2.0), 2.0, 1, 0.5)


def device_cloud(scene, thr, opacity, colors):
    xd, imd, pand, info, camd = to_dev(scene[:5])
    return panoptic_point_cloud(xd, imd, None, pand, info, camd, min_conf_thr=thr, opacity=opacity, colors=colors)


def clouds(name, which):
    """(the product's device cloud, cloud_ref's) of a scene at a threshold"""
    scene = scene_of(name)
    x, im, pan, info, cams, clean = scene
    thr, opacity = thresholds(scene)[which], SCENES[name][2]
    colors = default_colors(len(info) + 1)
    ref = C.cloud(x, im, pan, info, cams, min_conf_thr=thr, opacity=opacity, colors=colors)
    cloud = device_cloud(scene, thr, opacity, colors)
    assert len(cloud) == len(ref['index']) and (len(cloud) == 0) == (which == 'none')
    return cloud, ref


def ref_render(rc, cams, focals, shape, **kw):
    return R.render(rc['points'], rc['rgb'], rc['colors'], rc['pan'], cams, focals, shape, **kw)


def assert_same(got, want):
    assert isinstance(got, CloudRender)
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        assert tuple(g.shape) == w.shape and g.cpu().numpy().dtype == w.dtype, (k, tuple(g.shape), w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (k, int((bits(g) != bits(w)).sum()))
    assert np.array_equal(got.hit.cpu().numpy(), want['index'] >= 0)


def assert_equal_renders(a, b):
    for k in FIELDS:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def check_decides(want, what):
    """on the restatement alone: the comparison is not an empty one"""
    hit, many = want['index'] >= 0, want['candidates'] >= 2
    print('%s: %.1f %% of the pixels hit, %.1f %% with several candidates (at most %d)' % (what, 100 * hit.mean(), 100 * many.mean(), want['candidates'].max()))
    assert hit.any() and many.any(), what


def check_empty(want):
    assert (want['index'] == -1).all() and (want['depth'] == 0).all() and (want['pan'] == 0).all() and (want['rgb'] == 0).all() and (want['colors'] == 0).all()


@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
@pytest.mark.parametrize('name', list(SCENES))
def test_from_every_input_camera_at_its_own_shape(name, which, radius):
    cloud, rc = clouds(name, which)
    cams = scene_of(name)[4]
    for v, shape in enumerate(SCENES[name][0]):
        want = ref_render(rc, [cams[v]], focal_of(shape), shape, radius=radius)
        if which == 'none':
            check_empty(want)
        else:
            check_decides(want, '%s / %s / radius %d / view %d' % (name, which, radius, v))
        assert_same(cloud.render([torch.from_numpy(cams[v])], focal_of(shape), shape, radius=radius), want)


@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
@pytest.mark.parametrize('name', list(SCENES))
def test_from_novel_cameras_in_one_batched_call(name, which, radius):
    cloud, rc = clouds(name, which)
    cams = novel_cameras()
    assert len(cams) >= 4
    want = ref_render(rc, cams, focal_of(NOVEL), NOVEL, radius=radius)
    if which == 'none':
        check_empty(want)
    else:
        check_decides(want, '%s / %s / radius %d / novel cameras' % (name, which, radius))
        assert all((want['index'][b] == -1).any() and (want['index'][b] >= 0).any() for b in range(4))      # outside: the room and empty pixels around it
        assert want['behind'][4] > 0 and (want['index'][4] >= 0).any()                                      # inside: points behind the camera
        print('inside camera: %d of %d points behind it' % (want['behind'][4], len(rc['index'])))
    assert_same(cloud.render(cams, focal_of(NOVEL), NOVEL, radius=radius), want)


def test_voxel_cloud_with_its_default_point_size():
    """the voxels of the mixed scene (equal to voxel_ref's, test_hip_voxel.py) with point_size = voxel_size, from the novel cameras and from an input one"""
    name = 'mixed'
    cloud, rc = clouds(name, 'all')
    x, im, pan, info, cams, clean = scene_of(name)
    vs, opacity = SCENES[name][3], SCENES[name][2]
    rv = V.voxelize(rc['points'], rc['rgb'], rc['pan'], rc['index'], [s['id'] for s in rc['segments']], vs, default_colors(len(info) + 1), opacity)
    vox = cloud.voxelize(vs)
    assert len(vox) == len(rv['pan']) and 1 < len(vox) < len(cloud)
    for cs, f, shape in ((novel_cameras(), focal_of(NOVEL), NOVEL), ([cams[0]], focal_of((48, 64)), (48, 64))):
        want = R.render(rv['points'], rv['rgb'], rv['colors'], rv['pan'], cs, f, shape, point_size=vs)
        bare = R.render(rv['points'], rv['rgb'], rv['colors'], rv['pan'], cs, f, shape, point_size=0.0)
        check_decides(want, 'voxels of %s at %s' % (name, shape))
        grown = (want['index'] >= 0).sum(), (bare['index'] >= 0).sum()
        print('pixels hit with point_size = voxel_size: %d, with 0: %d' % grown)
        assert grown[0] > grown[1]                                             # the footprint closes holes
        assert_same(vox.render(cs, f, shape), want)
        assert_same(vox.render(cs, f, shape, point_size=0.0, radius=1), R.render(rv['points'], rv['rgb'], rv['colors'], rv['pan'], cs, f, shape, radius=1))


@pytest.mark.parametrize('name', list(SCENES))
def test_every_point_in_one_pixel(name):
    """maximum contention: a far camera with a tiny focal length; the winner is the restatement's"""
    cloud, rc = clouds(name, 'all')
    cam, shape = orbit_cameras((5.0, 5.0, 2.5), 1000.0, 1, 300.0), (5, 7)
    want = ref_render(rc, cam, 0.5, shape)
    assert (want['index'] >= 0).sum() == 1 and want['candidates'].max() == len(rc['index']) and want['index'][0, 2, 3] >= 0
    for precheck in (1, 0):
        old = hip.RENDER_PRECHECK
        try:
            hip.RENDER_PRECHECK = precheck
            assert_same(cloud.render(cam, 0.5, shape), want)
        finally:
            hip.RENDER_PRECHECK = old


def test_render_cameras_groups_the_shapes():
    name = 'mixed'
    cloud, rc = clouds(name, 'half')
    cams = scene_of(name)[4]
    cameras = [{'cam2world': torch.from_numpy(c), 'focal': focal_of(s), 'height': s[0], 'width': s[1]} for c, s in zip(cams, SCENES[name][0])]
    got = render_cameras(cloud, cameras, radius=1)
    assert len(got) == len(cameras) and len({(c['height'], c['width']) for c in cameras}) < len(cameras)      # some cameras share a shape
    for g, c, s in zip(got, cams, SCENES[name][0]):
        assert_equal_renders(g, render_cloud(cloud, [c], focal_of(s), s, radius=1))
        assert_same(g, ref_render(rc, [c], focal_of(s), s, radius=1))
    both = render_cloud(cloud, [cams[0], cams[3]], [focal_of((48, 64))] * 2, (48, 64), radius=1)               # ... and what a per-shape call gives
    assert_equal_renders(got[0], both[0])
    assert_equal_renders(got[3], both[1])


def test_calls_repeat_and_options_do_not_change_the_result(monkeypatch):
    cloud, rc = clouds('mixed', 'all')
    cams, f = novel_cameras(), focal_of(NOVEL)
    kw = dict(radius=1, point_size=0.2, max_radius=5, near=0.5, pp=(20.0, 21.5))
    want = ref_render(rc, cams, f, NOVEL, **kw)
    check_decides(want, 'options')
    a, b = render_cloud(cloud, cams, f, NOVEL, **kw), render_cloud(cloud, cams, f, NOVEL, **kw)
    assert_same(a, want)
    assert_equal_renders(a, b)                                                 # two calls: identical bytes
    monkeypatch.setattr(hip, 'RENDER_PRECHECK', 1 - hip.RENDER_PRECHECK)       # with and without the pre-check
    assert_equal_renders(a, render_cloud(cloud, cams, f, NOVEL, **kw))
    monkeypatch.setattr(render_mod, 'ZBUF_BYTES', 2 * 8 * NOVEL[0] * NOVEL[1])  # two cameras per launch
    assert_equal_renders(a, render_cloud(cloud, cams, f, NOVEL, **kw))
    # per-camera focals and principal points, cameras as one device tensor
    fs, pps = [f, 0.8 * f, 1.3 * f, f, 0.5 * f], [(25.5, 18.5), (20.0, 10.0), (30.0, 25.0), (0.0, 0.0), (25.0, 18.0)]
    got = render_cloud(cloud, torch.from_numpy(np.stack(cams)).to(cloud.pan.device), torch.tensor(fs), NOVEL, pp=pps)
    assert_same(got, ref_render(rc, cams, fs, NOVEL, pp=pps))
    # the holder
    h = a.cpu()
    assert h.index.device.type == 'cpu' and np.array_equal(bits(h.depth), bits(a.depth))
    u8 = np.floor((np.clip(want['colors'], F(0), F(1)) * F(255) + F(0.5)).astype(F)).astype(np.uint8)
    assert a.images_u8().dtype == torch.uint8 and np.array_equal(a.images_u8().cpu().numpy(), u8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render_cloud(cloud.cpu(), cams, f, NOVEL)


def test_nan_infinite_and_huge_points_are_left_out():
    shapes = [(32, 40), (40, 32)]
    scene = V.overlapping_scene(shapes, seed=6)
    x, cams = scene[0], scene[4]
    x[0]['pts3d'][3, 4, 1] = np.nan
    x[0]['pts3d'][3, 5, 0] = np.inf
    x[1]['pts3d'][7, 7, 2] = -np.inf
    x[1]['pts3d'][8, 8] = [3e38, 1e30, -2e25]
    x[1]['pts3d'][9, 9] = [3e38, 3e38, 3e38]
    info, colors = scene[3], default_colors(len(scene[3]) + 1)
    rc = C.cloud(*scene[:5], min_conf_thr=0.0, colors=colors)
    cloud = device_cloud(scene, 0.0, 0.5, colors)
    for v, shape in enumerate(shapes):
        want = ref_render(rc, [cams[v]], focal_of(shape), shape, radius=1)
        check_decides(want, 'bad points / view %d' % v)
        assert not np.isin(want['index'], [3 * 40 + 4, 3 * 40 + 5, 32 * 40 + 7 * 32 + 7, 32 * 40 + 8 * 32 + 8, 32 * 40 + 9 * 32 + 9]).any()
        assert_same(cloud.render([cams[v]], focal_of(shape), shape, radius=1), want)


@pytest.fixture(scope='module')
def bench_clouds():
    scene = V.overlapping_scene([(384, 512)] * 50, seed=4)
    x, im, pan, info, cams, clean = scene
    thr, colors = thresholds(scene)['all'], default_colors(len(info) + 1)
    return device_cloud(scene, thr, 0.5, colors), C.cloud(x, im, pan, info, cams, min_conf_thr=thr, opacity=0.5, colors=colors)


@pytest.mark.parametrize('radius', [0, 1])
def test_benchmark_shape(bench_clouds, radius):
    """50 views of 384 x 512 of one room, every point kept: about 9.8 M points on one 384 x 512 camera inside the room"""
    cloud, rc = bench_clouds
    assert len(cloud) == len(rc['index']) == 50 * 384 * 512
    shape = (384, 512)
    cam = orbit_cameras((5.0, 5.0, 2.2), 3.0, 1, 1.5)
    want = ref_render(rc, cam, focal_of(shape), shape, radius=radius)
    check_decides(want, 'benchmark shape / radius %d' % radius)
    assert_same(cloud.render(cam, focal_of(shape), shape, radius=radius), want)
