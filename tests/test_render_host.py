"""The host side of the cloud renderer (panst3r_amd/engine/render.py, csrc/render.hip), without a GPU: known answers that hold tests/render_ref.py - the
numpy restatement the kernels are compared with bit for bit in test_hip_render.py - to the contract itself; `orbit_cameras`; the argument checks of
`render_cloud`, which all come before any launch; and the library's new symbols."""
import ctypes
import types

import numpy as np
import pytest
import torch

import abi_header
import render_ref as R
import voxel_ref as V
from panst3r_amd.engine import render_cloud, render_cameras, orbit_cameras, CloudRender, PanopticCloud, VoxelCloud
from panst3r_amd.engine import render as render_mod

F = np.float32
EYE = [np.eye(4)]
SCENES = {'two views': ([(24, 32), (24, 32)], 2), 'mixed shapes': ([(48, 64), (64, 48), (37, 51), (48, 64), (30, 43)], 3)}      # those of test_hip_voxel.py


def render_points(points, shape, cams=EYE, focal=10.0, pan=None, **kw):
    """the restatement on bare points: rgb = the points, colors = their negatives, pan = row + 1 unless given"""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    pan = np.arange(1, len(p) + 1) if pan is None else pan
    return R.render(p, p, -p, pan, cams, focal, shape, **kw)


def assert_empty(out, sel=...):
    assert (out['index'][sel] == -1).all() and (out['depth'][sel] == 0).all() and (out['pan'][sel] == 0).all()
    assert (out['rgb'][sel] == 0).all() and (out['colors'][sel] == 0).all()


# ---------------------------------------------------------------- known answers on the restatement alone
@pytest.mark.parametrize('name', list(SCENES))
def test_a_view_re_rendered_from_its_own_camera_is_itself(name):
    """a view's local pointmap from the identity camera with the view's focal: pixel k holds point k, its z and its label, bit for bit"""
    shapes, seed = SCENES[name]
    x, im, pan, info, cams, clean = V.overlapping_scene(shapes, seed=seed)
    for v, (H, W) in enumerate(shapes):
        loc = x[v]['pts3d_local'].reshape(-1, 3)
        out = render_points(loc, (H, W), focal=0.55 * max(H, W), pan=pan[v].reshape(-1))
        assert np.array_equal(out['index'][0].reshape(-1), np.arange(H * W)), (name, v)
        assert np.array_equal(out['depth'][0].view(np.uint32), loc[:, 2].reshape(H, W).view(np.uint32))
        assert np.array_equal(out['pan'][0], pan[v]) and out['pan'].dtype == np.int32
        assert np.array_equal(out['rgb'][0].reshape(-1, 3), loc) and (out['candidates'] == 1).all()


def plane(z, H, W, f=10.0):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([(xs + 0.5 - W / 2) * z / f, (ys + 0.5 - H / 2) * z / f, np.full((H, W), z)], axis=-1).reshape(-1, 3).astype(F)


def test_the_nearer_of_two_planes_wins_and_ties_go_to_the_smaller_row():
    H, W = 6, 8
    far, near = plane(4.0, H, W), plane(2.0, H, W)
    for pts, first in ((np.concatenate([far, near]), H * W), (np.concatenate([near, far]), 0)):       # whichever comes first in the cloud
        out = render_points(pts, (H, W))
        assert np.array_equal(out['index'][0].reshape(-1), first + np.arange(H * W)) and (out['depth'] == 2.0).all() and (out['candidates'] == 2).all()
    # the identical point in rows 1, 3 and 4: the smallest row wins, wherever the copies stand
    p = np.array([[9, 9, 5], [0.05, 0.05, 3], [-9, 9, 5], [0.05, 0.05, 3], [0.05, 0.05, 3]], dtype=F)
    out = render_points(p, (H, W))
    assert out['index'][0, 3, 4] == 1 and out['candidates'][0, 3, 4] == 3 and out['pan'][0, 3, 4] == 2


def test_culled_and_off_screen_points_leave_no_trace():
    H, W = 6, 8
    p = np.array([[0, 0, -1], [0, 0, 0], [0, 0, 5e-4], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf], [0, 0, -np.inf], [0, 0, np.nan],
                  [50, 0, 1], [0, -50, 1], [3e38, 0, 1e-3], [1e30, 1e30, 1.0], [0.41, 0, 1.0], [-0.41, 0, 1.0], [0, 0.31, 1.0]], dtype=F)
    out = render_points(p, (H, W))
    assert_empty(out)
    assert out['behind'][0] == 3 and (out['candidates'] == 0).all()
    assert render_points(p[2:3], (H, W), near=1e-4)['index'][0, 3, 4] == 0          # the same point, inside a nearer near plane
    # `near` itself is kept
    assert render_points(np.array([[0, 0, 1e-3]], dtype=F), (H, W))['index'][0, 3, 4] == 0
    # the last pixel of each border is reached, one step further is outside
    q = np.array([[0.399, 0.299, 1.0], [-0.39, -0.29, 1.0]], dtype=F)
    out = render_points(q, (H, W))
    assert out['index'][0, 5, 7] == 0 and out['index'][0, 0, 0] == 1 and (out['index'] >= 0).sum() == 2


def test_a_footprint_at_the_border_is_clipped_not_wrapped():
    H, W = 6, 8
    p = np.array([[-0.39, 0.0, 1.0], [0.45, 0.29, 1.0]], dtype=F)                    # pixel (3, 0); pixel (5, 8): one column outside, its footprint reaches in
    out = render_points(p, (H, W), radius=1)
    want = np.full((H, W), -1)
    want[2:5, 0:2] = 0
    want[4:6, 7] = 1
    assert np.array_equal(out['index'][0], want)


@pytest.mark.parametrize('r', [0, 1, 3, 8])
def test_radius_paints_a_square(r):
    H, W = 21, 23
    out = render_points(np.array([[0.0, 0.0, 1.0]], dtype=F), (H, W), radius=r)
    hit = out['index'][0] >= 0
    assert hit.sum() == (2 * r + 1) ** 2 and hit[10 - r:10 + r + 1, 11 - r:11 + r + 1].all()
    assert (out['depth'][0][hit] == 1.0).all() and (out['pan'][0][hit] == 1).all()


def test_point_size_grows_the_footprint_as_depth_falls_up_to_max_radius():
    H, W, f, size = 41, 41, 10.0, 1.0
    for z, r in ((40.0, 0), (5.0, 1), (2.5, 2), (1.0, 5), (0.5, 8), (0.01, 8)):     # floor(f * size / 2 / z), capped by max_radius = 8
        out = render_points(np.array([[0.0, 0.0, z]], dtype=F), (H, W), focal=f, point_size=size)
        assert (out['index'][0] >= 0).sum() == (2 * r + 1) ** 2, (z, r)
    out = render_points(np.array([[0.0, 0.0, 0.5]], dtype=F), (H, W), focal=f, point_size=size, max_radius=3)
    assert (out['index'][0] >= 0).sum() == 49
    out = render_points(np.array([[0.0, 0.0, 40.0]], dtype=F), (H, W), focal=f, point_size=size, radius=2)      # `radius` is the minimum
    assert (out['index'][0] >= 0).sum() == 25
    out = render_points(np.array([[0.0, 0.0, 40.0]], dtype=F), (H, W), focal=f, point_size=size, radius=5, max_radius=3)
    assert (out['index'][0] >= 0).sum() == 49


def test_an_empty_cloud_gives_an_empty_render():
    out = render_points(np.zeros((0, 3), dtype=F), (5, 7), cams=EYE * 2)
    assert out['index'].shape == (2, 5, 7) and out['rgb'].shape == (2, 5, 7, 3) and out['depth'].dtype == F and out['index'].dtype == np.int64
    assert_empty(out)


def test_a_moved_camera_sees_what_the_moved_points_show():
    """the world -> camera step: rendering world points from a camera equals rendering the camera-frame points from the identity, up to the rounding of
    the transform - here an axis permutation, a translation by small integers and points on a grid of 2^-10, which are exact"""
    c2w = np.array([[0, 0, 1, 4], [1, 0, 0, -2], [0, 1, 0, 8], [0, 0, 0, 1]], dtype=np.float64)
    g = np.random.Generator(np.random.PCG64(5))
    local = (np.round((g.uniform(-1, 1, (200, 3)) * [2, 2, 1] + [0, 0, 4]) * 1024) / 1024).astype(F)          # multiples of 2^-10: the sums are exact
    world = (local.astype(np.float64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(F)
    a, b = render_points(local, (12, 16), pan=np.arange(200)), render_points(world, (12, 16), cams=[c2w], pan=np.arange(200))
    for k in ('index', 'depth', 'pan'):
        assert np.array_equal(a[k], b[k]), k
    assert (a['index'] >= 0).sum() > 50


# ---------------------------------------------------------------- orbit_cameras
@pytest.mark.parametrize('up', [(0, 0, 1), (0, 1, 0), (1, 2, -3)])
def test_orbit_cameras(up):
    target, n, radius, height = np.array([5.0, 4.0, 2.0]), 7, 3.0, 1.5
    cams = orbit_cameras(target, radius, n, height, up=up)
    assert len(cams) == n and all(c.shape == (4, 4) and c.dtype == np.float64 for c in cams)
    u = np.asarray(up, dtype=np.float64) / np.linalg.norm(up)
    eyes = np.stack([c[:3, 3] for c in cams])
    for c in cams:
        Rm, eye = c[:3, :3], c[:3, 3]
        assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12 and np.array_equal(c[3], [0, 0, 0, 1])
        to = target - eye
        assert np.allclose(Rm[:, 2], to / np.linalg.norm(to), atol=1e-12)             # z looks at the target
        assert abs(np.dot(Rm[:, 0], u)) < 1e-12 and np.dot(Rm[:, 1], u) < 0           # x is level, y points down
        d = eye - target
        assert abs(np.dot(d, u) - height) < 1e-12 and abs(np.linalg.norm(d - np.dot(d, u) * u) - radius) < 1e-12
    step = np.linalg.norm(eyes - np.roll(eyes, 1, axis=0), axis=1)
    assert np.allclose(step, 2 * radius * np.sin(np.pi / n), atol=1e-12)              # equally spaced: the chord of 2 pi / n
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(n=0), dict(radius=float('nan')), dict(up=(0, 0, 0))):
        with pytest.raises(ValueError):
            orbit_cameras(**{**dict(target=target, radius=radius, n=n, height=height, up=up), **bad})


def test_the_orbit_looks_at_the_room():
    """through the restatement: from every camera of a turntable around a small cluster of points, the cluster lands at the image centre"""
    g = np.random.Generator(np.random.PCG64(1))
    pts = (np.array([5.0, 5.0, 2.0]) + g.uniform(-0.05, 0.05, (50, 3))).astype(F)
    out = render_points(pts, (21, 31), cams=orbit_cameras((5, 5, 2), 4.0, 6, 2.0), focal=20.0)
    for b in range(6):
        ys, xs = np.nonzero(out['index'][b] >= 0)
        assert len(ys) and abs(ys.mean() - 10) <= 1 and abs(xs.mean() - 15) <= 1


# ---------------------------------------------------------------- render_cloud: every refusal comes before any launch
def cpu_cloud(M=10, device='cpu'):
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=device)
    return types.SimpleNamespace(points=e(M, 3), rgb=e(M, 3), colors=e(M, 3), pan=e(M, dt=torch.int32))


@pytest.fixture
def no_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a kernel was launched')
    monkeypatch.setattr(render_mod.hip, 'render_splat', refuse)
    monkeypatch.setattr(render_mod.hip, 'render_resolve', refuse)


def test_render_cloud_refuses_bad_arguments_before_any_launch(no_launch):
    from panst3r_amd import hip
    cloud, ok = cpu_cloud(), dict(cams2world=EYE, focals=10.0, shape=(6, 8))
    lim = hip.RENDER_MAX_RADIUS
    bad = [dict(cams2world=[]), dict(cams2world=np.zeros((0, 4, 4))), dict(cams2world=[np.eye(3)]), dict(cams2world=[np.eye(4)[:3]]),
           dict(cams2world=np.eye(4)), dict(cams2world=[np.eye(4), np.eye(4)[:3]]), dict(cams2world=[np.full((4, 4), np.nan)]),
           dict(focals=0.0), dict(focals=-3.0), dict(focals=float('nan')), dict(focals=float('inf')), dict(focals=[10.0, 11.0]),
           dict(near=0.0), dict(near=-1e-3), dict(near=float('nan')), dict(near=float('inf')), dict(near=1e-60),
           dict(radius=-1), dict(radius=lim + 1), dict(radius=1.5), dict(max_radius=-1), dict(max_radius=lim + 1),
           dict(point_size=-1.0), dict(point_size=float('nan')), dict(point_size=float('inf')),
           dict(shape=(0, 8)), dict(shape=(6, -1)), dict(shape=(2 ** 16, 2 ** 16)), dict(pp=(1.0, float('nan'))), dict(pp=(1.0, 2.0, 3.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            render_cloud(cloud, **{**ok, **kw})
    with pytest.raises(ValueError, match='2\\^32'):
        render_cloud(cpu_cloud(2 ** 32, device='meta'), **ok)
    # and with good arguments a CPU cloud is refused, as every stage refuses it
    for kw in (dict(), dict(radius=lim, max_radius=lim), dict(radius=0, max_radius=0, point_size=0.3, pp=(4.0, 3.0), near=0.5), dict(cams2world=np.stack(EYE * 3))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            render_cloud(cloud, **{**ok, **kw})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render_cloud(cpu_cloud(0), **ok)
    cams = [{'cam2world': torch.eye(4), 'focal': 10.0, 'height': 6, 'width': 8}, {'cam2world': torch.eye(4), 'focal': 12.0, 'height': 8, 'width': 6}]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        render_cameras(cloud, cams)
    with pytest.raises(ValueError):
        render_cameras(cloud, [dict(cams[0], focal=-1.0)])
    for cls in (PanopticCloud, VoxelCloud):
        assert callable(cls.render)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PanopticCloud(cloud.points, cloud.points, cloud.rgb, cloud.pan, cloud.colors, torch.zeros(10, dtype=torch.int64), [0, 10], []).render(EYE, 10.0, (6, 8))


def test_the_hip_wrappers_refuse_cpu_tensors():
    from panst3r_amd import hip
    cloud = cpu_cloud()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.render_splat(cloud.points, torch.zeros(1, 16), 6, 8, 0.0, 0, 8, torch.zeros(1, 6, 8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        z = torch.zeros(48, dtype=torch.int64)
        hip.render_resolve(z, cloud.rgb, cloud.colors, cloud.pan, z, torch.zeros(48), torch.zeros(48, dtype=torch.int32), torch.zeros(48, 3), torch.zeros(48, 3))


def test_the_camera_table_is_the_restatements():
    """the product's host step 1 and the restatement's agree to the bit, and hold the inverse of the pose"""
    g = np.random.Generator(np.random.PCG64(2))
    cams = orbit_cameras(g.uniform(-3, 3, 3), 2.5, 5, 0.7, up=(0.2, -0.1, 1.0))
    f, pp = [20.0, 21.5, 19.0, 33.0, 8.0], g.uniform(0, 30, (5, 2))
    for kw in (dict(), dict(pp=pp), dict(pp=pp[0], near=0.25)):
        a, b = render_mod.camera_table(cams, f, (37, 51), **kw), R.camera_table(cams, f, (37, 51), **kw)
        assert a.dtype == F and a.shape == (5, 16) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    a = render_mod.camera_table([torch.from_numpy(c) for c in cams], 20.0, (37, 51))
    assert np.array_equal(a[:, 12:], np.array([[20.0, 25.5, 18.5, F(1e-3)]] * 5, dtype=F))
    for c, row in zip(cams, a):
        w2c = np.linalg.inv(c)[:3]
        assert np.allclose(row[:12].reshape(3, 4), w2c, atol=1e-6)


def test_cloud_render_holder():
    r = CloudRender(torch.tensor([[[0.0, 2.0]]]), torch.tensor([[[0, 3]]], dtype=torch.int32), torch.zeros(1, 1, 2, 3), torch.tensor([[[[0.0, 0, 0], [0.5, 1.2, -1]]]]),
                    torch.tensor([[[-1, 4]]]))
    assert r.hit.tolist() == [[[False, True]]] and len(r) == 1 and r.cpu().index.tolist() == [[[-1, 4]]]
    assert r.images_u8().dtype == torch.uint8 and r.images_u8().tolist() == [[[[0, 0, 0], [128, 255, 0]]]]
    assert r[0].depth.shape == (1, 1, 2) and r[-1].pan.tolist() == [[[0, 3]]]


# ---------------------------------------------------------------- the library
def test_the_library_exports_the_render_entry_points():
    from panst3r_amd.build import build
    from panst3r_amd import hip
    lib = ctypes.CDLL(build(verbose=False))
    names = ('pst_render_max_radius', 'pst_render_splat', 'pst_render_resolve')
    protos = {p[0]: p for p in abi_header.prototypes()}
    for n in names:
        assert hasattr(lib, n) and n in hip.SIGNATURES and n in hip.EXPORTS and n in protos, n
    code = {'int': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for n in names:
        _, ret, params = protos[n]
        assert hip.SIGNATURES[n] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), n
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION'] == hip.lib().pst_abi_version()
    assert hip.render_max_radius() == hip.RENDER_MAX_RADIUS == abi_header.defines()['PST_RENDER_MAX_RADIUS'] >= 8
    # the entry points refuse what the contract excludes (no launch: the checks come first)
    L = hip.lib()
    assert L.pst_render_splat(None, 10, None, 1, 6, 8, 0.0, 0, 8, None, 1, None) != 0 and b'null' in L.pst_last_error()
    for args in ((0, 1, 6, 8, 0.0, 0, 8), (2 ** 32, 1, 6, 8, 0.0, 0, 8), (10, 0, 6, 8, 0.0, 0, 8), (10, 1, 0, 8, 0.0, 0, 8), (10, 4, 2 ** 15, 2 ** 15, 0.0, 0, 8),
                 (10, 1, 6, 8, -1.0, 0, 8), (10, 1, 6, 8, float('nan'), 0, 8), (10, 1, 6, 8, 0.0, -1, 8), (10, 1, 6, 8, 0.0, 0, hip.RENDER_MAX_RADIUS + 1)):
        M, B, H, W, half, r, mr = args
        assert L.pst_render_splat(None, M, None, B, H, W, half, r, mr, None, 1, None) != 0, args    # (the shape checks come before the null check)
        assert b'render_splat' in L.pst_last_error() and b'null' not in L.pst_last_error()
    none = (None,) * 8
    assert L.pst_render_resolve(None, 0, 10, *none, None) != 0 and L.pst_render_resolve(None, 48, 0, *none, None) != 0 and L.pst_render_resolve(None, 2 ** 31, 10, *none, None) != 0
    assert b'null' not in L.pst_last_error()
    assert L.pst_render_resolve(None, 48, 10, *none, None) != 0 and b'null' in L.pst_last_error()
