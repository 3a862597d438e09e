"""The host side of the surface mesh (panst3r_amd/engine/surface.py) and the properties of its contract, on the numpy restatement of
tests/surface_ref.py alone (no GPU here): face counts, windings, the valence of a regular triangulation, order, the islands, the ABI rows and the
wrappers' refusals."""
import functools
import types

import numpy as np
import pytest
import torch

import abi_header
import surface_ref as S
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_mesh, PanopticMesh, PanopticCloud
from panst3r_amd.engine import surface as surface_mod

F = np.float32
SURFACE = {'pst_surface_rows', 'pst_surface_count', 'pst_surface_emit', 'pst_surface_link', 'pst_surface_components', 'pst_surface_keep_count',
           'pst_surface_keep_emit'}


@functools.lru_cache(maxsize=None)
def grid(h, w, force=None):
    sc = S.grid_scene(h, w)
    return sc, S.of_scene(sc, 1.0, force_diagonal=force)


@pytest.mark.parametrize('h,w', [(2, 2), (5, 7), (12, 9)])
def test_a_fully_kept_smooth_grid_is_fully_triangulated(h, w):
    sc, (cloud, m) = grid(h, w)
    assert len(cloud['index']) == h * w and len(m['faces']) == 2 * (h - 1) * (w - 1)
    assert (m['corners'] == 4).all() and m['keep'].all()
    assert m['faces'].dtype == np.int32 and m['face_ids'].dtype == np.int32 and m['quad'].dtype == np.int64
    assert (m['face_ids'] == 1).all()
    local = sc[0][0]['pts3d_local'].reshape(-1, 3)
    assert (S.winding_z(local, m['faces']) < 0).all()                          # every face is wound towards the source camera
    assert (np.diff(m['quad']) >= 0).all()                                     # by quad in raster order ...
    q = m['quad'].reshape(-1, 2)
    assert (q[:, 0] == q[:, 1]).all() and (np.diff(q[:, 0]) > 0).all()         # ... T0 then T1 of each
    yy, xx = np.divmod(q[:, 0], w)
    assert (yy < h - 1).all() and (xx < w - 1).all() and (m['faces'][::2, 0] == q[:, 0]).all()    # corner a of every T0 is the quad's pixel


@pytest.mark.parametrize('force', ['ad', 'bc'])
def test_every_winding_faces_the_camera_and_an_interior_pixel_has_six_faces(force):
    h, w = 7, 9
    sc, (cloud, m) = grid(h, w, force)
    assert m['bc'].all() == (force == 'bc') and m['bc'].any() == (force == 'bc')
    assert (S.winding_z(sc[0][0]['pts3d_local'].reshape(-1, 3), m['faces']) < 0).all()
    valence = np.bincount(m['faces'].reshape(-1), minlength=h * w).reshape(h, w)
    assert (valence[1:-1, 1:-1] == 6).all() and valence.sum() == 3 * len(m['faces'])


def test_the_three_corner_triangles_face_the_camera_too():
    sc = S.grid_scene(2, 2)
    for missing, want in ((3, (0, 2, 1)), (0, (1, 2, 3)), (1, (0, 2, 3)), (2, (0, 3, 1))):
        conf = np.full((2, 2), 5.0, dtype=F)
        conf.reshape(-1)[missing] = 0
        x = [dict(sc[0][0], conf=conf)]
        cloud, m = S.of_scene((x,) + sc[1:], 1.0)
        pixel = cloud['index'][m['faces'][0]]                                  # rows -> pixels of the view
        assert len(m['faces']) == 1 and tuple(pixel) == want and not m['has'][0, 1]
        assert S.winding_z(sc[0][0]['pts3d_local'].reshape(-1, 3), [pixel])[0] < 0


def test_the_cut_and_the_face_id_rule():
    k = S.depth_bound(0.1)
    assert k == F(1.1) and S.depth_bound(0.0) == 1 and np.isinf(S.depth_bound(None))
    z = np.array([[1, 1], [S.EQ, 1]], dtype=F)
    one = lambda z, pan=(1, 1, 1, 1), ratio=0.1: S.mesh(np.arange(4), np.asarray(pan, dtype=np.int32), [(2, 2)], [np.asarray(z, dtype=F)], ratio)
    assert len(one(z)['faces']) == 2                                           # equality keeps
    z[1, 0] = np.nextafter(S.EQ, F(2))
    m = one(z)                                                                 # c one float32 higher: T0 = (a, c, d) goes, T1 = (a, d, b) stays
    assert m['faces'].tolist() == [[0, 3, 1]] and len(one(z, ratio=None)['faces']) == 2 and len(one(z, ratio=0.0)['faces']) == 1
    for bad in (0.0, -1.0, np.nan):
        z[1, 0] = bad
        assert one(z, ratio=None)['faces'].tolist() == [[0, 3, 1]]             # zmin > 0 and NaN hold without a cut as well
    z[1, 0] = np.inf
    assert len(one(z, ratio=None)['faces']) == 2 and len(one(z)['faces']) == 1
    flat = np.ones((2, 2), dtype=F)
    assert one(flat, (5, 5, 7, 9))['face_ids'].tolist() == [0, 5]              # (a, c, d) = 5 7 9 -> void; (a, d, b) = 5 9 5 -> 5
    assert one(flat, (5, 6, 7, 7))['face_ids'].tolist() == [7, 0]


def test_islands_and_drop_small():
    sc, (cloud, m) = grid(5, 7)
    M = len(cloud['index'])
    assert (S.face_component(m['faces'], M) == 0).all()
    for n in (1, 48):
        d = S.drop_small(m, M, n)
        assert all(np.array_equal(d[k], m[k]) for k in ('faces', 'face_ids', 'quad'))                 # 1 (and the patch's own size) keep everything
    assert len(S.drop_small(m, M, 49)['faces']) == 0
    faces = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8], [9, 10, 11], [11, 12, 6], [13, 14, 15]])     # a chain through vertex 2; a ring closed late; one alone
    comp = S.face_component(faces, 16)
    assert comp.tolist() == [0, 0, 6, 6, 6, 13]
    assert S.drop_small({'faces': faces, 'face_ids': np.arange(6), 'quad': np.arange(6)}, 16, 2)['face_ids'].tolist() == [0, 1, 2, 3, 4]
    assert S.face_component(np.zeros((0, 3), dtype=np.int32), 4).shape == (0,)


def test_abi_is_unchanged_and_the_prototype_table_matches():
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']
    assert hip.SURFACE_WG == abi_header.defines()['PST_SURFACE_WG']
    names = {p[0] for p in abi_header.prototypes()}
    assert SURFACE <= names and SURFACE <= set(hip.SIGNATURES)
    code = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for name, ret, params in abi_header.prototypes():
        if name in SURFACE:
            assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
    assert [n for n in hip.SIGNATURES if n.startswith('pst_surface_')] == [p[0] for p in abi_header.prototypes() if p[0].startswith('pst_surface_')]


def hand_cloud(source=None):
    z3, z1 = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    return PanopticCloud(z3, z3, z3, z1, z3, torch.arange(4), [0, 4], [], source=source)


def test_refusals_before_any_launch():
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        panoptic_mesh(hand_cloud())
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        hand_cloud().mesh()
    src = types.SimpleNamespace(N=4, shapes=[(2, 2)], table=None)
    for bad in (-0.1, float('nan'), float('inf'), -1, True, 'a', [0.1]):
        with pytest.raises(ValueError, match='max_depth_ratio'):
            panoptic_mesh(hand_cloud(src), max_depth_ratio=bad)
        with pytest.raises(ValueError, match='max_depth_ratio'):
            hand_cloud().mesh(max_depth_ratio=bad)                             # the argument is checked first
    with pytest.raises(RuntimeError, match='no CPU fallback'):                 # valid, but on the CPU
        panoptic_mesh(hand_cloud(src))
    with pytest.raises(ValueError, match='2\\^30'):
        panoptic_mesh(_too_large())
    assert surface_mod._depth_bound(None) == float('inf') and surface_mod._depth_bound(0.1) == float(F(1.1)) and surface_mod._depth_bound(0) == 1.0


def _too_large():
    c = hand_cloud(types.SimpleNamespace(N=2 ** 30 + 1, shapes=[(2, 2)], table=None))
    c.pan = types.SimpleNamespace(is_cuda=True, device='cuda:0', shape=(4,))    # the size check comes before any tensor is touched
    return c


def cpu_mesh(F_=2):
    i32 = torch.int32
    return PanopticMesh(torch.zeros(4, 3), torch.zeros(F_, 3, dtype=i32), torch.zeros(F_, dtype=i32), torch.zeros(4, dtype=i32), torch.zeros(4, 3),
                        torch.zeros(F_, dtype=torch.int64), [0, 4], [])


def test_mesh_object_and_min_faces():
    m = cpu_mesh()
    assert len(m) == 2 and len(m.cpu()) == 2 and len(cpu_mesh(0)) == 0
    for bad in (0, -3, True, False, 2.0, 1.5, '2', None):
        with pytest.raises(ValueError, match='min_faces'):
            m.drop_small(bad)
    for call in (lambda: m.drop_small(1), m.face_component, lambda: m.render([np.eye(4)], 10.0, (4, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_the_scene_meets_the_conditions_the_gpu_tests_rely_on():
    import test_hip_surface as T
    T.check_conditions()
    T.check_plane()
    T.check_strip()
