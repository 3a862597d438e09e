"""The host side of the mesh rasterisation (panst3r_amd/engine/mesh.py) and the properties of its contract, on the numpy restatement of tests/mesh_ref.py
alone (no GPU here): the top-left rule, exact and bounded depths, the camera table, validation, the PLY reader and the annotation rule."""
import functools

import numpy as np
import pytest
import torch

import abi_header
import mesh_ref as M
from camera_stage_cases import QUADS, inside_quad      # shared with the GPU cases of tests/test_hip_camera_stages.py
from panst3r_amd import hip
from panst3r_amd.engine import mesh as mesh_mod
from panst3r_amd.engine import render_mesh, ground_truth_maps, mesh_camera_table, load_ply_mesh, panoptic_vertex_ids, MeshRender
from panst3r_amd.engine.render import camera_table

F = np.float32
EYE = [np.eye(4)]


def pixel_camera(shape):
    """a camera whose u, v ARE the x, y of a vertex at z = 1: identity pose, focal 1, principal point 0"""
    return dict(cams2world=EYE, focals=1.0, shape=shape, pp=(0.0, 0.0), near=0.5, far=10.0)


def coverage(quads_as_faces, verts, shape):
    """how many faces cover each pixel centre: the candidates of the restatement"""
    r = M.render(verts, quads_as_faces, **pixel_camera(shape))
    return r['candidates'][0]


@pytest.mark.parametrize('quad', QUADS)
@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('diagonal', [0, 1])
def test_a_split_quad_covers_every_centre_inside_it_exactly_once(quad, reverse, diagonal):
    """the top-left rule: whichever diagonal splits the quad and however its corners are listed, a pixel centre strictly inside is covered by exactly one
    of the two triangles (also on the diagonal), one outside by none, one on the boundary by at most one"""
    H, W = 12, 16
    verts = np.array([(x, y, 1.0) for x, y in quad], dtype=F)
    faces = [(0, 1, 2), (0, 2, 3)] if diagonal == 0 else [(1, 2, 3), (1, 3, 0)]
    if reverse:
        faces = [f[::-1] for f in faces]
    n = coverage(faces, verts, (H, W))
    where = inside_quad(quad, H, W)
    assert (where == 1).sum() > 10 and ((where == 0).any() or quad is QUADS[2] or quad is QUADS[4])
    assert (n[where == 1] == 1).all() and (n[where == -1] == 0).all() and (n[where == 0] <= 1).all()


def test_quads_that_share_an_edge_through_pixel_centres_leave_no_crack_and_no_double_hit():
    H, W = 12, 16
    xs, ys = [1.5, 5.5, 9.5, 13.5], [1.5, 5.5, 9.5]
    verts = np.array([(x, y, 1.0) for y in ys for x in xs], dtype=F)
    k = lambda r, c: r * 4 + c
    faces = []
    for r in range(2):
        for c in range(3):
            a, b, d, e = k(r, c), k(r, c + 1), k(r + 1, c + 1), k(r + 1, c)
            faces += [(a, b, d), (a, d, e)] if (r + c) % 2 else [(b, d, e), (b, e, a)]
    n = coverage(faces, verts, (H, W))
    want = np.zeros((H, W), dtype=int)
    want[1:9, 1:13] = 1                                                        # centres 1.5 .. 8.5 x 1.5 .. 12.5: the top and left border in, the bottom and right out
    assert np.array_equal(n, want)


def test_a_fronto_parallel_face_renders_its_zc_exactly():
    """all zc equal: s = A / zc up to a few fp64 roundings (relative 2^-51), far below half an fp32 ulp (2^-25), so the rounded quotient IS zc"""
    verts = np.array([(1.25, 1.0, 3.3), (14.0, 2.5, 3.3), (6.0, 10.75, 3.3)], dtype=F)
    verts[:, :2] *= verts[:, 2:]                                               # u, v about the listed pixels
    r = M.render(verts, [(0, 1, 2)], EYE, 1.0, (12, 16), pp=(0.0, 0.0), near=0.5, far=10.0)
    hit = r['face'][0] == 0
    assert hit.sum() > 30 and (r['depth'][0][hit] == F(3.3)).all() and (r['depth'][0][~hit] == 0).all()


def test_plane_depth_is_the_ray_plane_depth_within_the_snapping_bound():
    """A tilted face.  The contract interpolates 1 / z between vertices whose screen positions were moved by at most d pixels per axis: d = 1 / 512 (the
    snap) + 2^-16 (two fp32 roundings of u < 64).  1 / z is affine on the screen, 1 / z = a u + b v + c; moving the three support points by at most d
    changes it inside the triangle by at most e = (|a| + |b|) d (the difference of two affine functions is affine: bounded by its corner values).  So
    |z' - z| <= z^2 e / (1 - z e), plus the final fp32 rounding z 2^-24."""
    fx, fy, cx, cy = 20.0, 23.0, 8.0, 6.0
    verts = np.array([(-0.9, -0.6, 2.0), (1.1, -0.4, 3.5), (0.1, 0.9, 2.75)], dtype=F)
    r = M.render(verts, [(0, 1, 2)], EYE, [[fx, fy]], (12, 16), pp=(cx, cy), near=0.5, far=10.0)
    p = verts.astype(np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    d = n @ p[0]
    a, b = n[0] / (d * fx), n[1] / (d * fy)
    e = (abs(a) + abs(b)) * (1 / 512 + 2.0 ** -16)
    hit = r['face'][0] == 0
    i, j = np.nonzero(hit)
    z = d / (n[0] * (j + 0.5 - cx) / fx + n[1] * (i + 0.5 - cy) / fy + n[2])
    bound = z * z * e / (1 - z * e) + z * 2.0 ** -24
    err = np.abs(r['depth'][0][hit].astype(np.float64) - z)
    print('%d pixels, slope (%.4f, %.4f) per pixel, largest error %.3e of a bound of %.3e' % (hit.sum(), a, b, err.max(), bound[err.argmax()]))
    assert hit.sum() > 20 and abs(a) + abs(b) > 1e-3 and (err <= bound).all()
    assert (err > 0).any()                                                     # a bound, not an identity


def test_bad_faces_and_the_planes():
    verts = np.array([(2.0, 2.0, 1.0), (10.0, 2.0, 1.0), (2.0, 10.0, 1.0), (np.nan, 0, 1.0), (4.0, 4.0, 0.4), (np.inf, 1.0, 1.0)], dtype=F)
    cam = pixel_camera((12, 16))
    good = M.render(verts, [(0, 1, 2)], **cam)
    assert (good['face'] == 0).sum() > 20
    for bad in ([(0, 1, 3)], [(0, 1, 6)], [(0, 1, -1)], [(0, 0, 1)], [(0, 1, 4)], [(0, 1, 5)]):      # NaN, indices, degenerate, behind near, infinite
        r = M.render(verts, bad, **cam)
        assert (r['face'] == -1).all() and (r['depth'] == 0).all() and (r['box'] == 0).all()
    assert (M.render(verts, [(0, 1, 2)], **dict(cam, far=0.9))['face'] == -1).all()          # beyond far
    assert (M.render(verts, [(0, 1, 2)], **dict(cam, near=1.5))['face'] == -1).all()         # nearer than near
    both = M.render(verts, [(0, 2, 1), (0, 1, 2)], **cam)                                    # no culling, equal depths: the smaller index
    assert np.array_equal(both['face'] == 0, good['face'] == 0) and (both['candidates'][both['face'] == 0] == 2).all()


def test_the_nearest_corner_gives_the_id_and_ties_go_to_the_first_listed():
    verts = np.array([(1.5, 2.0, 1.0), (9.5, 2.0, 1.0), (5.5, 10.0, 1.0)], dtype=F)      # symmetric about the centres u = 5.5
    cam = pixel_camera((12, 16))
    for faces, first in (([(0, 1, 2)], 10), ([(1, 0, 2)], 20), ([(2, 1, 0)], 20), ([(2, 0, 1)], 10)):
        r = M.render(verts, faces, vertex_ids=[10, 20, 30], **cam)
        assert r['ties'][0, 2, 5] and r['pan'][0, 2, 5] == first, faces          # the pixel centre (5.5, 2.5): corners 0 and 1 at equal distance
        assert r['pan'][0, 2, 2] == 10 and r['pan'][0, 2, 8] == 20 and r['pan'][0, 8, 5] == 30
        assert set(np.unique(r['pan'])) == {0, 10, 20, 30}                     # never a blend
    assert (M.render(verts, [(0, 1, 2)], face_ids=[7], **cam)['pan'].max() == 7) and (M.render(verts, [(0, 1, 2)], **cam)['pan'] == 0).all()


def test_area_filter():
    pan = np.zeros((2, 4, 5), dtype=np.int32)
    pan[0, :2] = 5; pan[0, 2, :3] = 9; pan[0, 3] = 7
    pan[1, 0, :2] = 5; pan[1, 1:] = 9
    out, counts = M.area_filter(pan, [9, 5], 3)
    assert counts.tolist() == [[3, 10], [15, 2]]
    assert (out[0] == np.where(pan[0] == 7, 0, pan[0])).all() and (out[1] == np.where(pan[1] == 9, 9, 0)).all()
    out0, _ = M.area_filter(pan, [9, 5], 0)
    assert (out0 == np.where(pan == 7, 0, pan)).all()                          # min_area = 0 only removes the unlisted id


def test_camera_table():
    rng = np.random.default_rng(1)
    cams = []
    for _ in range(3):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        c = np.eye(4)
        c[:3, :3], c[:3, 3] = q, rng.normal(size=3) * 3
        cams.append(c)
    shape = (37, 51)
    want = M.camera_table(cams, [[30.0, 31.5], [20.0, 20.0], [25.0, 24.0]], shape)
    got = mesh_camera_table(cams, [[30.0, 31.5], [20.0, 20.0], [25.0, 24.0]], shape)
    assert got.dtype == np.float32 and got.shape == (3, hip.MESH_CAM_FLOATS) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, :12], camera_table(cams, 1.0, shape)[:, :12])               # the twelve numbers of the render contract, unchanged
    assert np.array_equal(got[:, 14:], np.broadcast_to(F([25.5, 18.5]), (3, 2)))
    one = mesh_camera_table(torch.from_numpy(np.stack(cams)), 28.0, shape, pp=(20.0, 10.0))
    assert (one[:, 12:] == F([28.0, 28.0, 20.0, 10.0])).all()
    per = mesh_camera_table(cams, [28.0, 29.0, 30.0], shape, pp=[(1.0, 2.0), (3.0, 4.0), (5.0, 6.0)])
    assert per[:, 12].tolist() == per[:, 13].tolist() == [28.0, 29.0, 30.0] and per[:, 14:].tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    assert (mesh_camera_table(cams, [[28.0, 29.0]], shape)[:, 12:14] == F([28.0, 29.0])).all()
    for bad in (dict(focals=[1.0, 2.0]), dict(focals=-1.0), dict(focals=[[1.0, 2.0, 3.0]] * 3), dict(focals=float('nan')), dict(pp=(1.0, 2.0, 3.0)),
                dict(pp=(float('inf'), 0.0)), dict(focals=[[1.0, 0.0]])):
        with pytest.raises(ValueError):
            mesh_camera_table(cams, **dict(dict(focals=10.0, shape=shape), **bad))
    with pytest.raises(ValueError):
        mesh_camera_table([], 10.0, shape)
    with pytest.raises(ValueError):
        mesh_camera_table([np.eye(3)], 10.0, shape)
    with pytest.raises(ValueError):
        mesh_camera_table([np.full((4, 4), np.nan)], 10.0, shape)
    with pytest.raises(ValueError):
        mesh_camera_table([np.eye(4) * 1e39], 10.0, shape)


def test_render_mesh_validates_before_any_launch():
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    ok = dict(vertices=v, faces=f, cams2world=EYE, focals=10.0, shape=(8, 8))
    for bad in (dict(vertices=torch.zeros(4, 2)), dict(vertices=torch.zeros(4, 3, dtype=torch.int32)), dict(vertices=np.zeros((4, 3))), dict(faces=torch.zeros(1, 4, dtype=torch.int64)),
                dict(faces=torch.zeros(1, 3)), dict(faces=torch.zeros(0, 3, dtype=torch.int64)), dict(vertices=torch.zeros(0, 3)), dict(shape=(0, 8)),
                dict(shape=(2 ** 16, 2 ** 16)), dict(vertex_ids=torch.zeros(4, dtype=torch.int32), face_ids=torch.zeros(1, dtype=torch.int32)),
                dict(vertex_ids=torch.zeros(3, dtype=torch.int32)), dict(face_ids=torch.zeros(1)), dict(near=0.0), dict(near=1.0, far=1.0), dict(near=-1.0),
                dict(far=float('inf')), dict(far=1e39), dict(near=float('nan')), dict(focals=0.0), dict(cams2world=[])):
        with pytest.raises(ValueError):
            render_mesh(**dict(ok, **bad))
    with pytest.raises(RuntimeError, match='no CPU fallback'):                # valid, but on the CPU
        render_mesh(**ok)
    cams = M.camera_dicts(EYE, [(8, 8)])
    segs = [{'id': 5, 'category_id': 1}]
    for bad in (dict(min_area=-1), dict(min_area=2.5), dict(min_area=True), dict(cameras=[]), dict(segments=[{'id': 5, 'category_id': 1}, {'id': 5, 'category_id': 2}]),
                dict(segments=[{'id': 0, 'category_id': 1}]), dict(segments=[{'id': 3}]), dict(segments=[{'id': hip.EVAL_MAX_ID, 'category_id': 1}])):
        with pytest.raises(ValueError):
            ground_truth_maps(**dict(dict(vertices=v, faces=f, vertex_ids=torch.zeros(4, dtype=torch.int32), segments=segs, cameras=cams), **bad))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ground_truth_maps(v, f, np.zeros(4, dtype=np.int32), segs, cams)
    r = MeshRender(torch.zeros(2, 3, 4), torch.full((2, 3, 4), -1), torch.zeros(2, 3, 4, dtype=torch.int32))
    assert len(r) == 2 and not r.hit.any() and r[1].face.shape == (1, 3, 4) and r[-1].depth.shape == (1, 3, 4) and r.cpu().pan.shape == (2, 3, 4)


def write_ply(path, verts, faces, binary, index_type='int', extra=True):
    """a PLY as mesh tools write it: vertex colours after x y z (skipped by the reader), and optionally a per-face scalar in front of the list"""
    head = ['ply', 'format %s 1.0' % ('binary_little_endian' if binary else 'ascii'), 'comment made by the test', 'element vertex %d' % len(verts),
            'property float x', 'property float y', 'property float z'] + (['property uchar red', 'property double quality'] if extra else []) + \
           ['element face %d' % len(faces)] + (['property ushort flags'] if extra else []) + ['property list uchar %s vertex_indices' % index_type, 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode())
        if binary:
            vdt = np.dtype([('xyz', '<f4', (3,))] + ([('red', 'u1'), ('quality', '<f8')] if extra else []))
            v = np.zeros(len(verts), dtype=vdt)
            v['xyz'] = verts
            fh.write(v.tobytes())
            fdt = np.dtype(([('flags', '<u2')] if extra else []) + [('n', 'u1'), ('v', '<i4' if index_type == 'int' else '<u4', (3,))])
            f = np.zeros(len(faces), dtype=fdt)
            f['n'], f['v'] = 3, faces
            fh.write(f.tobytes())
        else:
            for p in verts:
                fh.write((' '.join(repr(float(x)) for x in p) + (' 200 0.5' if extra else '') + '\n').encode())
            for t in faces:
                fh.write((('7 ' if extra else '') + '3 %d %d %d\n' % tuple(t)).encode())


@pytest.mark.parametrize('extra', [False, True])
@pytest.mark.parametrize('index_type', ['int', 'uint'])
@pytest.mark.parametrize('binary', [False, True])
def test_ply_round_trip(tmp_path, binary, index_type, extra):
    rng = np.random.default_rng(2)
    verts, faces = rng.normal(size=(17, 3)).astype(F), rng.integers(0, 17, size=(9, 3))
    path = str(tmp_path / 'mesh.ply')
    write_ply(path, verts, faces, binary, index_type, extra)
    v, f = load_ply_mesh(path)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and tuple(v.shape) == (17, 3) and tuple(f.shape) == (9, 3)
    assert np.array_equal(v.numpy().view(np.uint32), verts.view(np.uint32)) and np.array_equal(f.numpy(), faces)


def test_ply_refusals(tmp_path):
    verts, faces = np.zeros((3, 3), dtype=F), np.array([[0, 1, 2]])
    good = str(tmp_path / 'good.ply')
    write_ply(good, verts, faces, binary=False)
    text = open(good).read()

    def refuse(name, content):
        p = str(tmp_path / name)
        with open(p, 'wb') as fh:
            fh.write(content if isinstance(content, bytes) else content.encode())
        with pytest.raises(ValueError):
            load_ply_mesh(p)
    refuse('a.ply', text.replace('ascii', 'binary_big_endian'))
    refuse('b.ply', text.replace('property float x', 'property double x'))
    refuse('c.ply', text.replace('property float z\n', ''))
    refuse('d.ply', text.replace('list uchar int', 'list ushort int'))
    refuse('e.ply', text.replace('7 3 0 1 2', '7 4 0 1 2 0'))                 # a quad
    refuse('f.ply', text.replace('element vertex 3', 'element edge 0\nelement vertex 3'))
    refuse('g.ply', 'not a ply\n')
    refuse('h.ply', text[:text.index('end_header') + 11] + '0 0 0 200 0.5\n')  # ends inside the vertices
    refuse('i.ply', text.replace('7 3 0 1 2\n', '7 3 0\n'))                   # ends inside the faces
    b = str(tmp_path / 'bin.ply')
    write_ply(b, verts, faces, binary=True)
    refuse('j.ply', open(b, 'rb').read()[:-4])


def test_panoptic_vertex_ids():
    seg_indices = [0, 0, 1, 2, 2, 3, 4, 4, 5]                                 # the over-segmentation: vertex -> segment
    groups = [{'label': 'chair', 'segments': [0, 1]},                         # inst 1
              {'label': 'alien', 'segments': [2]},                            # unknown: skipped, takes no instance number
              {'label': 'books', 'segments': [3]},                            # crowd: skipped
              {'label': 'table', 'segments': [1, 4]},                         # inst 2: overwrites segment 1
              {'label': 'chair', 'segments': [5]}]                            # inst 3
    segs, ids = panoptic_vertex_ids(seg_indices, groups, {'wall': 0, 'chair': 3, 'table': 7, 'books': 9}, crowd=('books',))
    assert ids.dtype == np.int32 and ids.tolist() == [259, 259, 519, 0, 0, 0, 519, 519, 771]
    assert [(s['id'], s['category_id'], s['instance_id'], s['label']) for s in segs] == [(259, 3, 1, 'chair'), (519, 7, 2, 'table'), (771, 3, 3, 'chair')]
    segs, ids = panoptic_vertex_ids(seg_indices, groups, {'chair': 3, 'books': 9}, cls_sep=1000)
    assert [s['id'] for s in segs] == [1003, 2009, 3003] and ids.tolist() == [1003, 1003, 1003, 0, 0, 2009, 0, 0, 3003]
    with pytest.raises(ValueError):
        panoptic_vertex_ids(seg_indices, groups, {'chair': 300})
    with pytest.raises(ValueError):
        panoptic_vertex_ids([0.5], groups, {'chair': 3})


def test_abi_is_unchanged_and_the_constants_agree():
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']
    assert hip.MESH_LANE_PIXELS == abi_header.defines()['PST_MESH_LANE_PIXELS'] == hip.mesh_lane_pixels()
    names = {p[0] for p in abi_header.prototypes()}
    mesh = {'pst_mesh_lane_pixels', 'pst_mesh_raster', 'pst_mesh_resolve', 'pst_mesh_area_count', 'pst_mesh_area_apply'}
    assert mesh <= names and mesh <= set(hip.SIGNATURES)
    code = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for name, ret, params in abi_header.prototypes():
        if name in mesh:
            assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
    assert hip.MESH_CAM_FLOATS == hip.RENDER_CAM_FLOATS == 16 and mesh_mod.ZBUF_BYTES > 0


@functools.lru_cache(maxsize=None)
def scene():
    return M.scene()


def test_the_scene_meets_the_conditions_the_gpu_tests_rely_on():
    """the generated scene, on the restatement: at most about 3 000 faces, and at 48 x 64 everything the GPU comparison is meant to exercise"""
    import test_hip_mesh as T
    s = scene()
    assert 2000 < len(s['faces']) <= 3100
    T.check_conditions(T.reference((48, 64)))
    cameras, (maps, segs, depths, counts) = T.reference_gt(1.0)
    assert 0 < len(segs) < len(s['segments']) and any(0 < n < T.MIN_AREA for c in counts for n in c)
    assert 0 < T.splat_reference()['pq'] <= 1                                  # the composition with the point renderer has something to score
