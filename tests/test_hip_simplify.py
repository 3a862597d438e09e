"""The mesh simplification on the GPU (csrc/simplify.hip and the voxel kernels it calls, panst3r_amd/engine/simplify.py) against the numpy restatement of
tests/simplify_ref.py: every output tensor and every stat BIT FOR BIT - integer work and the voxel stage's separately rounded operations leave no
tolerance to choose - then the hand-over to the mesh rasteriser, the PLY writer and reader, the islands, the normals and the 3-D score.

Conditions, not measurements: before the GPU is compared, `simplify_ref.scene_conditions` asserts ON THE RESTATEMENT that the hand-built scene (2 719
vertices: more than two 1 024-row workgroups of the voxel stage and a scan with a carry; 5 052 faces: twenty 256-face workgroups) holds what it was
built for - vertices no face uses (some inside an occupied cell), a NaN vertex and one beyond 2^20 cells each named by a face, cells with negative
coordinates, a vertex exactly on a cell wall, a cell with one member and one with 100 (a run across a wave's edge), a vote tie, a cell with void votes
only, faces with two and with three equal new corners, a face degenerate in the input, duplicates as a rotation, as a reversed winding (the reversed
copy first: its winding stays) and as a triple copy whose winner sits in a wave's last lane before a run of two in the next wave, duplicate pairs
split across workgroups (the two sheets), surviving faces with three, two and no equal ids.  (tests/test_simplify_host.py runs the same check
without a GPU.)"""
import functools

import numpy as np
import pytest
import torch

import mesh_ref
import simplify_ref as S
import surface_ref
from panst3r_amd.engine import PanopticMesh, FusedMesh, MeshRender, SimplifiedMesh, load_ply_mesh, score_reconstruction, simplify_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
KEYS = (('vertices', F), ('colors', F), ('vertex_ids', np.int32), ('faces', np.int32), ('face_ids', np.int32), ('quad', np.int64), ('src_face', np.int32),
        ('cluster', np.int32))
SEGMENTS = [{'id': i, 'query_id': i - 1, 'category_id': i % 3} for i in S.SEGMENT_IDS]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pose(deg, t):
    c = np.eye(4, dtype=F)
    c[:3, :3] = mesh_ref._rot(1, deg).astype(F)
    c[:3, 3] = t
    return c


SOURCE, NOVEL = _pose(0, (0.0, 0.0, -3.0)), _pose(-20, (-1.0, 0.2, -2.5))      # the sheets lie around the origin at z = 0.1


@functools.lru_cache(maxsize=None)
def scene():
    return S.scene()


@functools.lru_cache(maxsize=None)
def reference():
    """(with dedupe, without) of the scene by the restatement, after the conditions (computed once, shared, never written to)"""
    return S.scene_conditions(scene())


def device_mesh(sc, cls=PanopticMesh, segments=SEGMENTS, **kw):
    return cls(dev(sc['vertices']), dev(sc['faces']), torch.zeros(len(sc['faces']), dtype=torch.int32, device=DEV), dev(sc['vertex_ids']), dev(sc['colors']),
               dev(sc['quad']), [0, 7], segments, [SOURCE], **kw)


def assert_same(got, want, keys=KEYS):
    stats = got.simplify_stats if isinstance(got, PanopticMesh) else got.stats
    assert stats == want['stats'] and tuple(stats) == S.STAT_KEYS, (stats, want['stats'])
    for k, dtype in keys:
        g, w = getattr(got, k), want[k]
        assert g.is_cuda and tuple(g.shape) == w.shape and g.cpu().numpy().dtype == w.dtype == dtype, (k, tuple(g.shape), w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (k, int((bits(g) != bits(w)).sum()))


@pytest.mark.parametrize('dedupe', [True, False])
def test_every_output_and_every_stat_equals_the_restatement(dedupe):
    want = reference()[0 if dedupe else 1]
    mesh = device_mesh(scene())
    got = mesh.simplify(S.CELL, dedupe=dedupe)
    assert type(got) is PanopticMesh and len(got) == want['stats']['faces_out'] and got.vertices.shape[0] == want['stats']['vertices_out']
    assert_same(got, want)
    assert got.segments is mesh.segments and got.cameras is mesh.cameras and got.view_offsets == [0, 7]
    assert_same(mesh.simplify(S.CELL, dedupe=dedupe), want)                     # a second call: the same bytes
    if dedupe:
        assert_same(mesh.simplify(S.CELL), want)                                # the default


def test_two_calls_give_equal_bytes():
    mesh = device_mesh(scene())
    a, b = mesh.simplify(0.11), mesh.simplify(0.11)
    for k, _ in KEYS:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert a.simplify_stats == b.simplify_stats and 0 < len(a) < len(mesh)


def test_raw_tensors():
    sc = scene()
    listed = range(int(sc['vertex_ids'].max()) + 1)                             # with ids every non-negative id counts as listed: 99 votes here
    want = S.simplify(sc['vertices'], sc['colors'], sc['vertex_ids'], sc['faces'], np.zeros(len(sc['faces'])), listed, S.CELL)
    assert (want['vertex_ids'] == 99).any() and not (reference()[0]['vertex_ids'] == 99).any()
    got = simplify_mesh(dev(sc['vertices']), dev(sc['faces']).long(), S.CELL, colors=dev(sc['colors']), vertex_ids=dev(sc['vertex_ids']))
    assert isinstance(got, SimplifiedMesh)
    assert_same(got, want, [k for k in KEYS if k[0] != 'quad'])
    # without colours and ids: black, every vertex id 0
    zero = np.zeros_like(sc['vertices'])
    want = S.simplify(sc['vertices'], zero, np.zeros(len(zero)), sc['faces'], np.zeros(len(sc['faces'])), [], S.CELL, dedupe=False)
    got = simplify_mesh(dev(sc['vertices']), dev(sc['faces']), S.CELL, dedupe=False)
    assert_same(got, want, [k for k in KEYS if k[0] != 'quad'])
    assert not got.vertex_ids.any() and not got.face_ids.any() and not got.colors.any()


def assert_empty(got, M, stats):
    assert type(got) is PanopticMesh and len(got) == 0 and got.simplify_stats == stats
    for k, shape, dtype in (('vertices', (0, 3), torch.float32), ('colors', (0, 3), torch.float32), ('vertex_ids', (0,), torch.int32), ('faces', (0, 3), torch.int32),
                            ('face_ids', (0,), torch.int32), ('quad', (0,), torch.int64), ('src_face', (0,), torch.int32), ('cluster', (M,), torch.int32)):
        t = getattr(got, k)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda, k
    assert (got.cluster == -1).all() and not got.render([NOVEL], 20.0, (8, 8)).hit.any() and len(got.drop_small(2)) == 0


def test_a_mesh_without_faces_and_one_whose_every_face_collapses():
    sc = dict(scene(), faces=np.zeros((0, 3), np.int32), quad=np.zeros(0, np.int64))
    want = S.of_scene(sc)
    assert want['stats']['faces_in'] == 0 and want['stats']['vertices_in'] == len(sc['vertices'])
    assert_empty(device_mesh(sc).simplify(S.CELL), len(sc['vertices']), want['stats'])
    v = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1], [0.1, 0.4, 0.1], [0.1, 0.1, 0.4], [3.0, 3.0, 3.0]], dtype=F)
    tetra = {'vertices': v, 'colors': v, 'vertex_ids': np.ones(5, np.int32), 'faces': np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32),
             'quad': np.arange(4, dtype=np.int64)}
    want = S.of_scene(tetra, cell=1.0)
    assert want['stats']['faces_degenerate'] == 4 and want['stats']['vertices_used'] == 4 and want['stats']['vertices_out'] == 0
    for dedupe in (True, False):
        assert_empty(device_mesh(tetra).simplify(1.0, dedupe=dedupe), 5, want['stats'])
    nan = dict(tetra, vertices=np.full_like(v, np.nan))                          # every vertex left out: no new vertex at all
    want = S.of_scene(nan, cell=1.0)
    assert want['stats']['faces_left_out'] == 4 and want['stats']['vertices_left_out'] == 4
    assert_empty(device_mesh(nan).simplify(1.0), 5, want['stats'])


@pytest.mark.parametrize('M,Fn', [(1024, 256), (1025, 257)])
def test_exactly_one_workgroup_and_one_more(M, Fn):
    sc = S.random_mesh(M, Fn, seed=M)
    for cell, dedupe in ((0.5, True), (0.5, False), (2.5, True)):
        want = S.of_scene(sc, dedupe, cell=cell)
        assert 0 < want['stats']['faces_out'] and want['stats']['vertices_used'] < M
        assert_same(device_mesh(sc).simplify(cell, dedupe=dedupe), want)
    assert S.of_scene(sc, True, cell=2.5)["stats"]["faces_duplicate"] > 0


@pytest.mark.parametrize('bad', ['M', -1])
def test_a_corner_outside_the_vertices_is_refused_not_read(bad):
    sc = scene()
    faces = sc['faces'].copy()
    faces[len(faces) // 2, 1] = len(sc['vertices']) if bad == 'M' else -1
    with pytest.raises(ValueError):
        S.of_scene(dict(sc, faces=faces))
    for dedupe in (True, False):
        with pytest.raises(ValueError, match='outside the vertex rows'):
            device_mesh(dict(sc, faces=faces)).simplify(S.CELL, dedupe=dedupe)
    with pytest.raises(ValueError, match='outside the vertex rows'):
        simplify_mesh(dev(sc['vertices']), dev(faces).long() * (2 ** 32 + 1) if bad == 'M' else dev(faces), S.CELL)      # a corner beyond int32 does not wrap into range
    assert_same(device_mesh(sc).simplify(S.CELL), reference()[0])              # the device is as it was


# ---------------------------------------------------------------- composition
@functools.lru_cache(maxsize=None)
def reference_renders():
    want = reference()[0]
    return [surface_ref.render(want['vertices'], want, [c], f, shape) for c, f, shape in ((SOURCE, 40.0, (48, 64)), (NOVEL, 30.0, (40, 56)))]


def test_renders_of_the_simplified_mesh_equal_the_restatements():
    mesh = device_mesh(scene()).simplify(S.CELL)
    for (c, f, shape), want in zip(((SOURCE, 40.0, (48, 64)), (NOVEL, 30.0, (40, 56))), reference_renders()):
        assert (want['face'] >= 0).sum() > 200 and len(np.unique(want['pan'])) > 3
        got = mesh.render([c], f, shape)
        assert isinstance(got, MeshRender)
        for k in ('depth', 'face', 'pan'):
            g = getattr(got, k)
            assert tuple(g.shape) == want[k].shape and g.cpu().numpy().dtype == want[k].dtype and np.array_equal(bits(g), bits(want[k])), k


def test_ply_round_trip(tmp_path):
    mesh = device_mesh(scene()).simplify(S.CELL)
    path = mesh.write_ply(str(tmp_path / 'simplified.ply'))
    v, f = load_ply_mesh(path)
    assert np.array_equal(bits(v), bits(mesh.vertices)) and np.array_equal(f.numpy(), mesh.faces.cpu().numpy().astype(np.int64))
    raw = open(path, 'rb').read()
    assert len(raw) - raw.index(b'end_header\n') - 11 == 19 * mesh.vertices.shape[0] + 17 * len(mesh)


def test_the_stages_downstream_accept_the_result():
    sc, want = scene(), reference()[0]
    mesh = device_mesh(sc).simplify(S.CELL)
    comp = mesh.face_component().cpu().numpy()
    assert np.array_equal(comp, surface_ref.face_component(want['faces'], len(want['vertices'])))
    size = np.bincount(comp, minlength=len(want['vertices']))
    assert size.max() > 100 and (size[comp] < 4).any()                          # the sheet, and the lone triangles
    small = mesh.drop_small(4)
    assert 0 < len(small) < len(mesh) and small.vertices.data_ptr() == mesh.vertices.data_ptr()
    n = mesh.vertex_normals()
    assert tuple(n.shape) == tuple(mesh.vertices.shape) and bool(torch.isfinite(n).all()) and bool((n.norm(dim=1) > 0.99).any())
    r = score_reconstruction(small, dev(sc['vertices'][3:3 + S.N_SHEET ** 2]), dev(sc['faces'][:2 * (S.N_SHEET - 1) ** 2] - 3).long(), thresholds=[0.02, 0.3],
                             spacing=0.05, metric='surface')
    print('simplified sheet against the first sheet: precision %s recall %s' % (r['precision'], r['recall']))
    assert r["precision"][1] > 0.99 and r['recall'][1] > 0.9 and 0 < r['precision'][0] <= 1


def test_a_simplified_fused_mesh_is_a_panoptic_mesh():
    sc = scene()
    i32 = dict(dtype=torch.int32, device=DEV)
    fused = device_mesh(sc, FusedMesh, nodes=torch.zeros(1, 3, **i32), sdf=torch.zeros(1, device=DEV), weight=torch.zeros(1, **i32), tsdf_stats={}, voxel_size=0.1,
                        band=1, min_weight=1)
    got = fused.simplify(S.CELL)
    assert type(got) is PanopticMesh and not hasattr(got, 'nodes')
    assert_same(got, reference()[0])
