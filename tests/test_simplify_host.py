"""The numpy restatement of the mesh simplification (tests/simplify_ref.py) held to closed forms worked out on paper, the scene of the GPU test held to
the cases it was built for, and the refusals of panst3r_amd/engine/simplify.py that need no GPU.

The plane: (2k+1) x (2k+1) vertices, vertex (i, j) at ((i + 0.5) s, (j + 0.5) s, z), cells of edge 2 s, here s = 0.5 so that every number is exact in
float32 (inv = 1).  Along an axis vertex i lies in cell i // 2: cells 0 .. k-1 hold two vertices each, at offsets 0.25 and 0.75 of the cell, cell k holds
vertex 2k alone at offset 0.25.  So there are (k+1)^2 new vertices; new vertex (a, b) is the mean of its members: x = a + 0.5 for a < k, k + 0.25 for
a = k.  z = 0.3: the in-cell offset is floor(float32(0.3) * 65536) = 19660 sixteen-bit steps, the new z = 19660 / 65536 exactly.  A cell's smallest
member row is (2b) (2k+1) + 2a, ascending in (b, a): new vertex (a, b) is row b (k+1) + a.  A grid square (i, j) has its four corners in four different
cells iff i and j are both odd (i = 2a+1, j = 2b+1: k^2 squares); any other square has at most two cells under it, and both its triangles collapse.
So 2 k^2 faces survive, no two on the same corners, in the order of (b, a): (a,b) (a,b+1) (a+1,b+1) and (a,b) (a+1,b+1) (a+1,b)."""
import numpy as np
import pytest
import torch

import simplify_ref as S
from panst3r_amd import hip
from panst3r_amd.engine import PanopticMesh, simplify_mesh
from panst3r_amd.engine import simplify as E

F = np.float32
K, SP = 3, 0.5


def plane(copies=1, dedupe=True):
    v, f = S.grid_plane(K, SP)
    n = len(v)
    v, f = np.concatenate([v] * copies), np.concatenate([f + c * n for c in range(copies)])
    return S.simplify(v, np.full(v.shape, 0.5, F), np.ones(len(v), np.int32), f, np.arange(len(f)), [1], 2 * SP, dedupe)


def plane_expected():
    axis = np.array([a + 0.5 for a in range(K)] + [K + 0.25], dtype=F)
    verts = np.array([[axis[a], axis[b], 19660.0 / 65536.0] for b in range(K + 1) for a in range(K + 1)], dtype=F)
    row = lambda a, b: b * (K + 1) + a
    faces = []
    for b in range(K):
        for a in range(K):
            faces += [(row(a, b), row(a, b + 1), row(a + 1, b + 1)), (row(a, b), row(a + 1, b + 1), row(a + 1, b))]
    return verts, np.array(faces, dtype=np.int32)


def test_the_plane_in_closed_form():
    r = plane()
    verts, faces = plane_expected()
    assert len(verts) == (K + 1) ** 2 and len(faces) == 2 * K * K
    assert r['vertices'].dtype == F and np.array_equal(r['vertices'], verts)
    assert np.array_equal(r['faces'], faces) and (r['face_ids'] == 1).all() and (r['vertex_ids'] == 1).all()
    n = 2 * K + 1
    assert r['stats'] == dict(vertices_in=n * n, vertices_used=n * n, vertices_left_out=0, vertices_out=(K + 1) ** 2, faces_in=2 * (n - 1) ** 2, faces_left_out=0,
                              faces_degenerate=2 * (n - 1) ** 2 - 2 * K * K, faces_duplicate=0, faces_out=2 * K * K)
    assert np.array_equal(r['colors'], np.full((len(verts), 3), F(128.0 / 255.0)))          # 0.5 quantises to 128


def test_two_coincident_sheets_weld():
    verts, faces = plane_expected()
    r = plane(copies=2)
    assert np.array_equal(r['vertices'], verts) and np.array_equal(r['faces'], faces)
    assert r['stats']['faces_out'] == 2 * K * K == r['stats']['faces_duplicate'] and r['stats']['vertices_out'] == (K + 1) ** 2
    assert (r['src_face'] < 2 * (2 * K) ** 2).all()                             # the first sheet's faces win
    r0 = plane(copies=2, dedupe=False)
    assert r0['stats']['faces_out'] == 4 * K * K and r0['stats']['faces_duplicate'] == 0 and np.array_equal(r0['faces'], np.concatenate([faces, faces]))


def test_a_tetrahedron_inside_one_cell_vanishes():
    v = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.1], [0.1, 0.4, 0.1], [0.1, 0.1, 0.4]], dtype=F)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    r = S.simplify(v, v, np.zeros(4), f, np.arange(4), [], 1.0)
    assert r['vertices'].shape == (0, 3) and r['faces'].shape == (0, 3) and (r['cluster'] == -1).all()
    assert r['stats']['faces_degenerate'] == 4 and r['stats']['faces_out'] == 0 and r['stats']['vertices_out'] == 0 and r['stats']['vertices_used'] == 4


def test_a_cell_so_small_that_every_vertex_is_alone():
    g = np.random.Generator(np.random.PCG64(1))
    v = (np.arange(40)[:, None] * 0.37 + g.uniform(0, 0.1, (40, 3))).astype(F)
    used = np.array([1, 2, 3, 5, 8, 13, 21, 34, 39])
    f = np.stack([g.permutation(used)[:3] for _ in range(12)])
    f = f[np.unique(np.sort(f, axis=1), axis=0, return_index=True)[1]]          # no two faces on the same corners
    r = S.simplify(v, np.zeros_like(v), np.zeros(40), f, np.arange(len(f)), [], 1e-3)
    named = np.unique(f)
    rank = np.full(40, -1)
    rank[named] = np.arange(len(named))
    assert np.array_equal(r['faces'], rank[f]) and np.array_equal(r['cluster'], rank) and r['stats']['vertices_out'] == len(named)
    assert np.abs(r['vertices'] - v[named]).max() < 1e-3                        # inside the vertex's own cell


def test_the_vote_tie_and_the_void_rule():
    # three cells, one vertex triple each; ids per cell: {5, 3, 5, 3} -> 3 (a tie goes to the smaller id), {0, 99, -1} -> 0 (void only),
    # {0, 0, 8} -> 8 (void wins only alone)
    ids = [5, 3, 5, 3, 0, 99, -1, 0, 0, 8]
    v = np.array([[0.1 + 0.1 * k, 0.5, 0.5] for k in range(4)] + [[1.1 + 0.1 * k, 0.5, 0.5] for k in range(3)] + [[2.1 + 0.1 * k, 0.5, 0.5] for k in range(3)], dtype=F)
    f = np.array([[0, 4, 7], [1, 5, 8], [2, 6, 9], [3, 4, 7]])
    r = S.simplify(v, np.zeros_like(v), ids, f, np.arange(4), [3, 5, 8], 1.0)
    assert r['vertex_ids'].tolist() == [3, 0, 8] and r['faces'].tolist() == [[0, 1, 2]] and r['face_ids'].tolist() == [0] and r['stats']['faces_duplicate'] == 3
    r = S.simplify(v, np.zeros_like(v), ids, f, np.arange(4), [3, 8], 1.0)      # 5 is not listed any more: 3 wins alone
    assert r['vertex_ids'].tolist() == [3, 0, 8]
    r = S.simplify(v, np.zeros_like(v), [5, 5, 5, 3, 8, 8, 0, 0, 0, 8], f, np.arange(4), [3, 5, 8], 1.0)
    assert r['vertex_ids'].tolist() == [5, 8, 8] and r['face_ids'].tolist() == [8]


def test_the_scene_of_the_gpu_test_holds_its_cases():
    S.scene_conditions(S.scene())


def test_the_restatement_refuses_a_bad_corner():
    v = np.zeros((3, 3), F)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            S.simplify(v, v, np.zeros(3), [[0, 1, bad]], [0], [], 1.0)


def cpu_mesh():
    v, f = S.grid_plane(1, 0.5)
    t = torch.from_numpy
    return PanopticMesh(t(v), t(f), torch.zeros(len(f), dtype=torch.int32), torch.zeros(len(v), dtype=torch.int32), t(v), torch.zeros(len(f), dtype=torch.int64), [0],
                        [], None)


@pytest.mark.parametrize('cell', [0, -1.0, float('nan'), float('inf'), 1e-60, 1e60, 'a', None, True])
def test_cell_size_is_refused_before_anything_else(cell):
    m = cpu_mesh()
    with pytest.raises(ValueError, match='cell_size'):
        m.simplify(cell)
    with pytest.raises(ValueError, match='cell_size'):
        simplify_mesh(m.vertices, m.faces, cell)


def test_a_cpu_mesh_raises():
    m = cpu_mesh()
    with pytest.raises(RuntimeError, match='GPU only'):
        m.simplify(0.5)
    with pytest.raises(RuntimeError, match='GPU only'):
        simplify_mesh(m.vertices, m.faces, 0.5)
    with pytest.raises(ValueError, match='faces'):
        simplify_mesh(m.vertices, m.faces.float(), 0.5)


def test_the_cap_of_dedupe_names_the_limit_and_the_two_ways_out():
    assert hip.SIMPLIFY_MAX_KEYED == 2 ** 21 - 2 == S.MAX_KEYED
    E.check_dedupe_cap(2 ** 21 - 2, 0.01)
    with pytest.raises(ValueError) as e:
        E.check_dedupe_cap(2 ** 21 - 1, 0.01)
    msg = str(e.value)
    assert '2^21 - 2' in msg and 'larger cell_size' in msg and 'dedupe=False' in msg and str(2 ** 21 - 1) in msg


def test_a_bad_corner_is_a_value_error_and_a_full_table_a_runtime_error():
    E.check_simplify_status(0)
    with pytest.raises(ValueError, match='outside the vertex rows'):
        E.check_simplify_status(hip.SIMPLIFY_RANGE)
    with pytest.raises(ValueError):
        E.check_simplify_status(hip.SIMPLIFY_RANGE | hip.SIMPLIFY_FULL)
    with pytest.raises(RuntimeError, match='ran full'):
        E.check_simplify_status(hip.SIMPLIFY_FULL)


def test_the_stats_keys():
    assert E.STAT_KEYS == S.STAT_KEYS and tuple(plane()['stats']) == S.STAT_KEYS
