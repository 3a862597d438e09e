"""The host side of the 3-D scores (panst3r_amd/engine/score3d.py) and the properties of their contract, on the numpy restatement of
tests/nearest_ref.py alone (no GPU here): the sampler's counts, centroids, containment, exact edges and corner ties; the brute-force neighbour against
a k-d tree; the scores of known configurations; the camera alignment; validation; the ABI."""
import numpy as np
import pytest
import torch

import abi_header
import nearest_ref as N
from panst3r_amd import hip
from panst3r_amd.engine import sample_mesh, nearest_points, similarity_from_cameras, score_reconstruction, MeshSamples
from panst3r_amd.engine import score3d

F = np.float32
TRI = np.array([[0, 1, 2]])


def one_face(v, spacing, **kw):
    return N.sample_mesh(np.asarray(v, dtype=F), TRI, spacing, **kw)


def rot(axis, deg):
    a, c, s = np.eye(3)[axis], np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


@pytest.mark.parametrize('n', [1, 2, 3, 7, 20])
def test_a_face_of_n_subdivisions_yields_n_squared_samples_inside_it_around_its_centroid(n):
    rng = np.random.default_rng(n)
    v = rng.uniform(-1, 1, (3, 3)).astype(F)
    L = np.sqrt(max(((v[a].astype(np.float64) - v[b].astype(np.float64)) ** 2).sum() for a, b in ((0, 1), (1, 2), (2, 0))))
    s = one_face(v, L / (n - 0.5))                                              # (n - 1) spacing < L < n spacing, far from either
    assert s['n'].tolist() == [n] and len(s['points']) == n * n and (s['face'] == 0).all() and s['dropped_faces'] == 0 and s['clamped_faces'] == 0
    w = s['weights']
    assert (w > 0).all() and (w.sum(1) == 3 * n).all() and len({tuple(r) for r in w.tolist()}) == n * n        # strictly inside, all distinct
    # the weights of all sub-triangles sum to n^2 * n per corner: the mean of the samples is the centroid.  Every point is off by at most 3 roundings of
    # products and sums of magnitude <= 3n max|v|, one of the quotient and the cast to fp32: |error| <= max|v| (4 * 2^-53 + 2^-24) per point
    assert (w.sum(0) == n * n * n).all()
    v64 = v.astype(np.float64)
    bound = np.abs(v64).max() * (4 * 2.0 ** -53 + 2.0 ** -24)
    assert np.abs(s['points'].astype(np.float64).mean(0) - v64.mean(0)).max() <= bound
    exact = (w[:, :, None] * v64[None]).sum(1) / (3 * n)
    assert np.abs(s['points'].astype(np.float64) - exact).max() <= bound


def test_an_edge_of_exactly_n_spacings_gives_n_and_one_float_above_gives_n_plus_one():
    for n, spacing in ((1, 0.25), (3, 0.25), (7, 0.125), (1024, 2.0 ** -10)):
        e = F(n * spacing)
        assert float(e) == n * spacing
        at = one_face([[0, 0, 0], [e, 0, 0], [e / 2, e / 4, 0]], spacing, max_subdiv=2048)
        above = one_face([[0, 0, 0], [np.nextafter(e, F(np.inf)), 0, 0], [e / 2, e / 4, 0]], spacing, max_subdiv=2048)
        assert at['n'].tolist() == [n] and above['n'].tolist() == [n + 1], n


def test_the_clamp_is_counted_and_bad_faces_are_dropped():
    big = one_face([[0, 0, 0], [10, 0, 0], [0, 10, 0]], 0.1, max_subdiv=4)
    assert big['n'].tolist() == [4] and big['clamped_faces'] == 1 and len(big['points']) == 16
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan, 0, 0]], dtype=F)
    faces = np.array([[0, 1, 2], [0, 0, 3], [0, 1, 4], [0, 1, 5], [0, 1, -1], [0, 1, 3]])       # collinear, repeated corner, NaN, two bad indices, good
    s = N.sample_mesh(v, faces, 1.0)
    assert s['n'].tolist() == [0, 0, 0, 0, 0, 2] and s['dropped_faces'] == 5 and (s['face'] == 5).all()


def test_corner_ties_go_to_the_lower_corner():
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    ids = np.array([10, 20, 30], dtype=np.int32)
    assert N.sample_mesh(np.array(v, dtype=F), TRI, 2.0, vertex_ids=ids)['ids'].tolist() == [10]       # n = 1: weights (1, 1, 1)
    s = N.sample_mesh(np.array(v, dtype=F), TRI, 0.5, vertex_ids=ids)                                  # n = 3
    w = s['weights']
    tie01, tie12 = (w[:, 0] == w[:, 1]) & (w[:, 0] > w[:, 2]), (w[:, 1] == w[:, 2]) & (w[:, 1] > w[:, 0])
    assert tie01.any() and tie12.any() and (s['ids'][tie01] == 10).all() and (s['ids'][tie12] == 20).all()
    assert (s['ids'] == ids[np.argmax(w, 1)]).all() and set(s['ids'].tolist()) == {10, 20, 30}
    assert (N.sample_mesh(np.array(v, dtype=F), TRI, 0.5, face_ids=np.array([7]))['ids'] == 7).all()
    assert (N.sample_mesh(np.array(v, dtype=F), TRI, 0.5)['ids'] == 0).all()


def test_the_brute_force_neighbour_agrees_with_a_kd_tree():
    cKDTree = pytest.importorskip('scipy.spatial').cKDTree
    rng = np.random.default_rng(3)
    T, Q = rng.uniform(-1, 1, (1500, 3)).astype(F), rng.uniform(-1.1, 1.1, (1200, 3)).astype(F)
    radius = 0.15
    got = N.nearest(Q, T, radius)
    dist, idx = cKDTree(T.astype(np.float64)).query(Q.astype(np.float64), k=2)
    hit = got['row'] >= 0
    assert hit.sum() > 500 and (~hit).sum() > 50
    # where the two nearest distances differ by more than the rounding of the fp32 formula, both must name the same row
    clear = (dist[:, 1] - dist[:, 0]) > 1e-5
    assert clear.sum() > 1000
    inside, outside = dist[:, 0] < radius * (1 - 1e-5), dist[:, 0] > radius * (1 + 1e-5)
    assert (got['row'][clear & inside] == idx[clear & inside, 0]).all() and (got['row'][outside] == -1).all() and hit[inside].all()
    assert np.allclose(np.sqrt(got['d2'][hit].astype(np.float64)), dist[hit, 0], rtol=1e-5, atol=1e-7)


def test_ties_go_to_the_smaller_row_and_bad_points_are_left_out():
    T = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 0.5], [0, 0, 0.5], [3e6, 0, 0]], dtype=F)
    Q = np.array([[0, 0, 0], [0, 0, 0.5], [np.inf, 0, 0], [0, np.nan, 0], [50, 50, 50]], dtype=F)
    r = N.nearest(Q, T, 1.0)
    assert r['row'].tolist() == [4, 4, -1, -1, -1] and r['d2'][:2].tolist() == [0.25, 0.0] and np.isinf(r['d2'][2:]).all()
    assert r['dropped_targets'] == 2 and r['bad_queries'] == 2                   # the NaN target and the one 3e6 cells out
    assert N.nearest(Q[:1], T[:3], 1.0)['row'].tolist() == [0]                  # three targets at distance exactly 1 = the radius: accepted, row 0


def plane(n, z):
    g = (np.arange(n) * 0.25).astype(F)
    x, y = np.meshgrid(g, g, indexing='ij')
    return np.stack([x.ravel(), y.ravel(), np.full(n * n, z, dtype=F)], 1).astype(F)


def test_a_set_scored_against_itself_is_perfect():
    P = plane(12, 0.0)
    s = N.scores(P, P, [0.05, 0.1])
    assert s['precision'] == [1.0, 1.0] and s['recall'] == [1.0, 1.0] and s['fscore'] == [1.0, 1.0] and s['chamfer'] == 0.0
    assert s['accuracy_matched'] == s['completeness_matched'] == 1.0 and s['accuracy_median'] == 0.0
    assert (s['accuracy_rows'] == np.arange(len(P))).all()


def test_a_plane_shifted_by_exactly_tau_is_matched_and_one_float_above_is_not():
    tau = F(0.125)
    A = plane(10, 0.0)
    at, above = plane(10, tau), plane(10, np.nextafter(tau, F(np.inf)))
    s = N.scores(at, A, [tau])
    assert s['precision'] == [1.0] and s['recall'] == [1.0] and s['accuracy_mean'] == float(tau) and s['chamfer'] == 2 * float(tau)
    s = N.scores(above, A, [tau])
    assert s['precision'] == [0.0] and s['recall'] == [0.0] and s['fscore'] == [0.0] and s['accuracy_matched'] == 0.0 and np.isnan(s['chamfer'])
    s = N.scores(above, A, [tau], max_dist=0.2)                                 # found by the wider search, but still beyond the threshold
    assert s['pred_within'] == [0] and s['accuracy_matched'] == 1.0 and s['accuracy_median'] == float(np.sqrt(np.float64(np.nextafter(tau, F(np.inf)) ** 2)))


def cameras(centres, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for c in centres:
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot(int(rng.integers(3)), float(rng.uniform(0, 360))), c
        out.append(m)
    return out


def test_similarity_from_cameras_recovers_a_known_transform():
    rng = np.random.default_rng(5)
    centres = rng.uniform(-2, 2, (6, 3))
    scale, R, t = 2.5, rot(0, 33) @ rot(2, -71), np.array([0.5, -3.0, 4.0])
    pred = cameras(centres)
    gt = [N.similarity(1.0, R, scale * R @ m[:3, 3] + t - R @ m[:3, 3]) @ m for m in pred]      # centre -> scale R centre + t
    T = similarity_from_cameras(pred, gt)
    assert isinstance(T, torch.Tensor) and T.dtype == torch.float64 and tuple(T.shape) == (4, 4)
    assert np.allclose(T.numpy(), N.similarity(scale, R, t), atol=1e-12)
    assert np.allclose(np.linalg.det(T.numpy()[:3, :3]), scale ** 3)
    T = similarity_from_cameras(torch.tensor(np.stack(pred)), torch.tensor(np.stack(gt)).float())      # stacked tensors, either precision
    assert np.allclose(T.numpy(), N.similarity(scale, R, t), atol=1e-5)
    T = similarity_from_cameras(pred[:3], gt[:3])                                 # three cameras span a plane: enough
    assert np.allclose(T.numpy(), N.similarity(scale, R, t), atol=1e-10)


def test_similarity_from_cameras_refuses_what_does_not_determine_it():
    line = cameras([[k, 2 * k, -k] for k in range(5)])
    good = cameras(np.random.default_rng(1).uniform(-1, 1, (5, 3)))
    with pytest.raises(ValueError, match='at least 3'):
        similarity_from_cameras(good[:2], good[:2])
    with pytest.raises(ValueError, match='span a plane'):
        similarity_from_cameras(line, good)
    with pytest.raises(ValueError, match='span a plane'):
        similarity_from_cameras(good, line)
    with pytest.raises(ValueError, match='span a plane'):
        similarity_from_cameras(cameras([[1, 1, 1]] * 4), good[:4])
    with pytest.raises(ValueError, match='as many'):
        similarity_from_cameras(good, good[:4])
    with pytest.raises(ValueError):
        similarity_from_cameras([np.eye(3)] * 3, good[:3])


def test_arguments_are_checked_before_any_launch():
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for bad in (0, -1.0, float('nan'), float('inf'), 1e-50, 1e50, True, 'x', None):
        with pytest.raises(ValueError):
            sample_mesh(v, f, bad)
        with pytest.raises(ValueError):
            nearest_points(v, v, bad)
    with pytest.raises(ValueError):
        nearest_points(v, v, 1e-30)                                              # its square is not a positive float32
    for bad in (0, -1, 1.5, True, hip.MESH_SAMPLE_MAX_SUBDIV + 1):
        with pytest.raises(ValueError):
            sample_mesh(v, f, 0.1, max_subdiv=bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            nearest_points(v, v, 0.1, max_cell_points=bad)
    with pytest.raises(ValueError):
        sample_mesh(v, f, 0.1, vertex_ids=torch.zeros(4, dtype=torch.int32), face_ids=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        sample_mesh(v, f, 0.1, vertex_ids=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        sample_mesh(v, f.float(), 0.1)
    with pytest.raises(ValueError):
        sample_mesh(v[:, :2], f, 0.1)
    with pytest.raises(ValueError):
        nearest_points(torch.zeros(4, 2), v, 0.1)
    with pytest.raises(ValueError):
        nearest_points(v, torch.zeros(4, 3, dtype=torch.int32), 0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                   # valid arguments on the host: there is no CPU path
        sample_mesh(v, f, 0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        nearest_points(v, v, 0.1)
    kw = dict(thresholds=[0.1], spacing=0.05)
    with pytest.raises(ValueError):
        score_reconstruction(v, v, f, thresholds=[], spacing=0.05)
    with pytest.raises(ValueError):
        score_reconstruction(v, v, f, thresholds=[0.1, -1], spacing=0.05)
    with pytest.raises(ValueError, match='beyond the search radius'):
        score_reconstruction(v, v, f, max_dist=0.05, **kw)
    with pytest.raises(ValueError):
        score_reconstruction(v, v, f, transform=np.eye(3), **kw)
    with pytest.raises(ValueError, match='go together'):
        score_reconstruction(v, v, f, gt_vertex_ids=torch.zeros(4, dtype=torch.int32), **kw)
    with pytest.raises(ValueError):
        score_reconstruction([1, 2, 3], v, f, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        score_reconstruction(v, v, f, **kw)
    assert isinstance(MeshSamples(v, f[:, 0], f[:, 0], 1, 2).cpu(), MeshSamples)


def test_abi_is_unchanged_and_the_constants_agree():
    defines = abi_header.defines()
    assert hip.ABI_VERSION == 20 == defines['PST_ABI_VERSION']
    assert hip.MESH_SAMPLE_MAX_SUBDIV == defines['PST_MESH_SAMPLE_MAX_SUBDIV'] == N.MAX_SUBDIV
    assert hip.MESH_SAMPLE_TOTAL == defines['PST_MESH_SAMPLE_TOTAL'] and (hip.NN_FULL, hip.NN_LISTS) == (defines['PST_NN_FULL'], defines['PST_NN_LISTS'])
    names = {p[0] for p in abi_header.prototypes()}
    new = {'pst_mesh_sample_count', 'pst_mesh_sample_emit', 'pst_nn_insert', 'pst_nn_scatter', 'pst_nn_query'}
    assert new <= names and new <= set(hip.SIGNATURES)
    assert {n for n in names if n.startswith(('pst_nn_', 'pst_mesh_sample_'))} == new
    code = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for name, ret, params in abi_header.prototypes():
        if name in new:
            assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
    assert score3d.PLANE_RANK_TOL == 1e-6


def test_evaluate_3d_only_composes():
    from panst3r_amd.panst3r import PanSt3R
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match='gt_mesh'):
        PanSt3R.evaluate_3d(None, v, (v, f, None), thresholds=[0.1], spacing=0.05)
    with pytest.raises(ValueError, match='beyond the search radius'):           # the keywords reach score_reconstruction
        PanSt3R.evaluate_3d(None, v, (v, f), thresholds=[0.1], spacing=0.05, max_dist=0.05)
    with pytest.raises(ValueError, match='go together'):                         # ... and so do the labels of a four-entry mesh
        PanSt3R.evaluate_3d(None, v, (v, f, torch.zeros(4, dtype=torch.int32), None), thresholds=[0.1], spacing=0.05)
