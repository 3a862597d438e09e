"""The 3-D scores on the GPU (csrc/nearest.hip, panst3r_amd/engine/score3d.py) against the numpy restatement of tests/nearest_ref.py: the samples of a
mesh and the nearest points of a query set BIT FOR BIT - the contract is integer work and separately rounded fp32 / fp64 operations, so there is no
tolerance to choose - then the scores composed from them (counts and shares exactly, the float64 means within the bound of an N-term sum).

Conditions, not measurements: before the GPU is compared, every `check_*` asserts ON THE RESTATEMENT that the generated scene holds what it was built
for; the lists are in the docstrings of `sampler_scene` and `nn_scene`."""
import functools

import numpy as np
import pytest
import torch

import grid_lists as G
import mesh_ref as M
import nearest_ref as N
from panst3r_amd import hip
from panst3r_amd.engine import sample_mesh, nearest_points, score_reconstruction, similarity_from_cameras, panoptic_quality
from panst3r_amd.engine import PanopticCloud, PanopticMesh, VoxelCloud
from panst3r_amd.engine.pointmaps import rigid_points_registration
from panst3r_amd.engine.score3d import NearestIndex

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32


def rot(axis, deg):
    a, c, s = np.eye(3)[axis], np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


SPACING = 0.25
WG = 256


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


# ---------------------------------------------------------------- the sampler
@functools.lru_cache(maxsize=None)
def sampler_scene():
    """1100 small triangles with longest edges around 0.2, 0.4 and 0.7 (n = 1, 2, 3 at spacing 0.25) - more faces than one 1024-round of the scan, a few
    thousand samples - then the special faces, whose rows are in `special`: n = 7; one of 2.9 (n = 12: clamped when max_subdiv = 4 is passed, as the
    n = 7 face is); the pair with an edge of exactly 3 spacings and one float32 above; a degenerate face, one with a NaN vertex, one with an index
    beyond the vertices and one with a negative index.  Ids per face, and per vertex (every n = 1 face is a weight tie of all three corners)."""
    rng = np.random.default_rng(11)
    verts, faces = [], []

    def tri(c, L):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3)); w /= np.linalg.norm(w)
        k = len(verts)
        verts.extend([c, c + L * u, c + 0.5 * L * u + 0.3 * L * w])              # the other two edges are 0.58 L
        faces.append((k, k + 1, k + 2))
    for i in range(1100):
        tri(rng.uniform(-2, 2, 3), (0.2, 0.4, 0.7)[i % 3] * rng.uniform(0.9, 1.05))
    special = {}
    special['n7'] = len(faces); tri(np.array([3.0, 0, 0]), 1.7)
    special['n12'] = len(faces); tri(np.array([0, 3.0, 0]), 2.9)
    e = F(3 * SPACING)
    for name, x in (('exact', e), ('above', np.nextafter(e, F(np.inf)))):
        special[name] = len(faces)
        k = len(verts)
        verts.extend([np.zeros(3), np.array([x, 0, 0], dtype=np.float64), np.array([e / 2, e / 4, 0], dtype=np.float64)])
        faces.append((k, k + 1, k + 2))
    k = len(verts)
    verts.append(np.array([np.nan, 0.0, 1.0]))
    for name, f in (('degenerate', (0, 0, 1)), ('nan', (k, 0, 1)), ('index_high', (0, 1, 10 ** 6)), ('index_negative', (-1, 0, 1))):
        special[name] = len(faces)
        faces.append(f)
    tri(rng.uniform(-2, 2, 3), 0.4)                                              # a good face after the bad ones
    V, Fc = np.array(verts).astype(F), np.array(faces, dtype=np.int64)
    return dict(vertices=V, faces=Fc, special=special, vertex_ids=rng.integers(1, 50, len(V)).astype(np.int32),
                face_ids=rng.integers(1, 50, len(Fc)).astype(np.int32))


@functools.lru_cache(maxsize=None)
def sampler_reference(ids='none', max_subdiv=1024):
    s = sampler_scene()
    kw = {'vertex': dict(vertex_ids=s['vertex_ids']), 'face': dict(face_ids=s['face_ids']), 'none': {}}[ids]
    return N.sample_mesh(s['vertices'], s['faces'], SPACING, max_subdiv=max_subdiv, **kw)


def check_sampler_conditions():
    s, sp = sampler_scene(), sampler_scene()['special']
    want, clamped = sampler_reference(), sampler_reference(max_subdiv=4)
    n = want['n']
    assert len(n) > 1024 and 3000 < len(want['points']) < 20000                  # the scan takes a second round; several thousand samples
    assert {1, 2, 3, 7} <= set(n.tolist()) and n[sp['n7']] == 7 and n[sp['n12']] == 12 and want['clamped_faces'] == 0
    assert clamped['n'][sp['n12']] == 4 and clamped['n'][sp['n7']] == 4 and clamped['clamped_faces'] == 2 and clamped['n'][sp['exact']] == 3
    assert n[sp['exact']] == 3 and n[sp['above']] == 4
    for name in ('degenerate', 'nan', 'index_high', 'index_negative'):
        assert n[sp[name]] == 0, name
    assert want['dropped_faces'] == 4 and n[-1] > 0
    prefix = np.concatenate([[0], np.cumsum(n * n)])
    first, last = prefix[:-1][n > 0], prefix[1:][n > 0] - 1
    assert (first // WG != last // WG).any() and (first // 1024 != last // 1024).any()       # one face's samples straddle a workgroup, and a 1024 boundary
    w = sampler_reference('vertex')['weights']
    assert ((w[:, 0] == w[:, 1]) & (w[:, 0] >= w[:, 2])).any() and ((w[:, 1] == w[:, 2]) & (w[:, 1] > w[:, 0])).any()      # weight ties
    return want


def device_mesh():
    s = sampler_scene()
    return dev(s['vertices']), dev(s['faces']), dev(s['vertex_ids']), dev(s['face_ids'])


def assert_samples(got, want):
    assert len(got) == len(want['points']) and got.dropped_faces == want['dropped_faces'] and got.clamped_faces == want['clamped_faces']
    assert got.points.dtype == torch.float32 and got.face.dtype == torch.int32 and got.ids.dtype == torch.int32
    for k in ('face', 'ids', 'points'):
        g, w = bits(getattr(got, k)), bits(want[k])
        assert g.shape == w.shape and (g == w).all(), '%s: %d of %d differ' % (k, (g != w).sum(), w.size)


@pytest.mark.parametrize('ids', ['none', 'face', 'vertex'])
def test_the_samples_equal_the_restatement(ids):
    check_sampler_conditions()
    v, f, vid, fid = device_mesh()
    kw = {'vertex': dict(vertex_ids=vid), 'face': dict(face_ids=fid), 'none': {}}[ids]
    assert_samples(sample_mesh(v, f, SPACING, **kw), sampler_reference(ids))


def test_the_clamp_int32_faces_and_repeated_calls():
    check_sampler_conditions()
    v, f, vid, fid = device_mesh()
    assert_samples(sample_mesh(v, f, SPACING, max_subdiv=4, face_ids=fid), sampler_reference('face', 4))
    f32 = torch.where((f < 0) | (f >= len(v)), torch.full_like(f, -1), f).to(torch.int32)
    a, b = sample_mesh(v, f32, SPACING, vertex_ids=vid), sample_mesh(v, f, SPACING, vertex_ids=vid)
    assert_samples(a, sampler_reference('vertex'))
    for k in ('points', 'face', 'ids'):
        assert (bits(getattr(a, k)) == bits(getattr(b, k))).all()
    c = a.cpu()
    assert not c.points.is_cuda and (bits(c.points) == bits(a.points)).all()


def test_a_capacity_one_short_is_refused_with_nothing_written():
    want = check_sampler_conditions()
    v, f, _, _ = device_mesh()
    S = len(want['points'])
    with pytest.raises(ValueError, match='capacity'):
        sample_mesh(v, f, SPACING, capacity=S - 1)
    assert len(sample_mesh(v, f, SPACING, capacity=S)) == S
    # the entry point itself: outputs of S - 1 rows, filled with a mark
    f32 = torch.where((f < 0) | (f >= len(v)), torch.full_like(f, -1), f).to(torch.int32)
    i32 = dict(dtype=torch.int32, device=DEV)
    counts, prefix = torch.empty(len(f), **i32), torch.empty(len(f) + 1, **i32)
    total, status = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(4, **i32)
    hip.mesh_sample_count(v, f32, SPACING, 1024, counts, total, status)
    hip.cloud_scan(counts, prefix)
    assert int(total) == S == int(prefix[-1]) and (counts.cpu().numpy() == want['n'] ** 2).all()
    points, face, ids = torch.full((S - 1, 3), -7.0, device=DEV), torch.full((S - 1,), -7, **i32), torch.full((S - 1,), -7, **i32)
    with pytest.raises(RuntimeError, match='capacity'):
        hip.mesh_sample_emit(v, f32, prefix, S, None, None, points, face, ids, status)
    torch.cuda.synchronize()
    assert (points == -7).all() and (face == -7).all() and (ids == -7).all() and status.tolist()[0] == 0
    # a total that is not the prefix's: nothing written, the status bit set
    points, face, ids = torch.full((S, 3), -7.0, device=DEV), torch.full((S,), -7, **i32), torch.full((S,), -7, **i32)
    hip.mesh_sample_emit(v, f32, prefix, S - 1, None, None, points, face, ids, status)
    assert status.tolist()[0] == hip.MESH_SAMPLE_TOTAL and (points == -7).all() and (face == -7).all() and (ids == -7).all()


def test_an_empty_and_an_all_bad_mesh_give_no_samples():
    v = torch.zeros(3, 3, device=DEV)
    s = sample_mesh(v, torch.zeros(0, 3, dtype=torch.int64, device=DEV), SPACING)
    assert len(s) == 0 and tuple(s.points.shape) == (0, 3) and s.dropped_faces == 0
    s = sample_mesh(v, torch.tensor([[0, 1, 2], [0, 1, 5]], device=DEV), SPACING)
    assert len(s) == 0 and s.dropped_faces == 2


# ---------------------------------------------------------------- the nearest neighbour
RADIUS = 0.25


@functools.lru_cache(maxsize=None)
def nn_scene():
    """3001 targets and 2501 queries (no multiples of 64), random in a box of 24^3 cells around the origin, with planted rows far from the box (marks ->
    query row): a query equal to a target; two targets at the same distance in different cells; duplicated targets; a target at exactly d2 = radius^2
    and one a float32 above; for every axis and direction a query whose only neighbour lies in the next cell across that face, once more across
    coordinate 0 where the cells are negative; a query with no target in its 27 cells; NaN and inf queries; a NaN target and one beyond 2^20 cells."""
    rng = np.random.default_rng(7)
    T, Q = rng.uniform(-3, 3, (3001, 3)).astype(F), rng.uniform(-3.2, 3.2, (2501, 3)).astype(F)
    marks, t, q = {}, [0], [0]

    def put(name, query, targets):
        marks[name] = (q[0], t[0])
        Q[q[0]] = query; q[0] += 1
        for p in targets:
            T[t[0]] = p; t[0] += 1
    c = np.array([10.0, 10.0, 10.0])
    put('equal', T[2000], [])                                                    # a random target itself
    put('tie', c, [c - [0.125, 0, 0], c + [0.125, 0, 0]])                        # cells 39 and 40 along x
    put('duplicate', c * 2 + [0.05, 0.05, 0.05], [c * 2 + [0.1, 0.1, 0.1]] * 2)
    put('at_radius', c * 3, [c * 3 + [0.25, 0, 0]])
    put('above_radius', c * 4, [c * 4 + [np.nextafter(F(40.25), F(np.inf)) - 40.0, 0, 0]])
    k = 0
    for origin in (np.array([50.0, 50.0, 50.0]), np.zeros(3)):
        for axis in range(3):
            for sign in (-1, 1):
                if origin[0] == 0 and sign > 0:
                    continue                                                     # across coordinate 0: from cell 0 into cell -1
                base = origin + np.array([20.0 * k, 0, 0]) * (origin[0] != 0) + 0.125
                e = np.eye(3)[axis] * sign
                put('face_%d' % k, base + 0.115 * e, [base + 0.145 * e])
                k += 1
    put('alone', [100.0, 100.0, 100.0], [])
    put('nan', [np.nan, 0, 0], [[np.nan, 1.0, 1.0]])
    put('inf', [0, np.inf, 0], [[0.25 * 2 ** 20 * 1.5, 0, 0]])
    put('ninf', [0, 0, -np.inf], [])
    return Q, T, marks, k


@functools.lru_cache(maxsize=None)
def nn_reference():
    Q, T, _, _ = nn_scene()
    return N.nearest(Q, T, RADIUS)


def check_nn_conditions():
    Q, T, marks, nfaces = nn_scene()
    want = nn_reference()
    d2, row = want['d2'], want['row']
    cq, _, _ = N.cells(Q, RADIUS)
    ct, _, kept = N.cells(T, RADIUS)
    assert len(T) % 64 and len(Q) % 64 and len(T) % 256 and len(Q) % 256
    assert 1000 < (row >= 0).sum() < len(Q) - 500                               # hits and misses in numbers
    qi, _ = marks['equal']
    assert d2[qi] == 0 and (T[row[qi]] == Q[qi]).all()
    qi, ti = marks['tie']
    assert row[qi] == ti and want['second'][qi] == d2[qi] and (ct[ti] != ct[ti + 1]).any() and (T[ti] != T[ti + 1]).any()
    qi, ti = marks['duplicate']
    assert row[qi] == ti and (T[ti] == T[ti + 1]).all() and want['second'][qi] == d2[qi]
    r2 = F(RADIUS) * F(RADIUS)
    qi, ti = marks['at_radius']
    assert row[qi] == ti and d2[qi] == r2
    qi, ti = marks['above_radius']
    assert row[qi] == -1 and np.isinf(d2[qi])
    dx = Q[qi, 0] - T[ti, 0]
    assert np.nextafter(r2, F(0)) < dx * dx and dx * dx > r2 and dx * dx < r2 * F(1.0001)      # that target is a float or so beyond the radius, not far away
    seen = set()
    assert nfaces == 9
    for k in range(nfaces):
        qi, ti = marks['face_%d' % k]
        diff = ct[ti] - cq[qi]
        assert row[qi] == ti and np.abs(diff).sum() == 1, k                      # the nearest target lies across exactly one face
        seen.add((tuple(diff.astype(int).tolist()), bool((ct[ti] < 0).any())))
    assert {s[0] for s in seen} == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)} and sum(s[1] for s in seen) == 3
    qi, _ = marks['alone']
    assert row[qi] == -1 and (np.abs(ct[kept] - cq[qi]).max(1) > 1).all()       # no target in its 27 cells
    for name in ('nan', 'inf', 'ninf'):
        assert row[marks[name][0]] == -1 and np.isinf(d2[marks[name][0]])
    assert want['bad_queries'] == 3 and want['dropped_targets'] == 2 and not kept[marks['nan'][1]] and not kept[marks['inf'][1]]
    # the contract's precondition holds in this scene: every accepted pair lies in neighbouring cells, so the 27 cells see what all pairs see
    hit = row >= 0
    assert (np.abs(ct[row[hit]] - cq[hit]).max(1) <= 1).all()
    return want


def test_the_nearest_points_equal_the_restatement():
    want = check_nn_conditions()
    Q, T, _, _ = nn_scene()
    q, t = dev(Q), dev(T)
    d2, row = nearest_points(q, t, RADIUS)
    assert d2.dtype == torch.float32 and row.dtype == torch.int32 and tuple(d2.shape) == tuple(row.shape) == (len(Q),)
    assert (row.cpu().numpy() == want['row']).all() and (bits(d2) == bits(want['d2'])).all()
    again = nearest_points(q, t, RADIUS)
    assert (bits(again[0]) == bits(d2)).all() and (bits(again[1]) == bits(row)).all()
    index = NearestIndex(t, RADIUS)
    got = index.query(q)
    assert (bits(got[0]) == bits(d2)).all() and (bits(got[1]) == bits(row)).all()
    assert index.dropped == want['dropped_targets'] and index.check() == want['bad_queries'] and 1 <= index.max_occupancy < 64


def test_the_roles_exchanged_and_a_radius_that_is_no_power_of_two():
    Q, T, _, _ = nn_scene()
    T2 = np.where(np.isfinite(T), T, F(0)).astype(F)
    T2[np.abs(T2) > 1000] = 0
    for radius in (0.3, 0.15):
        want = N.nearest(T2, Q, radius)
        cq, _, _ = N.cells(T2, radius)
        ct, _, _ = N.cells(Q, radius)
        hit = want['row'] >= 0
        assert hit.sum() > 200 and (np.abs(ct[want['row'][hit]] - cq[hit]).max(1) <= 1).all()
        d2, row = nearest_points(dev(T2), dev(Q), radius)
        assert (row.cpu().numpy() == want['row']).all() and (bits(d2) == bits(want['d2'])).all()


def test_empty_queries_and_empty_targets_launch_nothing(monkeypatch):
    Q, T, _, _ = nn_scene()
    q, t, none = dev(Q[:100]), dev(T), torch.empty(0, 3, device=DEV)
    for name in ('nn_workspace', 'nn_insert', 'nn_scatter', 'nn_query'):         # neither a build nor a query, in all three cases
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail('a build or a launch for an empty set'))
    d2, row = nearest_points(none, none, RADIUS)
    assert tuple(d2.shape) == tuple(row.shape) == (0,)
    d2, row = nearest_points(q, none, RADIUS)
    assert (row == -1).all() and torch.isinf(d2).all() and d2.dtype == torch.float32 and row.dtype == torch.int32 and row.numel() == 100
    d2, row = nearest_points(none, t, RADIUS)
    assert tuple(d2.shape) == tuple(row.shape) == (0,) and d2.dtype == torch.float32 and row.dtype == torch.int32
    d2, row = nearest_points(none, t, RADIUS, max_cell_points=1)                 # no queries: the density of the targets is no matter
    assert row.numel() == 0
    with pytest.raises(ValueError):                                              # the arguments are still checked
        nearest_points(none, t, -1.0)


def test_a_full_cell_runs_and_a_fuller_one_is_refused_before_the_query(monkeypatch):
    rng = np.random.default_rng(2)
    K = 40
    T = np.concatenate([rng.uniform(1.0, 1.25, (K, 3)), rng.uniform(-3, 3, (200, 3))]).astype(F)        # K targets in the cell (4, 4, 4)
    Q = rng.uniform(0.9, 1.35, (333, 3)).astype(F)
    ct, _, _ = N.cells(T, RADIUS)
    _, occupancy = np.unique(ct, axis=0, return_counts=True)
    assert occupancy.max() == K and (ct[:K] == 4).all()
    want = N.nearest(Q, T, RADIUS)
    index = NearestIndex(dev(T), RADIUS, max_cell_points=K)
    assert index.max_occupancy == K
    d2, row = index.query(dev(Q))
    assert (row.cpu().numpy() == want['row']).all() and (bits(d2) == bits(want['d2'])).all() and (want['row'] >= 0).sum() > 300
    monkeypatch.setattr(hip, 'nn_query', lambda *a, **k: pytest.fail('the query was launched'))
    with pytest.raises(ValueError, match='too large for this density'):
        nearest_points(dev(Q), dev(T), RADIUS, max_cell_points=K - 1)


# ---------------------------------------------------------------- lists that are not the build's (the guards of csrc/voxel_table.h)
def lattice_query(q, t, ws):
    d2, row = torch.full((len(q),), -7.0, device=DEV), torch.full((len(q),), -7, dtype=torch.int32, device=DEV)
    hip.nn_query(q, t, float(N.radius_numbers(G.CELL)[1]), float(N.radius_numbers(G.CELL)[2]), ws, 4096, d2, row)
    return d2, row, ws['status'].tolist()


def test_the_query_refuses_a_list_that_leaves_the_rows_and_a_row_past_the_targets():
    touched, untouched = G.check_lattice()
    Q, T = G.lattice()
    q, t = G.padded(Q), G.padded(T)
    good = G.nn_build(t)
    assert good['status'].tolist() == [0, 0, 8, 0]
    want = N.nearest(Q, T, G.CELL)
    d2, row, status = lattice_query(q, t, G.fresh(good))                         # (d) the untampered workspace through the same helpers
    assert status == [0, 0, 0, 0] and (row.cpu().numpy() == want['row']).all() and (bits(d2) == bits(want['d2'])).all()
    slot, M = int(good['point_slot'][0]), len(T)
    for tamper in (lambda ws: G.move_list_out(ws, slot, M), lambda ws: G.first_entry_past_the_end(ws, slot, M)):      # (a), (b)
        ws = G.fresh(good)
        tamper(ws)
        bd2, brow, status = lattice_query(q, t, ws)
        assert status == [G.LISTS, 0, 0, 0]
        assert (bits(bd2)[untouched] == bits(d2)[untouched]).all() and (bits(brow)[untouched] == bits(row)[untouched]).all()
        assert bool(((brow >= -1) & (brow < M)).all()) and (bits(brow)[touched] != bits(row)[touched]).any()      # a target was lost, none past the end was taken
    assert (good['status'] == torch.tensor([0, 0, 8, 0], device=DEV)).all() and (bits(lattice_query(q, t, G.fresh(good))[0]) == bits(d2)).all()


def test_the_scatter_refuses_a_count_that_is_not_the_inserts():
    G.check_lattice()
    t = G.padded(G.lattice()[1])
    good = G.nn_build(t)
    G.assert_a_short_count_is_refused(good, lambda tamper: G.nn_build(t, tamper), lambda ws: int(ws['point_slot'][0]), len(t))


# ---------------------------------------------------------------- the composition
GT_SPACING, TAUS = 0.7, (0.125, 0.25, 0.5)


@functools.lru_cache(maxsize=None)
def room():
    """the generated room of the mesh tests as ground truth, and as prediction a noisy, partly missing copy of its own surface: its samples at another
    spacing, moved by up to 0.2 per axis, everything with x > 2 cut away, a tenth of the labels exchanged for a neighbour's"""
    s = M.scene()
    segs = [{'id': int(g['id']), 'category_id': int(g.get('category_id', g.get('class_id')))} for g in s['segments']]
    own = N.sample_mesh(s['vertices'], s['faces'], 0.6, vertex_ids=s['vertex_ids'])
    rng = np.random.default_rng(4)
    keep = own['points'][:, 0] <= 2
    pts = (own['points'][keep] + rng.uniform(-0.2, 0.2, (keep.sum(), 3)).astype(F)).astype(F)
    ids = own['ids'][keep].copy()
    swap = rng.random(len(ids)) < 0.1
    ids[swap] = np.roll(ids, 37)[swap]
    return dict(vertices=s['vertices'], faces=s['faces'], vertex_ids=s['vertex_ids'], face_ids=s['face_ids'], segments=segs, things=[M.THING, M.MARK],
                pred_points=pts, pred_ids=ids)


@functools.lru_cache(maxsize=None)
def room_samples():
    r = room()
    return N.sample_mesh(r['vertices'], r['faces'], GT_SPACING, vertex_ids=r['vertex_ids'])


def cloud_of(points, ids, segments):
    n = len(points)
    p = dev(points)
    return PanopticCloud(p, p.clone(), torch.full((n, 3), 0.5, device=DEV), dev(ids), torch.full((n, 3), 0.5, device=DEV),
                         torch.arange(n, device=DEV), [0, n], [dict(s) for s in segments])


def gt_args(r):
    return dev(r['vertices']), dev(r['faces'])


def assert_scores(got, want, n_terms):
    for k in ('n_pred', 'n_gt', 'pred_within', 'gt_within', 'precision', 'recall', 'fscore', 'accuracy_matched', 'completeness_matched', 'thresholds', 'max_dist'):
        assert got[k] == want[k], (k, got[k], want[k])
    tol = n_terms * 2.0 ** -52                                                   # an fp64 sum of N terms, in another order
    for k in ('accuracy_mean', 'accuracy_median', 'completeness_mean', 'completeness_median', 'chamfer'):
        assert abs(got[k] - want[k]) <= tol * abs(want[k]), (k, got[k], want[k])


def assert_pq(got, want_pred, want_gt, r, pred_segments=None):
    want = panoptic_quality(dev(want_pred)[None, None], pred_segments or r['segments'], dev(want_gt)[None, None], r['segments'], things=r['things'])
    for k in ('pq', 'sq', 'rq', 'pq_things', 'pq_stuff', 'miou', 'pixel_acc', 'n_pixels', 'void_pixels', 'per_class', 'matches'):
        assert got[k] == want[k], k
    assert (got['tables']['counts'] == want['tables']['counts']).all()
    return want


def test_a_noisy_partial_copy_of_the_room_scores_as_the_restatement_says():
    r, gt = room(), room_samples()
    want = N.scores(r['pred_points'], gt['points'], TAUS, pred_ids=r['pred_ids'], gt_ids=gt['ids'])
    # the scene decides something: neither perfect nor empty, the thresholds differ, the cut shows in the recall, labels both right and wrong
    assert 0 < want['precision'][0] < want['precision'][1] < want['precision'][2] <= 1 and 0 < want['recall'][0] < want['recall'][2] < 0.95
    assert 0 < want['accuracy_matched'] <= 1 and 0 < want['completeness_matched'] < 0.95 and want['accuracy_median'] != want['accuracy_mean']
    assert (want['pq_pred'] == 0).any() and (want['pq_pred'] == want['pq_gt']).sum() > 1000 and ((want['pq_pred'] != want['pq_gt']) & (want['pq_pred'] > 0)).sum() > 100
    assert gt['dropped_faces'] >= 4 and len(gt['points']) > 3000
    v, f = gt_args(r)
    got = score_reconstruction(cloud_of(r['pred_points'], r['pred_ids'], r['segments']), v, f, thresholds=TAUS, spacing=GT_SPACING,
                               gt_vertex_ids=dev(r['vertex_ids']), gt_segments=r['segments'], things=r['things'])
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert got['dropped_faces'] == gt['dropped_faces'] and got['clamped_faces'] == 0 and got['spacing'] == float(F(GT_SPACING))
    pq = assert_pq(got['pq3d'], want['pq_pred'], want['pq_gt'], r)
    assert 0 < pq['pq'] < 1 and pq['n_pixels'] == want['n_gt']
    plain = score_reconstruction(dev(r['pred_points']), v, f, thresholds=TAUS, spacing=GT_SPACING)       # bare points: the same geometry, no labels
    assert_scores(plain, want, max(want['n_pred'], want['n_gt']))
    assert plain['pq3d'] is None
    narrow = score_reconstruction(dev(r['pred_points']), v, f, thresholds=TAUS[:1], spacing=GT_SPACING, max_dist=0.2)
    assert_scores(narrow, N.scores(r['pred_points'], gt['points'], TAUS[:1], max_dist=0.2), max(want['n_pred'], want['n_gt']))


def test_the_ground_truth_scores_itself_perfectly():
    r, gt = room(), room_samples()
    v, f = gt_args(r)
    got = score_reconstruction(dev(gt['points']), v, f, thresholds=(0.01,), spacing=GT_SPACING)
    assert got['precision'] == [1.0] and got['recall'] == [1.0] and got['fscore'] == [1.0] and got['chamfer'] == 0.0 and got['n_gt'] == len(gt['points'])


def test_a_mesh_goes_through_the_sampler_and_voxels_through_their_points():
    r, gt = room(), room_samples()
    v, f = gt_args(r)
    # a PanopticMesh: the room's own mesh, moved by 0.1 along every axis, with its face ids
    moved = (r['vertices'] + F([0.1, 0.1, 0.1])).astype(F)
    f32 = np.where((r['faces'] < 0) | (r['faces'] >= len(moved)), -1, r['faces']).astype(np.int32)
    mesh = PanopticMesh(dev(moved), dev(f32), dev(r['face_ids']), dev(r['vertex_ids']), torch.zeros(len(moved), 3, device=DEV),
                        torch.zeros(len(f32), dtype=torch.int64, device=DEV), [0, 1], r['segments'])
    own = N.sample_mesh(moved, f32, GT_SPACING, face_ids=r['face_ids'])
    want = N.scores(own['points'], gt['points'], TAUS, pred_ids=own['ids'], gt_ids=gt['ids'])
    assert 0 < want['precision'][0] < want['precision'][2] and want['n_pred'] == len(own['points']) > 3000
    kw = dict(thresholds=TAUS, spacing=GT_SPACING, gt_vertex_ids=dev(r['vertex_ids']), gt_segments=r['segments'], things=r['things'])
    got = score_reconstruction(mesh, v, f, **kw)
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert_pq(got['pq3d'], want['pq_pred'], want['pq_gt'], r)
    # a VoxelCloud: the fusion of the noisy cloud; the restatement gets the voxels' points and ids as they are on the device
    vox = cloud_of(r['pred_points'], r['pred_ids'], r['segments']).voxelize(0.3)
    assert isinstance(vox, VoxelCloud) and 500 < len(vox) < len(r['pred_points'])
    want = N.scores(vox.points.cpu().numpy(), gt['points'], TAUS, pred_ids=vox.pan.cpu().numpy(), gt_ids=gt['ids'])
    got = score_reconstruction(vox, v, f, **kw)
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert 0 < len(vox.segments) <= len(r['segments'])                          # the voxels list the segments that own a voxel
    assert_pq(got['pq3d'], want['pq_pred'], want['pq_gt'], r, vox.segments)


def test_a_transform_is_applied_before_the_search_and_cameras_give_it():
    r, gt = room(), room_samples()
    v, f = gt_args(r)
    scale, R, t = 1.25, rot(1, 20) @ rot(0, -10), np.array([0.3, -0.2, 0.5])
    T = N.similarity(scale, R, t)
    away = ((r['pred_points'].astype(np.float64) - t) @ R / scale).astype(F)     # the prediction in a frame of its own: T carries it back, up to fp32
    A = dev(T, torch.float32)
    moved = (dev(away) @ A[:3, :3].T + A[:3, 3]).cpu().numpy()                   # as score_reconstruction does it: torch's matmul is not part of the contract
    want = N.scores(moved, gt['points'], TAUS)
    got = score_reconstruction(dev(away), v, f, thresholds=TAUS, spacing=GT_SPACING, transform=torch.from_numpy(T))
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    untransformed = score_reconstruction(dev(away), v, f, thresholds=TAUS, spacing=GT_SPACING)
    assert untransformed['precision'][0] < got['precision'][0]
    # a mesh is moved BEFORE it is sampled: `spacing` is a length of the ground truth's frame, whatever the scale.  The room's own mesh, shrunk by T^-1
    Ti = np.linalg.inv(T)
    small = (r['vertices'].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    f32 = np.where((r['faces'] < 0) | (r['faces'] >= len(small)), -1, r['faces']).astype(np.int32)
    mesh = PanopticMesh(dev(small), dev(f32), dev(r['face_ids']), dev(r['vertex_ids']), torch.zeros(len(small), 3, device=DEV),
                        torch.zeros(len(f32), dtype=torch.int64, device=DEV), [0, 1], r['segments'])
    back = (dev(small) @ A[:3, :3].T + A[:3, 3]).cpu().numpy()
    own, in_its_frame = N.sample_mesh(back, f32, GT_SPACING, face_ids=r['face_ids']), N.sample_mesh(small, f32, GT_SPACING, face_ids=r['face_ids'])
    assert len(own['points']) > 1.3 * len(in_its_frame['points'])                # sampling first would give the fewer samples of a mesh 1.25 times smaller
    want = N.scores(own['points'], gt['points'], TAUS)
    got = score_reconstruction(mesh, v, f, thresholds=TAUS, spacing=GT_SPACING, transform=T)
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert want['precision'][2] > 0.99
    # the same transform from five cameras, on the host and through the device registration with its scale
    rng = np.random.default_rng(9)
    gt_cams = [N.similarity(1.0, rot(2, 30.0 * k), rng.uniform(-2, 2, 3)) for k in range(5)]
    Ti = np.linalg.inv(T)
    pred_cams = [N.similarity(1.0, np.eye(3), Ti[:3, :3] @ c[:3, 3] + Ti[:3, 3]) for c in gt_cams]
    S = similarity_from_cameras(pred_cams, gt_cams)
    assert np.allclose(S.numpy(), T, atol=1e-10)
    x = dev(np.stack([c[:3, 3] for c in pred_cams])[None], torch.float32)
    y = dev(np.stack([c[:3, 3] for c in gt_cams])[None], torch.float32)
    Rd, td, sd = rigid_points_registration(x, y, compute_scaling=True)
    assert np.allclose(sd.numpy(), [scale], atol=1e-4) and np.allclose(Rd[0].numpy(), R, atol=1e-4) and np.allclose(td[0].numpy(), t, atol=1e-3)
    R0, t0 = rigid_points_registration(x, x)                                     # the unscaled call is what it was
    assert np.allclose(R0[0].numpy(), np.eye(3), atol=1e-5) and np.allclose(t0[0].numpy(), 0, atol=1e-4)
