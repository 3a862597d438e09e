"""The exact point-to-mesh distance on the GPU (csrc/meshdist.hip, panst3r_amd/engine/meshdist.py) against the numpy restatement of
tests/meshdist_ref.py: the per-face pair counts of the build, and d2, face and closest of the query BIT FOR BIT - the contract is integer work and
separately rounded fp32 / fp64 operations in a fixed order, so there is no tolerance to choose - then `score_reconstruction(metric='surface')` composed
from it (counts and shares exactly, the float64 means within the bound of an N-term sum).

Conditions, not measurements: before the GPU is compared, every `check_*` asserts ON THE RESTATEMENT that the generated scene holds what it was built
for; the lists are in the docstrings of `build_scene` and `query_scene`."""
import functools

import numpy as np
import pytest
import torch

import grid_lists as G
import mesh_ref as M
import meshdist_ref as MD
import nearest_ref as N
from panst3r_amd import hip
from panst3r_amd.engine import mesh_distance, score_reconstruction, panoptic_quality, PanopticCloud, PanopticMesh
from panst3r_amd.engine.meshdist import MeshIndex

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
RADIUS, OTHER_RADIUS, WG = 0.25, 0.3, 256


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def small_faces(rng, n, lo, hi, size):
    c = rng.uniform(lo, hi, (n, 1, 3))
    return (c + rng.normal(size=(n, 3, 3)) * rng.uniform(size[0], size[1], (n, 1, 1))).reshape(-1, 3)


# ---------------------------------------------------------------- the build
@functools.lru_cache(maxsize=None)
def build_scene():
    """1150 small triangles in a box of 24^3 cells around the origin (a few dozen pairs each) - more faces than one 1024-round of the scan - then the special
    faces, whose rows are in `special`: a flat face that spans 20 x 20 cells (over a thousand pairs from one face); a degenerate face, one with a NaN
    corner, one with an index beyond the vertices, one with a negative index, one beyond 2^20 cells; a good face after the bad ones."""
    rng = np.random.default_rng(21)
    verts = list(small_faces(rng, 1150, -3, 3, (0.02, 0.12)))
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(1150)]
    special = {}

    def tri(name, a, b, c):
        special[name] = len(faces)
        k = len(verts)
        verts.extend([np.asarray(a, float), np.asarray(b, float), np.asarray(c, float)])
        faces.append((k, k + 1, k + 2))
    tri('flat', (10.1, 10.1, 10.1), (14.9, 10.1, 10.1), (10.1, 14.9, 10.1))
    k = len(verts)
    verts.append(np.array([np.nan, 0.0, 1.0]))
    for name, f in (('degenerate', (0, 0, 1)), ('nan', (k, 0, 1)), ('index_high', (0, 1, 10 ** 6)), ('index_negative', (-1, 0, 1))):
        special[name] = len(faces)
        faces.append(f)
    tri('far', (0.25 * 2 ** 20 * 1.5, 0, 0), (0.25 * 2 ** 20 * 1.5 + 1, 0, 0), (0.25 * 2 ** 20 * 1.5, 1, 0))
    tri('last', (-2, -2, -2), (-1.9, -2, -2), (-2, -1.9, -2.05))
    return np.array(verts).astype(F), np.array(faces, dtype=np.int64), special


@functools.lru_cache(maxsize=None)
def build_reference():
    V, Fc, _ = build_scene()
    b = MD.binning(V, Fc, RADIUS)
    lists = MD.cell_lists(V, Fc, RADIUS)
    return b, max(len(v) for v in lists.values())


def check_build_conditions():
    V, Fc, sp = build_scene()
    b, fullest = build_reference()
    n = b['counts']
    assert len(Fc) > 1024 and 20000 < b['total'] < 200000
    for name in ('degenerate', 'nan', 'index_high', 'index_negative', 'far'):
        assert n[sp[name]] == 0 and not b['kept'][sp[name]], name
    assert b['dropped_faces'] == 5 and n[-1] > 0 and b['kept'].sum() == len(Fc) - 5
    assert b['ext'][sp['flat']].tolist() == [22, 22, 3] and n[sp['flat']] == 1452                  # cells 39 .. 60 in x and y: twenty and the dilation
    prefix = np.concatenate([[0], np.cumsum(n)])
    first, last = prefix[:-1][n > 0], prefix[1:][n > 0] - 1
    assert (first // WG != last // WG).any() and (first // 1024 != last // 1024).any()       # one face's pairs straddle a workgroup, and a multiple of 1024
    assert ((first // WG == last // WG) & (last > first)).any() and 4 <= fullest < 200
    return b, fullest


def device_index(**kw):
    V, Fc, _ = build_scene()
    return MeshIndex(dev(V), dev(Fc), RADIUS, **kw)


def test_the_per_face_pair_counts_equal_the_restated_binning():
    b, fullest = check_build_conditions()
    V, Fc, _ = build_scene()
    index = device_index()
    assert index.pairs == b['total'] and index.dropped_faces == b['dropped_faces'] and index.max_occupancy == fullest and index.check() == 0
    assert index.counts.dtype == torch.int32 and (index.counts.cpu().numpy() == b['counts']).all()
    assert int(index.prefix[-1]) == b['total'] and (index.prefix.cpu().numpy()[1:] == np.cumsum(b['counts'])).all()
    ws = index.ws
    assert int(ws['cell_count'].sum()) == b['total'] == int(ws['fill'].sum()) and int(ws['cell_count'].max()) == fullest
    # every list holds the faces the restated binning lists in that cell, in whatever order
    rows, start, cnt = ws['rows'].cpu().numpy(), ws['start'].cpu().numpy(), ws['cell_count'].cpu().numpy()
    lists = MD.cell_lists(V, Fc, RADIUS)
    got = sorted(tuple(sorted(rows[s:s + c].tolist())) for s, c in zip(start[cnt > 0], cnt[cnt > 0]))
    assert got == sorted(tuple(sorted(v)) for v in lists.values())
    # int32 faces (indices outside int32 made -1, as the engine does for int64) build the same index
    f32 = np.where((Fc < 0) | (Fc >= len(V)), -1, Fc).astype(np.int32)
    again = MeshIndex(dev(V), dev(f32), RADIUS)
    assert again.pairs == index.pairs and again.dropped_faces == index.dropped_faces and again.max_occupancy == fullest
    assert (bits(again.counts) == bits(index.counts)).all() and (bits(again.ws['cell_count'].sort().values) == bits(ws['cell_count'].sort().values)).all()


def test_max_pairs_one_short_is_refused_before_the_insert_and_a_full_cell_runs(monkeypatch):
    b, fullest = check_build_conditions()
    V, Fc, _ = build_scene()
    index = device_index(max_pairs=b['total'], max_cell_faces=fullest)              # exactly the total, exactly the fullest cell: both pass
    Q = np.random.default_rng(3).uniform(-3, 3, (500, 3)).astype(F)
    want = MD.mesh_distance(Q, V, Fc, RADIUS)
    d2, face, closest = index.query(dev(Q))
    assert (want['face'] >= 0).sum() > 100 and (face.cpu().numpy() == want['face']).all() and (bits(d2) == bits(want['d2'])).all()
    assert (bits(closest) == bits(want['closest'])).all() and index.check() == 0
    with monkeypatch.context() as m:
        m.setattr(hip, 'meshdist_query', lambda *a, **k: pytest.fail('the query was launched'))
        with pytest.raises(ValueError, match='a smaller radius makes shorter lists'):
            mesh_distance(dev(Q), dev(V), dev(Fc), RADIUS, max_cell_faces=fullest - 1)
    for name in ('meshdist_workspace', 'meshdist_insert', 'meshdist_scatter', 'meshdist_query'):
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail('something was allocated or launched for the pairs'))
    with pytest.raises(ValueError, match='a larger radius makes fewer pairs'):
        mesh_distance(dev(Q), dev(V), dev(Fc), RADIUS, max_pairs=b['total'] - 1)


def test_a_face_of_more_than_2_to_the_31_cells_is_refused_by_its_saturated_count():
    V = np.array([[-1000, -1000, 0], [1000, -1000, 0], [0, 1000, 100], [0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F)
    Fc = np.array([[0, 1, 2], [3, 4, 5]])
    b = MD.binning(V, Fc, RADIUS)
    assert b['counts'].tolist() == [MD.FACE_CAP, 147]
    with pytest.raises(ValueError, match='at least 2147483794'):
        MeshIndex(dev(V), dev(Fc), RADIUS, max_pairs=2 ** 30)


def test_the_launchers_refusals_leave_the_outputs_untouched():
    check_build_conditions()
    V, Fc, _ = build_scene()
    index = device_index()
    ws, P = index.ws, index.pairs
    q = dev(np.random.default_rng(1).uniform(-3, 3, (64, 3)).astype(F))
    i32 = dict(dtype=torch.int32, device=DEV)

    def outputs():
        return torch.full((64,), -7.0, device=DEV), torch.full((64,), -7, **i32), torch.full((64, 3), -7.0, device=DEV), torch.zeros(4, **i32)

    def untouched(d2, face, closest, status):
        torch.cuda.synchronize()
        return bool((d2 == -7).all() and (face == -7).all() and (closest == -7).all() and (status == 0).all())
    good = lambda d2, face, closest, status, **kw: hip.meshdist_query(q, index.vertices, index.faces, kw.get('inv', index.inv), kw.get('r2', index.r2),
                                                                        kw.get('ws', ws), kw.get('mcf', 4096), d2, face, closest, status)
    for kw in (dict(ws=dict(ws, cap=ws['cap'] - 1)), dict(ws=dict(ws, cap=ws['cap'] // 4)), dict(inv=float('inf')), dict(inv=float('nan')), dict(inv=0.0),
               dict(r2=float('inf')), dict(r2=float('nan')), dict(r2=-1.0), dict(mcf=0)):
        out = outputs()
        with pytest.raises(RuntimeError, match='meshdist_query'):
            good(*out, **kw)
        assert untouched(*out), kw
    out = outputs()
    for bad in ('queries', 'd2', 'face', 'status', 'keys', 'rows'):                # a null pointer, through the entry point itself
        ptr = lambda name, t: None if name == bad else t.data_ptr()
        with pytest.raises(RuntimeError, match='null operand'):
            hip._call('pst_meshdist_query', ptr('queries', q), 64, index.vertices.data_ptr(), len(V), index.faces.data_ptr(), len(Fc), index.inv, index.r2,
                      ptr('keys', ws['keys']), ws['cap'], ws['start'].data_ptr(), ws['cell_count'].data_ptr(), ptr('rows', ws['rows']), P, 4096,
                      ptr('d2', out[0]), ptr('face', out[1]), out[2].data_ptr(), ptr('status', out[3]))
    for Nq, nf in ((0, len(Fc)), (-1, len(Fc)), (2 ** 30 + 1, len(Fc)), (64, -1), (64, 2 ** 30 + 1)):
        with pytest.raises(RuntimeError, match='bad shape'):
            hip._call('pst_meshdist_query', q.data_ptr(), Nq, index.vertices.data_ptr(), len(V), index.faces.data_ptr(), nf, index.inv, index.r2,
                      ws['keys'].data_ptr(), ws['cap'], ws['start'].data_ptr(), ws['cell_count'].data_ptr(), ws['rows'].data_ptr(), P, 4096,
                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr())
    assert untouched(*out)
    good(*out)                                                                       # and the same outputs are written by a good call
    assert not (out[0] == -7).any() and out[3].tolist() == [0, 0, 0, 0]
    # a prefix whose last entry is not the total the workspaces were sized by: insert and scatter write nothing but the status bit
    fresh = hip.meshdist_workspace(P - 1, DEV)
    fresh['pair_slot'].fill_(-7); fresh['rows'].fill_(-7)
    status = torch.zeros(4, **i32)
    hip.meshdist_insert(index.vertices, index.faces, index.inv, index.prefix, fresh, status)
    fresh['start'] = torch.zeros_like(fresh['cell_count'])
    hip.meshdist_scatter(index.prefix, fresh, status)
    assert status.tolist() == [hip.MESHDIST_TOTAL, 0, 0, 0] and (fresh['pair_slot'] == -7).all() and (fresh['rows'] == -7).all()
    assert (fresh['keys'] == -1).all() and (fresh['cell_count'] == 0).all() and (fresh['fill'] == 0).all()
    small = dict(hip.meshdist_workspace(P, DEV), cap=ws['cap'] // 2)               # a table below twice the pairs
    with pytest.raises(RuntimeError, match='capacity'):
        hip.meshdist_insert(index.vertices, index.faces, index.inv, index.prefix, dict(small, keys=small['keys'][:small['cap']], cell_count=small['cell_count'][:small['cap']]), status)


# ---------------------------------------------------------------- the query
@functools.lru_cache(maxsize=None)
def query_scene():
    """1100 small triangles and 2901 queries (no multiple of 64) in a box of 24^3 cells around the origin, then planted faces and queries far from the box
    and from each other (marks -> (query row, first face)); coordinates on the grid of 1 / 64 where a result is to be exact:
      vertex / edge / inside   a query on a corner, on the middle of an edge and inside one face: d2 = 0
      tie, tie_exchanged       a query 1/8 below one face and 1/8 above another (no common nearest point): the smaller face wins, whichever it is
      shared_edge              a query above the common edge of two faces
      at_radius, above_radius  a query exactly `radius` above a face, and one whose d2 is the float32 after radius^2
      side_k, corner           the nearest face lies in a neighbouring cell alone - across each of the six sides of the query's cell, three of them
                               at negative cells, and across one corner: the query's cell lists it only through the dilation
      alone                    nothing within many cells
      nan, inf, ninf           non-finite queries
      sliver                   a face whose second edge is within 2e-5 of parallel to the first, as the nearest face"""
    rng = np.random.default_rng(8)
    verts, faces, Q, marks = list(small_faces(rng, 1100, -3, 3, (0.03, 0.15))), [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(1100)], [], {}

    def tri(a, b, c):
        k = len(verts)
        verts.extend([np.asarray(a, float), np.asarray(b, float), np.asarray(c, float)])
        faces.append((k, k + 1, k + 2))

    def put(name, query):
        marks[name] = (len(Q), len(faces))
        Q.append(np.asarray(query, float))
    put('vertex', (10.5, 10, 10)); put('edge', (10.25, 10, 10)); put('inside', (10.125, 10.125, 10))
    tri((10, 10, 10), (10.5, 10, 10), (10, 10.5, 10))
    for name, order in (('tie', (0.125, -0.125)), ('tie_exchanged', (-0.125, 0.125))):
        o = 20.0 if name == 'tie' else 30.0
        put(name, (o, o, o))
        for dz in order:                                                         # two faces with the query's foot inside, one above and one below
            tri((o - 0.5, o - 0.25, o + dz), (o + 0.5, o - 0.25, o + dz), (o, o + 0.5, o + dz))
    put('shared_edge', (40, 40, 40.125))
    tri((40, 39.5, 40), (40, 40.5, 40), (39.5, 40, 40)); tri((40, 40.5, 40), (40, 39.5, 40), (40.5, 40, 40))
    put('at_radius', (50.125, 50.125, 50.25))
    tri((50, 50, 50), (50.5, 50, 50), (50, 50.5, 50))
    put('above_radius', (64 - 5 * 2.0 ** -16, 0, 0.25))                           # beyond corner a by dx = 1.25 2^-14: D2 = 2^-4 + 1.5625 2^-28
    tri((64, 0, 0), (64.5, 0.25, 0), (64.5, -0.25, 0))
    k = 0
    for sign in (1, -1):
        for axis in range(3):
            e = np.eye(3)[axis] * sign
            base = sign * np.array([70.0 + 20 * k, 70.0, 70.0]) + 0.125
            put('side_%d' % k, base + 0.115 * e)
            u, w = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]
            tri(base + 0.145 * e - 0.02 * u, base + 0.15 * e + 0.02 * u, base + 0.145 * e + 0.02 * w)
            k += 1
    base = np.array([200.0, 70.0, 70.0]) + 0.125
    put('corner', base + 0.115)
    tri(base + 0.135, base + np.array([0.15, 0.135, 0.14]), base + np.array([0.135, 0.15, 0.14]))
    put('alone', (100, 100, 100))
    put('nan', (np.nan, 0, 0)); put('inf', (0, np.inf, 0)); put('ninf', (0, 0, -np.inf))
    put('sliver', (110.25, 0.05, 0.1))
    tri((110, 0, 0), (111, 0, 0), (110.5, 2.0 ** -17, 0))
    Q = np.concatenate([np.array(Q), rng.uniform(-3.2, 3.2, (2901 - len(Q), 3))]).astype(F)
    return Q, np.array(verts).astype(F), np.array(faces, dtype=np.int64), marks


@functools.lru_cache(maxsize=None)
def query_reference(radius=RADIUS):
    Q, V, Fc, _ = query_scene()
    return MD.mesh_distance(Q, V, Fc, radius)


def check_query_conditions():
    Q, V, Fc, marks = query_scene()
    want = query_reference()
    d2, face, region, second = want['d2'], want['face'], want['region'], want['second']
    r, _, r2 = N.radius_numbers(RADIUS)
    b = MD.binning(V, Fc, RADIUS)
    cq, _, _ = N.cells(Q, RADIUS)
    assert len(Q) % 64 and len(Q) % 256 and b['kept'].all() and 1000 < (face >= 0).sum() < len(Q) - 300        # hits and misses in numbers
    assert (np.bincount(region[face >= 0], minlength=7) >= 10).all(), np.bincount(region[face >= 0], minlength=7)      # every region wins at least 10 times
    for name, reg in (('vertex', 1), ('edge', 2), ('inside', 6)):
        qi, f = marks[name]
        assert d2[qi] == 0 and face[qi] == f and region[qi] == reg and (want['closest'][qi] == Q[qi]).all(), name
    for name in ('tie', 'tie_exchanged'):
        qi, f = marks[name]
        assert face[qi] == f and d2[qi] == F(0.015625) == second[qi] and region[qi] == 6
        assert want['closest'][qi, 2] == Q[qi, 2] + (0.125 if name == 'tie' else -0.125)             # the first of the two, above or below
    qi, f = marks['shared_edge']
    assert face[qi] == f and d2[qi] == F(0.015625) == second[qi] and region[qi] in (2, 4, 5) and (want['closest'][qi] == [40, 40, 40]).all()
    qi, f = marks['at_radius']
    assert face[qi] == f and d2[qi] == r2
    qi, f = marks['above_radius']
    x = np.float64(Q[qi]) - np.float64(V[Fc[f, 0]])
    assert face[qi] == -1 and np.isinf(d2[qi]) and F((x * x).sum()) == np.nextafter(r2, F(1)) and (want['closest'][qi] == Q[qi]).all()
    lo, hi = np.floor(V[Fc].min(1) * N.radius_numbers(RADIUS)[1]), np.floor(V[Fc].max(1) * N.radius_numbers(RADIUS)[1])      # the cells a face touches, undilated
    seen = set()
    for name in ['side_%d' % k for k in range(6)] + ['corner']:
        qi, f = marks[name]
        assert face[qi] == f and (lo[f] == hi[f]).all(), name                   # the face lies in one cell ...
        diff = (lo[f] - cq[qi]).astype(int)
        assert np.abs(diff).sum() == (3 if name == 'corner' else 1) and np.abs(diff).max() == 1, name      # ... next to the query's: listed there through the dilation alone
        seen.add((tuple(diff.tolist()), bool((cq[qi] < 0).any())))
    assert {s[0] for s in seen} == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1)} and sum(s[1] for s in seen) == 3
    qi, _ = marks['alone']
    assert face[qi] == -1 and (np.abs(np.floor(V * N.radius_numbers(RADIUS)[1]) - cq[qi]).max(1) > 4).all()
    for name in ('nan', 'inf', 'ninf'):
        qi = marks[name][0]
        assert face[qi] == -1 and np.isinf(d2[qi]) and (bits(want['closest'][qi]) == bits(Q[qi])).all()
    assert want['bad_queries'] == 3 and want['dropped_faces'] == 0
    qi, f = marks['sliver']
    e1, e2 = np.float64(V[Fc[f, 1]]) - np.float64(V[Fc[f, 0]]), np.float64(V[Fc[f, 2]]) - np.float64(V[Fc[f, 0]])
    assert face[qi] == f and 0 < np.linalg.norm(np.cross(e1, e2)) / np.linalg.norm(e1) / np.linalg.norm(e2) < 2e-5
    # the contract's precondition holds in this scene: the cell of every query lists its winner, so one cell's list sees what all faces see
    hit = face >= 0
    assert ((cq[hit] >= b['lo'][face[hit]]) & (cq[hit] < b['lo'][face[hit]] + b['ext'][face[hit]])).all()
    return want


def assert_result(got, want):
    d2, face, closest = got
    assert d2.dtype == torch.float32 and face.dtype == torch.int32 and closest.dtype == torch.float32
    assert tuple(d2.shape) == tuple(face.shape) == (len(want['d2']),) and tuple(closest.shape) == (len(want['d2']), 3)
    assert (face.cpu().numpy() == want['face']).all(), '%d faces differ' % (face.cpu().numpy() != want['face']).sum()
    assert (bits(d2) == bits(want['d2'])).all(), '%d d2 differ' % (bits(d2) != bits(want['d2'])).sum()
    assert (bits(closest) == bits(want['closest'])).all(), '%d closest differ' % (bits(closest) != bits(want['closest'])).any(1).sum()


def test_the_distances_faces_and_closest_points_equal_the_restatement():
    want = check_query_conditions()
    Q, V, Fc, _ = query_scene()
    q, v, f = dev(Q), dev(V), dev(Fc)
    got = mesh_distance(q, v, f, RADIUS)
    assert_result(got, want)
    again = mesh_distance(q, v, f, RADIUS)                                        # two calls give equal bytes
    assert all((bits(a) == bits(b)).all() for a, b in zip(got, again))
    index = MeshIndex(v, f, RADIUS)
    d2, face, none = index.query(q, closest=False)                                # closest null and non-null: the same d2 and face
    assert none is None and (bits(d2) == bits(got[0])).all() and (bits(face) == bits(got[1])).all()
    assert index.check() == want['bad_queries'] == 3 and index.dropped_faces == 0 and index.pairs == MD.binning(V, Fc, RADIUS)['total']


def test_a_radius_that_is_no_power_of_two_and_int32_faces():
    Q, V, Fc, _ = query_scene()
    want = query_reference(OTHER_RADIUS)
    b = MD.binning(V, Fc, OTHER_RADIUS)
    cq, _, _ = N.cells(Q, OTHER_RADIUS)
    hit = want['face'] >= 0
    assert hit.sum() > 1200 and ((cq[hit] >= b['lo'][want['face'][hit]]) & (cq[hit] < b['lo'][want['face'][hit]] + b['ext'][want['face'][hit]])).all()
    assert_result(mesh_distance(dev(Q), dev(V), dev(Fc.astype(np.int32)), OTHER_RADIUS), want)


def test_empty_queries_and_an_empty_mesh_launch_nothing(monkeypatch):
    Q, V, Fc, _ = query_scene()
    q, v, f = dev(Q[:100]), dev(V), dev(Fc)
    for name in ('meshdist_count', 'meshdist_workspace', 'meshdist_insert', 'meshdist_scatter', 'meshdist_query', 'cloud_scan'):
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail('a build or a launch for an empty set'))
    none, nof = torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int64, device=DEV)
    d2, face, closest = mesh_distance(none, v, f, RADIUS)
    assert tuple(d2.shape) == tuple(face.shape) == (0,) and tuple(closest.shape) == (0, 3) and d2.dtype == torch.float32 and face.dtype == torch.int32
    for vv, ff in ((v, nof), (torch.empty(0, 3, device=DEV), nof)):
        d2, face, closest = mesh_distance(q, vv, ff, RADIUS)
        assert (face == -1).all() and torch.isinf(d2).all() and face.numel() == 100 and (bits(closest) == bits(q)).all()
    index = MeshIndex(v, nof, RADIUS)
    d2, face, closest = index.query(q)
    assert index.pairs == 0 and index.check() == 0 and (face == -1).all() and (bits(closest) == bits(q)).all()
    with pytest.raises(ValueError):                                              # the arguments are still checked
        mesh_distance(none, v, f, -1.0)


def test_a_mesh_of_dropped_faces_alone_builds_nothing():
    V = dev(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=F))
    index = MeshIndex(V, dev(np.array([[0, 1, 2], [0, 1, 7]])), RADIUS)
    d2, face, closest = index.query(V)
    assert index.dropped_faces == 2 and index.pairs == 0 and index.ws is None and (face == -1).all() and torch.isinf(d2).all() and index.check() == 0


# ---------------------------------------------------------------- lists that are not the build's (the guards of csrc/voxel_table.h)
@functools.lru_cache(maxsize=None)
def two_faces():
    """two triangles under the lattice of queries of tests/grid_lists.py whose cell boxes both hold the cell (0, 0, 0), that of query 0"""
    V = np.array([[0.05, 0.05, 0.1], [0.45, 0.05, 0.1], [0.05, 0.45, 0.1], [0.3, 0.3, 0.3], [0.7, 0.3, 0.3], [0.3, 0.7, 0.3]], dtype=F)
    return V, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


def check_two_faces():
    """-> (the pair of face 0 in the cell of query 0, the queries of that cell, the others, the restated result)"""
    Q, _ = G.lattice()
    V, Fc = two_faces()
    b, cq = MD.binning(V, Fc, G.CELL), N.cells(Q, G.CELL)[0].astype(int)
    lo, ext = b['lo'].astype(int), b['ext'].astype(int)
    assert b['kept'].all() and (cq[0] == 0).all() and ((lo <= 0) & (lo + ext > 0)).all()        # both faces are listed in the cell (0, 0, 0)
    touched = (cq == 0).all(1)
    want = MD.mesh_distance(Q, V, Fc, G.CELL)
    assert touched.sum() >= 4 and (want['face'][touched] >= 0).all() and (want['face'][~touched] >= 0).sum() > 50 and (want['face'][~touched] < 0).sum() > 50
    assert (np.nonzero(~touched)[0] >= 256).any()
    return int(-lo[0, 0] + ext[0, 0] * (-lo[0, 1] + ext[0, 1] * -lo[0, 2])), touched, ~touched, want


def test_the_query_refuses_a_list_that_leaves_the_rows_and_a_face_past_the_mesh():
    pair, touched, untouched, want = check_two_faces()
    v, f, q = G.padded(two_faces()[0]), G.padded(two_faces()[1]), G.padded(G.lattice()[0])
    _, inv, r2 = (float(x) for x in N.radius_numbers(G.CELL))
    good = G.mesh_build(v, f)
    assert good['status'].tolist() == [0, 0, 2, 0] and good['P'] == MD.binning(*two_faces(), G.CELL)['total']

    def query(ws):
        out = torch.full((len(q),), -7.0, device=DEV), torch.full((len(q),), -7, dtype=torch.int32, device=DEV), torch.full((len(q), 3), -7.0, device=DEV)
        hip.meshdist_query(q, v, f, inv, r2, ws, 4096, *out, ws['status'])
        return out, ws['status'].tolist()
    got, status = query(G.fresh(good))                                           # (d) the untampered workspace through the same helpers
    assert status == [0, 0, 0, 0]
    assert_result(got, want)
    slot = int(good['pair_slot'][pair])
    assert sorted(G.lists_of(good)[slot]) == [0, 1]
    for case, tamper in (('a', lambda ws: G.move_list_out(ws, slot, good['P'])), ('b', lambda ws: G.first_entry_past_the_end(ws, slot, len(f)))):
        ws = G.fresh(good)
        tamper(ws)
        bad, status = query(ws)
        assert status == [G.LISTS, 0, 0, 0]
        assert all((bits(a)[untouched] == bits(b)[untouched]).all() for a, b in zip(bad, got))
        assert bool(((bad[1] >= -1) & (bad[1] < len(f))).all())                  # a face of the mesh or none
        assert case == 'b' or bool((bad[1][torch.from_numpy(touched).to(DEV)] == -1).all())      # (a): the refused list is not read at all


def test_the_scatter_refuses_a_count_that_is_not_the_inserts():
    pair = check_two_faces()[0]
    v, f = G.padded(two_faces()[0]), G.padded(two_faces()[1])
    good = G.mesh_build(v, f)
    G.assert_a_short_count_is_refused(good, lambda tamper: G.mesh_build(v, f, tamper), lambda ws: int(ws['pair_slot'][pair]), good['P'])


# ---------------------------------------------------------------- the composition
GT_SPACING, FINE_SPACING, TAUS = 0.7, 0.45, (0.125, 0.25, 0.5)


@functools.lru_cache(maxsize=None)
def room():
    """the generated room of the mesh tests (eight tiles per wall, so that the brute-force restatement stays quick) as ground truth, and as prediction
    the noisy, partly missing copy of its own surface that the 3-D score tests use: its samples at another spacing, moved by up to 0.2 per axis,
    everything with x > 2 cut away, a tenth of the labels exchanged for a neighbour's"""
    s = M.scene(n_wall=8)
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
def room_samples(spacing=GT_SPACING):
    r = room()
    return N.sample_mesh(r['vertices'], r['faces'], spacing, vertex_ids=r['vertex_ids'])


@functools.lru_cache(maxsize=None)
def room_scores(spacing=GT_SPACING):
    r, gt = room(), room_samples(spacing)
    return MD.scores(r['pred_points'], gt['points'], r['vertices'], r['faces'], TAUS, pred_ids=r['pred_ids'], gt_ids=gt['ids'])


def cloud_of(points, ids, segments):
    n = len(points)
    p = dev(points)
    return PanopticCloud(p, p.clone(), torch.full((n, 3), 0.5, device=DEV), dev(ids), torch.full((n, 3), 0.5, device=DEV),
                         torch.arange(n, device=DEV), [0, n], [dict(s) for s in segments])


def assert_scores(got, want, n_terms):
    for k in ('n_pred', 'n_gt', 'pred_within', 'gt_within', 'precision', 'recall', 'fscore', 'accuracy_matched', 'completeness_matched', 'thresholds', 'max_dist',
              'metric', 'gt_pairs'):
        assert got[k] == want[k], (k, got[k], want[k])
    tol = n_terms * 2.0 ** -52                                                   # an fp64 sum of N terms, in another order
    for k in ('accuracy_mean', 'accuracy_median', 'completeness_mean', 'completeness_median', 'chamfer'):
        assert abs(got[k] - want[k]) <= tol * abs(want[k]), (k, got[k], want[k])


def assert_pq(got, want_pred, want_gt, r):
    want = panoptic_quality(dev(want_pred)[None, None], r['segments'], dev(want_gt)[None, None], r['segments'], things=r['things'])
    for k in ('pq', 'sq', 'rq', 'pq_things', 'pq_stuff', 'miou', 'pixel_acc', 'n_pixels', 'void_pixels', 'per_class', 'matches'):
        assert got[k] == want[k], k
    assert (got['tables']['counts'] == want['tables']['counts']).all()
    return want


def score_kw(r):
    return dict(thresholds=TAUS, gt_vertex_ids=dev(r['vertex_ids']), gt_segments=r['segments'], things=r['things'])


def test_the_surface_metric_scores_the_noisy_room_as_the_restatement_says():
    r, gt, want = room(), room_samples(), room_scores()
    points_want = N.scores(r['pred_points'], gt['points'], TAUS, pred_ids=r['pred_ids'], gt_ids=gt['ids'])
    # the scene decides something: neither perfect nor empty, the thresholds differ, the cut shows in the recall, labels both right and wrong
    assert 0 < want['precision'][0] < want['precision'][1] <= want['precision'][2] <= 1 and 0 < want['recall'][0] < want['recall'][2] < 0.95
    assert 0 < want['accuracy_matched'] <= 1 and want['accuracy_median'] != want['accuracy_mean'] and want['n_pred'] > 2500 and want['n_gt'] > 3000
    assert (want['pq_pred'] == 0).any() and (want['pq_pred'] == want['pq_gt']).sum() > 1000
    # a sample can only be farther than the surface it lies on: every predicted point is at most as far from the surface, and most are nearer
    assert want['accuracy_mean'] < points_want['accuracy_mean'] and all(a >= b for a, b in zip(want['pred_within'], points_want['pred_within']))
    assert want['pred_within'][0] > points_want['pred_within'][0]
    v, f = dev(r['vertices']), dev(r['faces'])
    cloud = cloud_of(r['pred_points'], r['pred_ids'], r['segments'])
    got = score_reconstruction(cloud, v, f, spacing=GT_SPACING, metric='surface', **score_kw(r))
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert got['gt_max_cell_faces'] >= 1 and got['dropped_faces'] == gt['dropped_faces'] and got['spacing'] == float(F(GT_SPACING))
    assert_pq(got['pq3d'], want['pq_pred'], want['pq_gt'], r)
    # ground truth -> a cloud stays point to point: that direction is what 'points' gives
    points = score_reconstruction(cloud, v, f, spacing=GT_SPACING, metric='points', **score_kw(r))
    for k in ('gt_within', 'recall', 'completeness_matched', 'completeness_mean', 'completeness_median'):
        assert got[k] == points[k], k
    assert got['accuracy_mean'] < points['accuracy_mean']
    # metric='points' is the call without the keyword
    plain = score_reconstruction(cloud, v, f, spacing=GT_SPACING, **score_kw(r))
    assert plain['metric'] == 'points' and 'gt_pairs' not in plain and 'gt_max_cell_faces' not in plain and set(plain) == set(points)
    for k in plain:
        if k != 'pq3d':
            assert plain[k] == points[k], k
    assert all(plain['pq3d'][k] == points['pq3d'][k] for k in ('pq', 'sq', 'rq', 'miou', 'per_class', 'matches'))
    for k in ('n_pred', 'n_gt', 'pred_within', 'gt_within', 'precision', 'recall', 'fscore'):
        assert plain[k] == points_want[k], k


def test_pred_within_does_not_depend_on_the_spacing_under_the_surface_metric():
    r = room()
    want, fine_want = room_scores(), room_scores(FINE_SPACING)
    coarse_points = N.scores(r['pred_points'], room_samples()['points'], TAUS)
    fine_points = N.scores(r['pred_points'], room_samples(FINE_SPACING)['points'], TAUS)
    assert want['pred_within'] == fine_want['pred_within'] and want['n_gt'] != fine_want['n_gt'] and coarse_points['pred_within'] != fine_points['pred_within']
    v, f, p = dev(r['vertices']), dev(r['faces']), dev(r['pred_points'])
    got = {(m, s): score_reconstruction(p, v, f, thresholds=TAUS, spacing=s, metric=m) for m in ('surface', 'points') for s in (GT_SPACING, FINE_SPACING)}
    a, b = got['surface', GT_SPACING], got['surface', FINE_SPACING]
    for k in ('pred_within', 'precision', 'accuracy_matched', 'accuracy_mean', 'accuracy_median', 'gt_pairs', 'gt_max_cell_faces'):
        assert a[k] == b[k], k
    assert a['pred_within'] == want['pred_within'] and a['n_gt'] != b['n_gt'] and a['pq3d'] is None
    assert_scores(b, fine_want, max(fine_want['n_pred'], fine_want['n_gt']))
    assert got['points', GT_SPACING]['pred_within'] != got['points', FINE_SPACING]['pred_within']
    assert got['points', GT_SPACING]['pred_within'] == coarse_points['pred_within'] and got['points', FINE_SPACING]['pred_within'] == fine_points['pred_within']


def test_a_predicted_mesh_is_measured_surface_to_surface_in_both_directions():
    r, gt = room(), room_samples()
    v, f = dev(r['vertices']), dev(r['faces'])
    # a PanopticMesh: the room's own mesh, moved by a similarity transform, with its face ids; scored through the transform that carries it back
    scale, t = 1.25, np.array([0.3, -0.2, 0.5])
    T = N.similarity(scale, np.eye(3), t)
    Ti = np.linalg.inv(T)
    shift = F([0.2, 0.07, -0.05])
    small = ((r['vertices'].astype(np.float64) + shift) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    f32 = np.where((r['faces'] < 0) | (r['faces'] >= len(small)), -1, r['faces']).astype(np.int32)
    mesh = PanopticMesh(dev(small), dev(f32), dev(r['face_ids']), dev(r['vertex_ids']), torch.zeros(len(small), 3, device=DEV),
                        torch.zeros(len(f32), dtype=torch.int64, device=DEV), [0, 1], r['segments'])
    A = dev(T, torch.float32)
    back = (dev(small) @ A[:3, :3].T + A[:3, 3]).cpu().numpy()                    # as score_reconstruction moves it: torch's matmul is not part of the contract
    own = N.sample_mesh(back, f32, GT_SPACING, face_ids=r['face_ids'])
    want = MD.scores(own['points'], gt['points'], r['vertices'], r['faces'], TAUS, gt_ids=gt['ids'], pred_mesh=(back, f32, r['face_ids']))
    assert 0 < want['precision'][0] < 1 and 0 < want['recall'][0] < 1 and want['precision'][2] > 0.99 and want['n_pred'] == len(own['points']) > 3000
    assert (want['pq_pred'] == want['pq_gt']).sum() > 1000 and (want['pq_pred'] != want['pq_gt']).sum() > 10
    got = score_reconstruction(mesh, v, f, spacing=GT_SPACING, metric='surface', transform=T, **score_kw(r))
    assert_scores(got, want, max(want['n_pred'], want['n_gt']))
    assert_pq(got['pq3d'], want['pq_pred'], want['pq_gt'], r)
    points = score_reconstruction(mesh, v, f, spacing=GT_SPACING, transform=T, **score_kw(r))
    assert got['completeness_mean'] < points['completeness_mean'] and got['accuracy_mean'] < points['accuracy_mean']       # both directions are nearer now
    assert all(a >= b for a, b in zip(got['gt_within'], points['gt_within'])) and got['gt_within'][0] > points['gt_within'][0]
