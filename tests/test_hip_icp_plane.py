"""The point-to-plane ICP against the triangles on the GPU (csrc/meshdist.hip's icp_plane_step, panst3r_amd.engine.icp_to_mesh /
refine_alignment(target='surface') / score_reconstruction(refine={'target': 'surface'})) against the numpy restatement of tests/icp_plane_ref.py, BIT
FOR BIT: the move is separately rounded fp32, the search is the mesh distance's, the terms are separately rounded fp64 operations added in an order the
contract fixes, and the host step of the loop is the same numpy in the same process - there is no tolerance to choose.

Conditions, not measurements: before the GPU is compared, every `check_*` asserts ON THE RESTATEMENT that the generated scene holds what it was built
for; the lists are in the docstrings of `step_scene` and of `icp_plane_ref.room_scene`."""
import functools

import numpy as np
import pytest
import torch

import grid_lists as G
import icp_plane_ref as P
import icp_ref as I
import meshdist_ref as MD
import nearest_ref as N
import test_hip_icp as TI
from test_hip_meshdist import two_faces, check_two_faces
from panst3r_amd import hip
from panst3r_amd.engine import icp_to_mesh, refine_alignment, score_reconstruction, Alignment, PanopticMesh, VoxelCloud
from panst3r_amd.engine import meshdist, score3d
from panst3r_amd.engine.meshdist import MeshIndex

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
CHUNK = hip.ICP_CHUNK
bits, same, dev = TI.bits, TI.same, TI.dev


# ---------------------------------------------------------------- the step
CELL = P.MAX_DIST                                                                # 0.32 against quads of 0.5: every cell lists several faces
R2 = F(0.2) * F(0.2)                                                             # below the cell's
A = np.array([[0, 0, 2, 0.5], [2, 0, 0, -1], [0, 2, 0, 0.25]], dtype=F)          # m = (2 x2 + 0.5, 2 x0 - 1, 2 x1 + 0.25): exact for dyadic points
C0 = F([1.5, 0.375, 1.0])
SIZES = (1, 63, 64, 257, CHUNK, CHUNK + 1, 2 * CHUNK + 77)
TIE, VERTEX, EDGE, NONE, SHRUNK, NAN, INF, OUT, ON = range(9)
PLANTED = {TIE: (0.5, 0.125, 0.25), VERTEX: (3.0625, 0.0625, 2.0625), EDGE: (3.125, 0.0625, 1.1875), NONE: (1.5, 1.0, 1.5), SHRUNK: (1.0, 0.25, 1.5),
           OUT: (1000000.5, 0.5, 0.5), ON: (1.0, 0.0, 1.0)}


def unmoved(m):
    m = np.asarray(m, dtype=np.float64)
    return np.stack([(m[..., 1] + 1) / 2, (m[..., 2] - 0.25) / 2, (m[..., 0] - 0.5) / 2], -1)


@functools.lru_cache(maxsize=None)
def step_scene():
    """the room mesh (112 faces) and 2 x 4096 + 77 sources that A carries next to its faces - drawn on them, pushed up to 0.35 off along the normal and
    jittered, so that a good half match within r = 0.2, below the cell's edge of 0.32, some of them beyond the mesh's border.  Planted (dyadic
    numbers: no rounding in the move): `TIE` above an edge two floor faces share; `VERTEX` and `EDGE` beyond the floor's far corner and far edge;
    `NONE` a metre above the floor; `SHRUNK` 0.25 above it: inside the cell's radius, outside r; `NAN` and `INF` not finite; `OUT` a million units
    away, its cell out of range; `ON` exactly on a vertex of the floor: d2 = 0.  The prefixes of `SIZES` rows are the smaller cases."""
    rng = np.random.default_rng(29)
    V, Fc = P.room_mesh()
    n = SIZES[-1]
    pts, nrm = P._on_faces(rng, V, Fc, n)
    moved = pts + nrm * rng.uniform(-0.35, 0.35, (n, 1)) + rng.normal(0, 0.04, (n, 3))
    X = unmoved(moved).astype(F)
    for i, m in PLANTED.items():
        X[i] = unmoved(m)
    X[NAN], X[INF] = [np.nan, 0, 0], [0, np.inf, 0]
    return np.ascontiguousarray(X), V, Fc


@functools.lru_cache(maxsize=None)
def step_reference(n, r2=R2):
    X, V, Fc = step_scene()
    return P.step(X[:n], A, C0, V, Fc, CELL, r2)


def check_step_conditions():
    X, V, Fc = step_scene()
    want = step_reference(SIZES[-1])
    face, d2, moved = want['face'], want['d2'], want['moved']
    assert len(X) == 2 * CHUNK + 77 and len(Fc) == 112 and 0.3 <= (face >= 0).mean() <= 0.9
    assert max(len(v) for v in MD.cell_lists(V, Fc, CELL).values()) >= 6         # the cell lists hold several faces
    assert all((moved[i] == F(m)).all() for i, m in PLANTED.items())             # the move of the planted points is exact
    every = MD.closest_point(*(V[Fc].astype(np.float64)[:, k] for k in range(3)), moved[TIE].astype(np.float64))[0].astype(F)
    ties = np.flatnonzero(every == d2[TIE])
    assert len(ties) >= 2 and face[TIE] == ties.min() and want['second'][TIE] == d2[TIE] == F(0.125) * F(0.125)      # a tie, to the smaller face
    assert want['region'][VERTEX] in (0, 1, 3) and want['region'][EDGE] in (2, 4, 5) and (moved[[VERTEX, EDGE], 0] > V[:, 0].max()).all()
    assert face[VERTEX] >= 0 and face[EDGE] >= 0
    assert face[NONE] == -1 == want['wide_face'][NONE] and np.isinf(d2[NONE])
    assert face[SHRUNK] == -1 and want['wide_face'][SHRUNK] >= 0 and R2 < want['wide_d2'][SHRUNK] <= N.radius_numbers(CELL)[2]
    assert ((want['wide_face'] >= 0) & (face < 0)).sum() > 100                   # pairs the cell sees and the smaller r2 rejects
    assert want['bad'] == 2 and face[NAN] == -1 == face[INF] and not np.isfinite(moved[[NAN, INF]]).all(1).any()
    assert np.isfinite(moved[OUT]).all() and not N.cells(moved[OUT:OUT + 1], CELL)[2][0] and face[OUT] == -1
    assert d2[ON] == 0 and face[ON] >= 0
    Pn = want['partials']
    assert Pn.shape == (3, 40) and all(Pn[b, 0] > 30 for b in range(3)) and want['out'][0] == (face >= 0).sum() and (want['out'][38:] == 0).all()
    assert np.isfinite(want['out']).all() and (want['out'][[1, 8, 14, 19, 23, 26, 28]] > 0).all()      # the diagonal of the system
    return want


def run_step(index, x, n, r2=R2, outputs=True, matrix=A, c0=C0):
    iws = hip.icp_plane_workspace(n, DEV)
    iws['partials'].fill_(-7.0); iws['out'].fill_(-7.0)
    d2, face = (torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)) if outputs else (None, None)
    out = hip.icp_plane_step(x, matrix, c0, index.vertices, index.faces, index.inv, index.r2, float(r2), index.ws, index.max_cell_faces, iws, d2, face)
    assert out is iws['out']
    return iws, d2, face


@pytest.mark.parametrize('n', SIZES)
def test_one_step_equals_the_restatement(n):
    check_step_conditions()
    X, V, Fc = step_scene()
    want = step_reference(n)
    index = MeshIndex(dev(V), dev(Fc), CELL)
    x = dev(X[:n])
    iws, d2, face = run_step(index, x, n)
    assert same(iws['out'], want['out']), (iws['out'].cpu().numpy() - want['out'])
    assert same(iws['partials'], want['partials'])
    assert same(d2, want['d2']) and same(face, want['face'])
    assert iws['status'].tolist() == [0, 0, 0, want['bad']] and index.check() == 0      # (the index's own status words are not the step's)
    # the same matches through the public query on the restated moved points, accepted at the smaller r2
    qd2, qface, _ = index.query(dev(want['moved']))
    ok = (qface >= 0) & (qd2 <= float(R2))
    assert same(torch.where(ok, qd2, torch.full_like(qd2, float('inf'))), d2) and same(torch.where(ok, qface, torch.full_like(qface, -1)), face)
    # without d2 / face the same moments; and again: equal bytes
    quiet, none_d2, none_face = run_step(index, x, n, outputs=False)
    assert none_d2 is None and none_face is None and same(quiet['out'], iws['out']) and same(quiet['partials'], iws['partials'])
    again, d2b, faceb = run_step(index, x, n)
    assert same(again['out'], iws['out']) and same(again['partials'], iws['partials']) and same(d2b, d2) and same(faceb, face)
    if n in (SIZES[3], SIZES[-1]):
        # r2 = 0: only a source exactly on the surface is matched
        zero = step_reference(n, F(0))
        assert 1 <= zero['out'][0] < 10 and zero['face'][ON] >= 0 and zero['face'][TIE] == -1
        iws, d2, face = run_step(index, x, n, r2=0.0)
        assert same(iws['out'], zero['out']) and same(iws['partials'], zero['partials']) and same(d2, zero['d2']) and same(face, zero['face'])
        # at the cell's own r2 the step accepts what the query accepts
        wide = step_reference(n, N.radius_numbers(CELL)[2])
        iws, d2, face = run_step(index, x, n, r2=index.r2)
        assert same(iws['out'], wide['out']) and same(face, wide['face']) and same(face, qface) and wide['out'][0] > want['out'][0] and wide['face'][SHRUNK] >= 0
        with pytest.raises(ValueError, match='exceeds'):                         # the wrapper refuses a radius beyond the cells
            run_step(index, x, n, r2=float(np.nextafter(F(index.r2), F(1))))


def test_a_million_sources_take_the_reducer_round_its_loop_twice():
    """N = 256 x 4096 + 5: 257 rows of partials, so lane 0 of the reducer adds two of them.  The sources are a set of 4 099 distinct ones tiled: the
    restatement searches and evaluates the distinct rows once and only the fixed-order sum runs at full length."""
    X, V, Fc = step_scene()
    base, n = X[:CHUNK + 3], 256 * CHUNK + 5
    rows = np.arange(n) % len(base)
    moved = I.move(base, A)
    m = P.match(moved, V, Fc, CELL, R2)
    t = P.terms(moved, C0, V, Fc, m['d2'], m['face'])
    out, partials = P.moments(t[:, rows])
    d2, face = m['d2'][rows], m['face'][rows]
    assert n > 2 ** 20 and partials.shape == (257, 40) and partials[256, 0] >= 1 and 0.3 * n < out[0] == (face >= 0).sum() < 0.9 * n
    index = MeshIndex(dev(V), dev(Fc), CELL)
    iws, gd2, gface = run_step(index, dev(np.ascontiguousarray(base[rows])), n)
    assert same(iws['out'], out) and same(iws['partials'], partials) and same(gd2, d2) and same(gface, face)
    bad = int((~np.isfinite(moved).all(1))[rows].sum())
    assert bad == 2 * 256 and iws['status'].tolist() == [0, 0, 0, bad]          # NaN and inf once per copy of the set


def test_every_refusal_of_the_launcher_leaves_the_outputs_untouched():
    X, V, Fc = step_scene()
    n = 300
    index = MeshIndex(dev(V), dev(Fc), CELL)
    x, ws = dev(X[:n]), index.ws
    iws = hip.icp_plane_workspace(n, DEV)
    d2, face = torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    iws['partials'].fill_(-7.0); iws['out'].fill_(-7.0); iws['status'].fill_(-7)
    p = lambda t: t.data_ptr()
    good = dict(source=p(x), N=n, c0=[float(c) for c in C0], vertices=p(index.vertices), Nv=len(V), faces=p(index.faces), F=len(Fc), inv=index.inv,
                r2=float(R2), keys=p(ws['keys']), cap=ws['cap'], start=p(ws['start']), cell_count=p(ws['cell_count']), rows=p(ws['rows']), total=ws['P'],
                mcf=4096, d2=p(d2), face=p(face), partials=p(iws['partials']), out=p(iws['out']), status=p(iws['status']))

    def call(**change):
        a = dict(good, **change)
        return hip.lib().pst_plane_icp_step(a['source'], a['N'], *[float(v) for v in A.ravel()], *a['c0'], a['vertices'], a['Nv'], a['faces'], a['F'],
                                            a['inv'], a['r2'], a['keys'], a['cap'], a['start'], a['cell_count'], a['rows'], a['total'], a['mcf'], a['d2'],
                                            a['face'], a['partials'], a['out'], a['status'], torch.cuda.current_stream().cuda_stream)
    nan, inf = float('nan'), float('inf')
    refusals = [dict(source=None), dict(vertices=None), dict(faces=None), dict(keys=None), dict(start=None), dict(cell_count=None), dict(rows=None),
                dict(partials=None), dict(out=None), dict(status=None), dict(N=0), dict(N=-5), dict(N=2 ** 30 + 1), dict(d2=None), dict(face=None),
                dict(Nv=0), dict(F=0), dict(F=2 ** 30 + 1), dict(total=0), dict(total=2 ** 30 + 1), dict(cap=ws['cap'] - 1), dict(cap=ws['P']),
                dict(inv=0.0), dict(inv=-1.0), dict(inv=inf), dict(inv=nan), dict(r2=-1.0), dict(r2=nan), dict(r2=inf), dict(mcf=0),
                dict(c0=[nan, 0.0, 0.0]), dict(c0=[0.0, inf, 0.0]), dict(c0=[0.0, 0.0, -inf])]
    for change in refusals:
        assert call(**change) < 0, change
        assert b'plane_icp_step' in hip.lib().pst_last_error(), change
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (face == -7).all() and (iws['partials'] == -7).all() and (iws['out'] == -7).all() and (iws['status'] == -7).all()
    iws['status'].zero_()
    assert call() == 0 and call(d2=None, face=None) == 0                         # ... and the good call runs, with and without d2 / face
    assert same(iws['out'], step_reference(n)['out']) and same(face, step_reference(n)['face'])
    with pytest.raises(ValueError, match='go together'):
        hip.icp_plane_step(x, A, C0, index.vertices, index.faces, index.inv, index.r2, float(R2), ws, 4096, iws, d2, None)
    with pytest.raises(ValueError, match='3 x 4'):
        hip.icp_plane_step(x, np.eye(4), C0, index.vertices, index.faces, index.inv, index.r2, float(R2), ws, 4096, iws)
    with pytest.raises(ValueError, match='3 x 4'):
        hip.icp_plane_step(x, A, C0[:2], index.vertices, index.faces, index.inv, index.r2, float(R2), ws, 4096, iws)


def test_the_step_refuses_a_list_that_leaves_the_rows_and_a_face_past_the_mesh():
    """the search of the step is the query's: the same tampered lists (tests/grid_lists.py, the two faces of tests/test_hip_meshdist.py), refused
    through the STEP's status words"""
    pair, touched, untouched, _ = check_two_faces()
    V, Fc = two_faces()
    Q = G.lattice()[0]
    v, f, q = G.padded(V), G.padded(Fc), G.padded(Q)
    _, inv, r2 = (float(x) for x in N.radius_numbers(G.CELL))
    still = np.eye(3, 4, dtype=F)                                                # moves nothing
    good = G.mesh_build(v, f)

    def step(ws):
        iws = hip.icp_plane_workspace(len(Q), DEV)
        d2, face = torch.full((len(Q),), -7.0, device=DEV), torch.full((len(Q),), -7, dtype=torch.int32, device=DEV)
        hip.icp_plane_step(q, still, C0, v, f, inv, r2, r2, ws, 4096, iws, d2, face)
        assert ws['status'].tolist() == [0, 0, 0, 0]                             # the build's status words are not the step's
        return iws, d2, face
    want = P.step(Q, still, C0, V, Fc, G.CELL, F(r2))
    assert (want['moved'] == Q).all() and want['out'][0] > 50 and (want['face'][touched] >= 0).all()
    iws, d2, face = step(G.fresh(good))                                          # the untampered workspace through the same helpers
    assert iws['status'].tolist() == [0, 0, 0, 0] and same(iws['out'], want['out']) and same(d2, want['d2']) and same(face, want['face'])
    slot = int(good['pair_slot'][pair])
    for case, tamper in (('a', lambda ws: G.move_list_out(ws, slot, good['P'])), ('b', lambda ws: G.first_entry_past_the_end(ws, slot, len(f)))):
        ws = G.fresh(good)
        tamper(ws)
        bad, bd2, bface = step(ws)
        assert bad['status'].tolist() == [G.LISTS, 0, 0, 0], case
        assert (bits(bd2)[untouched] == bits(d2)[untouched]).all() and (bits(bface)[untouched] == bits(face)[untouched]).all()
        assert bool(((bface >= -1) & (bface < len(f))).all())                    # a face of the mesh or none
        assert case == 'b' or bool((bface[torch.from_numpy(touched).to(DEV)] == -1).all())      # (a): the refused list is not read at all


# ---------------------------------------------------------------- the loop
def assert_alignment(got, want, transform=None):
    assert isinstance(got, Alignment) and got.transform.dtype == torch.float64 and tuple(got.transform.shape) == (4, 4) and not got.transform.is_cuda
    assert (got.iterations, got.converged, got.reason) == (want['iterations'], want['converged'], want['reason'])
    assert len(got.history) == len(want['history'])
    for k, (g, w) in enumerate(zip(got.history, want['history'])):
        assert set(g) == {'radius', 'matched', 'rmse', 'plane_rmse'} and g['matched'] == w[1], (k, g, w)
        assert same(np.float64([g['radius'], g['rmse'], g['plane_rmse']]), np.float64([w[0], w[2], w[3]])), (k, g, w)
    assert same(got.transform, want['transform'] if transform is None else transform)


VARIANTS = [dict(), dict(noisy=True), dict(with_scale=False), dict(every=3), dict(init=True), dict(noisy=True, with_scale=False, every=3, init=True),
            dict(floor_only=True), dict(floor_only=True, init=True)]


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()) or 'room')
def test_the_loop_equals_the_restated_loop(variant):
    want = P.loop_reference(**variant)
    noisy, floor = variant.get('noisy', False), variant.get('floor_only', False)
    if floor:
        assert want['reason'] == 'degenerate' and want['iterations'] == 1 and want['transforms'] == []
    else:
        assert want['iterations'] >= 3 and want['reason'] == 'converged'
    s = P.room_scene(noisy, floor)
    kw = dict(P.NOISY_KW) if noisy else dict(max_dist=P.MAX_DIST)
    kw.update({k: v for k, v in variant.items() if k in ('with_scale', 'every')})
    if variant.get('init'):
        kw['init'] = torch.from_numpy(P.loop_init())
    x, v, f = dev(s['source']), dev(s['vertices']), dev(s['faces'])
    got = icp_to_mesh(x, v, f, **kw)
    assert_alignment(got, want)
    if floor:
        assert same(got.transform, P.loop_init() if variant.get('init') else np.eye(4))      # the transform of the step before: the start
        return
    # every T on the way: the loop is deterministic, so a run cut after k steps ends with the restated loop's k-th transform
    for k in (range(1, want['iterations']) if not variant else (1, 2)):
        cut = icp_to_mesh(x, v, f, **dict(kw, iters=k))
        assert cut.reason == 'iters' and cut.iterations == k and not cut.converged and same(cut.transform, want['transforms'][k - 1]), k
    if not variant:
        assert same(icp_to_mesh(x, v, dev(s['faces'].astype(np.int64)), **kw).transform, want['transform'])      # int64 faces


def test_empty_and_short_starts_on_the_device():
    s = P.room_scene()
    v, f = dev(s['vertices']), dev(s['faces'])
    with pytest.raises(ValueError, match='nothing within max_dist'):
        icp_to_mesh(dev(s['source'] + F(50)), v, f, max_dist=P.MAX_DIST)
    with pytest.raises(ValueError, match='at least 7'):
        icp_to_mesh(dev(s['source'][:6]), v, f, max_dist=P.MAX_DIST)
    with pytest.raises(ValueError, match='not finite'):
        icp_to_mesh(dev(np.concatenate([s['source'][:20], F([[np.nan, 0, 0]])])), v, f, max_dist=P.MAX_DIST)
    few = np.concatenate([s['source'][:5], s['source'][:5] + F(50)])            # five pairs, seven unknowns: degenerate, the start returned
    want = P.icp_to_mesh(few, s['vertices'], s['faces'], P.MAX_DIST)
    assert want['reason'] == 'degenerate' and want['history'][0][1] == 5
    assert_alignment(icp_to_mesh(dev(few), v, f, max_dist=P.MAX_DIST), want)
    with pytest.raises(ValueError, match='nothing within max_dist'):             # a mesh without a kept face
        icp_to_mesh(dev(s['source']), v, dev(np.array([[0, 0, 1], [2, 2, 2]], dtype=np.int32)), max_dist=P.MAX_DIST)


# ---------------------------------------------------------------- the opt-in: the room of the 3-D score tests
SURFACE_KW = dict(target='surface', iters=2, every=8)                            # (the restatement is brute force over 2 207 faces: a few hundred sources, two steps)


def test_refine_alignment_to_the_surface_on_a_tensor_a_voxel_cloud_and_a_mesh():
    r = TI.room()
    v, f = dev(r['vertices']), dev(r['faces'])
    kw = dict(spacing=TI.GT_SPACING, max_dist=TI.REFINE_DIST, **SURFACE_KW)
    ref = dict(iters=2, every=8)
    # a tensor, from a start that is not the identity: icp_to_mesh runs from the identity on the points moved by `init`, the result is T_icp @ init
    init = N.similarity(1.0, I.rotation((0, 1, 0), 1.0), np.array([0.02, 0.0, -0.02]))
    want = P.icp_to_mesh(TI.torch_moved(r['away'], init), r['vertices'], r['faces'], TI.REFINE_DIST, **ref)
    assert want['iterations'] == 2 and want['history'][-1][3] < want['history'][0][3] and want['history'][0][1] > 400
    got = refine_alignment(dev(r['away']), v, f, init=torch.from_numpy(init), **kw)
    assert_alignment(got, want, want['transform'] @ init)
    # the voxel fusion of the displaced cloud: its points as they are on the device
    vox = TI.cloud_of(r['away'], r['pred_ids'], r['segments']).voxelize(0.3)
    assert isinstance(vox, VoxelCloud) and 500 < len(vox) < len(r['away'])
    want = P.icp_to_mesh(vox.points.cpu().numpy(), r['vertices'], r['faces'], TI.REFINE_DIST, **ref)
    assert_alignment(refine_alignment(vox, v, f, **kw), want)
    # a PanopticMesh: the room's own mesh, displaced; `spacing` samples it, the ground truth is not sampled at all
    Di = np.linalg.inv(r['displacement'])
    moved = (r['vertices'].astype(np.float64) @ Di[:3, :3].T + Di[:3, 3]).astype(F)
    f32 = np.where((r['faces'] < 0) | (r['faces'] >= len(moved)), -1, r['faces']).astype(np.int32)
    mesh = PanopticMesh(dev(moved), dev(f32), dev(r['face_ids']), dev(r['vertex_ids']), torch.zeros(len(moved), 3, device=DEV),
                        torch.zeros(len(f32), dtype=torch.int64, device=DEV), [0, 1], r['segments'])
    own = N.sample_mesh(moved, f32, TI.GT_SPACING, face_ids=r['face_ids'])
    want = P.icp_to_mesh(own['points'], r['vertices'], r['faces'], TI.REFINE_DIST, **ref)
    assert want['history'][-1][3] < 0.5 * want['history'][0][3]                  # the mesh's own surface: the fit closes in
    assert_alignment(refine_alignment(mesh, v, f, **kw), want)


def test_score_reconstruction_opts_into_the_surface_and_keeps_its_default(monkeypatch):
    r = TI.room()
    v, f, gt = dev(r['vertices']), dev(r['faces']), r['gt']['points']
    kw = dict(thresholds=TI.TAUS, spacing=TI.GT_SPACING)
    # the opt-in: the alignment is the restated plane loop's, and the scores are taken under its transform
    want_T = P.icp_to_mesh(r['away'], r['vertices'], r['faces'], 4 * max(TI.TAUS), iters=2, every=8)
    got = score_reconstruction(dev(r['away']), v, f, refine=SURFACE_KW, metric='surface', **kw)
    assert_alignment(got['alignment'], want_T)
    under = MD.scores(TI.torch_moved(r['away'], want_T['transform']), gt, r['vertices'], r['faces'], TI.TAUS)
    plain = score_reconstruction(dev(r['away']), v, f, metric='surface', **kw)
    for k in ('fscore', 'precision', 'recall', 'pred_within', 'gt_within', 'n_pred', 'n_gt'):
        assert got[k] == under[k], (k, got[k], under[k])
    assert got['pred_within'] != plain['pred_within'] and got['fscore'][0] > plain['fscore'][0] and set(got) - set(plain) == {'alignment'}
    # its keywords: 4 x the search radius, this call's max_cell_faces / max_pairs, no max_cell_points
    seen, real = [], score3d.refine_alignment

    def spy(pred, gv, gf, **k):
        seen.append(dict(k))
        return real(pred, gv, gf, **k)
    monkeypatch.setattr(score3d, 'refine_alignment', spy)
    again = score_reconstruction(dev(r['away']), v, f, refine=SURFACE_KW, metric='surface', max_cell_faces=3000, max_pairs=2 ** 20, max_cell_points=777, **kw)
    assert len(seen) == 1 and set(seen[0]) == {'spacing', 'init', 'max_subdiv', 'max_dist', 'max_cell_faces', 'max_pairs'} | set(SURFACE_KW)
    assert seen[0]['max_dist'] == TI.REFINE_DIST and seen[0]['max_cell_faces'] == 3000 and seen[0]['max_pairs'] == 2 ** 20
    assert same(again['alignment'].transform, got['alignment'].transform) and again['pred_within'] == got['pred_within']
    # refine=True is what it was, under both metrics: the same keywords as ever reach refine_alignment, no `target`, and the call goes through `icp`,
    # never through `icp_to_mesh` (the call is cut to the steps restated for tests/test_hip_icp.py once its keywords are seen)
    seen.clear()

    def cut(pred, gv, gf, **k):
        seen.append(dict(k))
        return real(pred, gv, gf, **dict(k, iters=TI.REFINE_ITERS))

    def never(*a, **k):
        raise AssertionError('refine=True reached icp_to_mesh')
    monkeypatch.setattr(score3d, 'refine_alignment', cut)
    monkeypatch.setattr(meshdist, 'icp_to_mesh', never)
    old_T = I.icp(r['away'], gt, 4 * max(TI.TAUS), iters=TI.REFINE_ITERS)
    for metric in ('points', 'surface'):
        full = score_reconstruction(dev(r['away']), v, f, refine=True, max_cell_points=777, metric=metric, **kw)
        TI.assert_alignment(full['alignment'], old_T)                            # history keys and all: f11's Alignment, byte for byte
    monkeypatch.undo()
    assert len(seen) == 2 and all(set(k) == {'spacing', 'init', 'max_subdiv', 'max_dist', 'max_cell_points'} and k['max_cell_points'] == 777 for k in seen)
