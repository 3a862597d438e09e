"""The ICP refinement on the GPU (csrc/nearest.hip's icp_step, panst3r_amd.engine.icp / refine_alignment / score_reconstruction(refine=)) against
the numpy restatement of tests/icp_ref.py, BIT FOR BIT: the move is separately rounded fp32, the search is the one of the 3-D scores, the moments are
exact products added in an order the contract fixes, and the host step of the loop is the same numpy in the same process - there is no tolerance
to choose.

Conditions, not measurements: before the GPU is compared, every `check_*` asserts ON THE RESTATEMENT that the generated scene holds what it was built
for; the lists are in the docstrings of `step_scene` and of `icp_ref.loop_scene`."""
import functools

import numpy as np
import pytest
import torch

import grid_lists as G
import icp_ref as I
import mesh_ref as M
import nearest_ref as N
from panst3r_amd import hip
from panst3r_amd.engine import icp, refine_alignment, score_reconstruction, nearest_points, Alignment
from panst3r_amd.engine import PanopticCloud, PanopticMesh, VoxelCloud
from panst3r_amd.engine import score3d
from panst3r_amd.engine.score3d import NearestIndex

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
CHUNK = hip.ICP_CHUNK


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


# ---------------------------------------------------------------- the step
CELL = 0.25
R2 = F(0.2) * F(0.2)                                                             # below the cell's 0.0625
A = np.array([[1, 0.25, 0, 0.5], [-0.25, 1, 0.125, -1], [0, -0.125, 1, 2]], dtype=F)      # a shear, a rotation's off-diagonal signs and a shift; dyadic entries
SIZES = (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
TIE, NAN, INF, FAR_BLOCK = 3, 5, 7, 2


@functools.lru_cache(maxsize=None)
def step_scene():
    """3 002 targets, 3 000 of them random in a box of 5^3 (20^3 cells), and 3 x 4096 + 17 sources that A carries into a slightly larger box, so that
    about half find a target within r = 0.2, below the cell's edge of 0.25.  Planted: source 0 a hair from a target; source `TIE` moved EXACTLY (dyadic
    numbers: no rounding in the move) to the midpoint of two targets 0.25 apart in different cells, the pair being the last two rows; sources `NAN`
    and `INF` not finite; every source of block `FAR_BLOCK` carried 100 units away (a row of zeros in the partials); source 4096, the one row of the
    last block when N = 4097, a hair from a target.  The prefixes of `SIZES` rows are the smaller cases."""
    rng = np.random.default_rng(17)
    T = rng.uniform(-2.5, 2.5, (3002, 3)).astype(F)
    n = SIZES[-1]
    moved = rng.uniform(-2.7, 2.7, (n, 3))
    moved[0], moved[CHUNK] = T[100].astype(np.float64) + 0.01, T[200].astype(np.float64) - 0.01
    moved[FAR_BLOCK * CHUNK:(FAR_BLOCK + 1) * CHUNK] += 100.0
    X = ((moved - A[:, 3]) @ np.linalg.inv(A[:, :3].astype(np.float64)).T).astype(F)
    X[TIE] = [8, 4, 2]                                                           # -> (9.5, 1.25, 3.5) without a rounding
    T[-2], T[-1] = [9.375, 1.25, 3.5], [9.625, 1.25, 3.5]
    X[NAN], X[INF] = [np.nan, 0, 0], [0, np.inf, 0]
    return np.ascontiguousarray(X), np.ascontiguousarray(T)


@functools.lru_cache(maxsize=None)
def step_reference(n):
    X, T = step_scene()
    return I.step(X[:n], A, T, CELL, R2)


def check_step_conditions():
    X, T = step_scene()
    want = step_reference(SIZES[-1])
    row, d2 = want['row'], want['d2']
    assert len(X) == 3 * CHUNK + 17 and len(T) % 64 and 0.2 <= (row >= 0).mean() <= 0.8
    assert R2 < N.radius_numbers(CELL)[2] and ((want['wide_row'] >= 0) & (row < 0)).sum() > 100      # pairs the cells see and the smaller r2 rejects
    assert (want['moved'][TIE] == F([9.5, 1.25, 3.5])).all() and row[TIE] == len(T) - 2 and want['second'][TIE] == d2[TIE] == F(0.125) * F(0.125)
    ct, _, _ = N.cells(T, CELL)
    assert (ct[-2] != ct[-1]).any()
    assert want['bad'] == 2 and row[NAN] == -1 == row[INF] and np.isinf(d2[NAN]) and not np.isfinite(want['moved'][[NAN, INF]]).all(1).any()
    assert row[0] == 100 and row[CHUNK] == 200
    P = want['partials']
    assert P.shape == (4, 20) and (P[FAR_BLOCK] == 0).all() and (row[FAR_BLOCK * CHUNK:(FAR_BLOCK + 1) * CHUNK] == -1).all()
    assert all(P[b, 0] > 100 for b in (0, 1)) and 1 <= P[3, 0] <= 17 and want['out'][0] == (row >= 0).sum() and (want['out'][18:] == 0).all()
    # the contract's precondition holds: every accepted pair lies in neighbouring cells, so the 27 cells see what all pairs see
    cm, _, _ = N.cells(want['moved'], CELL)
    hit = want['wide_row'] >= 0
    assert (np.abs(ct[want['wide_row'][hit]] - cm[hit]).max(1) <= 1).all()
    one = step_reference(CHUNK + 1)
    assert one['partials'].shape == (2, 20) and one['partials'][1, 0] == 1 and one['row'][CHUNK] == 200          # a last block of one row, matched
    return want


def run_step(index, x, n, r2=R2, outputs=True, matrix=A):
    iws = hip.icp_workspace(n, DEV)
    iws['partials'].fill_(-7.0); iws['out'].fill_(-7.0)
    d2, row = (torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)) if outputs else (None, None)
    out = hip.icp_step(x, matrix, index.targets, index.inv, index.r2, float(r2), index.ws, index.max_cell_points, iws, d2, row)
    assert out is iws['out']
    return iws, d2, row


@pytest.mark.parametrize('n', SIZES)
def test_one_step_equals_the_restatement(n):
    check_step_conditions()
    X, T = step_scene()
    want = step_reference(n)
    index = NearestIndex(dev(T), CELL)
    x = dev(X[:n])
    iws, d2, row = run_step(index, x, n)
    assert same(iws['out'], want['out']), (iws['out'].cpu().numpy() - want['out'])
    assert same(iws['partials'], want['partials'])
    assert same(d2, want['d2']) and same(row, want['row'])
    assert iws['status'].tolist() == [0, 0, 0, want['bad']] and index.check() == 0      # (the index's own status words are not the step's)
    # the same pairs through the public search on the restated moved points, accepted at the smaller r2
    nd2, nrow = nearest_points(dev(want['moved']), dev(T), CELL)
    ok = (nrow >= 0) & (nd2 <= float(R2))
    assert same(torch.where(ok, nd2, torch.full_like(nd2, float('inf'))), d2) and same(torch.where(ok, nrow, torch.full_like(nrow, -1)), row)
    # without d2 / row the same moments; and again: equal bytes
    quiet, none_d2, none_row = run_step(index, x, n, outputs=False)
    assert none_d2 is None and none_row is None and same(quiet['out'], iws['out']) and same(quiet['partials'], iws['partials'])
    again, d2b, rowb = run_step(index, x, n)
    assert same(again['out'], iws['out']) and same(again['partials'], iws['partials']) and same(d2b, d2) and same(rowb, row)
    if n == SIZES[-1]:                                                           # at the cell's own r2 the step accepts what nn_query accepts
        wide = I.step(X, A, T, CELL, N.radius_numbers(CELL)[2])
        iws, d2, row = run_step(index, x, n, r2=index.r2)
        assert same(iws['out'], wide['out']) and same(row, wide['row']) and same(row, nrow) and wide['out'][0] > want['out'][0]
        with pytest.raises(ValueError, match='exceeds'):                         # the wrapper refuses a radius beyond the cells
            run_step(index, x, n, r2=float(np.nextafter(F(index.r2), F(1))))


def test_a_million_sources_take_the_reducer_round_its_loop_twice():
    """N = 256 x 4096 + 1: 257 rows of partials, so lane 0 of the reducer adds two of them, and the last one holds a single source.  The sources
    are a 4 097-point set tiled: the restatement searches the distinct points once and tiles the result."""
    X, T = step_scene()
    base, n = X[:CHUNK + 1], 256 * CHUNK + 1
    rows = np.arange(n) % len(base)
    rows[-1] = 0                                                                 # the single source of the last block is the matched source 0
    m = I.match(I.move(base, A), T, CELL, R2)
    d2, row = m['d2'][rows], m['row'][rows]
    big = np.ascontiguousarray(base[rows])
    out, partials = I.moments(big, T, d2, row)
    assert partials.shape == (257, 20) and partials[256, 0] == 1 and row[n - 1] >= 0 and 0.2 * n < out[0] == (row >= 0).sum() < 0.8 * n
    assert (m['row'][[TIE, NAN, INF]] == [len(T) - 2, -1, -1]).all()
    index = NearestIndex(dev(T), CELL)
    iws, gd2, grow = run_step(index, dev(big), n)
    assert same(iws['out'], out) and same(iws['partials'], partials) and same(gd2, d2) and same(grow, row)
    bad = int((~np.isfinite(I.move(base, A)).all(1))[rows].sum())
    assert bad == 2 * 256 and iws['status'].tolist() == [0, 0, 0, bad]          # NaN and inf once per copy of the set


def test_every_refusal_of_the_launcher_leaves_the_outputs_untouched():
    X, T = step_scene()
    n = 300
    index = NearestIndex(dev(T), CELL)
    x, ws = dev(X[:n]), index.ws
    iws = hip.icp_workspace(n, DEV)
    d2, row = torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    iws['partials'].fill_(-7.0); iws['out'].fill_(-7.0); iws['status'].fill_(-7)
    p = lambda t: t.data_ptr()
    good = dict(source=p(x), N=n, targets=p(index.targets), M=len(T), inv=index.inv, r2=float(R2), keys=p(ws['keys']), cap=ws['cap'], start=p(ws['start']),
                cell_count=p(ws['cell_count']), rows=p(ws['rows']), mcp=4096, d2=p(d2), row=p(row), partials=p(iws['partials']), out=p(iws['out']),
                status=p(iws['status']))

    def call(**change):
        a = dict(good, **change)
        return hip.lib().pst_icp_step(a['source'], a['N'], *[float(v) for v in A.ravel()], a['targets'], a['M'], a['inv'], a['r2'], a['keys'], a['cap'],
                                      a['start'], a['cell_count'], a['rows'], a['mcp'], a['d2'], a['row'], a['partials'], a['out'], a['status'],
                                      torch.cuda.current_stream().cuda_stream)
    refusals = [dict(source=None), dict(targets=None), dict(keys=None), dict(start=None), dict(cell_count=None), dict(rows=None), dict(partials=None),
                dict(out=None), dict(status=None), dict(N=0), dict(N=-5), dict(N=2 ** 30 + 1), dict(d2=None), dict(row=None), dict(M=0),
                dict(cap=ws['cap'] - 1), dict(inv=0.0), dict(inv=float('inf')), dict(r2=-1.0), dict(r2=float('nan')), dict(r2=float('inf')), dict(mcp=0)]
    for change in refusals:
        assert call(**change) < 0, change
        assert b'icp_step' in hip.lib().pst_last_error() or b'capacity' in hip.lib().pst_last_error(), change
    torch.cuda.synchronize()
    assert (d2 == -7).all() and (row == -7).all() and (iws['partials'] == -7).all() and (iws['out'] == -7).all() and (iws['status'] == -7).all()
    iws['status'].zero_()
    assert call() == 0 and call(d2=None, row=None) == 0                          # ... and the good call runs, with and without d2 / row
    assert same(iws['out'], step_reference(n)['out']) and same(row, step_reference(n)['row'])
    assert hip.lib().pst_icp_chunk() == CHUNK
    with pytest.raises(ValueError, match='go together'):
        hip.icp_step(x, A, index.targets, index.inv, index.r2, float(R2), ws, 4096, iws, d2, None)
    with pytest.raises(ValueError, match='3 x 4'):
        hip.icp_step(x, np.eye(4), index.targets, index.inv, index.r2, float(R2), ws, 4096, iws)


def test_the_step_refuses_a_list_that_leaves_the_rows_and_a_row_past_the_targets():
    """the search of the step is the query's: the same tampered lists (tests/grid_lists.py), refused through the STEP's status words"""
    touched, untouched = G.check_lattice()
    X, T = G.lattice()
    x, t = G.padded(X), G.padded(T)
    _, inv, r2 = (float(v) for v in N.radius_numbers(G.CELL))
    still = np.eye(3, 4, dtype=F)                                                # moves nothing: x 1 + y 0 + z 0 + 0 is x
    good = G.nn_build(t)

    def step(ws):
        iws = hip.icp_workspace(len(X), DEV)
        d2, row = torch.full((len(X),), -7.0, device=DEV), torch.full((len(X),), -7, dtype=torch.int32, device=DEV)
        hip.icp_step(x, still, t, inv, r2, r2, ws, 4096, iws, d2, row)
        assert ws['status'].tolist() == [0, 0, 0, 0]                             # the index's own status words are not the step's
        return iws, d2, row
    want = I.step(X, still, T, G.CELL, F(r2))
    assert (want['moved'] == X).all() and want['out'][0] == len(X)
    iws, d2, row = step(G.fresh(good))                                           # (d) the untampered workspace through the same helpers
    assert iws['status'].tolist() == [0, 0, 0, 0] and same(iws['out'], want['out']) and same(d2, want['d2']) and same(row, want['row'])
    slot, M = int(good['point_slot'][0]), len(T)
    for tamper in (lambda ws: G.move_list_out(ws, slot, M), lambda ws: G.first_entry_past_the_end(ws, slot, M)):      # (a), (b)
        ws = G.fresh(good)
        tamper(ws)
        bad, bd2, brow = step(ws)
        assert bad['status'].tolist() == [G.LISTS, 0, 0, 0]
        assert (bits(bd2)[untouched] == bits(d2)[untouched]).all() and (bits(brow)[untouched] == bits(row)[untouched]).all()
        assert bool(((brow >= -1) & (brow < M)).all()) and (bits(brow)[touched] != bits(row)[touched]).any()      # a target was lost, none past the end was taken


# ---------------------------------------------------------------- the loop
def assert_alignment(got, want, transform=None):
    assert isinstance(got, Alignment) and got.transform.dtype == torch.float64 and tuple(got.transform.shape) == (4, 4) and not got.transform.is_cuda
    assert (got.iterations, got.converged, got.reason) == (want['iterations'], want['converged'], want['reason'])
    assert len(got.history) == len(want['history'])
    for k, (g, w) in enumerate(zip(got.history, want['history'])):
        assert set(g) == {'radius', 'matched', 'rmse'} and g['matched'] == w[1] and same(np.float64([g['radius'], g['rmse']]), np.float64([w[0], w[2]])), (k, g, w)
    assert same(got.transform, want['transform'] if transform is None else transform)


VARIANTS = [dict(outliers=False), dict(outliers=True), dict(outliers=False, with_scale=False), dict(outliers=True, with_scale=False),
            dict(outliers=False, every=3), dict(outliers=True, every=3), dict(outliers=False, init=True), dict(outliers=True, init=True)]


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()))
def test_the_loop_equals_the_restated_loop(variant):
    outliers = variant['outliers']
    I.check_loop(outliers)                                                       # the scene recovers its similarity (tests/test_icp_host.py)
    want = I.loop_reference(**variant)
    assert want['iterations'] >= 5 and want['reason'] in ('converged', 'iters')
    s = I.loop_scene(outliers)
    kw = dict(I.LOOP_KW[outliers], **{k: v for k, v in variant.items() if k in ('with_scale', 'every')})
    if variant.get('init'):
        kw['init'] = torch.from_numpy(I.loop_init())
    x, y = dev(s['source']), dev(s['target'])
    assert_alignment(icp(x, y, **kw), want)
    # every T on the way: the loop is deterministic, so a run cut after k steps ends with the restated loop's k-th transform
    for k in (range(1, want['iterations']) if len(variant) == 1 else (1, 2)):
        cut = icp(x, y, iters=k, **kw)
        assert cut.reason == 'iters' and cut.iterations == k and not cut.converged and same(cut.transform, want['transforms'][k - 1]), k


def test_degenerate_and_empty_starts_on_the_device():
    s = I.loop_scene()
    y = dev(s['target'])
    line = np.stack([np.linspace(0.2, 2.5, 40), np.full(40, 0.01), np.full(40, 1.0)], 1).astype(F)
    want = I.icp(line, s['target'], I.MAX_DIST)
    assert want['reason'] == 'degenerate' and want['iterations'] == 1
    assert_alignment(icp(dev(line), y, max_dist=I.MAX_DIST), want)
    with pytest.raises(ValueError, match='nothing within max_dist'):
        icp(dev(line + F(50)), y, max_dist=I.MAX_DIST)
    with pytest.raises(ValueError, match='at least 3'):
        icp(dev(line[:2]), y, max_dist=I.MAX_DIST)


# ---------------------------------------------------------------- the composition: the room of the 3-D score tests
GT_SPACING, TAUS, REFINE_DIST, REFINE_ITERS = 0.7, (0.125, 0.25, 0.5), 2.0, 6


@functools.lru_cache(maxsize=None)
def room():
    """the generated room of the mesh tests as ground truth, and as prediction the noisy, partly missing copy of its own surface that
    tests/test_hip_score3d.py scores (samples at another spacing moved by up to 0.2 per axis, x > 2 cut away, a tenth of the labels exchanged), here
    DISPLACED by a rigid motion - 3 degrees about a skew axis and a shift of 0.15 - that no camera fit has seen: `away`"""
    s = M.scene()
    segs = [{'id': int(g['id']), 'category_id': int(g.get('category_id', g.get('class_id')))} for g in s['segments']]
    own = N.sample_mesh(s['vertices'], s['faces'], 0.6, vertex_ids=s['vertex_ids'])
    rng = np.random.default_rng(4)
    keep = own['points'][:, 0] <= 2
    pts = (own['points'][keep] + rng.uniform(-0.2, 0.2, (keep.sum(), 3)).astype(F)).astype(F)
    ids = own['ids'][keep].copy()
    swap = rng.random(len(ids)) < 0.1
    ids[swap] = np.roll(ids, 37)[swap]
    D = N.similarity(1.0, I.rotation((1, -1, 2), 3.0), np.array([0.1, -0.08, 0.08]))
    Di = np.linalg.inv(D)
    away = (pts.astype(np.float64) @ Di[:3, :3].T + Di[:3, 3]).astype(F)
    gt = N.sample_mesh(s['vertices'], s['faces'], GT_SPACING, vertex_ids=s['vertex_ids'])
    return dict(vertices=s['vertices'], faces=s['faces'], vertex_ids=s['vertex_ids'], face_ids=s['face_ids'], segments=segs, pred_points=pts, pred_ids=ids,
                away=away, displacement=D, gt=gt)


def cloud_of(points, ids, segments):
    n = len(points)
    p = dev(points)
    return PanopticCloud(p, p.clone(), torch.full((n, 3), 0.5, device=DEV), dev(ids), torch.full((n, 3), 0.5, device=DEV),
                         torch.arange(n, device=DEV), [0, n], [dict(s) for s in segments])


def torch_moved(points, T):
    """as score_reconstruction carries points: torch's matmul is not part of the contract"""
    B = dev(np.asarray(T), torch.float32)
    return (dev(points).float() @ B[:3, :3].T + B[:3, 3]).contiguous().cpu().numpy()


def test_refine_alignment_on_a_tensor_a_voxel_cloud_and_a_mesh():
    r = room()
    v, f, gt = dev(r['vertices']), dev(r['faces']), r['gt']['points']
    kw = dict(spacing=GT_SPACING, max_dist=REFINE_DIST, iters=REFINE_ITERS)
    # a tensor, from a start that is not the identity: icp runs from the identity on the points moved by `init`, the result is T_icp @ init
    init = N.similarity(1.0, I.rotation((0, 1, 0), 1.0), np.array([0.02, 0.0, -0.02]))
    want = I.icp(torch_moved(r['away'], init), gt, REFINE_DIST, iters=REFINE_ITERS)
    assert want['iterations'] == REFINE_ITERS and want['history'][-1][2] < want['history'][0][2] and want['history'][0][1] > 3000
    got = refine_alignment(dev(r['away']), v, f, init=torch.from_numpy(init), **kw)
    assert_alignment(got, want, want['transform'] @ init)
    # the voxel fusion of the displaced cloud: its points as they are on the device
    vox = cloud_of(r['away'], r['pred_ids'], r['segments']).voxelize(0.3)
    assert isinstance(vox, VoxelCloud) and 500 < len(vox) < len(r['away'])
    want = I.icp(vox.points.cpu().numpy(), gt, REFINE_DIST, iters=REFINE_ITERS)
    assert_alignment(refine_alignment(vox, v, f, **kw), want)
    # a PanopticMesh: the room's own mesh, displaced; it is sampled at the same spacing, with its face ids
    Di = np.linalg.inv(r['displacement'])
    moved = (r['vertices'].astype(np.float64) @ Di[:3, :3].T + Di[:3, 3]).astype(F)
    f32 = np.where((r['faces'] < 0) | (r['faces'] >= len(moved)), -1, r['faces']).astype(np.int32)
    mesh = PanopticMesh(dev(moved), dev(f32), dev(r['face_ids']), dev(r['vertex_ids']), torch.zeros(len(moved), 3, device=DEV),
                        torch.zeros(len(f32), dtype=torch.int64, device=DEV), [0, 1], r['segments'])
    own = N.sample_mesh(moved, f32, GT_SPACING, face_ids=r['face_ids'])
    want = I.icp(own['points'], gt, REFINE_DIST, iters=REFINE_ITERS)
    assert want['history'][-1][2] < 0.5 * want['history'][0][2]                  # the mesh's own surface: the fit closes in
    assert_alignment(refine_alignment(mesh, v, f, **kw), want)


def test_score_reconstruction_refines_before_it_scores(monkeypatch):
    r = room()
    v, f, gt = dev(r['vertices']), dev(r['faces']), r['gt']['points']
    kw = dict(thresholds=TAUS, spacing=GT_SPACING)
    want_T = I.icp(r['away'], gt, 4 * max(TAUS), iters=REFINE_ITERS)            # the default max_dist: 4 x the search radius
    assert 4 * max(TAUS) == REFINE_DIST
    unrefined, refined = N.scores(r['away'], gt, TAUS), N.scores(torch_moved(r['away'], want_T['transform']), gt, TAUS)
    assert refined['fscore'][0] > unrefined['fscore'][0] + 0.02 and refined['chamfer'] < unrefined['chamfer']      # the scene decides something
    plain = score_reconstruction(dev(r['away']), v, f, **kw)
    assert 'alignment' not in plain and plain['fscore'] == unrefined['fscore'] and plain['pred_within'] == unrefined['pred_within']
    got = score_reconstruction(dev(r['away']), v, f, refine={'iters': REFINE_ITERS}, **kw)
    assert_alignment(got['alignment'], want_T)
    for k in ('fscore', 'precision', 'recall', 'pred_within', 'gt_within', 'n_pred', 'n_gt'):
        assert got[k] == refined[k], (k, got[k], refined[k])
    assert got['fscore'][0] >= plain['fscore'][0]
    assert set(got) - set(plain) == {'alignment'}
    # refine=True: refine_alignment's own defaults, with 4 x the search radius as max_dist and this call's max_cell_points (the 50 steps of the default
    # would be 50 brute-force searches in the restatement: the call is cut to the steps restated above once its keywords are seen)
    seen, real = [], score3d.refine_alignment

    def cut(pred, gv, gf, **k):
        seen.append(dict(k))
        return real(pred, gv, gf, **dict(k, iters=REFINE_ITERS))
    monkeypatch.setattr(score3d, 'refine_alignment', cut)
    full = score_reconstruction(dev(r['away']), v, f, refine=True, max_cell_points=777, **kw)
    monkeypatch.undo()
    assert len(seen) == 1 and set(seen[0]) == {'spacing', 'init', 'max_subdiv', 'max_dist', 'max_cell_points'} and seen[0]['init'] is None
    assert seen[0]['max_dist'] == 4 * plain['max_dist'] == REFINE_DIST and seen[0]['max_cell_points'] == 777
    assert_alignment(full['alignment'], want_T)
    assert full['fscore'] == refined['fscore']
    start = N.similarity(1.0, np.eye(3), np.array([0.05, 0.0, 0.0]))
    got = score_reconstruction(dev(r['away']), v, f, transform=start, refine={'iters': 2}, **kw)
    want2 = I.icp(torch_moved(r['away'], start), gt, REFINE_DIST, iters=2)
    assert_alignment(got['alignment'], want2, want2['transform'] @ start)
