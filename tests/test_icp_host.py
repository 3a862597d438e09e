"""The host side of the ICP refinement (panst3r_amd.engine.icp / refine_alignment) and the properties of its contract, on the numpy restatement of
tests/icp_ref.py alone (no GPU here): the fixed-order sum against an exact one, the restated loop on the scenes the GPU test compares (a known
similarity recovered, with outliers too), the degenerate case, validation, the ABI."""
import math

import numpy as np
import pytest
import torch

import abi_header
import icp_ref as I
from panst3r_amd import hip
from panst3r_amd.engine import icp, refine_alignment, score_reconstruction, Alignment
from panst3r_amd.engine import score3d

F = np.float32


@pytest.mark.parametrize('n', [1, 257, 4096, 3 * 4096 + 17, 256 * 4096 + 1])
def test_the_fixed_order_sum_is_a_sum(n):
    """any order of n additions is within n 2^-52 sum |v| of the exact sum (n - 1 roundings of partial sums that never exceed sum |v|, each at most
    2^-53 of it, and one more for fsum's own)"""
    rng = np.random.default_rng(n)
    v = rng.normal(size=n) * 10.0 ** rng.integers(-6, 7, n)
    got, partials = I.fixed_sum(v)
    assert partials.shape == ((n + hip.ICP_CHUNK - 1) // hip.ICP_CHUNK,)
    assert abs(got - math.fsum(v.tolist())) <= n * 2.0 ** -52 * math.fsum(np.abs(v).tolist())
    # the partial of every block is the fixed-order sum of its rows, and rows of +0.0 after the end add nothing
    b = len(partials) - 1
    assert partials[b] == I.fixed_sum(v[b * hip.ICP_CHUNK:])[0]
    if (n + 5 + hip.ICP_CHUNK - 1) // hip.ICP_CHUNK == len(partials):
        assert I.fixed_sum(np.concatenate([v, np.zeros(5)]))[0] == got


def test_the_moments_are_those_of_the_matched_pairs():
    rng = np.random.default_rng(1)
    T = rng.uniform(-1, 1, (300, 3)).astype(F)
    A = np.array([[1, 0.25, 0, 0.5], [-0.25, 1, 0.125, -1], [0, -0.125, 1, 2]], dtype=F)
    X = ((rng.uniform(-1.2, 1.2, (700, 3)) - A[:, 3]) @ np.linalg.inv(A[:, :3].astype(np.float64)).T).astype(F)      # A carries them into the targets' box
    X[5] = [np.nan, 0, 0]
    X[7] = [-0.5, 1.0, -2.0]                                                     # moved exactly onto ...
    assert (I.move(X[7:8], A)[0] == [0.25, -0.125, -0.125]).all()
    T[9] = [0.25, -0.125, -0.125]
    s = I.step(X, A, T, 0.25, F(0.2) * F(0.2))
    hit = s['row'] >= 0
    assert 50 < hit.sum() < 650 and s['bad'] == 1 and s['row'][5] == -1 and s['row'][7] == 9 and s['d2'][7] == 0
    assert (s['d2'][hit] <= F(0.2) * F(0.2)).all() and np.isinf(s['d2'][~hit]).all()
    x, y = X[hit].astype(np.float64), T[s['row'][hit]].astype(np.float64)
    want = np.concatenate([[hit.sum()], x.sum(0), y.sum(0), (y.T @ x).ravel(), [(x * x).sum()], [s['d2'][hit].astype(np.float64).sum()], [0, 0]])
    assert s['out'].shape == (hip.ICP_MOMENTS,) == want.shape and s['out'][0] == hit.sum() and (s['out'][18:] == 0).all()
    assert np.allclose(s['out'], want, rtol=1e-12, atol=1e-12)
    # x is the ORIGINAL point: under another matrix with the same matches the moments of x stay what they are
    wide = I.match(I.move(X, A), T, 0.25, F(0.25) * F(0.25))
    assert (wide['row'] >= 0).sum() > hit.sum() and (wide['row'][hit] == s['row'][hit]).all()      # a smaller r2 only drops pairs


@pytest.mark.parametrize('outliers', [False, True])
def test_the_restated_loop_recovers_a_known_similarity(outliers):
    """fp32 coordinates round at 6e-8 relative and the solve is float64 over a thousand exact pairs: if the restatement misses 1e-5 of the extent, the
    scene is wrong, not the bound (`check_loop` asserts the conditions: convergence, the true pairs, outliers matched at first and shed at the end)"""
    res = I.check_loop(outliers)
    s = I.loop_scene(outliers)
    T, truth = res['transform'], s['truth']
    scale = np.cbrt(np.linalg.det(T[:3, :3]))
    assert abs(scale - 1.03) < 1e-6 and np.allclose(T[:3, :3] / scale, truth[:3, :3] / 1.03, atol=1e-6) and np.allclose(T[3], [0, 0, 0, 1])
    assert res['history'][-1][2] < 1e-6 < res['history'][0][2]                   # the residual of the last matches is fp32 rounding
    assert len(res['transforms']) == res['iterations'] == len(res['history'])
    rigid = I.loop_reference(outliers, with_scale=False)                         # without the scale the fit cannot close: det 1, a residual stays
    assert abs(np.linalg.det(rigid['transform'][:3, :3]) - 1) < 1e-12 and rigid['history'][-1][2] > 1e-3


def test_collinear_sources_are_degenerate_and_an_empty_first_step_raises():
    s = I.loop_scene()
    Y = s['target']
    line = np.stack([np.linspace(0.2, 2.5, 40), np.full(40, 0.01), np.full(40, 1.0)], 1).astype(F)      # a line just above the floor
    res = I.icp(line, Y, I.MAX_DIST)
    assert res['reason'] == 'degenerate' and not res['converged'] and res['iterations'] == 1 and res['history'][0][1] == 40
    assert (res['transform'] == np.eye(4)).all() and res['transforms'] == []     # the transform of the step before: the start
    with pytest.raises(ValueError, match='nothing within max_dist'):
        I.icp(line + F(50), Y, I.MAX_DIST)
    with pytest.raises(ValueError, match='nothing within max_dist'):             # two pairs at the first step raise as well
        I.icp(np.concatenate([line[:2], line[:3] + F(50)]), Y, I.MAX_DIST)


def test_the_radius_schedule_shrinks_to_its_floor_and_stays():
    rs = [I.radius_of(k, 0.32, 0.04, 0.85) for k in range(20)]
    assert rs[0][0] == F(0.32) and rs[0][1] == F(0.32) * F(0.32) and not rs[0][2]
    assert all(a[0] >= b[0] for a, b in zip(rs, rs[1:])) and rs[-1][0] == F(0.04) and rs[-1][2] and [r[2] for r in rs] == sorted(r[2] for r in rs)
    assert all(r[1] <= rs[0][1] for r in rs)                                     # never above the cell's
    for k in range(20):
        mine = score3d._icp_radius(k, float(F(0.32)), float(F(0.04)), 0.85)
        assert mine[0] == rs[k][0] and mine[1] == rs[k][1] and mine[2] == rs[k][2]
    assert I.radius_of(7, 0.32, None, 0.8) == (F(0.32), F(0.32) * F(0.32), True) == score3d._icp_radius(7, float(F(0.32)), None, 0.8)


def test_arguments_are_checked_before_the_gpu_is_touched():
    x, y = torch.zeros(10, 3), torch.zeros(12, 3)
    for bad in (0, -1.0, float('nan'), float('inf'), 1e-30, True, 'x', None):
        with pytest.raises(ValueError):
            icp(x, y, max_dist=bad)
    for kw in (dict(min_dist=0), dict(min_dist=0.2), dict(min_dist='x'), dict(shrink=0), dict(shrink=1), dict(shrink=1.5), dict(shrink=True),
               dict(tol=-1), dict(tol=float('nan')), dict(tol=None), dict(iters=0), dict(iters=2.5), dict(iters=True), dict(every=0), dict(every=1.0),
               dict(max_cell_points=0), dict(init=np.eye(3)), dict(init=np.full((4, 4), np.nan))):
        with pytest.raises(ValueError):
            icp(x, y, max_dist=0.1, **kw)
    with pytest.raises(ValueError):
        icp(torch.zeros(10, 2), y, max_dist=0.1)
    with pytest.raises(ValueError):
        icp(x, y.int(), max_dist=0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                   # valid arguments on the host: there is no CPU path
        icp(x, y, max_dist=0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        icp(x, y, max_dist=0.1, min_dist=0.05, shrink=0.5, tol=0, iters=3, every=2, init=torch.eye(4), with_scale=False)
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for kw in (dict(spacing=0, max_dist=0.1), dict(spacing=0.05, max_dist=-1), dict(spacing=0.05, max_dist=0.1, init=np.eye(3)),
               dict(spacing=0.05, max_dist=0.1, max_subdiv=0)):
        with pytest.raises(ValueError):
            refine_alignment(x, v, f, **kw)
    with pytest.raises(ValueError):
        refine_alignment([1, 2], v, f, spacing=0.05, max_dist=0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        refine_alignment(x, v, f, spacing=0.05, max_dist=0.1)
    for bad in ('yes', 1, [1]):
        with pytest.raises(ValueError, match='refine'):
            score_reconstruction(x, v, f, thresholds=[0.1], spacing=0.05, refine=bad)
    with pytest.raises(ValueError):                                              # the keywords reach refine_alignment and icp
        score_reconstruction(x, v, f, thresholds=[0.1], spacing=0.05, refine={'iters': 0})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        score_reconstruction(x, v, f, thresholds=[0.1], spacing=0.05, refine=True)
    a = Alignment(torch.eye(4, dtype=torch.float64), 2, True, 'converged', [{'radius': 0.1, 'matched': 5, 'rmse': 0.01}] * 2)
    assert a.iterations == 2 and a.converged and 'converged' in repr(a)


def test_the_abi_stays_20_and_the_constants_agree():
    defines = abi_header.defines()
    assert hip.ABI_VERSION == 20 == defines['PST_ABI_VERSION']
    assert (hip.ICP_CHUNK, hip.ICP_LANES, hip.ICP_MOMENTS) == (defines['PST_ICP_CHUNK'], defines['PST_ICP_LANES'], defines['PST_ICP_MOMENTS']) == (4096, 256, 20)
    assert (I.ICP_CHUNK, I.ICP_LANES, I.ICP_MOMENTS, I.LIVE + 2) == (hip.ICP_CHUNK, hip.ICP_LANES, hip.ICP_MOMENTS, hip.ICP_MOMENTS)
    assert I.PLANE_RANK_TOL == score3d.PLANE_RANK_TOL
    protos = {p[0]: p for p in abi_header.prototypes()}
    new = {'pst_icp_chunk', 'pst_icp_step'}
    assert {n for n in protos if n.startswith('pst_icp_')} == new <= set(hip.SIGNATURES)
    code = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for name in new:
        _, ret, params = protos[name]
        assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
    assert protos['pst_icp_step'][2].count('float') == 14                       # the matrix by value, inv and r2


def test_the_restated_host_step_is_the_products():
    """icp_ref.procrustes restates pointmaps.procrustes_from_moments operation for operation: equal bits, with and without the scale"""
    from panst3r_amd.engine.pointmaps import procrustes_from_moments
    s = I.loop_scene()
    mom = I.step(s['source'], np.eye(4)[:3], s['target'], I.MAX_DIST, F(I.MAX_DIST) * F(I.MAX_DIST))['out']
    R, t, sc = procrustes_from_moments(mom[0], mom[1:4], mom[4:7], mom[7:16].reshape(3, 3), mom[16])
    T = I.procrustes(mom, True)
    assert (T[:3, :3] == sc * R).all() and (T[:3, 3] == t).all()
    R, t = procrustes_from_moments(mom[0], mom[1:4], mom[4:7], mom[7:16].reshape(3, 3))
    T = I.procrustes(mom, False)
    assert (T[:3, :3] == R).all() and (T[:3, 3] == t).all()
    box = I.corners(s['source'])
    assert I.corner_shift(box, np.eye(4), T) == score3d._corner_shift(box, np.eye(4), T) > 0
