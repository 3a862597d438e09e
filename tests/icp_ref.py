"""numpy restatement of the fused ICP step (the icp section of include/panst3r_hip.h; csrc/nearest.hip) and of the loop around it
(panst3r_amd.engine.icp), the yardstick both are held to bit for bit.  The move is restated in fp32 as the contract writes it; the search is
`nearest_ref.nearest` - BRUTE FORCE over all pairs at the cell's radius, then the acceptance d2 <= r2 - and knows nothing of cells, so it checks the
cell logic of the kernel independently; the sums are restated in the fixed order of the contract, whose constants are read from panst3r_amd.hip
(plain Python numbers there).  numpy rounds every float operation on its own, as the contract asks.  Also the generated scenes that the host test and
the GPU test share."""
import functools

import numpy as np

import nearest_ref as N
from panst3r_amd.hip import ICP_CHUNK, ICP_LANES, ICP_MOMENTS

F32, F64 = np.float32, np.float64
LIVE = 18                                   # the moments that are sums; [18], [19] are +0.0
PLANE_RANK_TOL = 1e-6                       # engine/score3d.py's, restated


# ---------------------------------------------------------------- the step
def move(points, A):
    """m_r = ((a_r0 x0 + a_r1 x1) + a_r2 x2) + a_r3 in fp32"""
    X, A = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3), np.asarray(A, dtype=F32).reshape(3, 4)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.stack([((A[r, 0] * X[:, 0] + A[r, 1] * X[:, 1]) + A[r, 2] * X[:, 2]) + A[r, 3] for r in range(3)], 1)


def _block_sum(acc):
    """[..., 256] lane accumulators -> [...]: six butterfly steps inside every wave of 64, then ((w0 + w1) + w2) + w3"""
    a = acc.reshape(acc.shape[:-1] + (ICP_LANES // 64, 64))
    idx = np.arange(64)
    for k in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ k]
    assert (a == a[..., :1]).all()                                               # fp addition is commutative: all lanes agree
    w = a[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def fixed_sum(values):
    """the sum of values float64 [n] in the fixed order of the contract -> (the sum, the partial of every block [ceil(n / ICP_CHUNK)]); a skipped row
    is a +0.0 here (an accumulator that starts at +0.0 never holds -0.0, so adding +0.0 changes nothing)"""
    v = np.asarray(values, dtype=F64).reshape(-1)
    P, rows = (len(v) + ICP_CHUNK - 1) // ICP_CHUNK, ICP_CHUNK // ICP_LANES
    v = np.concatenate([v, np.zeros(P * ICP_CHUNK - len(v))]).reshape(P, rows, ICP_LANES)
    acc = np.zeros((P, ICP_LANES))
    for j in range(rows):
        acc = acc + v[:, j]
    partials = _block_sum(acc)
    R = (P + ICP_LANES - 1) // ICP_LANES
    p = np.concatenate([partials, np.zeros(R * ICP_LANES - P)]).reshape(R, ICP_LANES)
    acc = np.zeros(ICP_LANES)
    for r in range(R):
        acc = acc + p[r]
    return _block_sum(acc), partials


def terms(source, targets, d2, row):
    """the 18 summands of every source, float64 [18, n]; zeros where it is unmatched"""
    X, T = np.ascontiguousarray(source, dtype=F32).reshape(-1, 3), np.ascontiguousarray(targets, dtype=F32).reshape(-1, 3)
    hit = row >= 0
    x = np.where(hit[:, None], X, F32(0)).astype(F64)
    y = np.where(hit[:, None], T[np.maximum(row, 0)], F32(0)).astype(F64)
    t = np.zeros((LIVE, len(X)))
    t[0] = hit
    t[1:4], t[4:7] = x.T, y.T
    for r in range(3):
        for a in range(3):
            t[7 + 3 * r + a] = y[:, r] * x[:, a]                                 # exact: two widened fp32 values
    t[16] = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    t[17] = np.where(hit, d2, F32(0)).astype(F64)
    return t


def moments(source, targets, d2, row):
    """-> (out float64 [20], partials float64 [P, 20])"""
    t = terms(source, targets, d2, row)
    P = (t.shape[1] + ICP_CHUNK - 1) // ICP_CHUNK
    out, partials = np.zeros(ICP_MOMENTS), np.zeros((P, ICP_MOMENTS))
    for s in range(LIVE):
        out[s], partials[:, s] = fixed_sum(t[s])
    return out, partials


def match(moved, targets, cell_radius, r2):
    """the search of the moved points: all pairs at the cell's radius, then accepted iff d2 <= r2 (r2 <= float32(cell_radius)^2)"""
    assert F32(r2) <= N.radius_numbers(cell_radius)[2]
    res = N.nearest(moved, targets, cell_radius)
    ok = (res['row'] >= 0) & (res['d2'] <= F32(r2))
    return dict(d2=np.where(ok, res['d2'], F32(np.inf)).astype(F32), row=np.where(ok, res['row'], -1).astype(np.int32), bad=res['bad_queries'],
                second=res['second'], wide_row=res['row'])


def step(source, A, targets, cell_radius, r2):
    """one step -> dict: out [20], partials [P, 20], d2 fp32 [n], row int32 [n], bad (non-finite moved points), moved fp32 [n, 3], second"""
    moved = move(source, A)
    m = match(moved, targets, cell_radius, r2)
    out, partials = moments(source, targets, m['d2'], m['row'])
    return dict(out=out, partials=partials, moved=moved, **m)


# ---------------------------------------------------------------- the loop
def procrustes(mom, with_scale):
    """the host step on the 17 moments, the operations of pointmaps.procrustes_from_moments in their order -> [4, 4] with the scale folded in"""
    sw, sx, sy, syx, sxx = mom[0], mom[1:4], mom[4:7], mom[7:16].reshape(3, 3), mom[16]
    xm, ym = sx / sw, sy / sw
    M = syx - sw * np.outer(ym, xm)
    U, S, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    T = np.eye(4)
    if with_scale:
        s = float((S * np.diag(D)).sum() / (sxx - sw * (xm @ xm)))
        T[:3, :3], T[:3, 3] = s * R, ym - s * (R @ xm)
    else:
        T[:3, :3], T[:3, 3] = R, ym - R @ xm
    return T


def radius_of(k, max_dist, min_dist, shrink):
    """(r_k as float32, its fp32 square, at the floor); max_dist and min_dist are their float32 values"""
    md, mn = float(F32(max_dist)), None if min_dist is None else float(F32(min_dist))
    r = F32(md if mn is None else max(mn, md * float(shrink) ** k))
    return r, r * r, mn is None or md * float(shrink) ** k <= mn


def corners(points):
    P = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    lo, hi = P.min(0).astype(F64), P.max(0).astype(F64)
    return np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])


def corner_shift(box, T0, T1):
    a, b = box @ T0[:3, :3].T + T0[:3, 3], box @ T1[:3, :3].T + T1[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1)).max())


def icp(source, target, max_dist, init=None, with_scale=True, iters=50, min_dist=None, shrink=0.8, tol=1e-4, every=1):
    """the loop of panst3r_amd.engine.icp -> dict: transform [4, 4], iterations, converged, reason, history [(radius, matched, rmse)], transforms (the
    T after every iteration), last (the last step's dict: its matches)"""
    X = np.ascontiguousarray(source, dtype=F32).reshape(-1, 3)[::every]
    Y = np.ascontiguousarray(target, dtype=F32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, dtype=F64).copy()
    box = corners(X)
    history, transforms, reason, last = [], [], 'iters', None
    for k in range(iters):
        r, r2, floor = radius_of(k, max_dist, min_dist, shrink)
        last = step(X, T[:3].astype(F32), Y, max_dist, r2)
        mom = last['out']
        n = int(mom[0])
        history.append((float(r), n, float(np.sqrt(mom[17] / mom[0])) if n else float('nan')))
        if n < 3:
            if k == 0:
                raise ValueError('nothing within max_dist of the initial alignment')
            reason = 'degenerate'
            break
        xm, ym = mom[1:4] / mom[0], mom[4:7] / mom[0]
        s = np.linalg.svd(mom[7:16].reshape(3, 3) - mom[0] * np.outer(ym, xm), compute_uv=False)
        if s[1] <= PLANE_RANK_TOL * s[0]:
            reason = 'degenerate'
            break
        new = procrustes(mom, with_scale)
        shift = corner_shift(box, T, new)
        T = new
        transforms.append(T)
        if floor and shift <= tol * float(r):
            reason = 'converged'
            break
    return dict(transform=T, iterations=len(history), converged=reason == 'converged', reason=reason, history=history, transforms=transforms, last=last)


# ---------------------------------------------------------------- the scenes
SPACING = 0.08
MAX_DIST = 0.32


def rotation(axis, deg):
    a = np.asarray(axis, dtype=F64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


@functools.lru_cache(maxsize=None)
def loop_scene(outliers=False):
    """An asymmetric corner of a room as targets - a floor of 3 x 2, walls of 3 x 1.5 and 2 x 1.1, a box and a ramp, as jittered lattices `SPACING` apart
    (no two targets closer than 0.3 spacings) - and as sources 55 % of them under the INVERSE of a known similarity (4 degrees about a skew axis, scale
    1.03, a shift of half a spacing), rounded to fp32: `pair[i]` is the target row source i came from.  With `outliers`, a tenth more sources between
    1.4 and 3.5 spacings off every surface, inside the room (pair -1)."""
    rng = np.random.default_rng(21)
    h = SPACING

    def patch(origin, du, dv, nu, nv):
        i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
        uv = np.stack([i.ravel(), j.ravel()], 1) + 0.5 + rng.uniform(-0.35, 0.35, (nu * nv, 2))
        return np.asarray(origin) + h * uv[:, :1] * np.asarray(du, dtype=F64) + h * uv[:, 1:] * np.asarray(dv, dtype=F64)
    s = np.sqrt(0.5)
    Y = np.concatenate([patch((0, 0, 0), (1, 0, 0), (0, 0, 1), 37, 25), patch((0, 0, 0), (1, 0, 0), (0, 1, 0), 37, 18), patch((0, 0, 0), (0, 0, 1), (0, 1, 0), 25, 13),
                        patch((0.6, 0.5, 0.4), (1, 0, 0), (0, 0, 1), 10, 7), patch((1.8, 0, 0.9), (1, 0, 0), (0, s, s), 12, 11)]).astype(F32)
    truth = N.similarity(1.03, rotation((1, 2, -0.5), 4.0), np.array([0.5 * h, -0.3 * h, 0.4 * h]))
    inv = np.linalg.inv(truth)
    pair = np.flatnonzero(rng.random(len(Y)) < 0.55)
    X = (Y[pair].astype(F64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    if outliers:
        k = len(pair) // 10
        base = Y[rng.choice(len(Y), 3 * k)].astype(F64) + rng.uniform(1.5, 3.5, (3 * k, 1)) * h * np.array([1.0, 1.0, 1.0]) / np.sqrt(3)
        base = base[np.sqrt(((base[:, None] - Y[None].astype(F64)) ** 2).sum(2).min(1)) >= 1.4 * h][:k]      # off EVERY surface, the box and the ramp too
        assert len(base) == k
        X = np.concatenate([X, (base @ inv[:3, :3].T + inv[:3, 3]).astype(F32)])
        pair = np.concatenate([pair, np.full(k, -1)])
        order = rng.permutation(len(X))
        X, pair = X[order], pair[order]
    extent = float(np.linalg.norm(Y.max(0) - Y.min(0)))
    return dict(source=np.ascontiguousarray(X), target=np.ascontiguousarray(Y), pair=pair, truth=truth, extent=extent)


LOOP_KW = {False: dict(max_dist=MAX_DIST), True: dict(max_dist=MAX_DIST, min_dist=0.5 * SPACING, shrink=0.85)}


@functools.lru_cache(maxsize=None)
def loop_reference(outliers=False, with_scale=True, every=1, init=False):
    s = loop_scene(outliers)
    kw = dict(LOOP_KW[outliers], with_scale=with_scale, every=every)
    if init:
        kw['init'] = loop_init()
    return icp(s['source'], s['target'], **kw)


def loop_init():
    """a start that is not the identity: a degree about z and a shift of a quarter spacing"""
    return N.similarity(1.0, rotation((0, 0, 1), 1.0), np.array([0.25 * SPACING, 0.0, 0.0]))


def check_loop(outliers, res=None):
    """the scene holds what it was built for, asserted on the restated loop: it converges, the final matches are the true pairs (every inlier matched
    to the target it came from, every outlier unmatched) and T lies within 1e-5 of the scene's extent of the truth at every corner of the scene"""
    s = loop_scene(outliers)
    res = loop_reference(outliers) if res is None else res
    assert res['converged'] and res['reason'] == 'converged' and 3 <= res['iterations'] < 50
    assert 1500 < len(s['target']) < 4000 and len(set(s['pair'][s['pair'] >= 0].tolist())) == (s['pair'] >= 0).sum() < len(s['target'])      # a strict subset
    assert (res['last']['row'] == s['pair']).all()
    if outliers:
        assert (s['pair'] < 0).sum() >= len(s['pair']) // 11 and res['history'][0][1] > (s['pair'] >= 0).sum() * 0.5
        first = step(s['source'], np.eye(4)[:3], s['target'], MAX_DIST, F32(MAX_DIST) * F32(MAX_DIST))
        assert (first['row'][s['pair'] < 0] >= 0).sum() > (s['pair'] < 0).sum() // 2          # the outliers are matched at the first radius: the shrinking sheds them
        assert res['history'][-1][0] == float(F32(0.5 * SPACING)) < res['history'][0][0]
    box = corners(s['target'])
    assert corner_shift(box, res['transform'], s['truth']) <= 1e-5 * s['extent']
    return res
