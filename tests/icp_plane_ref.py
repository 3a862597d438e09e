"""numpy restatement of the fused point-to-plane ICP step (the icp-plane section of include/panst3r_hip.h; csrc/meshdist.hip), of the host solve
(panst3r_amd.engine.pointmaps.plane_step_from_moments) and of the loop around them (panst3r_amd.engine.icp_to_mesh), the yardstick all three are held
to bit for bit.  The move is `icp_ref.move`; the search is `meshdist_ref.mesh_distance` - BRUTE FORCE over all kept faces at the cell's radius, then
the acceptance d2 <= r2 - and knows nothing of cells; the terms are restated operation by operation as the contract writes them; the sums are
`icp_ref.fixed_sum`.  The host solve and the loop are written out here on their own, not imported from the engine.  numpy rounds every float
operation on its own, as the contract asks.  Also the generated scenes that the host test and the GPU test share."""
import functools

import numpy as np

import icp_ref as I
import meshdist_ref as MD
import nearest_ref as N
from panst3r_amd.hip import ICP_CHUNK, ICP_PLANE_MOMENTS

F32, F64 = np.float32, np.float64
LIVE = 38                                   # the moments that are sums; [38], [39] are +0.0
PLANE_SYSTEM_TOL = 1e-6                     # engine/pointmaps.py's, restated


# ---------------------------------------------------------------- the step
def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def terms(moved, c0, vertices, faces, d2, face):
    """the 38 summands of every source, float64 [38, n]; zeros where it is unmatched"""
    M, V = np.ascontiguousarray(moved, dtype=F32).reshape(-1, 3), np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    Fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    hit = face >= 0
    idx = np.flatnonzero(hit)
    t = np.zeros((LIVE, len(M)))
    if not len(idx):
        return t
    tri = V[Fc[face[idx]]].astype(F64)                                           # [k, corner, axis], widened once
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    m, c0 = M[idx].astype(F64), np.asarray(c0, dtype=F32).astype(F64)
    with np.errstate(all='ignore'):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        w = 1.0 / ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        p, u = m - c0, m - a
        rN = _dot(n, u)
        J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2], _dot(n, p)], 0)                 # [7, k]
        t[0, idx] = 1.0
        s = 1
        for i in range(7):
            g = w * J[i]
            for j in range(i, 7):
                t[s, idx] = g * J[j]
                s += 1
            t[29 + i, idx] = g * rN
        assert s == 29
        t[36, idx] = (w * rN) * rN
        t[37, idx] = d2[idx].astype(F64)
    return t


def moments(t):
    """the 38 rows of summands -> (out float64 [40], partials float64 [P, 40]) in the fixed order of the icp section"""
    P = (t.shape[1] + ICP_CHUNK - 1) // ICP_CHUNK
    out, partials = np.zeros(ICP_PLANE_MOMENTS), np.zeros((P, ICP_PLANE_MOMENTS))
    with np.errstate(all='ignore'):
        for s in range(LIVE):
            out[s], partials[:, s] = I.fixed_sum(t[s])
    return out, partials


def match(moved, vertices, faces, cell_radius, r2):
    """the search of the moved points: every kept face at the cell's radius, then accepted iff d2 <= r2 (r2 <= float32(cell_radius)^2)"""
    assert F32(r2) <= N.radius_numbers(cell_radius)[2]
    res = MD.mesh_distance(moved, vertices, faces, cell_radius)
    ok = (res['face'] >= 0) & (res['d2'] <= F32(r2))
    return dict(d2=np.where(ok, res['d2'], F32(np.inf)).astype(F32), face=np.where(ok, res['face'], -1).astype(np.int32), bad=res['bad_queries'],
                second=res['second'], wide_face=res['face'], wide_d2=res['d2'], region=np.where(ok, res['region'], -1))


def step(source, A, c0, vertices, faces, cell_radius, r2):
    """one step -> dict: out [40], partials [P, 40], d2 fp32 [n], face int32 [n], bad (non-finite moved points), moved fp32 [n, 3], second, region"""
    moved = I.move(source, A)
    m = match(moved, vertices, faces, cell_radius, r2)
    out, partials = moments(terms(moved, c0, vertices, faces, m['d2'], m['face']))
    return dict(out=out, partials=partials, moved=moved, **m)


# ---------------------------------------------------------------- the host solve
def system(mom):
    """the symmetric 7 x 7 matrix sum w J J^T and the right-hand side sum w J rN of the moments"""
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = mom[1:29]
    return A + np.triu(A, 1).T, mom[29:36]


def scaled_eigenvalues(mom, length, with_scale=True):
    """the eigenvalues, ascending, of the system with its rotation and scale columns divided by `length`: what the degeneracy test compares"""
    n = 7 if with_scale else 6
    A, _ = system(mom)
    d = np.ones(7)
    d[[0, 1, 2, 6]] = 1.0 / float(length)
    return np.linalg.eigvalsh((A * np.outer(d, d))[:n, :n])


def plane_solve(mom, centre, length, with_scale=True):
    """the operations of pointmaps.plane_step_from_moments in their order -> the [4, 4] increment, or None"""
    n = 7 if with_scale else 6
    A, b = system(mom)
    d = np.ones(7)
    d[[0, 1, 2, 6]] = 1.0 / float(length)
    As, bs = (A * np.outer(d, d))[:n, :n], (b * d)[:n]
    if not (np.isfinite(As).all() and np.isfinite(bs).all()):
        return None
    ev = np.linalg.eigvalsh(As)
    if not (ev[-1] > 0 and ev[0] > PLANE_SYSTEM_TOL * ev[-1]):
        return None
    x = np.zeros(7)
    x[:n] = d[:n] * np.linalg.solve(As, -bs)
    omega, tau, sigma = x[:3], x[3:6], x[6]
    theta = float(np.sqrt(omega @ omega))
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    R = np.eye(3) if theta == 0 else np.eye(3) + (np.sin(theta) / theta) * K + ((1.0 - np.cos(theta)) / (theta * theta)) * (K @ K)
    M = (1.0 + sigma) * R
    c = np.asarray(centre, dtype=F64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = M, (c - M @ c) + tau
    return T


# ---------------------------------------------------------------- the loop
def icp_to_mesh(source, vertices, faces, max_dist, init=None, with_scale=True, iters=50, min_dist=None, shrink=0.8, tol=1e-4, every=1):
    """the loop of panst3r_amd.engine.icp_to_mesh -> dict: transform [4, 4], iterations, converged, reason, history [(radius, matched, rmse,
    plane_rmse)], transforms (the T after every solved step), ratios (smallest / largest eigenvalue of the scaled system per step with enough
    pairs), last (the last step's dict: its matches)"""
    X = np.ascontiguousarray(source, dtype=F32).reshape(-1, 3)[::every]
    T = np.eye(4) if init is None else np.asarray(init, dtype=F64).copy()
    lo, hi = X.min(0).astype(F64), X.max(0).astype(F64)
    box = I.corners(X)
    centre, half = 0.5 * (lo + hi), 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))
    unknowns = 7 if with_scale else 6
    history, transforms, ratios, reason, last = [], [], [], 'iters', None
    for k in range(iters):
        r, r2, floor = I.radius_of(k, max_dist, min_dist, shrink)
        c0 = (T[:3, :3] @ centre + T[:3, 3]).astype(F32)
        length = half * float(np.cbrt(abs(np.linalg.det(T[:3, :3]))))
        last = step(X, T[:3].astype(F32), c0, vertices, faces, max_dist, r2)
        mom = last['out']
        n = int(mom[0])
        history.append((float(r), n, float(np.sqrt(mom[37] / mom[0])) if n else float('nan'), float(np.sqrt(mom[36] / mom[0])) if n else float('nan')))
        if n == 0 and k == 0:
            raise ValueError('nothing within max_dist of the initial alignment')
        inc = None
        if n >= unknowns:
            ev = scaled_eigenvalues(mom, length, with_scale)
            ratios.append(float(ev[0] / ev[-1]))
            inc = plane_solve(mom, c0.astype(F64), length, with_scale)
        if inc is None:
            reason = 'degenerate'
            break
        new = inc @ T
        shift = I.corner_shift(box, T, new)
        T = new
        transforms.append(T)
        if floor and shift <= tol * float(r):
            reason = 'converged'
            break
    return dict(transform=T, iterations=len(history), converged=reason == 'converged', reason=reason, history=history, transforms=transforms,
                ratios=ratios, last=last)


# ---------------------------------------------------------------- the scenes
MAX_DIST = I.MAX_DIST                                                            # 0.32
SPACING = I.SPACING                                                              # the point-to-point comparison samples the mesh at 0.08
N_SOURCES = 3000
NOISE, OUT_LO, OUT_HI = 0.003, 0.10, 0.28
NOISY_KW = dict(max_dist=MAX_DIST, min_dist=0.04, shrink=0.8, iters=16)


def _patch(origin, du, dv, su, sv, nu, nv, first):
    """a planar patch of su x sv as nu x nv quads, two triangles each -> (vertices float64 [(nu+1)(nv+1), 3], faces [2 nu nv, 3] from vertex `first`)"""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    V = np.asarray(origin, dtype=F64) + (su / nu) * i.reshape(-1, 1) * np.asarray(du, dtype=F64) + (sv / nv) * j.reshape(-1, 1) * np.asarray(dv, dtype=F64)
    q = (i[:-1, :-1] * (nv + 1) + j[:-1, :-1]).reshape(-1) + first
    a, b, c, d = q, q + (nv + 1), q + 1, q + (nv + 1) + 1
    return V, np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)])


@functools.lru_cache(maxsize=None)
def room_mesh(floor_only=False):
    """the five planar patches of `icp_ref.loop_scene` as a triangle mesh, fp32 vertices: a floor of 3 x 2 in 6 x 4 quads, walls of 3 x 1.5 in 6 x 3 and
    of 2 x 1.1 in 4 x 2, a box top of 0.8 x 0.56 in 2 x 1 and a ramp of 0.96 x 0.88 in 2 x 2: 56 quads, 112 triangles -> (vertices, faces int32)"""
    s = np.sqrt(0.5)
    spec = [((0, 0, 0), (1, 0, 0), (0, 0, 1), 3.0, 2.0, 6, 4), ((0, 0, 0), (1, 0, 0), (0, 1, 0), 3.0, 1.5, 6, 3), ((0, 0, 0), (0, 0, 1), (0, 1, 0), 2.0, 1.1, 4, 2),
            ((0.6, 0.5, 0.4), (1, 0, 0), (0, 0, 1), 0.8, 0.56, 2, 1), ((1.8, 0, 0.9), (1, 0, 0), (0, s, s), 0.96, 0.88, 2, 2)]
    Vs, Fs, first = [], [], 0
    for p in spec[:1] if floor_only else spec:
        V, Fc = _patch(*p, first)
        Vs.append(V); Fs.append(Fc)
        first += len(V)
    return np.ascontiguousarray(np.concatenate(Vs).astype(F32)), np.ascontiguousarray(np.concatenate(Fs).astype(np.int32))


def truth():
    """loop_scene's similarity: 4 degrees about (1, 2, -0.5), scale 1.03, a shift of (0.04, -0.024, 0.032)"""
    return N.similarity(1.03, I.rotation((1, 2, -0.5), 4.0), np.array([0.5 * I.SPACING, -0.3 * I.SPACING, 0.4 * I.SPACING]))


def _on_faces(rng, V, Fc, n):
    """n points uniform on the surface (float64) and the unit normal of each one's face"""
    tri = V[Fc].astype(F64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.sqrt((nrm ** 2).sum(1))
    f = rng.choice(len(Fc), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    P = (1 - r1)[:, None] * tri[f, 0] + (r1 * (1 - r2))[:, None] * tri[f, 1] + (r1 * r2)[:, None] * tri[f, 2]
    return P, nrm[f] / np.sqrt((nrm[f] ** 2).sum(1))[:, None]


@functools.lru_cache(maxsize=None)
def room_scene(noisy=False, floor_only=False):
    """The room mesh and 3 000 sources drawn uniformly on its faces, carried by the INVERSE of `truth()` and rounded to fp32.  `noisy`: 3 mm of Gaussian
    noise on every coordinate, and a tenth more sources 0.10 to 0.28 off the face they were drawn on, none closer than 0.10 to ANY face (inlier True /
    False per source), in a random order.  `floor_only`: the floor alone, its sources on it - a single plane."""
    rng = np.random.default_rng(33 + noisy + 2 * floor_only)
    V, Fc = room_mesh(floor_only)
    P, _ = _on_faces(rng, V, Fc, N_SOURCES)
    inlier = np.ones(N_SOURCES, dtype=bool)
    if noisy:
        P = P + rng.normal(0.0, NOISE, P.shape)
        k = N_SOURCES // 10
        Q, nq = _on_faces(rng, V, Fc, 4 * k)
        Q = Q + rng.uniform(OUT_LO, OUT_HI, (4 * k, 1)) * nq * np.where(rng.random((4 * k, 1)) < 0.5, -1.0, 1.0)
        far = MD.mesh_distance(Q.astype(F32), V, Fc, OUT_LO)['face'] < 0       # nothing within 0.10
        Q = Q[far][:k]
        assert len(Q) == k
        P, inlier = np.concatenate([P, Q]), np.concatenate([inlier, np.zeros(k, dtype=bool)])
        order = rng.permutation(len(P))
        P, inlier = P[order], inlier[order]
    inv = np.linalg.inv(truth())
    X = (P @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    extent = float(np.linalg.norm(V.max(0).astype(F64) - V.min(0).astype(F64)))
    return dict(source=np.ascontiguousarray(X), vertices=V, faces=Fc, inlier=inlier, truth=truth(), extent=extent)


def corner_error(scene, T):
    """the farthest that a corner of the mesh's bounding box lies from where the truth carries it, as a share of the scene's extent"""
    return I.corner_shift(I.corners(scene['vertices']), T, scene['truth']) / scene['extent']


def loop_init():
    return I.loop_init()


@functools.lru_cache(maxsize=None)
def loop_reference(noisy=False, floor_only=False, with_scale=True, every=1, init=False):
    s = room_scene(noisy, floor_only)
    kw = dict(NOISY_KW) if noisy else dict(max_dist=MAX_DIST)
    kw.update(with_scale=with_scale, every=every)
    if init:
        kw['init'] = loop_init()
    return icp_to_mesh(s['source'], s['vertices'], s['faces'], **kw)


@functools.lru_cache(maxsize=None)
def point_to_point_reference():
    """today's loop on the same sources: `icp_ref.icp` against `nearest_ref.sample_mesh` of the room at spacing 0.08"""
    s = room_scene()
    samples = N.sample_mesh(s['vertices'], s['faces'], SPACING)['points']
    return dict(I.icp(s['source'], samples, MAX_DIST), samples=len(samples))
