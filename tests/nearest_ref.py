"""numpy restatement of the two primitives of the 3-D scores (the score3d section of include/panst3r_hip.h; csrc/nearest.hip, engine/score3d.py), the
yardstick the kernels are held to bit for bit, and of the scores composed from them.  The sampler is restated step by step as the contract writes it;
the nearest neighbour is restated by BRUTE FORCE - all pairs, the same fp32 formula, the same (d2, row) minimum - and knows nothing of cells beyond which
targets the contract leaves out, so it checks the cell logic of the kernels independently.  numpy rounds every float operation on its own, as the
contract asks."""
import numpy as np

F32, F64 = np.float32, np.float64
LIM = 1 << 20
MAX_SUBDIV = 1 << 15


# ---------------------------------------------------------------- mesh surface sampler
def subdivisions(L2, s2, max_subdiv):
    """(n, clamped): the smallest n in [1, max_subdiv] with (n n) s2 >= L2, decided by the compare; a square root only as a first guess"""
    if not F64(max_subdiv) * F64(max_subdiv) * s2 >= L2:
        return max_subdiv, True
    n = int(min(max(np.ceil(np.sqrt(L2 / s2)), 1), max_subdiv))
    while n > 1 and F64(n - 1) * F64(n - 1) * s2 >= L2:
        n -= 1
    while not F64(n) * F64(n) * s2 >= L2:
        n += 1
    return n, False


def weights(n):
    """integer barycentric weights [n^2, 3] over 3n of the centroids of the n^2 sub-triangles, t ascending"""
    t = np.arange(n * n, dtype=np.int64)
    r = np.floor(np.sqrt(t.astype(F64))).astype(np.int64)
    r -= r * r > t
    r += (r + 1) * (r + 1) <= t
    c = t - r * r
    k = c >> 1
    up = np.stack([3 * (n - r) - 2, 3 * (r - k) + 1, 3 * k + 1], 1)
    inv = np.stack([3 * (n - r) - 1, 3 * (r - k) - 1, 3 * k + 2], 1)
    return np.where((c & 1)[:, None] == 1, inv, up)


def sample_mesh(vertices, faces, spacing, vertex_ids=None, face_ids=None, max_subdiv=1024):
    """-> dict: points fp32 [S,3], face int32 [S], ids int32 [S], n int [F] (0 = dropped), clamped bool [F], dropped_faces, clamped_faces, weights [S,3]"""
    assert vertex_ids is None or face_ids is None
    V = np.ascontiguousarray(vertices, dtype=F32)
    Fc = np.asarray(faces).astype(np.int64)
    s2 = F64(F32(spacing)) * F64(F32(spacing))
    ns, clamped = np.zeros(len(Fc), dtype=np.int64), np.zeros(len(Fc), dtype=bool)
    pts, fidx, ids, wts = [], [], [], []
    for f, idx in enumerate(Fc):
        if ((idx < 0) | (idx >= len(V))).any():
            continue
        v = V[idx].astype(F64)                                                   # [3 corners, 3 axes]
        if not np.isfinite(v).all():
            continue
        e1, e2 = v[1] - v[0], v[2] - v[0]
        cross = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        if (cross == 0).all():
            continue

        def edge2(a, b):
            d = a - b
            return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        L2 = max(edge2(v[1], v[0]), edge2(v[2], v[1]), edge2(v[0], v[2]))
        n, clamped[f] = subdivisions(L2, s2, max_subdiv)
        ns[f] = n
        w = weights(n)
        wd = w.astype(F64)
        p = ((wd[:, 0:1] * v[0] + wd[:, 1:2] * v[1]) + wd[:, 2:3] * v[2]) / F64(3 * n)
        pts.append(p.astype(F32)); fidx.append(np.full(n * n, f, dtype=np.int32)); wts.append(w)
        if face_ids is not None:
            ids.append(np.full(n * n, np.asarray(face_ids)[f], dtype=np.int32))
        elif vertex_ids is not None:
            best = np.argmax(w, 1)                                               # the first of equal maxima: the lower corner
            ids.append(np.asarray(vertex_ids)[idx[best]].astype(np.int32))
        else:
            ids.append(np.zeros(n * n, dtype=np.int32))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    return dict(points=cat(pts, (0, 3), F32), face=cat(fidx, (0,), np.int32), ids=cat(ids, (0,), np.int32), weights=cat(wts, (0, 3), np.int64), n=ns,
                clamped=clamped, dropped_faces=int((ns == 0).sum()), clamped_faces=int(clamped.sum()))


# ---------------------------------------------------------------- fixed-radius nearest neighbour
def radius_numbers(radius):
    r = F32(radius)
    return r, F32(1.0) / r, r * r


def cells(points, radius):
    """(cell float [N,3], finite [N], kept [N]): floor(fp32(x inv)); kept = finite and every cell inside (-2^20, 2^20).  Used for the left-out targets,
    and by the tests to say where the points of a scene lie; the search below does not look at cells."""
    P = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    _, inv, _ = radius_numbers(radius)
    with np.errstate(over='ignore', invalid='ignore'):
        c = np.floor(P * inv)
        finite = np.isfinite(P).all(1)
        kept = finite & (np.abs(c) < F32(LIM)).all(1)
    return c, finite, kept


def nearest(queries, targets, radius, chunk=512):
    """all pairs -> dict: d2 fp32 [Nq], row int32 [Nq], dropped_targets, bad_queries, second fp32 [Nq] (the second smallest d2 over the kept targets, for
    the tests: a tie or a near-tie shows there)"""
    Q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 3)
    T = np.ascontiguousarray(targets, dtype=F32).reshape(-1, 3)
    _, _, r2 = radius_numbers(radius)
    _, _, kept = cells(T, radius)
    rows = np.flatnonzero(kept)
    Tk = T[rows]
    qfinite = np.isfinite(Q).all(1)
    d2_out, row_out = np.full(len(Q), np.inf, dtype=F32), np.full(len(Q), -1, dtype=np.int32)
    second = np.full(len(Q), np.inf, dtype=F32)
    if len(Tk):
        for a in range(0, len(Q), chunk):
            q = Q[a:a + chunk]
            with np.errstate(over='ignore', invalid='ignore'):
                dx, dy, dz = (q[:, None, k] - Tk[None, :, k] for k in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz                               # float32 throughout
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)[None, :]
            best = key.min(1)
            bd2, brow = (best >> np.uint64(32)).astype(np.uint32).view(F32), (best & np.uint64(0xffffffff)).astype(np.int64)
            ok = qfinite[a:a + chunk] & (bd2 <= r2)
            d2_out[a:a + chunk] = np.where(ok, bd2, F32(np.inf))
            row_out[a:a + chunk] = np.where(ok, brow, -1)
            if len(Tk) > 1:
                second[a:a + chunk] = np.where(qfinite[a:a + chunk], np.partition(np.where(np.isnan(d2), F32(np.inf), d2), 1, axis=1)[:, 1], F32(np.inf))
    return dict(d2=d2_out, row=row_out, dropped_targets=int((~kept).sum()), bad_queries=int((~qfinite).sum()), second=second)


# ---------------------------------------------------------------- the scores composed from them
def _direction(d2, row):
    d = np.sqrt(d2[row >= 0].astype(F64))
    if len(d) == 0:
        return 0.0, float('nan'), float('nan')
    return len(d) / len(d2), float(d.sum() / len(d)), float(np.sort(d)[(len(d) - 1) // 2])


def scores(pred_points, gt_points, thresholds, max_dist=None, pred_ids=None, gt_ids=None):
    """the dict of engine.score_reconstruction from the two point sets (the ground-truth samples already made), and with both id arrays the two [S] id
    arrays that go through panoptic_quality: `pq_pred` (the id of the nearest predicted point, 0 without one) and `pq_gt`"""
    taus = [float(F32(t)) for t in thresholds]
    radius = max(taus) if max_dist is None else float(F32(max_dist))
    acc, comp = nearest(pred_points, gt_points, radius), nearest(gt_points, pred_points, radius)
    n_pred, n_gt = len(pred_points), len(gt_points)
    out = dict(thresholds=taus, max_dist=radius, n_pred=n_pred, n_gt=n_gt, precision=[], recall=[], fscore=[], pred_within=[], gt_within=[])
    for t in taus:
        t2 = F32(t) * F32(t)
        a, c = int((acc['d2'] <= t2).sum()), int((comp['d2'] <= t2).sum())
        p, r = (a / n_pred if n_pred else 0.0), (c / n_gt if n_gt else 0.0)
        out['pred_within'].append(a); out['gt_within'].append(c)
        out['precision'].append(p); out['recall'].append(r); out['fscore'].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    for name, res in (('accuracy', acc), ('completeness', comp)):
        out[name + '_matched'], out[name + '_mean'], out[name + '_median'] = _direction(res['d2'], res['row'])
    out['chamfer'] = out['accuracy_mean'] + out['completeness_mean']
    out['accuracy_rows'], out['completeness_rows'] = acc['row'], comp['row']
    if pred_ids is not None and gt_ids is not None:
        row = comp['row']
        out['pq_pred'] = np.where(row >= 0, np.asarray(pred_ids, dtype=np.int32)[np.maximum(row, 0)], 0).astype(np.int32) if n_pred else np.zeros(n_gt, np.int32)
        out['pq_gt'] = np.asarray(gt_ids, dtype=np.int32)
    return out


def similarity(scale, R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * np.asarray(R, dtype=F64), t
    return T
