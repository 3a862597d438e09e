"""numpy restatement of the exact point-to-mesh distance (the meshdist section of include/panst3r_hip.h; csrc/meshdist.hip, engine/meshdist.py), the
yardstick the kernels are held to bit for bit, and of the scores composed from it.  The closest point of a triangle is restated operation by operation
as the contract writes it (vectorised; np.where picks the region).  The search is BRUTE FORCE - every query against every kept face, the same (d2,
face) minimum - and knows nothing of cells beyond which faces the contract leaves out, so it checks the cell logic of the kernels independently.  The
binning is restated on its own (`binning`): the cell box of every face and its pair count.  numpy rounds every float operation on its own, as the
contract asks."""
import numpy as np

import nearest_ref as N

F32, F64 = np.float32, np.float64
LIM = 1 << 20
FACE_CAP = 2 ** 31 - 1
REGIONS = ('A', 'B', 'AB', 'C', 'AC', 'BC', 'interior')


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _clamp(t):
    return np.where(t > 0, np.minimum(t, 1.0), 0.0)                              # a NaN fails the compare: 0


def closest_point(a, b, c, q):
    """step 5 of the contract on float64 arrays [..., 3] (broadcast against each other) -> (D2 [...], x [..., 3], region int [...] indexing REGIONS)"""
    a, b, c, q = (np.asarray(t, dtype=F64) for t in (a, b, c, q))
    with np.errstate(all='ignore'):
        ab, ac, ap, bp, cp = b - a, c - a, q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        region = np.full(np.broadcast(d1, d1).shape, 6, dtype=np.int64)
        for k in range(5, -1, -1):                                               # the FIRST region that holds
            region = np.where(conds[k], k, region)
        tab, tac, tbc = _clamp(d1 / (d1 - d3)), _clamp(d2 / (d2 - d6)), _clamp((d4 - d3) / ((d4 - d3) + (d5 - d6)))
        den = 1.0 / ((va + vb) + vc)
        v, w = _clamp(vb * den), _clamp(vc * den)
        shape = region.shape + (3,)
        xs = [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + tab[..., None] * ab, np.broadcast_to(c, shape), a + tac[..., None] * ac,
              b + tbc[..., None] * (c - b), (a + v[..., None] * ab) + w[..., None] * ac]
        x = xs[6]
        for k in range(5, -1, -1):
            x = np.where((region == k)[..., None], xs[k], x)
        e = q - x
        D2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return D2, x, region


def binning(vertices, faces, radius):
    """steps 2 and 3 -> dict: kept bool [F], lo int64 [F,3] and ext int64 [F,3] (the cell box, 0 where dropped), counts int64 [F] (saturated at FACE_CAP),
    total, dropped_faces"""
    V = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    Fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    _, inv, _ = N.radius_numbers(radius)
    inside = ((Fc >= 0) & (Fc < len(V))).all(1)
    T = V[np.where(inside[:, None], Fc, 0)] if len(V) else np.zeros((len(Fc), 3, 3), F32)      # [F, corner, axis] fp32
    with np.errstate(all='ignore'):
        finite = np.isfinite(T).all((1, 2))
        t64 = T.astype(F64)
        e1, e2 = t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]
        cross = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        area = ~(cross == 0).all(1)
        cl = np.floor(T.min(1) * inv) - F32(1)                                   # fp32: whole numbers, exact inside the range
        ch = np.floor(T.max(1) * inv) + F32(1)
        in_range = ((cl > -F32(LIM)) & (ch < F32(LIM))).all(1)
    kept = inside & finite & area & in_range
    lo = np.where(kept[:, None], cl, 0).astype(np.int64)
    ext = np.where(kept[:, None], np.where(kept[:, None], ch, 0).astype(np.int64) - lo + 1, 0)
    counts = np.minimum(ext.prod(1), FACE_CAP)                                   # three factors below 2^21: inside int64
    return dict(kept=kept, lo=lo, ext=ext, counts=counts, total=int(counts.sum()), dropped_faces=int((~kept).sum()))


def cell_lists(vertices, faces, radius):
    """the lists of step 3 as a dict cell (x, y, z) -> sorted faces (small scenes only: one entry per pair)"""
    b = binning(vertices, faces, radius)
    lists = {}
    for f in np.flatnonzero(b['kept']):
        lo, ext = b['lo'][f], b['ext'][f]
        for t in range(int(b['counts'][f])):
            cell = (int(lo[0] + t % ext[0]), int(lo[1] + (t // ext[0]) % ext[1]), int(lo[2] + t // (ext[0] * ext[1])))
            lists.setdefault(cell, []).append(int(f))
    return lists


def mesh_distance(queries, vertices, faces, radius, chunk=256):
    """every query against every kept face -> dict: d2 fp32 [Nq], face int32 [Nq], closest fp32 [Nq,3], region int [Nq] (the winner's region, -1 without
    a hit), D2 fp64 [Nq] (the winner's, before the cast; inf without a hit), second fp32 [Nq] (the second smallest d2 over the kept faces, for the
    tests: a tie shows there), dropped_faces, bad_queries"""
    Q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 3)
    V = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    Fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    _, _, r2 = N.radius_numbers(radius)
    b = binning(V, Fc, radius)
    rows = np.flatnonzero(b['kept'])
    tri = V[Fc[rows]].astype(F64) if len(rows) else np.zeros((0, 3, 3))          # [K, corner, axis]
    qfinite = np.isfinite(Q).all(1)
    n = len(Q)
    out = dict(d2=np.full(n, np.inf, F32), face=np.full(n, -1, np.int32), closest=Q.copy(), region=np.full(n, -1, np.int64), D2=np.full(n, np.inf),
               second=np.full(n, np.inf, F32), dropped_faces=b['dropped_faces'], bad_queries=int((~qfinite).sum()))
    if len(rows):
        for s in range(0, n, chunk):
            q = Q[s:s + chunk].astype(F64)
            D2, x, region = closest_point(tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], q[:, None, :])
            with np.errstate(over='ignore', invalid='ignore'):
                d2 = D2.astype(F32)
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)[None, :]
            col = key.argmin(1)                                                  # keys are distinct: the minimum is one column
            best = key[np.arange(len(q)), col]
            bd2 = (best >> np.uint64(32)).astype(np.uint32).view(F32)
            ok = qfinite[s:s + chunk] & (bd2 <= r2)
            pick = np.arange(len(q))
            out['d2'][s:s + chunk] = np.where(ok, bd2, F32(np.inf))
            out['face'][s:s + chunk] = np.where(ok, rows[col], -1)
            out['closest'][s:s + chunk] = np.where(ok[:, None], x[pick, col].astype(F32), Q[s:s + chunk])
            out['region'][s:s + chunk] = np.where(ok, region[pick, col], -1)
            out['D2'][s:s + chunk] = np.where(ok, D2[pick, col], np.inf)
            if len(rows) > 1:
                out['second'][s:s + chunk] = np.where(qfinite[s:s + chunk], np.partition(np.where(np.isnan(d2), F32(np.inf), d2), 1, axis=1)[:, 1], F32(np.inf))
    return out


# ---------------------------------------------------------------- the scores composed from it
def scores(pred_points, gt_points, gt_vertices, gt_faces, thresholds, max_dist=None, pred_ids=None, gt_ids=None, pred_mesh=None):
    """the dict of engine.score_reconstruction(metric='surface') (the samples of both surfaces already made): predicted points -> the ground truth's
    triangles; ground-truth samples -> the triangles of `pred_mesh` = (vertices, faces, face_ids) when the prediction is a surface, else -> the
    predicted points by nearest_ref.nearest.  With ids the two [S] arrays that go through panoptic_quality, `pq_pred` and `pq_gt`."""
    taus = [float(F32(t)) for t in thresholds]
    radius = max(taus) if max_dist is None else float(F32(max_dist))
    acc = mesh_distance(pred_points, gt_vertices, gt_faces, radius)
    acc['row'] = acc['face']
    if pred_mesh is not None:
        comp = mesh_distance(gt_points, pred_mesh[0], pred_mesh[1], radius)
        comp['row'] = comp['face']
        pred_ids = pred_mesh[2]
    else:
        comp = N.nearest(gt_points, pred_points, radius)
    n_pred, n_gt = len(pred_points), len(gt_points)
    out = dict(thresholds=taus, max_dist=radius, n_pred=n_pred, n_gt=n_gt, precision=[], recall=[], fscore=[], pred_within=[], gt_within=[], metric='surface',
               gt_pairs=binning(gt_vertices, gt_faces, radius)['total'])
    for t in taus:
        t2 = F32(t) * F32(t)
        a, c = int((acc['d2'] <= t2).sum()), int((comp['d2'] <= t2).sum())
        p, r = (a / n_pred if n_pred else 0.0), (c / n_gt if n_gt else 0.0)
        out['pred_within'].append(a); out['gt_within'].append(c)
        out['precision'].append(p); out['recall'].append(r); out['fscore'].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    for name, res in (('accuracy', acc), ('completeness', comp)):
        out[name + '_matched'], out[name + '_mean'], out[name + '_median'] = N._direction(res['d2'], res['row'])
    out['chamfer'] = out['accuracy_mean'] + out['completeness_mean']
    if pred_ids is not None and gt_ids is not None:
        row = comp['row']
        out['pq_pred'] = np.where(row >= 0, np.asarray(pred_ids, dtype=np.int32)[np.maximum(row, 0)], 0).astype(np.int32)
        out['pq_gt'] = np.asarray(gt_ids, dtype=np.int32)
    return out
