"""numpy restatement of the depth evaluation (the depth-evaluation section of include/panst3r_hip.h; csrc/depth_eval.hip,
panst3r_amd/engine/depth_eval.py), the yardstick both are held to bit for bit.  Validity in fp32 as the contract writes it; the medians by a sort
(which knows nothing of radix passes); the alignment and the errors in float64, every operation on its own (numpy rounds each separately); the sums
in the fixed order of the contract, whose constants are read from panst3r_amd.hip (plain Python numbers there): blocks of ICP_CHUNK pixels of ONE
view, 256 lane accumulators, the butterfly, the four waves in order, then the slab's rows of partials the same way.  Also the generated cases the
host test and the GPU test share."""
import math

import numpy as np

from panst3r_amd.hip import ICP_CHUNK, ICP_LANES, DEPTH_MOMENTS

F32, F64 = np.float32, np.float64
ALIGNS = ('none', 'median', 'scale', 'scale_shift')
METRICS = ('abs_rel', 'sq_rel', 'rmse', 'mae')


# ---------------------------------------------------------------- the fixed order
def block_sum(acc):
    """[..., 256] lane accumulators -> [...]: six butterfly steps inside every wave of 64, then ((w0 + w1) + w2) + w3"""
    a = acc.reshape(acc.shape[:-1] + (ICP_LANES // 64, 64))
    idx = np.arange(64)
    for k in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ k]
    w = a[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def view_partials(values):
    """the row of partials of every block of ONE view: values float64 [npix], +0.0 where the pixel is invalid (an accumulator that starts at +0.0
    never holds -0.0, so adding +0.0 changes nothing) -> float64 [ceil(npix / ICP_CHUNK)]"""
    v = np.asarray(values, dtype=F64).reshape(-1)
    P, rows = (len(v) + ICP_CHUNK - 1) // ICP_CHUNK, ICP_CHUNK // ICP_LANES
    v = np.concatenate([v, np.zeros(P * ICP_CHUNK - len(v))]).reshape(P, rows, ICP_LANES)
    acc = np.zeros((P, ICP_LANES))
    for j in range(rows):
        acc = acc + v[:, j]
    return block_sum(acc)


def reduce_rows(partials):
    """the reducer of a slab: lane l adds its rows l, l + 256, ... ascending, then the block sum"""
    p = np.asarray(partials, dtype=F64).reshape(-1)
    R = (len(p) + ICP_LANES - 1) // ICP_LANES
    p = np.concatenate([p, np.zeros(R * ICP_LANES - len(p))]).reshape(R, ICP_LANES)
    acc = np.zeros(ICP_LANES)
    for r in range(R):
        acc = acc + p[r]
    return block_sum(acc)


def slab_sum(per_view_values):
    """the sum of a slab: the partials of its views' blocks, concatenated in view order, through the reducer"""
    return reduce_rows(np.concatenate([view_partials(v) for v in per_view_values]))


# ---------------------------------------------------------------- the steps
def valid(p, g, conf, thr, min_depth, max_depth):
    """step 1, in fp32"""
    p, g = np.asarray(p, dtype=F32).reshape(-1), np.asarray(g, dtype=F32).reshape(-1)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(g) & (g > F32(min_depth)) & (g <= F32(max_depth)) & np.isfinite(p) & (p > F32(0))
        if conf is not None and thr is not None:
            ok &= np.asarray(conf, dtype=F32).reshape(-1) >= F32(thr)
    return ok


def median32(x):
    """the exact fp32 median of positive finite values: the middle element, or (a + b) * 0.5f in fp32"""
    x = np.sort(np.asarray(x, dtype=F32))
    n = len(x)
    if n == 0:
        return F32(np.nan)
    with np.errstate(over='ignore'):
        return x[n // 2] if n & 1 else F32(F32(x[(n - 1) // 2] + x[n // 2]) * F32(0.5))


def align_terms(p, g, ok):
    """float64 [5, npix]: 1, p, g, pp, pg where valid, +0.0 elsewhere"""
    p, g = np.where(ok, p, F32(0)).astype(F64), np.where(ok, g, F32(0)).astype(F64)
    return np.stack([ok.astype(F64), p, g, p * p, p * g])


def error_terms(p, g, ok, s, b, thresholds):
    """float64 [5 + K, npix] under p' = s p + b: 1, |d|/g, dd/g, dd, |d|, the K inlier flags where valid, +0.0 elsewhere"""
    pv, gv = np.where(ok, p, F32(1)).astype(F64), np.where(ok, g, F32(1)).astype(F64)
    with np.errstate(over='ignore', invalid='ignore'):
        pa = F64(s) * pv
        pa = pa + F64(b)
        d = pa - gv
        ad, dd = np.abs(d), d * d
        rows = [np.ones_like(pv), ad / gv, dd / gv, dd, ad] + [((pa < F64(t) * gv) & (gv < F64(t) * pa)).astype(F64) for t in thresholds]
    return np.stack([np.where(ok, r, 0.0) for r in rows])


def solve(align, n, mom, med):
    """step 4 on the host, float64 -> (s, b) or None"""
    if n == 0:
        return None
    if align == 'none':
        return 1.0, 0.0
    if isinstance(align, float):
        return align, 0.0
    if align == 'median':
        mp, mg = float(med[0]), float(med[1])
        return (mg / mp, 0.0) if mp > 0.0 else None
    sp, sg, spp, spg = (float(x) for x in mom[1:5])
    if align == 'scale':
        return (spg / spp, 0.0) if spp > 0.0 else None
    den = n * spp - sp * sp
    if not den > 0.0:
        return None
    s = (n * spg - sp * sg) / den
    return s, (sg - s * sp) / n


def metrics(m, K):
    n = float(m[0])
    return {'abs_rel': float(m[1]) / n, 'sq_rel': float(m[2]) / n, 'rmse': math.sqrt(float(m[3]) / n), 'mae': float(m[4]) / n,
            'delta': tuple(float(m[5 + k]) / n for k in range(K))}


def depth_quality(pred, gt, *, conf=None, min_conf_thr=None, align='median', scope='view', min_depth=0.0, max_depth=float('inf'),
                  thresholds=(1.03, 1.25, 1.25 ** 2, 1.25 ** 3)):
    """the engine's result on host arrays: pred = V depth maps [H, W] (fp32), gt likewise, conf likewise or None"""
    assert scope in ('view', 'scene') and (align in ALIGNS or isinstance(align, float))
    V, K = len(pred), len(thresholds)
    P, G = [np.asarray(p, dtype=F32).reshape(-1) for p in pred], [np.asarray(g, dtype=F32).reshape(-1) for g in gt]
    ok = [valid(P[v], G[v], None if conf is None else conf[v], min_conf_thr, min_depth, max_depth) for v in range(V)]
    groups = [[v] for v in range(V)] if scope == 'view' else [list(range(V))]
    S = len(groups)
    mom, amom, slabs = np.zeros((S, DEPTH_MOMENTS)), None, []
    if align in ('scale', 'scale_shift'):
        amom = np.zeros((S, DEPTH_MOMENTS))
    for s, views in enumerate(groups):
        n = int(sum(ok[v].sum() for v in views))
        med = None
        if align == 'median':
            med = (median32(np.concatenate([P[v][ok[v]] for v in views])), median32(np.concatenate([G[v][ok[v]] for v in views])))
        if amom is not None:
            t = [align_terms(P[v], G[v], ok[v]) for v in views]
            for k in range(5):
                amom[s, k] = slab_sum([x[k] for x in t])
            assert amom[s, 0] == n
        sb = solve(align, n, None if amom is None else amom[s], med)
        a, b = sb if sb is not None else (1.0, 0.0)
        t = [error_terms(P[v], G[v], ok[v], a, b, thresholds) for v in views]
        for k in range(5 + K):
            mom[s, k] = slab_sum([x[k] for x in t])
        assert mom[s, 0] == n
        good = n > 0 and sb is not None
        row = metrics(mom[s], K) if good else dict({k: None for k in METRICS}, delta=None)
        row.update(n_valid=n, scale=float(a) if good else None, shift=float(b) if good else None,
                   median_pred=float(med[0]) if med is not None and n > 0 else None, median_gt=float(med[1]) if med is not None and n > 0 else None)
        slabs.append(row)
    out = {'scope': scope, 'align': align, 'thresholds': tuple(float(t) for t in thresholds), 'n_valid': sum(r['n_valid'] for r in slabs), 'slabs': slabs,
           'moments': mom, 'align_moments': amom}
    scored = [s for s in range(S) if slabs[s]['abs_rel'] is not None]
    if scope == 'scene':
        out.update({k: slabs[0][k] for k in METRICS + ('delta',)})
        return out
    for k in METRICS:
        out[k] = sum(slabs[s][k] for s in scored) / len(scored) if scored else None
    out['delta'] = tuple(sum(slabs[s]['delta'][k] for s in scored) / len(scored) for k in range(K)) if scored else None
    pooled = np.zeros(DEPTH_MOMENTS)
    for s in scored:
        pooled = pooled + mom[s]
    out['pooled'] = dict(metrics(pooled, K), n_valid=int(pooled[0])) if scored else dict({k: None for k in METRICS}, delta=None, n_valid=0)
    return out


# ---------------------------------------------------------------- generated cases
def random_views(shapes, seed, *, holes=0.15, bad=0.05, with_conf=True):
    """V views of ground truth in [0.5, 8) with `holes` zeros, predictions = gt times a common scale near 0.4 with 5 % noise, `bad` of them NaN,
    +-inf, 0 or negative, and a confidence in [0, 4) with some NaN -> (pred, gt, conf) lists of fp32 [H, W]"""
    r = np.random.Generator(np.random.PCG64(seed))
    pred, gt, conf = [], [], []
    for H, W in shapes:
        g = r.uniform(0.5, 8.0, (H, W)).astype(F32)
        p = (g * F32(0.4) * r.normal(1.0, 0.05, (H, W)).astype(F32)).astype(F32)
        g[r.random((H, W)) < holes] = 0
        junk = r.random((H, W))
        for i, val in enumerate((np.nan, np.inf, -np.inf, 0.0, -1.5)):
            p[(junk >= bad * i / 5) & (junk < bad * (i + 1) / 5)] = val
        c = r.uniform(0.0, 4.0, (H, W)).astype(F32)
        c[r.random((H, W)) < 0.02] = np.nan
        pred.append(p); gt.append(g); conf.append(c)
    return pred, gt, (conf if with_conf else None)
