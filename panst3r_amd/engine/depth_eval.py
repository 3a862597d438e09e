"""Predicted depth scored against ground-truth depth on the device (stage f16): AbsRel, SqRel, RMSE, MAE and the inlier ratios delta < t, per view or
per scene, after one of the alignments the literature uses (none, a given scale, median, least-squares scale, least-squares scale and shift).  It
scores what the other stages leave on the device - `x_out[v]['pts3d_local'][..., 2]`, the `depth` of `render_cloud` / `mesh.render` - against the
`depths` that `ground_truth_maps` returns, without a copy of the maps to the host.

The reference has no such stage: *restated, unpinned*.  The rules are written out in include/panst3r_hip.h (the depth-evaluation section) and
restated in numpy in tests/depth_eval_ref.py; csrc/depth_eval.hip is held to that bit for bit.  With p a predicted depth, g the ground truth:
  1 valid     g finite and min_depth < g <= max_depth; p finite and p > 0; with `conf` and `min_conf_thr`, conf >= min_conf_thr (a NaN confidence is
              invalid: the cloud stage's rule).  Validity never depends on the alignment.
  2 slabs     scope='view': every view is aligned and scored on its own (S = V); scope='scene': one alignment for all views (S = 1), the honest
              reading for a model that predicts all views in one common scale, and the counterpart of `panoptic_quality(scope='scene')`.
  3 align     p' = s p + b in fp64.  'none': (1, 0); a float: that scale (e.g. the scale of `similarity_from_cameras` or of an `Alignment`, for
              metric evaluation); 'median': s = median g / median p, exact fp32 medians; 'scale': s = sum pg / sum pp; 'scale_shift': the least-squares
              pair, s = (n sum pg - sum p sum g) / (n sum pp - (sum p)^2), b = (sum g - s sum p) / n.  A slab without a valid pixel, or with a
              degenerate solve (n sum pp - (sum p)^2 <= 0, sum pp <= 0, a median p of 0), reports None for everything and is left out of the means.
  4 errors    d = p' - g: |d| / g, d d / g, d d, |d|, and per threshold t an inlier iff p' < t g and g < t p' (strict), summed in fp64 in a fixed order
              (blocks of 4096 pixels of one view, 256 lanes, then one reducer per slab: csrc/icp_sum.h), so two calls return equal bytes.
  5 metrics   float64 on the host: abs_rel, sq_rel, rmse = sqrt(sum dd / n), mae, delta[k] = count_k / n.
Log-space metrics (rmse_log, SILog) are left out on purpose: a device `log` is not bit-identical to numpy's.  No per-pixel error maps."""
import math

import numpy as np
import torch

from .. import hip

ALIGNS = ('none', 'median', 'scale', 'scale_shift')
METRICS = ('abs_rel', 'sq_rel', 'rmse', 'mae')


def _depth_plane(t, shape, v):
    """-> (tensor kept alive, element stride) for a depth map [H, W] or a pointmap [..., H, W, 3] (z read in place), never a copy of a plane that is
    uniformly strided"""
    H, W = shape
    if not isinstance(t, torch.Tensor):
        raise ValueError('depth_quality: view %d: a prediction is a device tensor, got %s' % (v, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError('depth_quality got a prediction on %s: it runs on the GPU only (no CPU fallback)' % t.device)
    if t.dtype != torch.float32:
        raise ValueError('depth_quality: view %d: predictions are fp32, got %s' % (v, t.dtype))
    if t.numel() == H * W and tuple(t.shape[-2:]) == (H, W):
        z = t.reshape(H, W) if t.ndim != 2 else t
    elif t.ndim >= 3 and tuple(t.shape[-3:]) == (H, W, 3) and t.numel() == 3 * H * W:
        z = t.reshape(H, W, 3)[..., 2]
    else:
        raise ValueError('depth_quality: view %d: the prediction is %s, the ground truth %s' % (v, tuple(t.shape), (H, W)))
    s0, s1 = z.stride()
    if W == 1 and s0 >= 1:
        return z, s0
    if s1 >= 1 and (H == 1 or s0 == W * s1):
        return z, s1
    return z.contiguous(), 1


def _host_metrics(m, K):
    """step 5 on a row of error moments"""
    n = m[0]
    out = {'abs_rel': m[1] / n, 'sq_rel': m[2] / n, 'rmse': math.sqrt(m[3] / n), 'mae': m[4] / n}
    out['delta'] = tuple(m[5 + k] / n for k in range(K))
    return {k: (float(x) if k != 'delta' else tuple(float(y) for y in x)) for k, x in out.items()}


def _solve(align, n, mom, med):
    """(s, b) of a slab, or None: step 3 in float64"""
    if n == 0:
        return None
    if align == 'none':
        return 1.0, 0.0
    if isinstance(align, float):
        return align, 0.0
    if align == 'median':
        mp, mg = float(med[0]), float(med[1])
        return None if not mp > 0.0 else (mg / mp, 0.0)
    sp, sg, spp, spg = (float(x) for x in mom[1:5])
    if align == 'scale':
        return None if not spp > 0.0 else (spg / spp, 0.0)
    den = n * spp - sp * sp
    if not den > 0.0:
        return None
    s = (n * spg - sp * sg) / den
    return s, (sg - s * sp) / n


def _none_row():
    return dict({k: None for k in METRICS}, delta=None)


@torch.no_grad()
def depth_quality(pred, gt_depths, *, conf=None, min_conf_thr=None, align='median', scope='view', min_depth=0.0, max_depth=float('inf'),
                  thresholds=(1.03, 1.25, 1.25 ** 2, 1.25 ** 3)):
    """Score V predicted depths against V ground-truth depth maps (module docstring for the rules).  `pred`: a list of V device fp32 tensors, each a
    depth map [H_v, W_v] or a pointmap [..., H_v, W_v, 3] whose component 2 is read in place; or a list of `x_out` dicts ('pts3d_local' is scored
    and 'conf' is the confidence unless `conf=` is given).  `gt_depths`: V maps of the same shapes as `ground_truth_maps` returns them (0 = no
    surface), tensors or numpy arrays, moved to the predictions' device.  `conf` filters only together with `min_conf_thr`.  Mixed shapes are one
    launch per stage.  Returns a dict: scope, align, thresholds, n_valid; `slabs`, one dict per view (scope='view') or one for the scene with
    abs_rel, sq_rel, rmse, mae, delta (a tuple, one per threshold), n_valid, scale, shift, median_pred, median_gt (the medians only for
    align='median') - None where the slab has no valid pixel or no alignment; `moments` float64 [S, 16], the error sums as the device left them
    (n, sum |d|/g, sum dd/g, sum dd, sum |d|, inlier counts), and `align_moments` (n, sum p, sum g, sum pp, sum pg) for 'scale' / 'scale_shift'.
    At the top level the metrics of the scene (scope='scene'), or their means over the scored views in ascending order and `pooled`, the same
    formulas on the moments summed over those views (scope='view').  Two host syncs (one for align='none' or a float).  GPU only."""
    if scope not in ('view', 'scene'):
        raise ValueError("depth_quality: scope must be 'view' or 'scene', got %r" % (scope,))
    if isinstance(align, bool) or not (align in ALIGNS if isinstance(align, str) else isinstance(align, (int, float))):
        raise ValueError('depth_quality: align must be one of %s or a scale, got %r' % (ALIGNS, align))
    if not isinstance(align, str):
        align = float(align)
        if not math.isfinite(align):
            raise ValueError('depth_quality: the scale must be finite, got %r' % align)
    thresholds = tuple(float(t) for t in thresholds)
    if any(not t > 1.0 for t in thresholds):
        raise ValueError('depth_quality: thresholds must be > 1, got %s' % (thresholds,))
    if len(thresholds) > hip.DEPTH_MAX_THRESHOLDS:
        raise ValueError('depth_quality: at most %d thresholds per call, got %d' % (hip.DEPTH_MAX_THRESHOLDS, len(thresholds)))
    min_depth, max_depth = float(min_depth), float(max_depth)
    if not min_depth >= 0.0 or not max_depth > min_depth:
        raise ValueError('depth_quality: needs 0 <= min_depth < max_depth, got %r and %r' % (min_depth, max_depth))
    if not isinstance(pred, (list, tuple)) or not isinstance(gt_depths, (list, tuple, np.ndarray, torch.Tensor)):
        raise ValueError('depth_quality: pred is a list of V tensors (or x_out dicts), gt_depths V maps')
    pred, gts = list(pred), list(gt_depths)
    if pred and all(isinstance(p, dict) for p in pred):
        if conf is None:
            conf = [p['conf'] for p in pred]
        pred = [p['pts3d_local'] for p in pred]
    V = len(pred)
    if V == 0 or len(gts) != V or (conf is not None and len(conf) != V):
        raise ValueError('depth_quality: needs V >= 1 predictions, as many ground-truth maps and, if given, confidences; got %d, %d and %s'
                         % (V, len(gts), None if conf is None else len(conf)))
    use_conf = conf is not None and min_conf_thr is not None
    for v, g in enumerate(gts):
        if g.ndim != 2 or g.shape[0] * g.shape[1] == 0:
            raise ValueError('depth_quality: view %d: a ground-truth depth map is a non-empty [H, W], got %s' % (v, tuple(g.shape)))
    shapes = [(int(g.shape[0]), int(g.shape[1])) for g in gts]
    planes = [_depth_plane(p, s, v) for v, (p, s) in enumerate(zip(pred, shapes))]
    if sum(h * w for h, w in shapes) >= 2 ** 31:
        raise ValueError('depth_quality: the maps hold %d pixels; one call takes at most 2^31 - 1' % sum(h * w for h, w in shapes))
    dev = planes[0][0].device
    views = []
    for v, ((z, stride), g, (H, W)) in enumerate(zip(planes, gts, shapes)):
        g = (g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))).to(device=dev, dtype=torch.float32).contiguous()
        c = None
        if use_conf:
            c = conf[v]
            if not isinstance(c, torch.Tensor) or c.numel() != H * W:
                raise ValueError('depth_quality: view %d: the confidence does not match the %d x %d map' % (v, H, W))
            c = c.to(device=dev, dtype=torch.float32).contiguous()
        views.append((z, stride, g, c))
    S = V if scope == 'view' else 1
    table = hip.depth_table(views, list(range(V)) if scope == 'view' else [0] * V, dev)
    thr = float(min_conf_thr) if use_conf else 0.0
    ws = hip.depth_workspace(table, dev)
    K = len(thresholds)

    # the alignment stage: one host sync, none for 'none' or a given scale
    med = cnt = amom = None
    if align == 'median':
        count, median = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, 2, dtype=torch.float32, device=dev)
        hip.depth_median(table, min_depth, max_depth, thr, count, median)
        res = torch.cat([count, median.view(torch.int32).reshape(-1)]).cpu().numpy()
        cnt, med = res[:S].astype(np.int64), res[S:].copy().view(np.float32).reshape(S, 2)
    elif align in ('scale', 'scale_shift'):
        hip.depth_moments(table, min_depth, max_depth, thr, ws)
        amom = ws['out'].cpu().numpy()
        cnt = amom[:, 0].astype(np.int64)
    if cnt is None:
        sb = [(1.0, 0.0) if align == 'none' else (align, 0.0)] * S          # n is not known yet: an empty slab is found at the end
    else:
        sb = [_solve(align, int(cnt[s]), None if amom is None else amom[s], None if med is None else med[s]) for s in range(S)]
    al = torch.tensor([x if x is not None else (1.0, 0.0) for x in sb], dtype=torch.float64).to(dev)
    hip.depth_errors(table, min_depth, max_depth, thr, al, thresholds, ws)
    mom = ws['out'].cpu().numpy()                                            # the last host sync

    slabs = []
    for s in range(S):
        n = int(mom[s, 0])
        ok = n > 0 and sb[s] is not None
        row = _host_metrics(mom[s], K) if ok else _none_row()
        row.update(n_valid=n, scale=float(sb[s][0]) if ok else None, shift=float(sb[s][1]) if ok else None,
                   median_pred=float(med[s, 0]) if med is not None and n > 0 else None, median_gt=float(med[s, 1]) if med is not None and n > 0 else None)
        slabs.append(row)
    out = {'scope': scope, 'align': align, 'thresholds': thresholds, 'n_valid': sum(r['n_valid'] for r in slabs), 'slabs': slabs, 'moments': mom,
           'align_moments': amom}
    scored = [s for s in range(S) if slabs[s]['abs_rel'] is not None]
    if scope == 'scene':
        out.update({k: slabs[0][k] for k in METRICS + ('delta',)})
        return out
    for k in METRICS:
        out[k] = sum(slabs[s][k] for s in scored) / len(scored) if scored else None
    out['delta'] = tuple(sum(slabs[s]['delta'][k] for s in scored) / len(scored) for k in range(K)) if scored else None
    pooled = np.zeros(hip.DEPTH_MOMENTS)
    for s in scored:
        pooled = pooled + mom[s]
    out['pooled'] = dict(_host_metrics(pooled, K), n_valid=int(pooled[0])) if scored else dict(_none_row(), n_valid=0)
    return out
