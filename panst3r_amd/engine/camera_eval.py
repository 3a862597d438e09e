"""Predicted cameras scored against ground-truth cameras (stage f16): relative rotation and translation accuracy over all pairs, mAA, the absolute
trajectory error after a similarity alignment, the relative focal error.  Poses are host values in this project and there are at most a few hundred
of them: float64 numpy on the host, no kernel.

The reference has no such stage: *restated, unpinned*.  The conventions are CHOICES, the ones of the published relative-pose protocols:
  poses       rigid camera-to-world matrices [4, 4] (or [3, 4]): the rotation block is a rotation, the last column the camera centre.  A prediction
              in another frame and scale keeps rigid poses: R_i -> R R_i, c_i -> s R c_i + t.
  pairs       all i < j; the relative pose inv(T_i) T_j = (R_i^T R_j, R_i^T (c_j - c_i)) of the prediction and of the ground truth.
  rotation    the angle of E = R_pred_rel^T R_gt_rel as atan2(0.5 |(E32 - E23, E13 - E31, E21 - E12)|, 0.5 (tr E - 1)), in degrees: well conditioned
              at 0 and at 180, where acos of the trace is not.
  translation the angle between the two relative translations, atan2(|a x b|, a . b), in degrees: the direction only, the scale of a baseline is not
              judged.  ambiguity=True takes min(e, 180 - e), as the published RTA does (the sign of a baseline is not judged either).  A pair whose
              predicted or ground-truth baseline has zero length has no direction: it is left out of RTA and mAA and counted in `n_no_baseline`.
  RRA / RTA   the share of pairs with an error < tau, strictly.  mAA@30: the mean over tau = 1 .. 30 degrees of the share of pairs (with a
              direction) whose max(rotation, translation) error is < tau.
  ATE         the RMSE of the camera centres after `similarity_from_cameras` has carried the prediction into the ground truth's frame; None, with
              the reason under `ate_reason`, where that function raises (fewer than 3 cameras, centres that do not span a plane).
  focals      mean |f_pred - f_gt| / f_gt over the views (and over fx, fy where both are given)."""
import numpy as np
import torch

from .score3d import similarity_from_cameras


def _poses(cams, name):
    c = np.stack([np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64) for m in cams]) if len(cams) else np.zeros((0, 4, 4))
    if c.ndim != 3 or c.shape[1] < 3 or c.shape[2] != 4:
        raise ValueError('%s must be V camera-to-world matrices [4, 4] (or [3, 4]), got %s' % (name, c.shape))
    if not np.isfinite(c).all():
        raise ValueError('%s holds a non-finite entry' % name)
    return c[:, :3, :3], c[:, :3, 3]


def _relative(R, c, i, j):
    return R[i].T @ R[j], R[i].T @ (c[j] - c[i])


def _share(errs, tau):
    return float(np.mean(np.asarray(errs) < tau)) if len(errs) else None


def camera_quality(pred_cams2world, gt_cams2world, *, pred_focals=None, gt_focals=None, taus=(5, 15, 30), ambiguity=True):
    """Score V >= 2 predicted cameras against the ground truth's (module docstring for the conventions; *restated, unpinned*).  Returns a dict:
    pairs [(i, j)], rot_err_deg and trans_err_deg per pair (None for a pair without a direction), rra and rta {tau: share}, maa_30, n_pairs,
    n_no_baseline, ate_rmse and ate_reason, focal_rel_err (None without focals)."""
    Rp, cp = _poses(pred_cams2world, 'pred_cams2world')
    Rg, cg = _poses(gt_cams2world, 'gt_cams2world')
    V = len(Rp)
    if V != len(Rg) or V < 2:
        raise ValueError('camera_quality needs V >= 2 predicted cameras and as many ground-truth ones, got %d and %d' % (V, len(Rg)))
    pairs, rot, trans = [], [], []
    for i in range(V):
        for j in range(i + 1, V):
            (Ra, a), (Rb, b) = _relative(Rp, cp, i, j), _relative(Rg, cg, i, j)
            E = Ra.T @ Rb
            w = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
            rot.append(float(np.degrees(np.arctan2(0.5 * np.linalg.norm(w), 0.5 * (np.trace(E) - 1.0)))))
            if np.linalg.norm(a) == 0.0 or np.linalg.norm(b) == 0.0:
                trans.append(None)
            else:
                e = float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), float(a @ b))))
                trans.append(min(e, 180.0 - e) if ambiguity else e)
            pairs.append((i, j))
    directed = [(r, t) for r, t in zip(rot, trans) if t is not None]
    both = [max(r, t) for r, t in directed]
    out = {'pairs': pairs, 'rot_err_deg': rot, 'trans_err_deg': trans, 'n_pairs': len(pairs), 'n_no_baseline': len(pairs) - len(directed),
           'rra': {t: _share(rot, t) for t in taus}, 'rta': {t: _share([t_ for _, t_ in directed], t) for t in taus},
           'maa_30': float(np.mean([_share(both, tau) for tau in range(1, 31)])) if both else None}
    try:
        T = similarity_from_cameras(pred_cams2world, gt_cams2world).numpy()
        moved = cp @ T[:3, :3].T + T[:3, 3]
        out['ate_rmse'], out['ate_reason'] = float(np.sqrt(np.mean(np.sum((moved - cg) ** 2, axis=1)))), None
    except ValueError as e:
        out['ate_rmse'], out['ate_reason'] = None, str(e)
    out['focal_rel_err'] = None
    if pred_focals is not None or gt_focals is not None:
        if pred_focals is None or gt_focals is None:
            raise ValueError('camera_quality: pred_focals and gt_focals go together')
        as_rows = lambda f: np.stack([np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1) for x in f])
        fp, fg = as_rows(pred_focals), as_rows(gt_focals)
        if len(fp) != V or len(fg) != V or fp.shape[1] not in (1, fg.shape[1]) and fg.shape[1] != 1:
            raise ValueError('camera_quality: needs one focal (or fx, fy) per camera, got %s and %s' % (fp.shape, fg.shape))
        out['focal_rel_err'] = float(np.mean(np.abs(fp - fg) / fg))
    return out
