"""Cross-view depth consistency of a scene's pointmaps on the device (stage f14): every pixel of every view is projected into every other view and
compared with the depth that view measured there.  Per pixel: `agree`, the number of other views that measured the same surface; `violate`, the number
of other views that see THROUGH the point - it lies in front of what they measured along that ray, the signature of the confident "floaters" that
DUSt3R-family pointmaps smear into free space at depth discontinuities; `same_label`, the number of agreeing views that also give it the same panoptic id.
`ViewConsistency.keep` turns the counts into a filter and `PanopticCloud.filter_consistent` applies it to a cloud.

The reference has no such stage: *restated, unpinned*, like the cloud and the renderer.  tests/consistency_ref.py restates the contract of
include/panst3r_hip.h in numpy; csrc/consistency.hip is held to it bit for bit (separately rounded fp32 operations, a quotient rounded once, no atomics).

What it does not do: no bilinear sampling of the target's depth (the nearest pixel centre is compared), no weighting of a pair by normal or grazing
angle, no frustum pre-cull of (workgroup, target) pairs."""
import math

import numpy as np
import torch

from .. import hip
from .cloud import host_c34
from .render import camera_table, _host64


class ViewConsistency:
    """agree, violate int32 [N], same_label int32 [N] or None, depth fp32 [N] (every pixel's depth in its own camera, 0 where the view measured nothing)
    over the N pixels of the concatenated scene: view v owns [view_offsets[v], view_offsets[v + 1]) and has the shape shapes[v]."""

    def __init__(self, agree, violate, same_label, depth, view_offsets, shapes):
        self.agree, self.violate, self.same_label, self.depth = agree, violate, same_label, depth
        self.view_offsets, self.shapes = view_offsets, shapes

    def __len__(self):
        return int(self.agree.shape[0])

    def maps(self, name):
        """the per-view [H, W] views of the field `name` ('agree', 'violate', 'same_label', 'depth')"""
        if name not in ('agree', 'violate', 'same_label', 'depth'):
            raise ValueError("maps() takes 'agree', 'violate', 'same_label' or 'depth', got %r" % (name,))
        t = getattr(self, name)
        if t is None:
            raise ValueError('this result holds no %s (it was computed without panoptic maps)' % name)
        return [t[a:b].view(H, W) for a, b, (H, W) in zip(self.view_offsets[:-1], self.view_offsets[1:], self.shapes)]

    def keep(self, min_views=1, max_violations=0):
        """bool [N]: agree >= min_views and violate <= max_violations"""
        return keep_mask(self.agree, self.violate, min_views, max_violations)


def check_keep(min_views, max_violations):
    for name, k in (('min_views', min_views), ('max_violations', max_violations)):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError('%s must be an integer >= 0, got %r' % (name, k))
    return int(min_views), int(max_violations)


def keep_mask(agree, violate, min_views=1, max_violations=0):
    """bool tensor: agree >= min_views and violate <= max_violations (both integers >= 0)"""
    min_views, max_violations = check_keep(min_views, max_violations)
    return (agree >= min_views) & (violate <= max_violations)


def masked_conf(conf, keep):
    """a copy of the confidence plane `conf` in which every pixel outside `keep` is NaN: the value every stage's `conf >= thr` drops, whatever the
    threshold (csrc/cloud.hip: a NaN confidence is not kept; a finite marker such as -1 would come back under a lower threshold)"""
    return torch.where(keep.reshape(conf.shape), conf, torch.full((), float('nan'), dtype=conf.dtype, device=conf.device))


def _check_rel_tol(rel_tol):
    r = float(rel_tol)
    if not (math.isfinite(r) and 0 <= r and float(np.float32(r)) < 1):
        raise ValueError('rel_tol must be a finite number in [0, 1), got %r' % (rel_tol,))
    return r


def own_camera_table(cams2world, focals, shapes, pp=None, near=1e-3):
    """float32 [V, 16]: `render.camera_table` of every view's own camera at its own shape (pp: one (cx, cy) for all, one per view, or None for the centre
    (W / 2, H / 2) of each view)"""
    V = len(shapes)
    if focals is None:
        raise ValueError('view_consistency needs the focals: without them there is no projection')
    f = _host64([float(x) for x in focals] if isinstance(focals, (list, tuple)) else focals).reshape(-1)
    if f.size == 1:
        f = np.repeat(f, V)
    if len(cams2world) != V or f.size != V:
        raise ValueError('x_out, cams2world and focals must list the same number of views (or one focal for all)')
    if pp is not None:
        p = _host64(pp)
        if p.size not in (2, 2 * V):
            raise ValueError('pp must be a (cx, cy) pair, one per view or one for all, got %r' % (pp,))
        p = np.broadcast_to(p.reshape(-1, 2), (V, 2))
    return np.concatenate([camera_table([cams2world[v]], f[v:v + 1], shapes[v], None if pp is None else p[v], near) for v in range(V)])


@torch.no_grad()
def consistency_of_views(views, shapes, c34, cams2world, focals, min_conf_thr, rel_tol, local_pointmaps, pp, near):
    """the two kernels over views = [(conf, pts3d, pts3d_local, pan or None)] (contiguous fp32 / int32 device tensors) -> ViewConsistency"""
    rel = _check_rel_tol(rel_tol)
    cams = own_camera_table(cams2world, focals, shapes, pp, near)
    for ten in views:
        for t in ten:
            if t is not None and not t.is_cuda:
                raise RuntimeError('view_consistency got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
    dev = views[0][0].device
    table, camd, dims, nwg, N = hip.consist_view_table(views, c34, cams, shapes, dev)
    V = len(views)
    labels = all(v[3] is not None for v in views)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    agree, violate = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    same = torch.empty(N, dtype=torch.int32, device=dev) if labels else None
    hip.consist_depth(table, camd, V, nwg, float(min_conf_thr), local_pointmaps, depth)
    hip.consist_count(table, camd, dims, V, nwg, rel, local_pointmaps, depth, agree, violate, same)
    offsets = [0] + list(np.cumsum([h * w for h, w in shapes]).tolist())
    return ViewConsistency(agree, violate, same, depth, offsets, list(shapes))


@torch.no_grad()
def view_consistency(x_out, cams2world, focals, *, min_conf_thr=3.0, rel_tol=0.03, pan=None, local_pointmaps=False, pp=None, near=1e-3):
    """x_out: list[V] of dict(pts3d, pts3d_local [H,W,3], conf [H,W]) as `pointmaps.cameras_from_pointmaps` returns it (fp32, device), with its
    cams2world (list of [4,4]) and focals (pixels, one per view; required - without them there is no projection: ValueError); views may differ in shape.
    -> `ViewConsistency`.  A pixel takes part if conf >= min_conf_thr, its point is finite and at least `near` in front of its own camera; its point
    is `pts3d`, or with local_pointmaps `pts3d_local` moved by its camera, as the cloud's.  In every other view the point projects to the nearest pixel
    centre (pp: the principal point(s), default (W / 2, H / 2); pixel x sits at u = x, the pointmaps' convention) and meets that view's depth d there:
    it AGREES if |z - d| <= rel_tol * d, VIOLATES if it is nearer than that (the other view sees through it), and is occluded - counts for nothing -
    if it is farther; outside the image, or on a pixel that view did not measure, it is unseen.  `pan`: list of int32 [H,W] panoptic maps; with them
    `same_label` counts the agreeing views that give the pixel its own id (> 0).  `rel_tol` = 0.03 is a CHOICE (3 % of the depth, a few times the
    depth noise of a good pointmap), not a measured optimum, like `max_depth_ratio` of the surface.  No host sync when the cameras are host values.
    GPU only: a CPU tensor raises."""
    V = len(x_out)
    if focals is None:
        raise ValueError('view_consistency needs the focals: without them there is no projection')
    _check_rel_tol(rel_tol)
    if V == 0 or len(cams2world) != V or (pan is not None and len(pan) != V):
        raise ValueError('x_out, cams2world and pan must list the same (non-zero) number of views')
    shapes = [tuple(int(s) for s in xo['conf'].shape[-2:]) for xo in x_out]
    views = []
    for k, (xo, (H, W)) in enumerate(zip(x_out, shapes)):
        ten = (xo['conf'], xo['pts3d'], xo['pts3d_local']) + ((pan[k],) if pan is not None else ())
        for t in ten:
            if not t.is_cuda:
                raise RuntimeError('view_consistency got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
        if pan is not None and tuple(pan[k].shape[-2:]) != (H, W):
            raise ValueError('panoptic map %s does not match the pointmap %s' % (tuple(pan[k].shape), (H, W)))
        views.append(tuple(t.float().contiguous() for t in ten[:3]) + (pan[k].to(torch.int32).contiguous() if pan is not None else None,))
    return consistency_of_views(views, shapes, host_c34(cams2world), cams2world, focals, min_conf_thr, rel_tol, local_pointmaps, pp, near)
