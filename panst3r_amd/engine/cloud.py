"""The labelled 3-D panoptic point cloud of a scene on the device: every point with a colour and a panoptic instance id, one 3-D anchor per
segment, one frustum per camera.  The reference builds it on the host in numpy (tools/demo_panst3r.py:279-300 and
ViserVisualizer.show_pointcloud :622-687) after moving every pointmap, image and panoptic map to the CPU, and filters it again each time a
slider moves (:582-590); here it is four kernels of csrc/cloud.hip on the tensors the forward path left on the GPU.

The demo module cannot be imported (gradio / viser / roma at its top) and dust3r's `geotrf` / `rgb` are not vendored, so this stage is
*restated, unpinned*: tests/cloud_ref.py restates it in numpy with the arithmetic order fixed in include/panst3r_hip.h, and the kernels are
held to that restatement bit for bit.

Differences from the demo, on purpose: the colour table is an input (the demo draws random pastel colours from an unseeded generator,
:137-174); the default is `default_colors`, deterministic and keyed by segment id.  Void (id 0) and ids outside the table are black.
"""
import copy
import math

import numpy as np
import torch

from .. import hip


def default_colors(n_ids):
    """[n_ids, 3] float32 pastel table indexed by segment id; row 0 (void) black.  Row i >= 1: hue = frac(i * 0.6180339887498949) (golden-ratio
    spacing, as the demo's `pastel_colors(distinct=True)`), saturation 0.25 + 0.35 frac(i * 0.7548776662466927), value
    0.92 + 0.08 frac(i * 0.5698402909980532) (the demo's ranges), HSV -> RGB in float64, rounded to float32."""
    i = np.arange(n_ids, dtype=np.float64)
    h = (i * 0.6180339887498949) % 1.0
    s = 0.25 + 0.35 * ((i * 0.7548776662466927) % 1.0)
    v = 0.92 + 0.08 * ((i * 0.5698402909980532) % 1.0)
    k = np.floor(h * 6.0)
    f = h * 6.0 - k
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    k = k.astype(np.int64) % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    out = np.stack([r, g, b], axis=1).astype(np.float32)
    if n_ids:
        out[0] = 0
    return out


def quaternion_wxyz(R):
    """unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (float64, largest-component branch)"""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q)
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def camera_frusta(shapes, focals, cams2world):
    """the demo's per-camera numbers (:669-683): fov = 2 atan2(H / 2, focal), aspect = W / H, wxyz of c2w[:3, :3], position.  Host side."""
    out = []
    for (H, W), f, c2w in zip(shapes, focals, cams2world):
        c = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64)
        out.append({'fov': 2 * math.atan2(H / 2, float(f)), 'aspect': W / H, 'wxyz': quaternion_wxyz(c[:3, :3]), 'position': c[:3, 3].copy(),
                    'focal': float(f), 'height': int(H), 'width': int(W)})
    return out


def ply_colors_u8(c):
    """uchar = floor(clip(c, 0, 1) * 255 + 0.5), in float32"""
    return torch.floor(c.float().clamp(0, 1) * 255 + 0.5).to(torch.uint8)


class PanopticCloud:
    """points [M,3] (pts3d, or the world-frame local pointmaps with local_pointmaps), points_local [M,3], rgb [M,3], pan [M] int32, colors [M,3],
    index [M] int64 (position in the concatenated scene: view v holds [view_offsets[v], view_offsets[v+1]), pixel = index - view_offsets[v]),
    segments = [{'id', 'query_id', 'category_id', 'count', 'median'}] for the entries of segments_info with a kept point, cameras = frusta or None."""

    def __init__(self, points, points_local, rgb, pan, colors, index, view_offsets, segments, cameras=None, min_conf_thr=None, opacity=None, source=None):
        self.points, self.points_local, self.rgb, self.pan, self.colors, self.index = points, points_local, rgb, pan, colors, index
        self.view_offsets, self.segments, self.cameras = view_offsets, segments, cameras
        self.min_conf_thr, self.opacity = min_conf_thr, opacity
        self._source = source

    def __len__(self):
        return int(self.pan.shape[0])

    def _again(self, **kw):
        if self._source is None:
            raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
        return self._source.assemble(**kw)

    def rethreshold(self, min_conf_thr):
        """the demo's confidence slider (:582-590): a new cloud from the inputs kept on the device"""
        return self._again(min_conf_thr=min_conf_thr, opacity=self.opacity, colors=None)

    def recolor(self, opacity=None, colors=None):
        """the demo's opacity slider, and a new colour table"""
        return self._again(min_conf_thr=self.min_conf_thr, opacity=self.opacity if opacity is None else opacity, colors=colors)

    def voxelize(self, voxel_size, **kw):
        """engine.voxels.voxelize_cloud of this cloud"""
        from .voxels import voxelize_cloud
        return voxelize_cloud(self, voxel_size, **kw)

    def render(self, cams2world, focals, shape, **kw):
        """engine.render.render_cloud of this cloud"""
        from .render import render_cloud
        return render_cloud(self, cams2world, focals, shape, **kw)

    def mesh(self, **kw):
        """engine.surface.panoptic_mesh of this cloud"""
        from .surface import panoptic_mesh
        return panoptic_mesh(self, **kw)

    def fused_mesh(self, voxel_size, **kw):
        """engine.tsdf.fuse_surface of this cloud: ONE surface fused from all views in a volume, where `mesh` gives a sheet per view"""
        from .tsdf import fuse_surface
        return fuse_surface(self, voxel_size, **kw)

    def consistency(self, **kw):
        """engine.consistency.view_consistency of this cloud's own source - its views, cameras, confidence threshold and `local_pointmaps` - with the
        panoptic maps (labels=False: without them); `rel_tol`, `pp`, `near` as there -> `ViewConsistency` over the pixels of the scene"""
        if self._source is None:
            raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
        return self._source.consistency(self.min_conf_thr, **kw)

    def filter_consistent(self, min_views=1, max_violations=0, **kw):
        """A new cloud without the pixels that other views contradict: kept are the pixels that at least `min_views` other views agree with and at
        most `max_violations` other views see through (`ViewConsistency.keep`; `rel_tol`, `pp`, `near` go to `consistency`).  The result is built
        from a new source whose confidence planes are copies in which a dropped pixel is NaN - the value every stage's `conf >= thr` drops - so
        `rethreshold`, `recolor`, `voxelize`, `mesh`, `render`, the segment medians and `write_ply` work on it unchanged and stay filtered."""
        if self._source is None:
            raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
        return self._source.filtered(self.min_conf_thr, min_views, max_violations, **kw).assemble(self.min_conf_thr, self.opacity)

    def cpu(self):
        f = lambda t: t.cpu()
        return PanopticCloud(f(self.points), f(self.points_local), f(self.rgb), f(self.pan), f(self.colors), f(self.index), list(self.view_offsets),
                             [dict(s) for s in self.segments], self.cameras, self.min_conf_thr, self.opacity)

    def write_ply(self, path):
        """binary little-endian PLY: x y z float, red green blue uchar (of `colors`), label int (the panoptic id).  The 19-byte rows are packed
        where the cloud lives: one device-to-host copy."""
        M = len(self)
        rows = torch.empty(M, 19, dtype=torch.uint8, device=self.pan.device)
        rows[:, 0:12] = self.points.contiguous().view(torch.uint8).reshape(M, 12)
        rows[:, 12:15] = ply_colors_u8(self.colors)
        rows[:, 15:19] = self.pan.contiguous().view(torch.uint8).reshape(M, 4)
        header = ('ply\nformat binary_little_endian 1.0\ncomment panst3r_amd panoptic point cloud\nelement vertex %d\nproperty float x\nproperty float y\n'
                  'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nend_header\n' % M)
        with open(path, 'wb') as f:
            f.write(header.encode('ascii'))
            f.write(rows.cpu().numpy().tobytes())
        return path


def host_c34(cams2world):
    """the float32 [3, 4] camera-to-world rows of every view on the host: c2w of the kernels' view table (hip.cloud_view_table)"""
    return [np.asarray(torch.as_tensor(c).detach().cpu().numpy(), dtype=np.float32)[:3, :4] for c in cams2world]


class _Source:
    """the inputs of a scene's cloud, kept on the device: the view table of the kernels, the tensors it points into, the segment table"""

    def __init__(self, x_out, imgs, true_shape, pan, segments_info, cams2world, focals, colors, local_pointmaps):
        V = len(x_out)
        if not (len(imgs) == len(pan) == len(cams2world) == V) or V == 0:
            raise ValueError('x_out, imgs, pan and cams2world must list the same (non-zero) number of views')
        self.shapes = [tuple(int(s) for s in xo['conf'].shape[-2:]) for xo in x_out]
        if true_shape is not None:
            ts = torch.as_tensor(true_shape).reshape(-1, 2).tolist()
            if len(ts) != V or any(tuple(int(a) for a in t) != s for t, s in zip(ts, self.shapes)):
                raise ValueError('true_shape %s does not match the pointmaps %s' % (ts, self.shapes))
        views = []
        for xo, im, p, (H, W) in zip(x_out, imgs, pan, self.shapes):
            im = im[0] if im.dim() == 4 else im
            ten = (xo['conf'], xo['pts3d'], xo['pts3d_local'], im, p)
            for t in ten:
                if not t.is_cuda:
                    raise RuntimeError('panoptic_point_cloud got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
            if tuple(im.shape) != (3, H, W) or tuple(p.shape[-2:]) != (H, W):
                raise ValueError('image %s / panoptic map %s do not match the pointmap %s' % (tuple(im.shape), tuple(p.shape), (H, W)))
            views.append(tuple(t.float().contiguous() for t in ten[:4]) + (p.to(torch.int32).contiguous(),))
        self.device = views[0][0].device
        c34 = host_c34(cams2world)
        self.views = views                                                     # keeps the tensors the table points into alive
        self.c34, self.cams2world, self.focals = c34, list(cams2world), focals  # (the consistency stage builds its own tables from them)
        self.table, self.nwg, self.N = hip.cloud_view_table(views, c34, self.device)
        self.view_offsets = [0] + list(np.cumsum([h * w for h, w in self.shapes]).tolist())
        self.segments_info = [dict(s) for s in segments_info]
        ids = [int(s['id']) for s in self.segments_info]
        self.ntab = max(ids + [0]) + 1
        self.colors = None
        self.set_colors(colors)
        # the wrapper's check (the kernels never index with an id outside a table, but are not asked to survive one either)
        if any(i <= 0 for i in ids) or len(set(ids)) != len(ids):
            raise ValueError('segments_info ids must be distinct and positive (0 is void), got %s' % ids)
        if ids and max(ids) >= self.colors.shape[0]:
            raise ValueError('segments_info id %d does not fit the colour table of %d rows' % (max(ids), self.colors.shape[0]))
        row = np.full(self.ntab, -1, dtype=np.int32)
        for r, i in enumerate(ids):
            row[i] = r
        self.id2row = torch.from_numpy(row).to(self.device)
        self.cameras = None if focals is None else camera_frusta(self.shapes, focals, cams2world)
        self.local_pointmaps = bool(local_pointmaps)
        self.surface_dims = None                                               # (table, workgroups) of the quad kernels, built by engine.surface on first use

    def set_colors(self, colors):
        if colors is None:
            if self.colors is not None:
                return
            colors = default_colors(max(self.ntab, 2))
        c = torch.as_tensor(colors, dtype=torch.float32).reshape(-1, 3)
        if not 1 <= c.shape[0] <= hip.CLOUD_MAX_COLORS:
            raise ValueError('the colour table must have 1 .. %d rows, got %d' % (hip.CLOUD_MAX_COLORS, c.shape[0]))
        ids = [int(s['id']) for s in self.segments_info]
        if ids and max(ids) >= c.shape[0]:
            raise ValueError('segments_info id %d does not fit the colour table of %d rows' % (max(ids), c.shape[0]))
        self.colors = c.to(self.device).contiguous()

    def consistency(self, min_conf_thr, *, rel_tol=0.03, pp=None, near=1e-3, labels=True):
        """engine.consistency.view_consistency of the source's views at the threshold `min_conf_thr`"""
        from .consistency import consistency_of_views
        if self.focals is None:
            raise ValueError('the consistency of a cloud needs its focals: build it with panoptic_point_cloud(..., focals)')
        views = [(conf, pts, loc, p if labels else None) for conf, pts, loc, _, p in self.views]
        return consistency_of_views(views, self.shapes, self.c34, self.cams2world, self.focals, min_conf_thr, rel_tol, self.local_pointmaps, pp, near)

    @torch.no_grad()
    def filtered(self, min_conf_thr, min_views=1, max_violations=0, **kw):
        """a new source that shares everything with this one but the confidence planes: copies in which the pixels that fail
        `ViewConsistency.keep(min_views, max_violations)` at this threshold are NaN, and the view table that points to them"""
        from .consistency import masked_conf, check_keep
        check_keep(min_views, max_violations)                                  # a bad argument raises before anything is launched
        keep = self.consistency(min_conf_thr, labels=False, **kw).keep(min_views, max_violations)
        src = copy.copy(self)
        src.views = [(masked_conf(v[0], keep[a:b]).contiguous(),) + tuple(v[1:]) for v, a, b in zip(self.views, self.view_offsets[:-1], self.view_offsets[1:])]
        src.table, src.nwg, src.N = hip.cloud_view_table(src.views, self.c34, self.device)
        return src

    @torch.no_grad()
    def assemble(self, min_conf_thr, opacity, colors=None):
        self.set_colors(colors)
        dev, N, S = self.device, self.N, len(self.segments_info)
        thr = float(min_conf_thr)
        w1, w2 = float(np.float32(1.0 - float(opacity))), float(np.float32(float(opacity)))
        _, counts, base = hip.scan_buffers(dev, nwg=self.nwg)
        f3 = lambda: torch.empty(N, 3, dtype=torch.float32, device=dev)
        points, local, rgb, col = f3(), f3(), f3(), f3()
        pan = torch.empty(N, dtype=torch.int32, device=dev)
        index = torch.empty(N, dtype=torch.int64, device=dev)
        V = len(self.views)
        hip.cloud_count(self.table, V, self.nwg, thr, counts)
        hip.cloud_scan(counts, base)
        hip.cloud_compact(self.table, V, self.nwg, thr, base, self.colors, w1, w2, points, local, rgb, pan, col, index)
        res = base[self.nwg:]
        if S:
            count = torch.empty(S, dtype=torch.int32, device=dev)
            median = torch.empty(S, 3, dtype=torch.float32, device=dev)
            hip.cloud_segment_median(local, pan, res, self.id2row, S, count, median)
            res = torch.cat([res, count, median.view(torch.int32).reshape(-1)])
        res = res.cpu().numpy()                                                  # the only host sync: M and the segment table
        M = int(res[0])
        segments = decode_segments(res, self.segments_info, 1)
        points, local = points[:M], local[:M]
        return PanopticCloud(local if self.local_pointmaps else points, local, rgb[:M], pan[:M], col[:M], index[:M], list(self.view_offsets), segments,
                             self.cameras, thr, float(opacity), source=self)


def decode_segments(res, infos, at):
    """the segment table of a result buffer on the host, int32 [.., count[S] from `at`, median[S, 3] as bits] -> the `segments` list: one entry per
    segment of `infos` with a kept point"""
    S = len(infos)
    med = res[at + S:].view(np.float32).reshape(S, 3)
    return [{'id': s['id'], 'query_id': s.get('query_id'), 'category_id': s.get('category_id'), 'count': int(res[at + r]), 'median': med[r].copy()}
            for r, s in enumerate(infos) if res[at + r] > 0]


@torch.no_grad()
def panoptic_point_cloud(x_out, imgs, true_shape, pan, segments_info, cams2world, focals=None, *, min_conf_thr=3.0, opacity=0.5, colors=None,
                         local_pointmaps=False, consistency=None):
    """x_out: list[V] of dict(pts3d, pts3d_local [H,W,3], conf [H,W]) as `pointmaps.cameras_from_pointmaps` returns it (fp32, device); imgs: list of
    [3,H,W] in [-1, 1]; pan: list of int32 [H,W] and segments_info as `panoptic_inference_*` return them; cams2world: list of [4,4]; views may
    differ in shape.  Semantics (demo line numbers): views flattened and concatenated in order (:627-631), pts3d_local moved to the world frame
    (:293), rgb = img * 0.5 + 0.5 (:284); points with conf >= min_conf_thr kept in their original order (:633-639); colour =
    (1 - opacity) * rgb + opacity * colors[pan] (:351-352, 645); per entry of segments_info with a kept point the per-axis median of its
    world-frame local points (:654-657); per camera the frustum numbers (:669-683, when focals is given).  `colors`: [n_ids, 3] float table
    indexed by segment id (default: `default_colors`).  One host sync.  The outputs are views of scene-sized buffers (M is only known on the device
    when they are allocated): `.clone()` a tensor to keep it beyond the cloud.
    `consistency` (default None: off, the result is what it always was): True, or a dict of the keywords of `PanopticCloud.filter_consistent`
    (min_views, max_violations, rel_tol, pp, near) - the cloud is then built from the pixels that pass the cross-view depth check of
    engine/consistency.py, exactly as `panoptic_point_cloud(...).filter_consistent(...)` would; it needs `focals`."""
    kw = consistency_keywords(consistency)
    src = _Source(x_out, imgs, true_shape, pan, segments_info, cams2world, focals, colors, local_pointmaps)
    if kw is not None:
        src = src.filtered(float(min_conf_thr), **kw)
    return src.assemble(min_conf_thr, opacity)


def consistency_keywords(consistency):
    """the `consistency=` argument of `panoptic_point_cloud` / `PanSt3R.reconstruct` -> None (off) or the keywords of `filter_consistent`"""
    if consistency is None or consistency is False:
        return None
    if consistency is True:
        return {}
    if not isinstance(consistency, dict) or set(consistency) - {'min_views', 'max_violations', 'rel_tol', 'pp', 'near'}:
        raise ValueError('consistency must be None, True or a dict of min_views, max_violations, rel_tol, pp, near; got %r' % (consistency,))
    return dict(consistency)
