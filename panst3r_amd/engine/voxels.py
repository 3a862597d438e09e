"""Voxel fusion of a scene's panoptic point cloud on the device: the cloud of `panoptic_point_cloud` concatenates every view's kept pixels, so a
surface seen by eight views is in it eight times with eight independent 2-D label decisions.  `voxelize_cloud` downsamples it on a grid of cubic
cells and lets the points of a cell vote on its panoptic id: one point per occupied cell (mean position, mean colour, voted id, agreement), the cell
of every cloud point, and - projected back - per-view panoptic maps that agree across views.

The reference has no such stage (its viewer shows the raw concatenation): *restated, unpinned*, like the cloud.  tests/voxel_ref.py restates the
five steps of the contract in include/panst3r_hip.h in numpy; csrc/voxel.hip is held to it bit for bit (integer sums, separately rounded fp32 /
fp64 operations, integer atomics only)."""
import math

import numpy as np
import torch

from .. import hip
from .cloud import decode_segments, default_colors, ply_colors_u8


class VoxelCloud:
    """For the Mv occupied voxels, ordered by each voxel's first point in cloud order: points [Mv,3] (mean position), rgb [Mv,3] (mean colour), pan [Mv]
    int32 (voted id), colors [Mv,3], count [Mv] int32 (points of the voxel), votes [Mv] int32 (points that voted for the winner), first_index [Mv] int64
    (scene index of the voxel's first point); point_voxel [M] int32 (voxel row of every cloud point, -1 for a point left out); segments as the cloud's
    ('count' = voxels, 'median' over voxel positions); cameras, view_offsets as the cloud's; voxel_size; dropped (points left out); cells [Mv,3] int32
    (the integer cell of every voxel: what `components` and `clean_labels` work on; None for a cloud built by hand without it).  A cloud that
    `clean_labels` returned also holds `relabelled` and `floaters`, the voxels that took a neighbour's id / became void."""

    def __init__(self, points, rgb, pan, colors, count, votes, first_index, point_voxel, segments, cameras, view_offsets, voxel_size, dropped, opacity=None,
                 point_pan=None, point_index=None, source=None, cells=None, color_table=None):
        self.points, self.rgb, self.pan, self.colors, self.count, self.votes, self.first_index = points, rgb, pan, colors, count, votes, first_index
        self.point_voxel, self.segments, self.cameras, self.view_offsets = point_voxel, segments, cameras, view_offsets
        self.voxel_size, self.dropped, self.opacity = voxel_size, dropped, opacity
        self._point_pan, self._point_index, self._source = point_pan, point_index, source
        self.cells, self._color_table = cells, color_table
        self.relabelled = self.floaters = None

    def __len__(self):
        return int(self.pan.shape[0])

    def cpu(self):
        f = lambda t: None if t is None else t.cpu()
        return VoxelCloud(f(self.points), f(self.rgb), f(self.pan), f(self.colors), f(self.count), f(self.votes), f(self.first_index), f(self.point_voxel),
                          [dict(s) for s in self.segments], self.cameras, list(self.view_offsets), self.voxel_size, self.dropped, self.opacity,
                          f(self._point_pan), f(self._point_index), cells=f(self.cells), color_table=f(self._color_table))._counts(self)

    def _counts(self, other):
        self.relabelled, self.floaters = other.relabelled, other.floaters
        return self

    def components(self, connectivity=26):
        """`voxel_components` of this cloud"""
        return voxel_components(self, connectivity)

    def clean_labels(self, min_voxels, connectivity=26):
        """`clean_voxel_labels` of this cloud"""
        return clean_voxel_labels(self, min_voxels, connectivity)

    def write_ply(self, path):
        """binary little-endian PLY: the cloud's row (x y z float, red green blue uchar of `colors`, label int) plus `int count`.  The 23-byte rows are
        packed where the voxels live: one device-to-host copy."""
        M = len(self)
        rows = torch.empty(M, 23, dtype=torch.uint8, device=self.pan.device)
        rows[:, 0:12] = self.points.contiguous().view(torch.uint8).reshape(M, 12)
        rows[:, 12:15] = ply_colors_u8(self.colors)
        rows[:, 15:19] = self.pan.contiguous().view(torch.uint8).reshape(M, 4)
        rows[:, 19:23] = self.count.contiguous().view(torch.uint8).reshape(M, 4)
        header = ('ply\nformat binary_little_endian 1.0\ncomment panst3r_amd voxel cloud, voxel_size %r\nelement vertex %d\nproperty float x\nproperty float y\n'
                  'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nproperty int count\nend_header\n'
                  % (self.voxel_size, M))
        with open(path, 'wb') as f:
            f.write(header.encode('ascii'))
            f.write(rows.cpu().numpy().tobytes())
        return path

    def render(self, cams2world, focals, shape, **kw):
        """engine.render.render_cloud of the voxels; the default point_size is voxel_size, so that neighbouring voxels close up"""
        from .render import render_cloud
        return render_cloud(self, cams2world, focals, shape, **kw)

    def point_labels(self):
        """[M] int32: the voted label of every cloud point; a point left out keeps its own"""
        if self._point_pan is None:
            raise RuntimeError('this voxel cloud does not hold the labels of its points (it was built by hand)')
        pv = self.point_voxel.long()
        if len(self) == 0:
            return self._point_pan.clone()
        return torch.where(pv >= 0, self.pan[pv.clamp(min=0)], self._point_pan)

    def consistent_maps(self):
        """list over views of int32 [H, W]: a kept pixel gets its voxel's voted id, a pixel below the confidence threshold keeps its 2-D id"""
        if self._source is None:
            raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
        flat = torch.cat([v[4].reshape(-1) for v in self._source.views])
        flat[self._point_index] = self.point_labels()
        off = self.view_offsets
        return [flat[off[v]:off[v + 1]].reshape(self._source.shapes[v]) for v in range(len(off) - 1)]


class VoxelComponents:
    """The same-label connected components of a `VoxelCloud`.  Per voxel: component [Mv] int32 (rank of the component, -1 for a void voxel), root [Mv]
    int32 (smallest voxel row of the component, -1 for void).  Per component, in the order of their roots: pan, size (voxels) int32 [C], points int64 [C]
    (cloud points), cell_lo, cell_hi int32 [C,3] (the box in cells, inclusive), box_lo, box_hi float64 [C,3] (the metric box: cell_lo * voxel_size and
    (cell_hi + 1) * voxel_size).  voxel_size and connectivity as they were given."""

    FIELDS = ('component', 'root', 'pan', 'size', 'points', 'cell_lo', 'cell_hi', 'box_lo', 'box_hi')

    def __init__(self, component, root, pan, size, points, cell_lo, cell_hi, box_lo, box_hi, voxel_size, connectivity):
        self.component, self.root, self.pan, self.size, self.points = component, root, pan, size, points
        self.cell_lo, self.cell_hi, self.box_lo, self.box_hi = cell_lo, cell_hi, box_lo, box_hi
        self.voxel_size, self.connectivity = voxel_size, connectivity

    def __len__(self):
        return int(self.pan.shape[0])

    def cpu(self):
        return VoxelComponents(*(getattr(self, k).cpu() for k in self.FIELDS), self.voxel_size, self.connectivity)


def _check_voxel_size(voxel_size):
    vs = float(voxel_size)
    if not (math.isfinite(vs) and vs > 0):
        raise ValueError('voxel_size must be a positive finite number, got %r' % (voxel_size,))
    with np.errstate(over='ignore'):
        inv = float(np.float32(1.0 / vs))
    if not (math.isfinite(inv) and inv > 0):
        raise ValueError('voxel_size %r has no positive finite float32 inverse' % (voxel_size,))
    return vs, inv


def check_status(status):
    """the device status word of one fusion, as it arrives with the result copy: non-zero = an open-addressing table ran full (a kernel gave up instead
    of spinning) and the outputs are not complete"""
    if int(status) != 0:
        raise RuntimeError('voxelize_cloud: an open-addressing table ran full on the device (status %d); no result' % int(status))


@torch.no_grad()
def voxelize_cloud(cloud, voxel_size, *, colors=None, opacity=None):
    """Fuse a device `PanopticCloud` on a grid of cubic cells of edge `voxel_size` (the unit of `cloud.points`) -> `VoxelCloud`.  Per occupied cell:
    mean position and colour of its points, the panoptic id most of them carry (ties to the smallest id; void - ids <= 0 or not among the cloud's
    segments - only wins alone), colour = (1 - opacity) * rgb + opacity * colors[pan] with the cloud's table and opacity unless given.  A point with a
    non-finite coordinate or a cell index beyond +-2^20 is left out and counted in `dropped`.  Voxels come in the order of their first points.
    One host sync.  GPU only: a CPU cloud raises."""
    vs, inv = _check_voxel_size(voxel_size)
    for t in (cloud.points, cloud.rgb, cloud.pan, cloud.index):
        if not t.is_cuda:
            raise RuntimeError('voxelize_cloud got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
    dev = cloud.pan.device
    M = len(cloud)
    src = cloud._source
    infos = cloud.segments
    ids = [int(s['id']) for s in infos]
    ntab = max(ids + [0]) + 1
    if colors is None:
        colors = src.colors if src is not None else default_colors(max(ntab, 2))
    ctab = torch.as_tensor(colors, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
    if not 1 <= ctab.shape[0] <= hip.CLOUD_MAX_COLORS:
        raise ValueError('the colour table must have 1 .. %d rows, got %d' % (hip.CLOUD_MAX_COLORS, ctab.shape[0]))
    if ids and max(ids) >= ctab.shape[0]:
        raise ValueError('segment id %d does not fit the colour table of %d rows' % (max(ids), ctab.shape[0]))
    if opacity is None:
        opacity = 0.5 if cloud.opacity is None else cloud.opacity
    w1, w2 = float(np.float32(1.0 - float(opacity))), float(np.float32(float(opacity)))
    f3 = lambda n: torch.empty(n, 3, dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    common = dict(cameras=cloud.cameras, view_offsets=list(cloud.view_offsets), voxel_size=vs, opacity=float(opacity), point_pan=cloud.pan,
                  point_index=cloud.index, source=src)
    if M == 0:
        return VoxelCloud(f3(0), f3(0), torch.empty(0, **i32), f3(0), torch.empty(0, **i32), torch.empty(0, **i32), torch.empty(0, dtype=torch.int64, device=dev),
                          torch.empty(0, **i32), [], dropped=0, cells=torch.empty(0, 3, **i32), color_table=ctab, **common)
    row = np.full(ntab, -1, dtype=np.int32)
    for r, i in enumerate(ids):
        row[i] = r
    id2row = torch.from_numpy(row).to(dev)
    points, rgb, pan, index = cloud.points.float().contiguous(), cloud.rgb.float().contiguous(), cloud.pan.to(torch.int32).contiguous(), cloud.index.contiguous()
    ws = hip.voxel_workspace(M, dev)
    nwg, counts, base = hip.scan_buffers(dev, M)
    point_voxel = torch.empty(M, **i32)
    out_points, out_rgb, out_colors = f3(M), f3(M), f3(M)
    out_pan, out_votes, out_first = torch.empty(M, **i32), torch.empty(M, **i32), torch.empty(M, dtype=torch.int64, device=dev)
    hip.voxel_insert(points, inv, ws)
    hip.voxel_count(ws, counts)
    hip.cloud_scan(counts, base)
    hip.voxel_rank(ws, base)
    cells = torch.empty(M, 3, **i32)
    hip.vcc_cells(points, ws['first_row'], base[nwg:], inv, cells)           # while the workspace is alive: the cell of every voxel's first point
    hip.voxel_accumulate(points, rgb, pan, inv, id2row, ws, point_voxel)
    hip.voxel_vote(ws)
    mv = base[nwg:]
    hip.voxel_emit(points, index, mv, inv, vs, ws, ctab, w1, w2, out_points, out_rgb, out_pan, out_colors, out_votes, out_first)
    res = torch.cat([mv, ws['status']])
    S = len(infos)
    if S:
        count = torch.empty(S, **i32)
        median = torch.empty(S, 3, dtype=torch.float32, device=dev)
        hip.cloud_segment_median(out_points, out_pan, mv, id2row, S, count, median)      # the cloud's median, over voxel positions
        res = torch.cat([res, count, median.view(torch.int32).reshape(-1)])
    res = res.cpu().numpy()                                                  # the only host sync: Mv, the status words, the segment table
    check_status(res[1])
    Mv, dropped = int(res[0]), int(res[2])
    segments = decode_segments(res, infos, 3)
    return VoxelCloud(out_points[:Mv], out_rgb[:Mv], out_pan[:Mv], out_colors[:Mv], ws['cnt'][:Mv], out_votes[:Mv], out_first[:Mv], point_voxel, segments,
                      dropped=dropped, cells=cells[:Mv], color_table=ctab, **common)


# ---------------------------------------------------------------- connected components of the voxels and label despeckling (csrc/components.hip)
CONNECTIVITIES = (6, 18, 26)


def _check_connectivity(connectivity):
    if connectivity not in CONNECTIVITIES:
        raise ValueError('connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    return int(connectivity)


def _check_min_voxels(min_voxels):
    if isinstance(min_voxels, bool) or int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError('min_voxels must be an integer >= 1, got %r' % (min_voxels,))
    return min(int(min_voxels), 2 ** 31 - 1)


def check_vcc_status(status):
    """the device status word of one labelling, as it arrives with the result copy: non-zero = a table ran full, two voxels share a cell, a cell lies
    outside +-2^20 or a bounded find / union loop gave up; the outputs are not complete"""
    status = int(status)
    if status != 0:
        what = [t for b, t in ((hip.VCC_FULL, 'an open-addressing table ran full'), (hip.VCC_DUPLICATE, 'two voxels share one cell'),
                               (hip.VCC_RANGE, 'a cell lies outside +-2^20'), (hip.VCC_LOOP, 'a find / union loop reached its bound')) if status & b]
        raise RuntimeError('voxel components: %s on the device (status %d); no result' % (', '.join(what) or 'unknown failure', status))


def _vcc_inputs(vox):
    if vox.cells is None:
        raise RuntimeError('this voxel cloud does not hold the cells of its voxels (it was built by hand without `cells`)')
    for t in (vox.cells, vox.pan, vox.count):
        if not t.is_cuda:
            raise RuntimeError('voxel components got a %s tensor: they run on the GPU only (no CPU fallback)' % t.device)
    return vox.cells.to(torch.int32).contiguous(), vox.pan.to(torch.int32).contiguous(), vox.count.to(torch.int32).contiguous()


def _label(cells, pan, count, connectivity, pairs=0):
    """build, link, flatten and number the components of Mv >= 1 voxels -> (workspace, base, component, table); nothing is copied to the host"""
    dev, Mv = pan.device, pan.numel()
    i32 = dict(dtype=torch.int32, device=dev)
    ws = hip.vcc_workspace(Mv, dev, pairs)
    nwg, counts, base = hip.scan_buffers(dev, Mv)
    component = torch.empty(Mv, **i32)
    table = {'root': torch.empty(Mv, **i32), 'pan': torch.empty(Mv, **i32), 'size': torch.empty(Mv, **i32), 'points': torch.empty(Mv, dtype=torch.int64, device=dev),
             'cell_lo': torch.empty(Mv, 3, **i32), 'cell_hi': torch.empty(Mv, 3, **i32)}
    hip.vcc_build(cells, pan, ws)
    hip.vcc_link(cells, pan, connectivity, ws)
    hip.vcc_flatten(count, cells, ws)
    hip.vcc_count(ws, counts)
    hip.cloud_scan(counts, base)
    hip.vcc_rank(pan, ws, base, component, table)
    return ws, base[nwg:], component, table


@torch.no_grad()
def voxel_components(vox, connectivity=26):
    """Split a device `VoxelCloud` into its same-label connected components -> `VoxelComponents`.  Two voxels touch when their cells differ by at most 1 on
    every axis and on exactly one axis (connectivity 6), one or two (18) or one to three (26); a component is a maximal set of voxels of one id > 0 that
    is connected through touching voxels of that id.  Void voxels (id <= 0) belong to none.  One host sync.  GPU only: a CPU cloud raises, and so does
    a cloud without `cells`."""
    connectivity = _check_connectivity(connectivity)
    cells, pan, count = _vcc_inputs(vox)
    dev, Mv = pan.device, pan.numel()
    if Mv == 0:
        e = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
        return VoxelComponents(e(0), e(0), e(0), e(0), e(0, dtype=torch.int64), e(0, 3), e(0, 3), e(0, 3, dtype=torch.float64), e(0, 3, dtype=torch.float64),
                               vox.voxel_size, connectivity)
    ws, c_ptr, component, table = _label(cells, pan, count, connectivity)
    res = torch.cat([c_ptr, ws['status']]).cpu().numpy()                       # the only host sync: C and the status words
    check_vcc_status(res[1])
    C = int(res[0])
    lo, hi = table['cell_lo'][:C], table['cell_hi'][:C]
    vs = float(vox.voxel_size)
    return VoxelComponents(component, ws['root'], table['pan'][:C], table['size'][:C], table['points'][:C], lo, hi, lo.double() * vs, (hi.double() + 1.0) * vs,
                           vox.voxel_size, connectivity)


@torch.no_grad()
def clean_voxel_labels(vox, min_voxels, connectivity=26):
    """Despeckle the labels of a device `VoxelCloud` -> a new `VoxelCloud` (the input is untouched).  Every component of fewer than `min_voxels` voxels
    (`voxel_components` at this connectivity) takes the id that most of its touching voxels in components that are NOT small carry - one vote per
    (voxel of the component, touching voxel) pair, ties to the smallest id - or becomes void (id 0) when it touches none.  One round.  `colors` is
    re-blended with the cloud's table and opacity and the segment table rebuilt; count, votes, points, rgb, first_index and point_voxel are the input's.
    The result's `relabelled` / `floaters` count the voxels that took another id / became void.  One host sync.  GPU only."""
    min_voxels, connectivity = _check_min_voxels(min_voxels), _check_connectivity(connectivity)
    cells, pan, count = _vcc_inputs(vox)
    dev, Mv = pan.device, pan.numel()
    infos = vox.segments
    ids = [int(s['id']) for s in infos]
    ntab = max(ids + [0]) + 1
    ctab = vox._color_table
    if ctab is None:
        ctab = torch.as_tensor(default_colors(max(ntab, 2)), dtype=torch.float32).reshape(-1, 3)
    ctab = ctab.to(dev).contiguous()
    opacity = 0.5 if vox.opacity is None else vox.opacity
    w1, w2 = float(np.float32(1.0 - float(opacity))), float(np.float32(float(opacity)))
    common = dict(cameras=vox.cameras, view_offsets=list(vox.view_offsets), voxel_size=vox.voxel_size, opacity=vox.opacity, point_pan=vox._point_pan,
                  point_index=vox._point_index, source=vox._source, cells=vox.cells, color_table=vox._color_table)
    done = lambda p, c, seg, n: VoxelCloud(vox.points, vox.rgb, p, c, vox.count, vox.votes, vox.first_index, vox.point_voxel, seg, dropped=vox.dropped,
                                           **common)._counts(n)
    if Mv == 0:
        out = done(vox.pan.clone(), vox.colors.clone(), [dict(s) for s in infos], vox)
        out.relabelled = out.floaters = 0
        return out
    rgb = vox.rgb.float().contiguous()
    ws, c_ptr, component, table = _label(cells, pan, count, connectivity, pairs=hip.vcc_pair_capacity(Mv, len(ids) or 26))
    out_pan, out_colors = torch.empty(Mv, dtype=torch.int32, device=dev), torch.empty(Mv, 3, dtype=torch.float32, device=dev)
    hip.vcc_votes(cells, pan, connectivity, min_voxels, ws)
    hip.voxel_vote({'cap': ws['pair_cap'], 'pair_keys': ws['pair_keys'], 'pair_cnt': ws['pair_cnt'], 'best': ws['best']})
    hip.vcc_apply(pan, min_voxels, rgb, ctab, w1, w2, ws, out_pan, out_colors)
    res = ws['status']
    S = len(infos)
    if S:
        row = np.full(ntab, -1, dtype=np.int32)
        for r, i in enumerate(ids):
            row[i] = r
        seg_count = torch.empty(S, dtype=torch.int32, device=dev)
        median = torch.empty(S, 3, dtype=torch.float32, device=dev)
        hip.cloud_segment_median(vox.points.float().contiguous(), out_pan, torch.tensor([Mv], dtype=torch.int32).to(dev), torch.from_numpy(row).to(dev), S, seg_count,
                                 median)                                      # the voxel cloud's median, over the positions of the relabelled voxels
        res = torch.cat([res, seg_count, median.view(torch.int32).reshape(-1)])
    res = res.cpu().numpy()                                                    # the only host sync: the status words, the segment table
    check_vcc_status(res[0])
    segments = []
    if S:
        med = res[4 + S:].view(np.float32).reshape(S, 3)
        for r, s in enumerate(infos):
            if res[4 + r] > 0:
                segments.append(dict(s, count=int(res[4 + r]), median=med[r].copy()))
    out = done(out_pan, out_colors, segments, vox)
    out.relabelled, out.floaters = int(res[1]), int(res[2])
    return out
