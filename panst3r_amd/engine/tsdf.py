"""One fused surface out of all views (stage f15): `cloud.mesh()` triangulates each view's pointmap grid on its own, so a wall seen by eight views is
eight overlapping sheets.  `fuse_surface` averages the views' depths in a volume instead - a truncated signed distance on the lattice nodes around the
occupied voxels, every view contributing along its own rays, free space carved by the views that see through it - and extracts ONE sheet by naive
surface nets: a `FusedMesh`, which is a `PanopticMesh` and goes wherever one goes (render, write_ply, drop_small, score_reconstruction, evaluate_3d).

    cloud, cameras, pan_preds = model.reconstruct(imgs, true_shape, classes)
    mesh = cloud.fused_mesh(0.02).drop_small(64)

No counterpart in the reference: *restated, unpinned*.  The contract is the tsdf section of include/panst3r_hip.h, restated in numpy in
tests/tsdf_ref.py; csrc/tsdf.hip is held to it bit for bit (separately rounded fp32 operations, fp64 crossings in a stated order, no float atomics).

What it does not do: no confidence weighting of a view (every measured pair counts once), no bilinear sampling of the depth (the nearest pixel centre),
no marching-cubes case table (one vertex per surface cell, so thin features collapse), no vertex normals of its own (stage f17 computes area-weighted
ones on demand: `mesh.vertex_normals()`, engine/shade.py).  Cells exist only where the cloud has points +- band: a hole in the cloud is a hole in the mesh."""
import numpy as np
import torch

from .. import hip
from .consistency import own_camera_table
from .surface import PanopticMesh
from .voxels import _check_voxel_size


class FusedMesh(PanopticMesh):
    """A `PanopticMesh` whose vertices are the surface cells of the fused volume: vertices [Nv,3] fp32, vertex_ids [Nv] int32 and colors [Nv,3] of a
    voxel at or next to the cell, faces [F,3] int32 wound so that the normal points from inside to outside (towards the cameras), face_ids [F] int32
    (the id two of its corners share, else 0), quad [F] int64 = 3 rank + axis of the lattice edge the face crosses (the node `rank` of `nodes`, the
    edge running along +axis from it), in the order rank, axis, first triangle before second.  Also the volume itself, in the nodes' canonical order:
    nodes int32 [Nn,3] (the node n sits at n * voxel_size), sdf fp32 [Nn] (the mean truncated distance, 0 where no view measured), weight int32 [Nn]
    (the views that measured), and tsdf_stats = {'active_nodes', 'valid_nodes', 'surface_cells'}; voxel_size, band, min_weight as they were given."""

    def __init__(self, vertices, faces, face_ids, vertex_ids, colors, quad, view_offsets, segments, cameras=None, *, nodes, sdf, weight, tsdf_stats, voxel_size,
                 band, min_weight):
        super().__init__(vertices, faces, face_ids, vertex_ids, colors, quad, view_offsets, segments, cameras)
        self.nodes, self.sdf, self.weight, self.tsdf_stats = nodes, sdf, weight, tsdf_stats
        self.voxel_size, self.band, self.min_weight = voxel_size, band, min_weight

    def _volume(self, f=lambda t: t):
        return dict(nodes=f(self.nodes), sdf=f(self.sdf), weight=f(self.weight), tsdf_stats=dict(self.tsdf_stats), voxel_size=self.voxel_size, band=self.band,
                    min_weight=self.min_weight)

    def _with_faces(self, faces, face_ids, quad):
        return FusedMesh(self.vertices, faces, face_ids, self.vertex_ids, self.colors, quad, list(self.view_offsets), self.segments, self.cameras, **self._volume())

    def cpu(self):
        f = lambda t: t.cpu()
        return FusedMesh(f(self.vertices), f(self.faces), f(self.face_ids), f(self.vertex_ids), f(self.colors), f(self.quad), list(self.view_offsets),
                         [dict(s) for s in self.segments], self.cameras, **self._volume(f))


def check_fuse_arguments(voxel_size, band=2, min_weight=1):
    """-> (voxel size as a float, band, min_weight), or ValueError"""
    vs, _ = _check_voxel_size(voxel_size)
    with np.errstate(over='ignore'):
        vs32 = np.float32(vs)
    if not (np.isfinite(vs32) and vs32 > 0):
        raise ValueError('voxel_size %r is no positive finite float32' % (voxel_size,))
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or not 1 <= band <= hip.TSDF_MAX_BAND:
        raise ValueError('band must be an integer in 1 .. %d, got %r' % (hip.TSDF_MAX_BAND, band))
    if isinstance(min_weight, bool) or not isinstance(min_weight, (int, np.integer)) or not 1 <= min_weight <= 2 ** 31 - 1:
        raise ValueError('min_weight must be an integer >= 1, got %r' % (min_weight,))
    return vs, int(band), int(min_weight)


def fused_mesh_keywords(fused_mesh):
    """the `fused_mesh=` argument of `PanSt3R.reconstruct` -> None (off) or the keywords of `fuse_surface` (voxel_size among them), checked"""
    if fused_mesh is None:
        return None
    if isinstance(fused_mesh, dict):
        kw = dict(fused_mesh)
        if 'voxel_size' not in kw or set(kw) - {'voxel_size', 'band', 'min_weight', 'pp', 'near'}:
            raise ValueError('fused_mesh as a dict holds voxel_size and optionally band, min_weight, pp, near; got %r' % (fused_mesh,))
    elif isinstance(fused_mesh, bool) or not isinstance(fused_mesh, (int, float, np.integer, np.floating)):
        raise ValueError('fused_mesh must be None, a voxel size or a dict of the keywords of fuse_surface; got %r' % (fused_mesh,))
    else:
        kw = {'voxel_size': fused_mesh}
    check_fuse_arguments(kw['voxel_size'], kw.get('band', 2), kw.get('min_weight', 1))
    return kw


def check_tsdf_status(status):
    """the device status word of one fusion, as it arrives with a result copy: non-zero = a node lies outside +-2^20 or the node table ran full; the
    outputs are not complete"""
    status = int(status)
    if status != 0:
        what = [t for b, t in ((hip.TSDF_FULL, 'the node table ran full'), (hip.TSDF_RANGE, 'a lattice node lies outside +-2^20')) if status & b]
        raise RuntimeError('fuse_surface: %s on the device (status %d); no result' % (', '.join(what) or 'unknown failure', status))


@torch.no_grad()
def fuse_surface(cloud, voxel_size, *, band=2, min_weight=1, vox=None, pp=None, near=1e-3):
    """Fuse the views of a device `PanopticCloud` into one surface -> `FusedMesh`.  The cloud must still hold its source (its views, cameras, focals
    and confidence threshold, as `cloud.consistency()` uses them).  `vox`: the cloud's `VoxelCloud` at `voxel_size` (built here if not given; it must
    hold its integer `cells`).  Around every occupied cell the (2 band)^3 nearest lattice nodes are active; a node p seen by view j at depth zc, where
    j measured the depth d (the nearest pixel centre; pp, near as `view_consistency`), contributes s = d - zc clamped to +band * voxel_size, unless
    s < -band * voxel_size (the node is hidden behind what j saw: nothing is known).  The node's distance is the mean over its `weight` contributing
    views; it is valid with weight >= min_weight.  A view that sees THROUGH a node pulls it outside: floaters that one view put into free space are
    carved away by the others.  One vertex per cell whose eight corners are valid and change sign (the mean of the sign changes along its edges), two
    triangles per lattice edge that changes sign, normals towards the cameras; the id and colour of a vertex are those of the voxel at its cell,
    else of the fullest neighbouring voxel.  `band` = 2 (1 .. 4) and `min_weight` = 1 are CHOICES, not measured optima, like `rel_tol` of the
    consistency check and `max_depth_ratio` of `cloud.mesh()`: a wider band bridges more depth noise and costs (2 band)^3 nodes per voxel.
    An empty cloud, or a volume without a surface cell, gives a mesh of zero faces.  THREE host syncs: the number of nodes, the number of vertices,
    and the number of faces together with the status word (the voxel fusion adds its own one when `vox` is not given).  GPU only: a CPU cloud raises."""
    vs, band, min_weight = check_fuse_arguments(voxel_size, band, min_weight)
    src = getattr(cloud, '_source', None)
    if src is None:
        raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
    if not cloud.pan.is_cuda:
        raise RuntimeError('fuse_surface got a %s cloud: it runs on the GPU only (no CPU fallback)' % cloud.pan.device)
    if src.focals is None:
        raise ValueError('fuse_surface needs the focals of the cloud: build it with panoptic_point_cloud(..., focals)')
    if vox is None:
        vox = cloud.voxelize(vs)
    elif float(vox.voxel_size) != vs:
        raise ValueError('the voxel cloud was built at voxel_size %r, not %r' % (vox.voxel_size, vs))
    if vox.cells is None:
        raise RuntimeError('this voxel cloud does not hold the cells of its voxels (it was built by hand without `cells`)')
    for t in (vox.cells, vox.pan, vox.count, vox.colors):
        if not t.is_cuda:
            raise RuntimeError('fuse_surface got a %s voxel cloud: it runs on the GPU only (no CPU fallback)' % t.device)
    dev, Mv = cloud.pan.device, len(vox)
    i32 = dict(dtype=torch.int32, device=dev)
    e = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
    volume = dict(voxel_size=vs, band=band, min_weight=min_weight)
    vs32 = float(np.float32(vs))                                                # the contract's vs: the lattice spacing as the kernels see it

    def result(vertices, vertex_ids, colors, faces, face_ids, edge, nodes, sdf, weight, stats):
        return FusedMesh(vertices, faces, face_ids, vertex_ids, colors, edge, list(cloud.view_offsets), cloud.segments, cloud.cameras, nodes=nodes, sdf=sdf,
                         weight=weight, tsdf_stats=stats, **volume)

    def no_faces(nodes, sdf, weight, stats):
        return result(e(0, 3, dtype=torch.float32), e(0), e(0, 3, dtype=torch.float32), e(0, 3), e(0), e(0, dtype=torch.int64), nodes, sdf, weight, stats)
    if Mv == 0:
        return no_faces(e(0, 3), e(0, dtype=torch.float32), e(0), {'active_nodes': 0, 'valid_nodes': 0, 'surface_cells': 0})
    P = hip.tsdf_pairs(Mv, band)
    if P > hip.TSDF_MAX_PAIRS:
        raise ValueError('%d voxels at band %d are %d (voxel, offset) pairs: more than the 2^30 - 1 the kernels take' % (Mv, band, P))
    cells = vox.cells.to(torch.int32).contiguous()
    ws = hip.tsdf_workspace(Mv, band, dev)
    nwg, counts, base = hip.scan_buffers(dev, P)
    hip.tsdf_insert(cells, band, ws)
    hip.voxel_count(ws, counts)                                                 # a pair is a point, a node a voxel: ranks in the order of the first pairs
    hip.cloud_scan(counts, base)
    hip.voxel_rank(ws, base)
    Nn, status = torch.cat([base[nwg:], ws['status'][:1]]).tolist()            # host sync 1: the number of nodes (with the status of the insert)
    check_tsdf_status(status)
    # the depth planes of the cloud's own views at its own threshold, as cloud.consistency() takes them
    shapes, V = src.shapes, len(src.views)
    views = [(conf, pts, loc, None) for conf, pts, loc, _, _ in src.views]
    table, camd, dims, vwg, N = hip.consist_view_table(views, src.c34, own_camera_table(src.cams2world, src.focals, shapes, pp, near), shapes, dev)
    depth = e(N, dtype=torch.float32)
    hip.consist_depth(table, camd, V, vwg, float(cloud.min_conf_thr), src.local_pointmaps, depth)
    nodes, voxel_row = e(Nn, 3), torch.full((Nn,), -1, **i32)
    sdf, weight = e(Nn, dtype=torch.float32), e(Nn)
    hip.tsdf_nodes(cells, band, Nn, ws, nodes, voxel_row)
    hip.tsdf_integrate(nodes, vs32, band, table, camd, dims, V, depth, sdf, weight)
    cell_vertex, face_mask = e(Nn), e(Nn)
    nwg, counts, base = hip.scan_buffers(dev, Nn)
    hip.tsdf_cells(nodes, ws, sdf, weight, min_weight, cell_vertex, counts)
    hip.cloud_scan(counts, base)
    Nv, valid, status = torch.cat([base[nwg:], (weight >= min_weight).sum(dtype=torch.int32).reshape(1), ws['status'][:1]]).tolist()      # host sync 2: the number of vertices
    check_tsdf_status(status)
    stats = {'active_nodes': Nn, 'valid_nodes': valid, 'surface_cells': Nv}
    if Nv == 0:
        return no_faces(nodes, sdf, weight, stats)
    vertices, vertex_ids, colors = e(Nv, 3, dtype=torch.float32), e(Nv), e(Nv, 3, dtype=torch.float32)
    hip.tsdf_vertices(nodes, ws, sdf, weight, min_weight, voxel_row, vox.count.to(torch.int32).contiguous(), vox.pan.to(torch.int32).contiguous(),
                      vox.colors.float().contiguous(), vs32, base, cell_vertex, vertices, vertex_ids, colors)
    fbase = torch.empty_like(base)
    hip.tsdf_face_count(nodes, ws, sdf, weight, min_weight, cell_vertex, face_mask, counts)
    hip.cloud_scan(counts, fbase)
    faces, face_ids, edge = e(6 * Nv, 3), e(6 * Nv), e(6 * Nv, dtype=torch.int64)         # an edge has four surface cells, a cell twelve edges: F <= 6 Nv
    hip.tsdf_face_emit(nodes, ws, sdf, cell_vertex, face_mask, vertex_ids, fbase, faces, face_ids, edge)
    F, status = torch.cat([fbase[nwg:], ws['status'][:1]]).tolist()            # host sync 3: the number of faces and the status word
    check_tsdf_status(status)
    return result(vertices, vertex_ids, colors, faces[:F], face_ids[:F], edge[:F], nodes, sdf, weight, stats)
