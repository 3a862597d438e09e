"""Mesh simplification by vertex clustering on the device (stage f18): the vertices of a mesh that fall into one cubic cell of edge `cell_size` become
ONE vertex - the voxel stage's mean position, mean colour and voted panoptic id - the faces are rewritten onto the new vertices, the ones that
collapsed are dropped and the ones that then coincide are removed.  `cloud.mesh()` is one sheet per view that share no vertex: where the sheets
coincide they are welded, and the new vertex's id is the multi-view vote.

    mesh = cloud.mesh().simplify(0.02)                       # a PanopticMesh a viewer can take; mesh.simplify_stats, mesh.src_face
    small = simplify_mesh(vertices, faces, 0.05)             # raw tensors, for instance a ground-truth mesh of load_ply_mesh

No counterpart in the reference (its demo hands the viewer the raw points): *restated, unpinned*.  The contract is the mesh simplification section of
include/panst3r_hip.h, restated in numpy in tests/simplify_ref.py; csrc/simplify.hip and the voxel kernels it calls are held to it bit for bit.

Limits, on purpose: clustering preserves neither topology nor manifoldness (two sheets closer than a cell merge, a thin wall can become a fin); a
collapse can flip a face's winding and nothing corrects it; the representative is the cell's mean, not a quadric optimum; there is no protection of
boundaries or of label edges; `dedupe` packs a face into 3 x 21 bits and so takes at most 2^21 - 2 new vertices."""
import numpy as np
import torch

from .. import hip
from .voxels import _check_voxel_size, check_status as _check_voxel_status

STAT_KEYS = ('vertices_in', 'vertices_used', 'vertices_left_out', 'vertices_out', 'faces_in', 'faces_left_out', 'faces_degenerate', 'faces_duplicate',
             'faces_out')
MAX_ID_TABLE = 1 << 24              # simplify_mesh(vertex_ids=...): the largest id + 1 it lists


class SimplifiedMesh:
    """what `simplify_mesh` returns: vertices [Mv,3] fp32, faces [F',3] int32 (rows of `vertices`), face_ids [F'] int32, vertex_ids [Mv] int32, colors
    [Mv,3] fp32, cluster [M] int32 (the new row of every input vertex, -1 for an unused one or one left out), src_face [F'] int32 (the input face of
    every output face), stats (the dict of `PanopticMesh.simplify_stats`)."""

    def __init__(self, vertices, faces, face_ids, vertex_ids, colors, cluster, src_face, stats, quad=None):
        self.vertices, self.faces, self.face_ids, self.vertex_ids, self.colors = vertices, faces, face_ids, vertex_ids, colors
        self.cluster, self.src_face, self.stats, self.quad = cluster, src_face, stats, quad

    def __len__(self):
        return int(self.faces.shape[0])


def check_cell_size(cell_size):
    """-> (cell_size, float32 inverse) or ValueError: a positive finite number with a positive finite float32 inverse"""
    if isinstance(cell_size, bool) or not isinstance(cell_size, (int, float, np.integer, np.floating)):
        raise ValueError('cell_size must be a positive finite number, got %r' % (cell_size,))
    try:
        return _check_voxel_size(cell_size)
    except ValueError as e:
        raise ValueError(str(e).replace('voxel_size', 'cell_size')) from None


def check_dedupe_cap(vertices_out, cell_size):
    """dedupe keys a face by its three new vertex rows in 21 bits each"""
    if vertices_out > hip.SIMPLIFY_MAX_KEYED:
        raise ValueError('simplify: cell_size %r leaves %d vertices, more than the 2^21 - 2 = %d that dedupe=True takes (a face is keyed by 3 x 21 bits): '
                         'use a larger cell_size, or dedupe=False' % (cell_size, vertices_out, hip.SIMPLIFY_MAX_KEYED))


def check_simplify_status(status):
    """the device status word of one simplification, as it arrives with a result copy"""
    status = int(status)
    if status & hip.SIMPLIFY_RANGE:
        raise ValueError('simplify: a face names a vertex outside the vertex rows (status %d); no result' % status)
    if status:
        raise RuntimeError('simplify: the face table ran full on the device (status %d); no result' % status)


def _stats(M, F, used=0, left=0, vout=0, f_left=0, f_deg=0, f_dup=0, f_out=0):
    return dict(zip(STAT_KEYS, (int(M), int(used), int(left), int(vout), int(F), int(f_left), int(f_deg), int(f_dup), int(f_out))))


@torch.no_grad()
def _simplify(vertices, colors, vertex_ids, faces, quad, id2row, cell_size, inv, dedupe):
    """the five steps on device tensors (vertices, colors fp32 [M,3], vertex_ids int32 [M], faces int32 [F,3], quad int64 [F], id2row int32: all
    contiguous) -> `SimplifiedMesh` with quad.  Two host syncs: the new vertex count (the 2^21 cap is refused before any face is rewritten, a bad
    corner as well), then the face count."""
    M, F, dev = int(vertices.shape[0]), int(faces.shape[0]), faces.device
    i32 = dict(dtype=torch.int32, device=dev)
    f3 = lambda n: torch.empty(n, 3, dtype=torch.float32, device=dev)

    def empty(stats, cluster=None):
        return SimplifiedMesh(f3(0), torch.empty(0, 3, **i32), torch.empty(0, **i32), torch.empty(0, **i32), f3(0),
                              torch.full((M,), -1, **i32) if cluster is None else cluster, torch.empty(0, **i32), stats,
                              torch.empty(0, dtype=torch.int64, device=dev))
    if F == 0:
        return empty(_stats(M, 0))
    if M == 0:
        raise ValueError('simplify: %d faces on a mesh without vertices' % F)
    ws = hip.simplify_workspace(M, F, dev)
    masked = f3(M)
    hip.simplify_used(faces, ws)
    hip.simplify_mask(vertices, ws, masked)
    # step 2: the voxel stage on the masked vertices (an unused vertex is NaN there: left out, its cluster -1)
    vws = hip.voxel_workspace(M, dev)
    nwg, counts, base = hip.scan_buffers(dev, M)
    cluster = torch.empty(M, **i32)
    out_points, out_rgb, out_colors = f3(M), f3(M), f3(M)
    out_ids, out_votes, out_first = torch.empty(M, **i32), torch.empty(M, **i32), torch.empty(M, dtype=torch.int64, device=dev)
    hip.voxel_insert(masked, inv, vws)
    hip.voxel_count(vws, counts)
    hip.cloud_scan(counts, base)
    hip.voxel_rank(vws, base)
    hip.voxel_accumulate(masked, colors, vertex_ids, inv, id2row, vws, cluster)
    hip.voxel_vote(vws)
    mv = base[nwg:]
    rows = torch.arange(M, dtype=torch.int64, device=dev)                       # the `index` of the voxel stage: out_first = the first member row
    palette = torch.zeros(1, 3, dtype=torch.float32, device=dev)                # palette weight 0: the colour is the mean itself
    hip.voxel_emit(masked, rows, mv, inv, cell_size, vws, palette, 1.0, 0.0, out_points, out_rgb, out_ids, out_colors, out_votes, out_first)
    res = torch.cat([mv, vws['status'], ws['status']]).tolist()                 # host sync 1: Mv, the voxel status words, the simplify status words
    Mv, used = res[0], res[4]
    check_simplify_status(res[3])
    _check_voxel_status(res[1])
    left = res[2] - (M - used)                                                  # the voxel stage counted the unused vertices as left out as well
    if Mv == 0:
        return empty(_stats(M, F, used, left, 0, F), cluster)
    if dedupe:
        check_dedupe_cap(Mv, cell_size)
        hip.simplify_table(ws)
    # steps 3-5
    fn, fcounts, fbase = hip.scan_buffers(dev, F, hip.SURFACE_WG)
    out_faces, out_face_ids, out_quad, src_face = torch.empty(F, 3, **i32), torch.empty(F, **i32), torch.empty(F, dtype=torch.int64, device=dev), torch.empty(F, **i32)
    hip.simplify_remap(faces, cluster, Mv, dedupe, ws)
    hip.simplify_count(dedupe, ws, fcounts)
    hip.cloud_scan(fcounts, fbase)
    hip.simplify_emit(faces, quad, cluster, out_ids, Mv, dedupe, ws, fbase, out_faces, out_face_ids, out_quad, src_face)
    res = torch.cat([fbase[fn:], ws['status']]).tolist()                        # host sync 2: F' and the face counts
    check_simplify_status(res[1])
    Fo, f_left, f_deg, cand = res[0], res[3], res[4], res[5]
    if Fo == 0:                                                                 # every face collapsed: no face names a vertex any more, none is kept
        return empty(_stats(M, F, used, left, 0, f_left, f_deg, cand, 0))
    stats = _stats(M, F, used, left, Mv, f_left, f_deg, cand - Fo, Fo)
    return SimplifiedMesh(out_points[:Mv], out_faces[:Fo], out_face_ids[:Fo], out_ids[:Mv], out_rgb[:Mv], cluster, src_face[:Fo], stats, out_quad[:Fo])


def _id2row(ids, device):
    """the table of the voxel stage's vote: id -> a row >= 0 where the id is listed, -1 where not"""
    ntab = max(list(ids) + [0]) + 1
    row = np.full(ntab, -1, dtype=np.int32)
    for r, i in enumerate(ids):
        row[i] = r
    return torch.from_numpy(row).to(device)


def simplify_panoptic_mesh(mesh, cell_size, *, dedupe=True):
    """`PanopticMesh.simplify`: see there"""
    from .surface import PanopticMesh
    cell_size, inv = check_cell_size(cell_size)
    mesh._on_device('PanopticMesh.simplify')
    dev = mesh.faces.device
    ids = [int(s['id']) for s in mesh.segments]
    if ids and (min(ids) < 0 or max(ids) >= MAX_ID_TABLE):
        raise ValueError('simplify: segment ids must lie in [0, 2^24), got %d .. %d' % (min(ids), max(ids)))
    r = _simplify(mesh.vertices.float().contiguous(), mesh.colors.float().contiguous(), mesh.vertex_ids.to(torch.int32).contiguous(),
                  mesh.faces.to(torch.int32).contiguous(), mesh.quad.to(torch.int64).contiguous(), _id2row(ids, dev), cell_size, inv, bool(dedupe))
    out = PanopticMesh(r.vertices, r.faces, r.face_ids, r.vertex_ids, r.colors, r.quad, list(mesh.view_offsets), mesh.segments, mesh.cameras)
    out.simplify_stats, out.src_face, out.cluster = r.stats, r.src_face, r.cluster
    return out


def simplify_mesh(vertices, faces, cell_size, *, colors=None, vertex_ids=None, dedupe=True):
    """Simplify a raw triangle mesh on the device by vertex clustering at `cell_size` (the unit of `vertices`) -> `SimplifiedMesh`.  vertices [M,3]
    floating point, faces [F,3] integer rows of it; colors [M,3] in [0, 1] (default: black), vertex_ids [M] integer panoptic ids (default: every vertex
    id 0; given, every id > 0 is listed and votes, ids <= 0 are void - one more host sync, for the largest id, which must be below 2^24).  The steps are
    `PanopticMesh.simplify`'s.  GPU only: CPU tensors raise."""
    cell_size, inv = check_cell_size(cell_size)
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.dtype.is_floating_point:
        raise ValueError('vertices must be a floating-point [M, 3] tensor')
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('faces must be an int32 or int64 [F, 3] tensor')
    M, F = int(vertices.shape[0]), int(faces.shape[0])
    if colors is not None and (not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (M, 3) or not colors.dtype.is_floating_point):
        raise ValueError('colors must be a floating-point [%d, 3] tensor' % M)
    if vertex_ids is not None and (not isinstance(vertex_ids, torch.Tensor) or tuple(vertex_ids.shape) != (M,) or vertex_ids.dtype not in (torch.int32, torch.int64)):
        raise ValueError('vertex_ids must be an int32 or int64 [%d] tensor' % M)
    for t in (vertices, faces, colors, vertex_ids):
        if t is not None and not t.is_cuda:
            raise RuntimeError('simplify_mesh got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
    dev = faces.device
    if faces.dtype == torch.int64:                                              # an index beyond int32 must stay out of range, not wrap into it
        faces = faces.clamp(-1, 2 ** 31 - 1)
    ntab = 1
    if vertex_ids is not None and M:
        top = int(vertex_ids.max())
        if top >= MAX_ID_TABLE:
            raise ValueError('simplify_mesh: vertex ids must be below 2^24, got %d' % top)
        ntab = max(top, 0) + 1
    id2row = torch.zeros(ntab, dtype=torch.int32, device=dev)                  # every id of the table is listed (id 0 is void by the vote's rule)
    colors = torch.zeros(M, 3, dtype=torch.float32, device=dev) if colors is None else colors.float().contiguous()
    vertex_ids = torch.zeros(M, dtype=torch.int32, device=dev) if vertex_ids is None else vertex_ids.clamp(min=-1).to(torch.int32).contiguous()
    return _simplify(vertices.float().contiguous(), colors, vertex_ids, faces.to(torch.int32).contiguous(), torch.zeros(F, dtype=torch.int64, device=dev),
                     id2row, cell_size, inv, bool(dedupe))
