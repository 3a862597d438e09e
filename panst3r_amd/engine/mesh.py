"""Ground truth out of a labelled mesh (stage f8): a triangle mesh with one panoptic id per vertex (or per face) rasterised from any pinhole camera
into depth, face index and id per pixel, and - after the per-view minimum-area filter - the `gt_maps, gt_segments` pair that `panoptic_quality` /
`PanSt3R.evaluate` take.  Mesh, cameras and annotations in, PQ out, all on the device:

    verts, faces = load_ply_mesh(path); segments, ids = panoptic_vertex_ids(seg_indices, seg_groups, label2id)
    gt_maps, gt_segments, depths = ground_truth_maps(verts.cuda(), faces.cuda(), ids, segments, cameras)
    model.evaluate(pan_preds, gt_maps, gt_segments)

The reference produces these maps in tools/preprocess_scannetpp.py:395-494 through pyrender / OpenGL (SKIP_CULL_FACES | SEG_VERT, znear 0.05, zfar 20,
ids with fewer than MIN_INST_AREA = 50 pixels in a view become void), which a ROCm compute node does not offer: *restated, unpinned*.  The contract is
the mesh section of include/panst3r_hip.h, restated in numpy in tests/mesh_ref.py; csrc/mesh.hip is held to it bit for bit (fixed-point coverage with
the top-left rule, fp64 perspective-correct depth rounded once, integer atomics only).  A stated limit: a face with a vertex nearer than `near` (or
behind the camera) is left out whole - there is no near-plane clipping."""
import math
import struct

import numpy as np
import torch

from .. import hip
from .render import ZBUF_BYTES, _host64, image_shape, one_camera, world_to_camera, zbuf_chunks


class MeshRender:
    """B views of one mesh at one shape: depth [B,H,W] fp32 (the camera-frame z of the nearest face at the pixel centre, 0 where none), face [B,H,W]
    int64 (its row in `faces`, -1 where none), pan [B,H,W] int32 (its id, 0 where none)."""

    def __init__(self, depth, face, pan):
        self.depth, self.face, self.pan = depth, face, pan

    def __len__(self):
        return int(self.face.shape[0])

    @property
    def hit(self):
        """[B,H,W] bool: a face covers the pixel"""
        return self.face >= 0

    def cpu(self):
        return MeshRender(self.depth.cpu(), self.face.cpu(), self.pan.cpu())

    def __getitem__(self, b):
        """the render of camera b alone, [1,H,W] views"""
        s = one_camera(b, len(self))
        return MeshRender(self.depth[s], self.face[s], self.pan[s])


def mesh_camera_table(cams2world, focals, shape, pp=None):
    """the float32 [B, 16] table of the mesh kernels (include/panst3r_hip.h, mesh step 1) of B camera-to-world matrices, on the host in float64: per
    camera the rows of [R^T | -R^T t] rounded to float32 exactly as `camera_table` does, then fx, fy, cx, cy.  focals: one number, one per camera, or
    (fx, fy) pairs ([B, 2], or [1, 2] for all); pp: (cx, cy), one pair or one per camera, default (W / 2, H / 2).  Raises ValueError for anything
    unusable."""
    rows, p = world_to_camera(cams2world, shape, pp, 'render_mesh')
    B = rows.shape[0]
    f = _host64(focals)
    if f.ndim == 2 and f.shape[1] == 2 and f.shape[0] in (1, B):
        f = np.broadcast_to(f, (B, 2))
    elif f.size == 1:
        f = np.full((B, 2), float(f.reshape(-1)[0]))
    elif f.ndim == 1 and f.size == B:
        f = np.stack([f, f], axis=1)
    else:
        raise ValueError('focals must be one number, one per camera or (fx, fy) pairs [B, 2], got shape %s for %d cameras' % (tuple(f.shape), B))
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError('focals must be positive finite numbers, got %s' % (f.tolist(),))
    tab = np.empty((B, hip.MESH_CAM_FLOATS), dtype=np.float32)
    with np.errstate(over='ignore'):
        tab[:, :12], tab[:, 12:14], tab[:, 14:16] = rows, f, p
    if not (np.isfinite(tab).all() and (tab[:, 12:14] > 0).all()):
        raise ValueError('a camera does not fit float32 (matrix, focals or principal point)')
    return tab


def _check_planes(near, far):
    nr, fr = float(near), float(far)
    with np.errstate(over='ignore'):
        n32, f32 = np.float32(nr), np.float32(fr)
    if not (math.isfinite(nr) and math.isfinite(fr) and np.isfinite(f32) and 0 < n32 < f32):
        raise ValueError('near and far must be finite float32 with 0 < near < far, got %r, %r' % (near, far))
    return float(n32), float(f32)


def _check_mesh(vertices, faces, vertex_ids, face_ids):
    for name, t in (('vertices', vertices), ('faces', faces), ('vertex_ids', vertex_ids), ('face_ids', face_ids)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise ValueError('%s must be a torch tensor, got %s' % (name, type(t).__name__))
    if vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.dtype.is_floating_point:
        raise ValueError('vertices must be a floating-point [Nv, 3] tensor, got %s %s' % (vertices.dtype, tuple(vertices.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('faces must be an int32 / int64 [Nf, 3] tensor, got %s %s' % (faces.dtype, tuple(faces.shape)))
    Nv, Nf = int(vertices.shape[0]), int(faces.shape[0])
    if not (1 <= Nv <= 2 ** 31 - 1 and 1 <= Nf <= 2 ** 31 - 1):
        raise ValueError('a mesh has 1 .. 2^31 - 1 vertices and faces, got %d and %d' % (Nv, Nf))
    if vertex_ids is not None and face_ids is not None:
        raise ValueError('give vertex_ids or face_ids, not both')
    for name, t, n in (('vertex_ids', vertex_ids, Nv), ('face_ids', face_ids, Nf)):
        if t is not None and (t.dim() != 1 or t.shape[0] != n or t.dtype.is_floating_point or t.dtype == torch.bool):
            raise ValueError('%s must be an integer [%d] tensor, got %s %s' % (name, n, t.dtype, tuple(t.shape)))
    return Nv, Nf


@torch.no_grad()
def render_mesh(vertices, faces, cams2world, focals, shape, *, vertex_ids=None, face_ids=None, pp=None, near=0.05, far=20.0):
    """Rasterise a device mesh (vertices [Nv,3] float, faces [Nf,3] int, world frame) from B cameras at one output shape (H, W) -> `MeshRender`.
    cams2world: [B,4,4] or a list of [4,4] camera-to-world matrices (x right, y down, z forward); focals: pixels - one number, one per camera, or
    (fx, fy) pairs; pp: principal point(s) (cx, cy), default (W / 2, H / 2).  Per pixel centre the nearest face between `near` and `far` wins (equal
    depths: the smallest face index); both sides of a face are seen (no culling).  `face_ids` [Nf] gives the pixel its face's id, `vertex_ids` [Nv]
    the id of the face's nearest corner (never a blend); with neither `pan` is all zero.  A face with a vertex behind `near`, a non-finite vertex or
    an index outside the vertices is left out whole (no near-plane clipping).  Cameras are taken in chunks so that the z-buffer stays under
    `ZBUF_BYTES`.  No host sync when the cameras are host values.  GPU only: CPU tensors raise."""
    H, W = image_shape(shape)
    Nv, Nf = _check_mesh(vertices, faces, vertex_ids, face_ids)
    tab = mesh_camera_table(cams2world, focals, (H, W), pp)
    near, far = _check_planes(near, far)
    for t in (vertices, faces, vertex_ids, face_ids):
        if t is not None and not t.is_cuda:
            raise RuntimeError('render_mesh got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
    dev = vertices.device
    B = tab.shape[0]
    verts = vertices.float().contiguous()
    if faces.dtype == torch.int64:                                            # an index that does not fit int32 is outside the vertices: keep it so
        faces = torch.where((faces < 0) | (faces >= Nv), torch.full_like(faces, -1), faces)
    faces = faces.to(torch.int32).contiguous()
    vid = None if vertex_ids is None else vertex_ids.to(torch.int32).contiguous()
    fid = None if face_ids is None else face_ids.to(torch.int32).contiguous()
    cams = torch.from_numpy(tab).to(dev)
    out = MeshRender(torch.empty(B, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.int64, device=dev),
                     torch.empty(B, H, W, dtype=torch.int32, device=dev))
    ws = None
    for b0, b1, z in zbuf_chunks(B, H, W, dev, ZBUF_BYTES):
        if ws is None:
            ws = hip.mesh_workspace(b1 - b0, Nf, dev)                         # the first chunk is the largest
        hip.mesh_raster(verts, faces, cams[b0:b1], H, W, near, far, z, ws)
        hip.mesh_resolve(z, verts, faces, cams[b0:b1], near, vid, fid, out.face[b0:b1], out.depth[b0:b1], out.pan[b0:b1])
    return out


def _segment_rows(segments):
    ids, cats = [], []
    for s in segments:
        if 'category_id' not in s and 'class_id' not in s:
            raise ValueError("ground_truth_maps: segment %r has neither 'category_id' nor 'class_id'" % (s.get('id'),))
        ids.append(int(s['id']))
        cats.append(int(s['category_id'] if 'category_id' in s else s['class_id']))
    if len(set(ids)) != len(ids) or any(not 0 < i < hip.EVAL_MAX_ID for i in ids):
        raise ValueError('ground_truth_maps: the ids of the segments must be unique and in (0, %d), got %s' % (hip.EVAL_MAX_ID, sorted(ids)[:8]))
    tab = np.full(max(ids + [0]) + 1, -1, dtype=np.int32)
    tab[ids] = np.arange(len(ids), dtype=np.int32)
    return ids, cats, tab


def _camera_fields(c):
    if 'fx' in c:
        return (float(c['fx']), float(c['fy'])), (float(c['cx']), float(c['cy']))
    h, w = int(c['height']), int(c['width'])
    return (float(c['focal']), float(c['focal'])), (w / 2, h / 2)              # reconstruct()'s camera dicts: one focal, the principal point centred


@torch.no_grad()
def ground_truth_maps(vertices, faces, vertex_ids, segments, cameras, *, min_area=50, near=0.05, far=20.0):
    """The ground truth of a labelled mesh for `panoptic_quality`: -> (gt_maps, gt_segments, depths), lists aligned with `cameras` of device int32 [H, W]
    id maps and fp32 [H, W] depth maps (0 where no face), and the segments that own a pixel of some map.  vertex_ids: one panoptic id per vertex (a
    tensor or an array, as `panoptic_vertex_ids` returns it); segments: dicts with 'id' and 'category_id' (the reference's 'class_id' is accepted) - an
    id that is not among them renders as void.  cameras: `reconstruct`'s camera dicts ('cam2world', 'focal', 'height', 'width') or dicts with
    'cam2world', 'fx', 'fy', 'cx', 'cy', 'height', 'width'; they are grouped by shape, one `render_mesh` call per shape.  A listed id with fewer than
    `min_area` pixels in a view becomes void in that view (the reference's MIN_INST_AREA).  `gt_segments` are {'id', 'category_id', 'area'} in the order
    of `segments`, ids unchanged.  One host sync."""
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or not 0 <= min_area <= 2 ** 31 - 1:
        raise ValueError('min_area must be an integer in 0 .. 2^31 - 1, got %r' % (min_area,))
    cameras = list(cameras)
    if not cameras:
        raise ValueError('ground_truth_maps needs at least one camera')
    ids, cats, tab = _segment_rows(segments)
    S = len(ids)
    if not isinstance(vertex_ids, torch.Tensor):
        vertex_ids = torch.from_numpy(np.ascontiguousarray(np.asarray(vertex_ids)))
        if isinstance(vertices, torch.Tensor):
            vertex_ids = vertex_ids.to(vertices.device)
    groups = {}
    for k, c in enumerate(cameras):
        groups.setdefault((int(c['height']), int(c['width'])), []).append(k)
    maps, depths, counts = [None] * len(cameras), [None] * len(cameras), [None] * len(cameras)
    id2row = None
    for shape, ks in groups.items():
        fields = [_camera_fields(cameras[k]) for k in ks]
        r = render_mesh(vertices, faces, [cameras[k]['cam2world'] for k in ks], [f for f, _ in fields], shape, vertex_ids=vertex_ids,
                        pp=[p for _, p in fields], near=near, far=far)
        dev = r.pan.device
        if S == 0:
            kept, cnt = torch.zeros_like(r.pan), None                          # nothing is listed: every id is void
        else:
            if id2row is None:
                id2row = torch.from_numpy(tab).to(dev)
            cnt = torch.zeros(len(ks), S, dtype=torch.int32, device=dev)
            kept = torch.empty_like(r.pan)
            hip.mesh_area_count(r.pan, id2row, cnt)
            hip.mesh_area_apply(r.pan, id2row, cnt, int(min_area), kept)
        for j, k in enumerate(ks):
            maps[k], depths[k] = kept[j], r.depth[j]
            counts[k] = None if cnt is None else cnt[j]
    area = np.zeros(S, dtype=np.int64)
    if S:
        per = torch.stack(counts).cpu().numpy().astype(np.int64)              # the only host sync
        area = np.where(per >= int(min_area), per, 0).sum(axis=0)
    gt_segments = [{'id': ids[s], 'category_id': cats[s], 'area': int(area[s])} for s in range(S) if area[s] > 0]
    return maps, gt_segments, depths


# ---------------------------------------------------------------- host helpers: the mesh file and the annotation rule
_PLY_TYPES = {'char': 'b', 'int8': 'b', 'uchar': 'B', 'uint8': 'B', 'short': 'h', 'int16': 'h', 'ushort': 'H', 'uint16': 'H', 'int': 'i', 'int32': 'i',
              'uint': 'I', 'uint32': 'I', 'float': 'f', 'float32': 'f', 'double': 'd', 'float64': 'd'}


def load_ply_mesh(path):
    """Read a triangle mesh from a PLY file, ascii or binary_little_endian: -> (vertices float32 [Nv, 3], faces int64 [Nf, 3]) as CPU tensors.  The vertex
    element needs float properties x, y, z, the face element a `list uchar int|uint vertex_indices` (or vertex_index) of triangles; other scalar
    properties of the two elements are skipped; anything else (another format, other elements before them, a polygon that is no triangle) raises
    ValueError."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError('%s is not a PLY file' % path)
    nl = data.find(b'\n', end)
    if nl < 0:
        raise ValueError('%s: the PLY header does not end' % path)
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element' and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property' and elements:
            elements[-1][2].append(tuple(w[1:]))
        else:
            raise ValueError('%s: cannot read the PLY header line %r' % (path, line))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError('%s: PLY format %r is not supported (ascii and binary_little_endian are)' % (path, fmt))
    if [e[0] for e in elements[:2]] != ['vertex', 'face']:
        raise ValueError("%s: the PLY elements must start with 'vertex' and 'face', got %s" % (path, [e[0] for e in elements]))
    (_, nv, vprops), (_, nf, fprops) = elements[:2]
    for p in vprops:
        if len(p) != 2 or p[0] not in _PLY_TYPES:
            raise ValueError('%s: cannot read the vertex property %r' % (path, ' '.join(p)))
    names = [p[1] for p in vprops]
    if any(a not in names or vprops[names.index(a)][0] not in ('float', 'float32') for a in 'xyz'):
        raise ValueError('%s: the vertex element needs float properties x, y, z' % path)
    xyz = [names.index(a) for a in 'xyz']
    lists = [i for i, p in enumerate(fprops) if p[0] == 'list']
    if len(lists) != 1 or len(fprops[lists[0]]) != 4 or fprops[lists[0]][1] not in ('uchar', 'uint8') or fprops[lists[0]][2] not in ('int', 'int32', 'uint', 'uint32') \
            or fprops[lists[0]][3] not in ('vertex_indices', 'vertex_index'):
        raise ValueError('%s: the face element needs one `list uchar int|uint vertex_indices` property' % path)
    for i, p in enumerate(fprops):
        if i != lists[0] and (len(p) != 2 or p[0] not in _PLY_TYPES):
            raise ValueError('%s: cannot read the face property %r' % (path, ' '.join(p)))
    li = lists[0]
    body = data[nl + 1:]
    if fmt == 'ascii':
        tok = body.split()
        need = nv * len(vprops)
        if len(tok) < need:
            raise ValueError('%s: the file ends inside the vertices' % path)
        try:
            verts = np.array(tok[:need], dtype=np.float64).reshape(nv, len(vprops))[:, xyz].astype(np.float32)
            faces, at = np.empty((nf, 3), dtype=np.int64), need
            for f in range(nf):
                for i in range(len(fprops)):
                    if i != li:
                        float(tok[at])
                        at += 1
                        continue
                    if int(tok[at]) != 3:
                        raise ValueError('%s: face %d has %s vertices; only triangles are read' % (path, f, tok[at].decode()))
                    faces[f] = [int(tok[at + 1]), int(tok[at + 2]), int(tok[at + 3])]
                    at += 4
        except IndexError:
            raise ValueError('%s: the file ends inside the faces' % path) from None
    else:
        vdt = np.dtype([('p%d' % i, '<' + _PLY_TYPES[p[0]]) for i, p in enumerate(vprops)])
        if len(body) < nv * vdt.itemsize:
            raise ValueError('%s: the file ends inside the vertices' % path)
        v = np.frombuffer(body, dtype=vdt, count=nv)
        verts = np.stack([v['p%d' % i] for i in xyz], axis=1).astype(np.float32)
        fields = []
        for i, p in enumerate(fprops):
            fields += [('n', 'u1'), ('v', '<' + _PLY_TYPES[p[2]], (3,))] if i == li else [('p%d' % i, '<' + _PLY_TYPES[p[0]])]
        fdt = np.dtype(fields)                                                # the record of a triangle: every face must be one
        rest = body[nv * vdt.itemsize:]
        if len(rest) < nf * fdt.itemsize:
            raise ValueError('%s: the file ends inside the faces (or a face is no triangle)' % path)
        f = np.frombuffer(rest, dtype=fdt, count=nf)
        if nf and not (f['n'] == 3).all():
            raise ValueError('%s: a face is no triangle; only triangles are read' % path)
        faces = f['v'].astype(np.int64).reshape(nf, 3)
    return torch.from_numpy(np.ascontiguousarray(verts)), torch.from_numpy(np.ascontiguousarray(faces))


def panoptic_vertex_ids(seg_indices, seg_groups, label2id, *, cls_sep=256, crowd=()):
    """The per-vertex panoptic ids of a ScanNet++ annotation, by the rule of the reference's read_semantics (tools/preprocess_scannetpp.py:231-268):
    seg_indices [Nv] = the over-segmentation's segment of every vertex, seg_groups = the annotation's groups ({'label', 'segments'}), label2id = the
    class list.  Groups are taken in order; a group whose label is unknown or in `crowd` is skipped; a kept group gets inst = 1, 2, ... and
    id = inst * cls_sep + label2id[label], written to the vertices of its segments - a later group overwrites an earlier one.
    -> (segments [{'id', 'category_id', 'instance_id', 'label'}], vertex_ids int32 numpy [Nv], 0 = unlabelled)."""
    seg = np.asarray(seg_indices).reshape(-1)
    if seg.dtype.kind not in 'iu':
        raise ValueError('seg_indices must be integers, got %s' % seg.dtype)
    cls_sep = int(cls_sep)
    if cls_sep < 1 or any(not 0 <= int(c) < cls_sep for c in label2id.values()):
        raise ValueError('every class id must be in [0, cls_sep = %d)' % cls_sep)
    crowd = set(crowd)
    ids = np.zeros(seg.shape[0], dtype=np.int32)
    segments, inst = [], 1
    for g in seg_groups:
        label = g['label']
        if label not in label2id or label in crowd:
            continue
        pid = inst * cls_sep + int(label2id[label])
        if pid >= 2 ** 31:
            raise ValueError('the panoptic id %d of group %d does not fit int32' % (pid, inst))
        segments.append({'id': pid, 'category_id': int(label2id[label]), 'instance_id': inst, 'label': label})
        ids[np.isin(seg, np.asarray(g['segments'], dtype=np.int64))] = pid
        inst += 1
    return segments, ids
