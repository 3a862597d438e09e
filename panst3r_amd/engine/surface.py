"""The predicted scene as a surface (stage f9): every view's pointmap is a grid, so pixel neighbours are surface neighbours - the grids of a
`PanopticCloud` triangulated into ONE labelled triangle mesh whose vertices are the cloud's rows.  Faces across depth discontinuities are cut, every
face carries a panoptic id, floating islands can be dropped, and `PanopticMesh.render` hands the result to the mesh rasteriser of stage f8: hole-free
depth and panoptic maps from any camera, where the point splatter of `cloud.render` shows holes as soon as the camera moves closer than the source views.

    cloud, cameras, pan_preds = model.reconstruct(imgs, true_shape, classes)
    mesh = cloud.mesh().drop_small(64)
    views = mesh.render(orbit_cameras(...), focal, (H, W));  mesh.write_ply('scene.ply')

No counterpart in the reference (the DUSt3R family's demos export such a mesh on the host): *restated, unpinned*.  The contract is the surface section of
include/panst3r_hip.h, restated in numpy in tests/surface_ref.py; csrc/surface.hip is held to it bit for bit (integer work and fp32 compares only)."""
import math

import numpy as np
import torch

from .. import hip
from .cloud import ply_colors_u8
from .mesh import MeshRender, mesh_camera_table, render_mesh
from .shade import color_and_shade, vertex_normals

FACE_ROW_BYTES = 17        # a face of the PLY file: uchar 3, three int vertex indices, int label


def _depth_bound(max_depth_ratio):
    """k of the contract's cut: float32(1 + max_depth_ratio), taken in double; None -> +inf (no cut)"""
    if max_depth_ratio is None:
        return math.inf
    r = max_depth_ratio
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not math.isfinite(float(r)) or float(r) < 0:
        raise ValueError('max_depth_ratio must be a finite number >= 0, or None for no cut, got %r' % (max_depth_ratio,))
    with np.errstate(over='ignore'):
        return float(np.float32(1.0 + float(r)))


def _check_min_faces(min_faces):
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)) or not 1 <= min_faces <= 2 ** 31 - 1:
        raise ValueError('min_faces must be an integer >= 1, got %r' % (min_faces,))
    return int(min_faces)


class PanopticMesh:
    """vertices [M,3] fp32, vertex_ids [M] int32, colors [M,3] fp32: the cloud's points, pan and colors themselves (no copies; a vertex that no face
    uses is allowed).  faces [F,3] int32 (rows of the cloud, wound towards the source camera), face_ids [F] int32 (the id two of its corners share, else
    0), quad [F] int64 (the scene pixel of the face's quad corner (y, x): view v holds [view_offsets[v], view_offsets[v+1])), in the order view, quad
    (y, then x), first triangle before second.  segments, cameras: the cloud's."""

    def __init__(self, vertices, faces, face_ids, vertex_ids, colors, quad, view_offsets, segments, cameras=None):
        self.vertices, self.faces, self.face_ids, self.vertex_ids, self.colors, self.quad = vertices, faces, face_ids, vertex_ids, colors, quad
        self.view_offsets, self.segments, self.cameras = view_offsets, segments, cameras
        self._labelled = None                                                    # (component, workspace) of the islands, once computed
        self._normals = None                                                     # vertex_normals() of THESE faces, once computed (_with_faces starts anew)

    def __len__(self):
        return int(self.faces.shape[0])

    def _with_faces(self, faces, face_ids, quad):
        return PanopticMesh(self.vertices, faces, face_ids, self.vertex_ids, self.colors, quad, list(self.view_offsets), self.segments, self.cameras)

    def cpu(self):
        f = lambda t: t.cpu()
        return PanopticMesh(f(self.vertices), f(self.faces), f(self.face_ids), f(self.vertex_ids), f(self.colors), f(self.quad), list(self.view_offsets),
                            [dict(s) for s in self.segments], self.cameras)

    def _on_device(self, what):
        if not self.faces.is_cuda:
            raise RuntimeError('%s got a %s mesh: it runs on the GPU only (no CPU fallback)' % (what, self.faces.device))

    def render(self, cams2world, focals, shape, **kw):
        """engine.mesh.render_mesh of this mesh with its face ids -> `MeshRender` (depth, face, pan per pixel).  An empty mesh renders as all misses."""
        self._on_device('PanopticMesh.render')
        if len(self) == 0:
            H, W = (int(s) for s in shape)
            B, dev = mesh_camera_table(cams2world, focals, (H, W), kw.get('pp')).shape[0], self.faces.device
            return MeshRender(torch.zeros(B, H, W, dtype=torch.float32, device=dev), torch.full((B, H, W), -1, dtype=torch.int64, device=dev),
                              torch.zeros(B, H, W, dtype=torch.int32, device=dev))
        return render_mesh(self.vertices, self.faces, cams2world, focals, shape, face_ids=self.face_ids, **kw)

    @torch.no_grad()
    def _label(self):
        """the islands of the faces (contract step 6), computed once: (component int32 [F], workspace); no host sync"""
        if self._labelled is None:
            ws = hip.surface_workspace(int(self.vertices.shape[0]), self.faces.device)
            component = torch.empty(len(self), dtype=torch.int32, device=self.faces.device)
            faces = self.faces.contiguous()
            hip.surface_link(faces, ws)
            hip.surface_components(faces, ws, component)
            self._labelled = (component, ws)
        return self._labelled

    @staticmethod
    def _check_status(status):
        if status:
            raise RuntimeError('the face components did not finish (status %d): a face index outside the vertices, or a loop bound reached' % status)

    def face_component(self):
        """int32 [F]: the smallest vertex row of the face's component (faces are connected when they share a vertex row) - canonical, so comparable"""
        self._on_device('PanopticMesh.face_component')
        if len(self) == 0:
            return torch.empty(0, dtype=torch.int32, device=self.faces.device)
        component, ws = self._label()
        self._check_status(int(ws['status']))
        return component

    @torch.no_grad()
    def drop_small(self, min_faces):
        """a new mesh without the floating islands: a face survives iff its component has at least `min_faces` faces; survivors keep their order, the
        vertices are untouched.  `min_faces` is an integer >= 1 (1 keeps everything).  One host sync."""
        min_faces = _check_min_faces(min_faces)
        self._on_device('PanopticMesh.drop_small')
        F, dev = len(self), self.faces.device
        if F == 0:
            return self._with_faces(self.faces, self.face_ids, self.quad)
        component, ws = self._label()
        n, counts, base = hip.scan_buffers(dev, F, hip.SURFACE_WG)
        faces, face_ids, quad = torch.empty(F, 3, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int64, device=dev)
        hip.surface_keep_count(component, ws, min_faces, counts)
        hip.cloud_scan(counts, base)
        hip.surface_keep_emit(self.faces.contiguous(), self.face_ids.contiguous(), self.quad.contiguous(), component, ws, min_faces, base, faces, face_ids, quad)
        kept, status = torch.cat([base[n:], ws['status']]).tolist()               # the host sync
        self._check_status(status)
        return self._with_faces(faces[:kept], face_ids[:kept], quad[:kept])

    def simplify(self, cell_size, *, dedupe=True):
        """a new, smaller `PanopticMesh` by vertex clustering (engine/simplify.py, stage f18): the vertices that a face uses and that fall into one cubic
        cell of edge `cell_size` become one vertex - the voxel stage's mean position, mean colour and voted id (ties to the smallest id, void only
        alone) - in the order of their first rows; a face is rewritten onto them and dropped if it lost a corner (a non-finite vertex, a cell beyond
        +-2^20) or if two of its corners merged; with `dedupe` only the first of the faces with one unordered corner set stays, whatever its winding.
        Survivors keep their order, their corner order and their `quad`; face ids are re-derived from the new vertex ids.  segments, cameras and
        view_offsets are carried over.  The result holds `simplify_stats` (vertices_in, vertices_used, vertices_left_out, vertices_out, faces_in,
        faces_left_out, faces_degenerate, faces_duplicate, faces_out), `src_face` int32 [F'] (the face of THIS mesh behind every new face) and
        `cluster` int32 [M] (the new row of every vertex of this mesh, -1 for none).  A `FusedMesh` gives a plain `PanopticMesh`: the volume no longer
        describes it.  An empty mesh, or one whose every face collapses, gives zero faces and zero vertices.  dedupe=True takes at most 2^21 - 2 new
        vertices (ValueError: use a larger cell or dedupe=False); a face naming a row outside the vertices is a ValueError.  Neither topology nor
        winding is preserved.  Two host syncs.  GPU only."""
        from .simplify import simplify_panoptic_mesh
        return simplify_panoptic_mesh(self, cell_size, dedupe=dedupe)

    def vertex_normals(self):
        """engine.shade.vertex_normals of this mesh, fp32 [M,3], computed once (a mesh made by `drop_small` computes its own); an empty mesh: all zero"""
        self._on_device('PanopticMesh.vertex_normals')
        if self._normals is None:
            self._normals = torch.zeros(int(self.vertices.shape[0]), 3, dtype=torch.float32, device=self.faces.device) if len(self) == 0 or \
                self.vertices.shape[0] == 0 else vertex_normals(self.vertices, self.faces)
        return self._normals

    @torch.no_grad()
    def render_color(self, cams2world, focals, shape, *, colors=None, shading='smooth', ambient=0.3, background=(0, 0, 0), **kw):
        """`render` and a colour picture of it -> (`MeshRender`, rgb uint8 [B,H,W,3]): the vertex colours interpolated over every face (engine.shade),
        times ambient + (1 - ambient) * shade, the headlight shade of the interpolated vertex normals ('smooth'), of the face's own normal ('flat') or
        none (None: the colours as they are).  rgb = ply_colors_u8(colour * (ambient + (1 - ambient) * shade)), the product in separately issued fp32
        operations; `background` (three floats in [0, 1]) fills the pixels without a face.  `colors` [M,3] overrides `self.colors`, for example with a
        palette colour per `vertex_ids`.  `ambient` = 0.3 is a choice, not a measured optimum.  **kw: pp, near, far as `render` takes them.  An empty
        mesh renders as background."""
        self._on_device('PanopticMesh.render_color')
        if shading not in ('smooth', 'flat', None):
            raise ValueError("shading must be 'smooth', 'flat' or None, got %r" % (shading,))
        if isinstance(ambient, bool) or not isinstance(ambient, (int, float)) or not 0 <= float(ambient) <= 1:
            raise ValueError('ambient must be a number in [0, 1], got %r' % (ambient,))
        bg = [float(x) for x in background]
        if len(bg) != 3 or not all(math.isfinite(x) for x in bg):
            raise ValueError('background must be three finite numbers, got %r' % (background,))
        colors = self.colors if colors is None else colors
        M = int(self.vertices.shape[0])
        if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (M, 3) or not colors.dtype.is_floating_point:
            raise ValueError('colors must be a floating-point [%d, 3] tensor' % M)
        views = self.render(cams2world, focals, shape, **kw)
        dev = self.faces.device
        back = ply_colors_u8(torch.tensor(bg, dtype=torch.float32, device=dev))
        if len(self) == 0:
            return views, back.expand(*views.face.shape, 3).contiguous()
        col, shade = color_and_shade(views, self.vertices, self.faces, cams2world, focals, colors, normals=self.vertex_normals() if shading == 'smooth' else None,
                                     flat=shading == 'flat', pp=kw.get('pp'), near=kw.get('near', 0.05))
        if shade is not None:
            a = float(ambient)
            light = shade * torch.tensor(1.0 - a, dtype=torch.float32, device=dev)       # fp32(1 - ambient), the difference taken in double
            light = light + torch.tensor(a, dtype=torch.float32, device=dev)
            col = col * light.unsqueeze(-1)
        rgb = torch.where(views.hit.unsqueeze(-1), ply_colors_u8(col), back)
        return views, rgb

    def write_ply(self, path, normals=False):
        """binary little-endian PLY that `load_ply_mesh` reads back: the vertex element is the cloud's 19-byte rows (x y z float, red green blue uchar of
        `colors`, label int = the vertex id), the face element `list uchar int vertex_indices` plus `int label` (the face id).  Both are packed where the
        mesh lives, into one buffer: one device-to-host copy.  normals=True adds `float nx, ny, nz` (`vertex_normals()`) to the vertex element, 31-byte
        rows; the default writes the same bytes as before the argument existed."""
        M, F, dev = int(self.vertices.shape[0]), len(self), self.faces.device
        row = 31 if normals else 19
        buf = torch.empty(M * row + F * FACE_ROW_BYTES, dtype=torch.uint8, device=dev)
        v, f = buf[:M * row].view(M, row), buf[M * row:].view(F, FACE_ROW_BYTES)
        v[:, 0:12] = self.vertices.contiguous().view(torch.uint8).reshape(M, 12)
        v[:, 12:15] = ply_colors_u8(self.colors)
        v[:, 15:19] = self.vertex_ids.contiguous().view(torch.uint8).reshape(M, 4)
        if normals:
            v[:, 19:31] = self.vertex_normals().contiguous().view(torch.uint8).reshape(M, 12)
        f[:, 0] = 3
        f[:, 1:13] = self.faces.contiguous().view(torch.uint8).reshape(F, 12)
        f[:, 13:17] = self.face_ids.contiguous().view(torch.uint8).reshape(F, 4)
        header = ('ply\nformat binary_little_endian 1.0\ncomment panst3r_amd panoptic surface mesh\nelement vertex %d\nproperty float x\nproperty float y\n'
                  'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\n%selement face %d\n'
                  'property list uchar int vertex_indices\nproperty int label\nend_header\n' %
                  (M, 'property float nx\nproperty float ny\nproperty float nz\n' if normals else '', F))
        with open(path, 'wb') as fh:
            fh.write(header.encode('ascii'))
            fh.write(buf.cpu().numpy().tobytes())
        return path


@torch.no_grad()
def panoptic_mesh(cloud, *, max_depth_ratio=0.1):
    """Triangulate the pointmap grids of a `PanopticCloud` into a `PanopticMesh` on the cloud's rows.  The cloud must still hold its device inputs (as
    `rethreshold` needs them): the shapes of the views and their camera-frame pointmaps come from there.  Per quad of four neighbouring pixels: with all
    four kept by the cloud's confidence threshold two triangles, split along the diagonal whose ends are closer in depth; with three, the one triangle
    of them; else nothing.  A triangle is kept iff its nearest corner has depth > 0 and its farthest corner is at most (1 + max_depth_ratio) times as
    deep - faces across depth discontinuities are cut.  `max_depth_ratio`: a finite number >= 0, or None for no cut; the default 0.1 is a CHOICE (a 10 %
    depth step between neighbouring pixels), not a measured optimum.  A face takes the id two of its corners share, else 0.  Everything else is the
    surface section of include/panst3r_hip.h.  An empty result (no kept point, or every face cut) is a mesh of zero faces.  One host sync (F).  The
    face tensors are views of scene-sized buffers: `.clone()` one to keep it beyond the mesh.  The depths are read from the `pts3d_local` tensors the cloud
    was built from (the cloud's own `points_local` is in the world frame), so those input tensors must not have been modified in place since.  GPU only."""
    k = _depth_bound(max_depth_ratio)
    src = getattr(cloud, '_source', None)
    if src is None:
        raise RuntimeError('this cloud does not hold its device inputs (it was moved to the CPU or built by hand)')
    if not cloud.pan.is_cuda:
        raise RuntimeError('panoptic_mesh got a %s cloud: it runs on the GPU only (no CPU fallback)' % cloud.pan.device)
    N, V, M, dev = int(src.N), len(src.shapes), len(cloud), cloud.pan.device
    if N > hip.SURFACE_MAX_PIXELS:
        raise ValueError('a scene of %d pixels exceeds the 2^30 the surface kernels take' % N)
    if src.surface_dims is None:
        src.surface_dims = hip.surface_dims(src.shapes, dev)
    dims, nwg = src.surface_dims
    i32 = dict(dtype=torch.int32, device=dev)

    def result(faces, face_ids, quad):
        return PanopticMesh(cloud.points, faces, face_ids, cloud.pan, cloud.colors, quad, list(cloud.view_offsets), cloud.segments, cloud.cameras)
    if M == 0 or nwg == 0:
        return result(torch.empty(0, 3, **i32), torch.empty(0, **i32), torch.empty(0, dtype=torch.int64, device=dev))
    row = torch.empty(N, **i32)
    _, counts, base = hip.scan_buffers(dev, nwg=nwg)
    cap = 2 * hip.SURFACE_WG * nwg                                               # two faces per quad, whole workgroups
    faces, face_ids, quad = torch.empty(cap, 3, **i32), torch.empty(cap, **i32), torch.empty(cap, dtype=torch.int64, device=dev)
    hip.surface_rows(cloud.index.contiguous(), N, row)
    hip.surface_count(src.table, dims, V, nwg, row, k, counts)
    hip.cloud_scan(counts, base)
    hip.surface_emit(src.table, dims, V, nwg, row, k, cloud.pan.contiguous(), base, faces, face_ids, quad)
    F = int(base[nwg])                                                           # the only host sync
    return result(faces[:F], face_ids[:F], quad[:F])
