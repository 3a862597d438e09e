"""Shade and colour mesh renders (stage f17): area-weighted vertex normals, any per-vertex quantity interpolated over the pixels of a `MeshRender`, and
a headlight shade term - together colour and shaded novel views of every mesh the geometry stages produce (the ground truth, `cloud.mesh()`, the fused
TSDF surface), and any per-vertex number (a confidence, a consistency count, a palette colour per panoptic id) drawn through the same call.

    mesh = cloud.fused_mesh(0.02).drop_small(64)
    views, rgb = mesh.render_color(orbit_cameras(...), focal, (H, W))            # uint8 [B, H, W, 3]
    conf_img = interpolate_render(views, mesh.vertices, mesh.faces, cams, focal, conf[:, None])

No counterpart in the reference: *restated, unpinned*.  The contract is the mesh shading section of include/panst3r_hip.h, restated in numpy in
tests/mesh_shade_ref.py; csrc/mesh_normals.hip and pst_mesh_interp of csrc/mesh.hip are held to it bit for bit (exact two-limb integer sums for the
normals, the rasteriser's own edge values and 1 / zc as the interpolation weights, a square root made of IEEE divisions only).

Stated limits: the normals are weighted by face AREA, not by angle; the shade is a two-sided headlight at the camera - no shadows, no textures; at most
16 channels per call; no near-plane clipping (inherited from the rasteriser: a face with a vertex behind `near` is a miss); `ambient` of `render_color`
is a choice, not a measured optimum."""
import math

import numpy as np
import torch

from .. import hip
from .mesh import MeshRender, _check_mesh, mesh_camera_table
from .render import ZBUF_BYTES, chunk_step          # ZBUF_BYTES: this module's own name, as engine/mesh.py has one (tests set it to force chunks)

MAX_CHANNELS = hip.MESH_INTERP_MAX_CHANNELS


def _device_mesh(who, vertices, faces):
    """-> (vertices fp32 [Nv,3], faces int32 [Nf,3]) as the kernels take them; an int64 index that does not fit int32 is outside the vertices: kept so"""
    Nv, _ = _check_mesh(vertices, faces, None, None)
    for t in (vertices, faces):
        if not t.is_cuda:
            raise RuntimeError('%s got a %s tensor: it runs on the GPU only (no CPU fallback)' % (who, t.device))
    if faces.dtype == torch.int64:
        faces = torch.where((faces < 0) | (faces >= Nv), torch.full_like(faces, -1), faces)
    return vertices.float().contiguous(), faces.to(torch.int32).contiguous()


def normals_shift(lo, hi):
    """the scale exponent `sh` of the contract's step 3 from the per-axis extrema of the finite coordinates (float32 values, +inf / -inf for an axis
    without one): D = the largest max - min in float64, ex = frexp(D)'s exponent, sh = 51 - 2 ex; 0 when D == 0 or nothing is finite"""
    ext = [float(np.float64(np.float32(h)) - np.float64(np.float32(l))) for l, h in zip(lo, hi) if math.isfinite(l) and math.isfinite(h)]
    D = max(ext) if ext else 0.0
    return 51 - 2 * math.frexp(D)[1] if D > 0 else 0


@torch.no_grad()
def vertex_normals(vertices, faces):
    """Area-weighted unit normals of a device mesh (vertices [Nv,3] float, faces [Nf,3] int) -> fp32 [Nv,3]; a vertex on no valid face (or whose faces
    cancel) gets (0, 0, 0).  A face with an index outside the vertices or a non-finite coordinate adds nothing.  Bit-reproducible: the sums are exact
    integers, so neither the order of the faces nor scheduling changes a bit.  One host sync (the extent of the vertices, which sets the quantum).
    GPU only: CPU tensors raise."""
    verts, faces = _device_mesh('vertex_normals', vertices, faces)
    Nv, dev = int(verts.shape[0]), verts.device
    finite = torch.isfinite(verts)
    inf = torch.tensor(math.inf, dtype=torch.float32, device=dev)
    ext = torch.stack([torch.where(finite, verts, inf).amin(dim=0), torch.where(finite, verts, -inf).amax(dim=0)]).cpu().numpy()       # the host sync
    sh = normals_shift(ext[0].tolist(), ext[1].tolist())
    out = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    hip.mesh_normals(verts, faces, sh, torch.empty(Nv, 3, 2, dtype=torch.int64, device=dev), out)
    return out


def _face_map(x):
    face = x.face if isinstance(x, MeshRender) else x
    if not isinstance(face, torch.Tensor) or face.dim() != 3 or face.dtype != torch.int64:
        raise ValueError('a MeshRender or its face map (an int64 [B, H, W] tensor) is needed, got %s' %
                         ('%s %s' % (face.dtype, tuple(face.shape)) if isinstance(face, torch.Tensor) else type(face).__name__))
    if not face.is_cuda:
        raise RuntimeError('the face map is a %s tensor: this runs on the GPU only (no CPU fallback)' % face.device)
    return face.contiguous()


def _check_near(near):
    nr = float(near)
    with np.errstate(over='ignore'):
        n32 = np.float32(nr)
    if not (math.isfinite(nr) and np.isfinite(n32) and n32 > 0):
        raise ValueError('near must be a finite float32 > 0, got %r' % (near,))
    return float(n32)


def _interp(who, render, vertices, faces, cams2world, focals, pp, near, attr=None, fill=0.0, shade_mode=hip.MESH_SHADE_NONE, normals=None):
    """the chunked launch behind the public entry points -> (out_attr or None, out_shade or None)"""
    face = _face_map(render)
    B, H, W = (int(s) for s in face.shape)
    verts, faces = _device_mesh(who, vertices, faces)
    tab = mesh_camera_table(cams2world, focals, (H, W), pp)
    if tab.shape[0] != B:
        raise ValueError('%s: %d cameras for a face map of %d views' % (who, tab.shape[0], B))
    near = _check_near(near)
    dev = verts.device
    cams = torch.from_numpy(tab).to(dev)
    out_attr = None if attr is None else torch.empty(B, H, W, attr.shape[1], dtype=torch.float32, device=dev)
    out_shade = None if shade_mode == hip.MESH_SHADE_NONE else torch.empty(B, H, W, dtype=torch.float32, device=dev)
    step = chunk_step(B, H, W, ZBUF_BYTES)                                    # render_mesh's chunks
    for b0 in range(0, B, step):
        b1 = min(b0 + step, B)
        hip.mesh_interp(face[b0:b1], verts, faces, cams[b0:b1], near, attr=attr, fill=fill, out_attr=None if out_attr is None else out_attr[b0:b1],
                        shade_mode=shade_mode, normals=normals, out_shade=None if out_shade is None else out_shade[b0:b1])
    return out_attr, out_shade


def _rows(who, name, t, Nv, width):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.dtype.is_floating_point or t.shape[0] != Nv or (width is not None and t.shape[1] != width):
        raise ValueError('%s: %s must be a floating-point [%d, %s] tensor, got %s' %
                         (who, name, Nv, 'C' if width is None else width, '%s %s' % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError('%s: %s is a %s tensor: it runs on the GPU only (no CPU fallback)' % (who, name, t.device))
    return t.float().contiguous()


@torch.no_grad()
def interpolate_render(render, vertices, faces, cams2world, focals, attributes, *, pp=None, near=0.05, fill=0.0):
    """Per-vertex attributes [Nv, C] (1 <= C <= 16) interpolated perspective-correctly over the pixels of a `MeshRender` (or its int64 [B,H,W] face map)
    of the same mesh and cameras -> fp32 [B,H,W,C].  The weights are the rasteriser's own: the attribute 'camera z of the vertex' comes back as the
    rendered depth (bit for bit where the products w_k z_k are exact, as at power-of-two depths; to rounding otherwise).  A pixel without a face - or, in a hand-made map, naming a face that does not cover it - gets `fill` in every channel.
    cams2world, focals, pp, near: as `render_mesh` took them.  No host sync when the cameras are host values.  GPU only: CPU tensors raise."""
    who = 'interpolate_render'
    attr = _rows(who, 'attributes', attributes, _check_mesh(vertices, faces, None, None)[0], None)
    if not 1 <= attr.shape[1] <= MAX_CHANNELS:
        raise ValueError('%s: 1 .. %d channels per call, got %d' % (who, MAX_CHANNELS, attr.shape[1]))
    if isinstance(fill, bool) or not isinstance(fill, (int, float, np.integer, np.floating)) or not math.isfinite(float(fill)) or not np.isfinite(np.float32(fill)):
        raise ValueError('%s: fill must be a finite float32, got %r' % (who, fill))
    return _interp(who, render, vertices, faces, cams2world, focals, pp, near, attr=attr, fill=float(fill))[0]


@torch.no_grad()
def shade_render(render, vertices, faces, cams2world, focals, *, normals=None, pp=None, near=0.05):
    """The headlight shade of a `MeshRender` (or its face map) -> fp32 [B,H,W]: |cos| of the angle between the surface normal and the pixel's view ray,
    two-sided, 0 where no face.  normals=None shades every face flat by its own normal; normals [Nv,3] (`vertex_normals`) are interpolated over the
    face - smooth.  No shadows, no textures.  GPU only: CPU tensors raise."""
    who = 'shade_render'
    if normals is None:
        return _interp(who, render, vertices, faces, cams2world, focals, pp, near, shade_mode=hip.MESH_SHADE_FLAT)[1]
    n = _rows(who, 'normals', normals, _check_mesh(vertices, faces, None, None)[0], 3)
    return _interp(who, render, vertices, faces, cams2world, focals, pp, near, shade_mode=hip.MESH_SHADE_SMOOTH, normals=n)[1]


@torch.no_grad()
def color_and_shade(render, vertices, faces, cams2world, focals, colors, *, normals=None, flat=False, pp=None, near=0.05):
    """colours [Nv,3] and the shade from ONE launch per chunk -> (fp32 [B,H,W,3], 0 on a miss; fp32 [B,H,W] or None): what `PanopticMesh.render_color`
    uses.  Shade: smooth with `normals`, flat with flat=True, else none."""
    who = 'render_color'
    Nv = _check_mesh(vertices, faces, None, None)[0]
    attr = _rows(who, 'colors', colors, Nv, 3)
    mode = hip.MESH_SHADE_SMOOTH if normals is not None else hip.MESH_SHADE_FLAT if flat else hip.MESH_SHADE_NONE
    n = None if normals is None else _rows(who, 'normals', normals, Nv, 3)
    return _interp(who, render, vertices, faces, cams2world, focals, pp, near, attr=attr, fill=0.0, shade_mode=mode, normals=n)
