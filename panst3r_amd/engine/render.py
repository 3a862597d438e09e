"""Images out of the 3-D result: a device `PanopticCloud` or `VoxelCloud` rendered from any pinhole camera by a z-buffered point splatter - per pixel
the nearest point's depth, panoptic id, colours and row.  That is the panoptic segmentation (and the depth map) of a view that was not an input, the
reprojection check of the fused labels on a view that was, and - over `orbit_cameras` - the turntable the demo's viewer offers.

The reference has no such stage (its demo hands the cloud to an interactive viewer): *restated, unpinned*, like the cloud and the voxels.
tests/render_ref.py restates the six steps of the contract in include/panst3r_hip.h in numpy; csrc/render.hip is held to it bit for bit (separately
rounded fp32 operations, a quotient rounded once, integer atomics only)."""
import math

import numpy as np
import torch

from .. import hip
from .cloud import ply_colors_u8

ZBUF_BYTES = 256 << 20     # the z-buffer of one launch (8 bytes per camera pixel) stays under this: more cameras are rendered in chunks


def one_camera(b, n):
    """the slice that keeps camera b of n (b < 0 counts from the end) as a batch of one"""
    return slice(b, b + 1) if b >= 0 else slice(b + n, b + n + 1)


def image_shape(shape):
    H, W = (int(s) for s in shape)
    if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
        raise ValueError('shape must be (H, W) with 1 <= H * W < 2^31, got %r' % (tuple(shape),))
    return H, W


def chunk_step(B, H, W, budget):
    """cameras per launch of the z-buffer loop (and of what walks a render in the same chunks, engine/shade.py): a chunk's int64 [step, H, W] buffer
    stays under `budget` bytes and inside one launch's limits (65 535 cameras, 2^31 - 1 pixels); at least one camera"""
    return max(1, min(budget // (8 * H * W), 65535, (2 ** 31 - 1) // (H * W), B))


def zbuf_chunks(B, H, W, dev, budget):
    """the z-buffer loop of `render_cloud` and `mesh.render_mesh`: B cameras in chunks whose int64 [b1 - b0, H, W] buffer stays under `budget` bytes (the
    caller's `ZBUF_BYTES`) and inside one launch's limits -> (b0, b1, z) per chunk, z cleared to all ones, the empty key.  The first chunk is the largest."""
    step = chunk_step(B, H, W, budget)
    zbuf = torch.empty(step, H, W, dtype=torch.int64, device=dev)
    for b0 in range(0, B, step):
        b1 = min(b0 + step, B)
        z = zbuf[:b1 - b0]
        z.fill_(-1)
        yield b0, b1, z


class CloudRender:
    """B views of one cloud at one shape: depth [B,H,W] fp32 (the camera-frame z of the pixel's nearest point, 0 where no point landed), pan [B,H,W] int32
    (its panoptic id, 0 where empty), rgb, colors [B,H,W,3] fp32 (its image colour and its blended colour, 0 where empty), index [B,H,W] int64 (its row
    in the cloud, -1 where empty)."""

    def __init__(self, depth, pan, rgb, colors, index):
        self.depth, self.pan, self.rgb, self.colors, self.index = depth, pan, rgb, colors, index

    def __len__(self):
        return int(self.index.shape[0])

    @property
    def hit(self):
        """[B,H,W] bool: a point landed on the pixel"""
        return self.index >= 0

    def cpu(self):
        return CloudRender(self.depth.cpu(), self.pan.cpu(), self.rgb.cpu(), self.colors.cpu(), self.index.cpu())

    def images_u8(self):
        """[B,H,W,3] uint8 of `colors`, as write_ply rounds them"""
        return ply_colors_u8(self.colors)

    def __getitem__(self, b):
        """the render of camera b alone, [1,H,W] views"""
        s = one_camera(b, len(self))
        return CloudRender(self.depth[s], self.pan[s], self.rgb[s], self.colors[s], self.index[s])


def _host64(x):
    return np.asarray(torch.as_tensor(x).detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def world_to_camera(cams2world, shape, pp, who):
    """what `camera_table` and `mesh.mesh_camera_table` share, on the host in float64: B camera-to-world matrices ([B, 4, 4] or a list of [4, 4]) ->
    (float32 [B, 12], per camera the rows of [R^T | -R^T t] rounded to float32 (include/panst3r_hip.h, step 1), and float64 [B, 2], the principal
    points: `pp` as one (cx, cy) pair or one per camera, default (W / 2, H / 2)).  `who` is the caller's name in the message.  Raises ValueError."""
    H, W = (int(s) for s in shape)
    if isinstance(cams2world, (list, tuple)):
        mats = [_host64(c) for c in cams2world]
        if any(m.shape != (4, 4) for m in mats):
            raise ValueError('every camera-to-world matrix must be [4, 4], got %s' % sorted({tuple(m.shape) for m in mats}))
        c = np.stack(mats) if mats else np.zeros((0, 4, 4))
    else:
        c = _host64(cams2world)
        if c.ndim != 3 or c.shape[1:] != (4, 4):
            raise ValueError('cams2world must be [B, 4, 4] (or a list of [4, 4]), got %s' % (tuple(c.shape),))
    B = c.shape[0]
    if B == 0:
        raise ValueError('%s needs at least one camera' % who)
    if not np.isfinite(c).all():
        raise ValueError('a camera-to-world matrix has a non-finite entry')
    p = np.array([W / 2, H / 2]) if pp is None else _host64(pp)
    if p.size not in (2, 2 * B) or not np.isfinite(p).all():
        raise ValueError('pp must be a finite (cx, cy) pair, one per camera or one for all, got %r' % (pp,))
    rows = np.empty((B, 12), dtype=np.float32)
    with np.errstate(over='ignore'):
        for b in range(B):
            R, t = c[b, :3, :3], c[b, :3, 3]
            for a in range(3):
                rows[b, 4 * a:4 * a + 3] = R[:, a]                                                 # row a of R^T
                rows[b, 4 * a + 3] = -((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2])
    return rows, np.broadcast_to(p.reshape(-1, 2), (B, 2))


def camera_table(cams2world, focals, shape, pp=None, near=1e-3):
    """the float32 [B, 16] table of the kernels (include/panst3r_hip.h, step 1) of B camera-to-world matrices, on the host in float64: per camera the rows
    of [R^T | -R^T t] rounded to float32, then focal, principal point (default (W / 2, H / 2)) and near.  Raises ValueError for anything unusable."""
    rows, p = world_to_camera(cams2world, shape, pp, 'render_cloud')
    B = rows.shape[0]
    f = _host64(focals).reshape(-1)
    if f.size == 1:
        f = np.repeat(f, B)
    if f.size != B or not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError('focals must be one positive finite number per camera (or one for all), got %s' % (f.tolist(),))
    nr = float(near)
    if not (math.isfinite(nr) and np.float32(nr) > 0):
        raise ValueError('near must be a positive finite float32, got %r' % (near,))
    tab = np.empty((B, hip.RENDER_CAM_FLOATS), dtype=np.float32)
    with np.errstate(over='ignore'):
        tab[:, :12], tab[:, 12], tab[:, 13:15], tab[:, 15] = rows, f, p, nr
    if not (np.isfinite(tab).all() and (tab[:, 12] > 0).all()):
        raise ValueError('a camera does not fit float32 (matrix, focal or principal point)')
    return tab


def _check_footprint(cloud, radius, point_size, max_radius):
    lim = hip.RENDER_MAX_RADIUS
    for name, r in (('radius', radius), ('max_radius', max_radius)):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r <= lim:
            raise ValueError('%s must be an integer in 0 .. %d (PST_RENDER_MAX_RADIUS), got %r' % (name, lim, r))
    if point_size is None:
        point_size = getattr(cloud, 'voxel_size', None) or 0.0                # a voxel cloud renders without holes
    ps = float(point_size)
    with np.errstate(over='ignore'):
        half = float(np.float32(ps / 2))
    if not (math.isfinite(half) and half >= 0):
        raise ValueError('point_size must be a finite number >= 0 (world units), got %r' % (point_size,))
    return int(radius), int(max_radius), half


@torch.no_grad()
def render_cloud(cloud, cams2world, focals, shape, *, pp=None, radius=0, point_size=None, max_radius=8, near=1e-3):
    """Render a device `PanopticCloud` or `VoxelCloud` (anything with points, rgb, colors [M,3] and pan [M]) from B cameras at one output shape (H, W) ->
    `CloudRender`.  cams2world: [B,4,4] or a list of [4,4] camera-to-world matrices (x right, y down, z forward, as the pointmaps'); focals: pixels, one
    per camera or one for all; pp: principal point(s) (cx, cy), default (W / 2, H / 2), the demo's convention.  A point lands on the pixel its projection
    falls into and on the `(2r + 1)^2` pixels around it, r = min(max_radius, max(radius, floor(focal * point_size / 2 / z))): `radius` is a minimum in
    pixels, `point_size` the point's extent in world units (default 0 for a panoptic cloud, `voxel_size` for a voxel cloud, so that it renders without
    holes).  Per pixel the nearest point wins (equal depths: the smallest row); points behind the camera, nearer than `near`, non-finite or off-screen
    leave no trace.  Cameras are taken in chunks so that the z-buffer stays under `ZBUF_BYTES`.  No host sync when the cameras are host values.
    GPU only: a CPU cloud raises."""
    H, W = image_shape(shape)
    tab = camera_table(cams2world, focals, (H, W), pp, near)
    radius, max_radius, half = _check_footprint(cloud, radius, point_size, max_radius)
    M = int(cloud.pan.shape[0])
    if M >= 2 ** 32:
        raise ValueError('a cloud of %d points exceeds the 2^32 - 1 rows a z-buffer key holds' % M)
    for t in (cloud.points, cloud.rgb, cloud.colors, cloud.pan):
        if not t.is_cuda:
            raise RuntimeError('render_cloud got a %s tensor: it runs on the GPU only (no CPU fallback)' % t.device)
    dev = cloud.pan.device
    B = tab.shape[0]
    if M == 0:
        z3 = lambda: torch.zeros(B, H, W, 3, dtype=torch.float32, device=dev)
        return CloudRender(torch.zeros(B, H, W, dtype=torch.float32, device=dev), torch.zeros(B, H, W, dtype=torch.int32, device=dev), z3(), z3(),
                           torch.full((B, H, W), -1, dtype=torch.int64, device=dev))
    points, rgb, colors = (t.float().contiguous() for t in (cloud.points, cloud.rgb, cloud.colors))
    pan = cloud.pan.to(torch.int32).contiguous()
    cams = torch.from_numpy(tab).to(dev)
    e3 = lambda: torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    out = CloudRender(torch.empty(B, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.int32, device=dev), e3(), e3(),
                      torch.empty(B, H, W, dtype=torch.int64, device=dev))
    for b0, b1, z in zbuf_chunks(B, H, W, dev, ZBUF_BYTES):
        hip.render_splat(points, cams[b0:b1], H, W, half, radius, max_radius, z)
        hip.render_resolve(z, rgb, colors, pan, out.index[b0:b1], out.depth[b0:b1], out.pan[b0:b1], out.rgb[b0:b1], out.colors[b0:b1])
    return out


def render_cameras(cloud, cameras, **kw):
    """Render the cloud from the camera dicts `PanSt3R.reconstruct` returns ('cam2world', 'focal', 'height', 'width'), each at its own shape: the cameras
    are grouped by shape, one `render_cloud` call per group -> a list of one-view `CloudRender`s aligned with `cameras`."""
    groups = {}
    for k, c in enumerate(cameras):
        groups.setdefault((int(c['height']), int(c['width'])), []).append(k)
    out = [None] * len(cameras)
    for shape, ks in groups.items():
        r = render_cloud(cloud, [cameras[k]['cam2world'] for k in ks], [float(cameras[k]['focal']) for k in ks], shape, **kw)
        for j, k in enumerate(ks):
            out[k] = r[j]
    return out


def orbit_cameras(target, radius, n, height, up=(0, 0, 1)):
    """n camera-to-world matrices (float64 [4,4], x right, y down, z forward) equally spaced on a circle of `radius` around `target` in the plane
    perpendicular to `up`, raised by `height` along it, each looking at `target`: the viewer's turntable.  Host side."""
    target, up = np.asarray(target, dtype=np.float64).reshape(3), np.asarray(up, dtype=np.float64).reshape(3)
    radius, height, n = float(radius), float(height), int(n)
    if not (np.isfinite(target).all() and np.isfinite(up).all() and np.linalg.norm(up) > 0):
        raise ValueError('target and up must be finite, up non-zero')
    if not (math.isfinite(radius) and radius > 0 and math.isfinite(height) and n >= 1):
        raise ValueError('orbit_cameras needs radius > 0, a finite height and n >= 1, got %r, %r, %r' % (radius, height, n))
    up = up / np.linalg.norm(up)
    a = np.eye(3)[int(np.argmin(np.abs(up)))]                                 # the axis least aligned with up
    e1 = a - np.dot(a, up) * up
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    out = []
    for k in range(n):
        ang = 2 * math.pi * k / n
        eye = target + radius * (math.cos(ang) * e1 + math.sin(ang) * e2) + height * up
        z = target - eye
        z = z / np.linalg.norm(z)
        x = np.cross(z, up)
        x = x / np.linalg.norm(x)
        c = np.eye(4)
        c[:3, 0], c[:3, 1], c[:3, 2], c[:3, 3] = x, np.cross(z, x), z, eye
        out.append(c)
    return out
