"""numpy restatement of the z-buffered point rendering of a cloud (panst3r_amd/engine/render.py, csrc/render.hip), the yardstick the kernels are held to
bit for bit.

Own design (the reference has no such stage).  The six steps of the contract in include/panst3r_hip.h:
  1 camera    float64 on the host: W = R^T, s_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2) of the camera-to-world [R | t], rounded to float32; then
              xc = ((W00 x + W01 y) + W02 z) + s0 ... in float32.
  2 cull      xc, yc, zc finite and zc >= near, or the point is left out.
  3 project   u = (f xc) / zc + cx, v = (f yc) / zc + cy, the quotient taken in float64 and rounded once; |u|, |v| <= 2^20 or the point is left out;
              px = floor(u), py = floor(v).
  4 footprint r = min(max_radius, max(radius, floor((f half_size) / zc))), half_size = float32(point_size / 2); the (2r + 1)^2 pixels around (px, py),
              clipped to the image.
  5 depth     key = (uint64(bits(zc)) << 32) | uint32(row); np.minimum.at into a uint64 buffer of all ones.
  6 resolve   an empty cell, or a key whose row is >= M: index -1, zeros; otherwise the key's row and depth, and that row's pan, rgb, colors.
Elementwise float32 numpy rounds every operation on its own, which is what the kernels promise; the minimum of integers is exact in any order."""
import numpy as np

F = np.float32
LIM = F(2 ** 20)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera_table(cams2world, focals, shape, pp=None, near=1e-3):
    """float32 [B, 16] of step 1: W00 W01 W02 s0 W10 W11 W12 s1 W20 W21 W22 s2 f cx cy near"""
    H, W = shape
    c = np.stack([np.asarray(m, dtype=np.float64) for m in cams2world]).reshape(-1, 4, 4)
    B = len(c)
    f = np.broadcast_to(np.asarray(focals, dtype=np.float64).reshape(-1), (B,))
    p = np.broadcast_to(np.asarray([W / 2, H / 2] if pp is None else pp, dtype=np.float64).reshape(-1, 2), (B, 2))
    tab = np.empty((B, 16), dtype=F)
    for b in range(B):
        R, t = c[b, :3, :3], c[b, :3, 3]
        for a in range(3):
            tab[b, 4 * a:4 * a + 3] = R[:, a]
            tab[b, 4 * a + 3] = -((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2])           # numpy float64 scalars: every operation rounded on its own
        tab[b, 12:] = (f[b], p[b, 0], p[b, 1], near)
    return tab


def quotient(a, b):
    """float32(float64(a) / float64(b))"""
    return (np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)).astype(F)


def camera_coords(points, cam):
    """step 1 on the device side: three float32 [M] arrays"""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return [((cam[4 * a] * x + cam[4 * a + 1] * y) + cam[4 * a + 2] * z) + cam[4 * a + 3] for a in range(3)]


def splat(points, cam, H, W, half_size, radius, max_radius):
    """steps 1 - 5 for one camera -> (zbuf uint64 [H * W], candidates int64 [H * W] = the number of keys that reached each cell, behind = the number of
    finite points culled by zc < near)"""
    f, cx, cy, near = cam[12], cam[13], cam[14], cam[15]
    zbuf, cand = np.full(H * W, EMPTY, dtype=np.uint64), np.zeros(H * W, dtype=np.int64)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        xc, yc, zc = camera_coords(points, cam)
        finite = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
        keep = finite & (zc >= near)                                                                # step 2
        behind = int((finite & ~keep).sum())
        rows = np.nonzero(keep)[0]
        xc, yc, zc = xc[keep], yc[keep], zc[keep]
        u = (quotient(f * xc, zc) + cx).astype(F)                                                   # step 3
        v = (quotient(f * yc, zc) + cy).astype(F)
        ok = (np.abs(u) <= LIM) & (np.abs(v) <= LIM)                                                # a NaN fails
        rows, zc, u, v = rows[ok], zc[ok], u[ok], v[ok]
        px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        rs = np.minimum(np.floor(quotient(F(f * half_size), zc)), F(max_radius)).astype(np.int64)   # step 4
    r = np.minimum(max_radius, np.maximum(radius, rs))
    key = (np.ascontiguousarray(zc).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)     # step 5
    top = int(r.max()) if len(r) else -1
    for dy in range(-top, top + 1):
        for dx in range(-top, top + 1):
            xx, yy = px + dx, py + dy
            m = (r >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)          # clipped, not wrapped
            cell = (yy * W + xx)[m]
            np.minimum.at(zbuf, cell, key[m])
            cand += np.bincount(cell, minlength=H * W)
    return zbuf, cand, behind


def resolve(zbuf, rgb, colors, pan):
    """step 6 on the flat uint64 cells of any number of cameras -> (index int64, depth float32, pan int32, rgb, colors float32 [., 3]); a cell is empty if it
    is all ones or if its key names a row >= M = len(pan)"""
    zbuf = np.asarray(zbuf, dtype=np.uint64).reshape(-1)
    low = zbuf & np.uint64(0xFFFFFFFF)
    hit = (zbuf != EMPTY) & (low < np.uint64(len(pan)))
    row = np.where(hit, low, np.uint64(0)).astype(np.int64)
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    gather = lambda t, zero: np.where(hit.reshape((-1,) + (1,) * (t.ndim - 1)), t[row], zero).astype(t.dtype) if len(t) else np.zeros((len(zbuf),) + t.shape[1:], t.dtype)
    return np.where(hit, row, -1), depth, gather(pan, np.int32(0)), gather(rgb, F(0)), gather(colors, F(0))


def render(points, rgb, colors, pan, cams2world, focals, shape, pp=None, radius=0, point_size=0.0, max_radius=8, near=1e-3):
    """-> dict(depth [B,H,W] float32, pan [B,H,W] int32, rgb, colors [B,H,W,3] float32, index [B,H,W] int64) and, about the run itself,
    candidates [B,H,W] int64 and behind [B]"""
    H, W = shape
    rgb, colors = np.asarray(rgb, dtype=F).reshape(-1, 3), np.asarray(colors, dtype=F).reshape(-1, 3)
    pan = np.asarray(pan).reshape(-1).astype(np.int32)
    tab = camera_table(cams2world, focals, shape, pp, near)
    half = F(float(point_size) / 2)
    out = {k: [] for k in ('depth', 'pan', 'rgb', 'colors', 'index', 'candidates', 'behind')}
    for cam in tab:
        zbuf, cand, behind = splat(points, cam, H, W, half, int(radius), int(max_radius))
        index, depth, opan, orgb, ocolors = resolve(zbuf, rgb, colors, pan)                          # step 6
        out['index'].append(index.reshape(H, W))
        out['depth'].append(depth.reshape(H, W))
        out['pan'].append(opan.reshape(H, W))
        out['rgb'].append(orgb.reshape(H, W, 3))
        out['colors'].append(ocolors.reshape(H, W, 3))
        out['candidates'].append(cand.reshape(H, W))
        out['behind'].append(behind)
    return {k: np.stack(v) for k, v in out.items()}
