"""numpy restatement of the cross-view depth consistency of the pointmaps (panst3r_amd/engine/consistency.py, csrc/consistency.hip), the yardstick
the kernels are held to bit for bit.

Own design (the reference has no such stage).  The contract of include/panst3r_hip.h:
  world    a pixel's world point: pts3d, or with local_pointmaps pts3d_local moved by its camera, ((R00 x + R01 y) + R02 z) + t0 ... (cloud_ref.geotrf)
  camera   xc = ((W00 X + W01 Y) + W02 Z) + s0 ... with the float32 [16] table of render_ref.camera_table (render_ref.camera_coords)
  depth    zc in the pixel's OWN camera if conf >= thr, xc, yc, zc finite and zc >= near; else 0 = "this view measured nothing here"
  count    a pixel with depth 0 gets zeros; any other, for every view j but its own: cull on non-finite coordinates and !(zc >= near_j);
           u = (f xc) / zc + cx, v likewise, the quotient taken in float64 and rounded once; cull unless |u|, |v| <= 2^20; px = floor(u + 0.5),
           py = floor(v + 0.5) - the nearest pixel centre; outside the image: unseen; d = depth_j[py, px]; d == 0: unseen; tol = rel_tol d;
           agree if |zc - d| <= tol, else violate if d - zc > tol, else occluded; same_label += 1 on an agreeing pair whose source id > 0 equals
           view j's id at that pixel.
Elementwise float32 numpy rounds every operation on its own, which is what the kernels promise.  Also here: the two closed-form scenes of the tests
(a fronto-parallel plane seen by translated cameras, and the same with a patch of floaters), where every quantity is exact in float32."""
import numpy as np

import cloud_ref
import render_ref

F = np.float32
LIM = F(2 ** 20)


def camera_tables(cams2world, focals, shapes, pp=None, near=1e-3):
    """float32 [V, 16]: every view's own camera at its own shape (pp: None = the centre (W / 2, H / 2) of each view, one pair, or one pair per view)"""
    V = len(shapes)
    f = np.broadcast_to(np.asarray(focals, dtype=np.float64).reshape(-1), (V,))
    p = None if pp is None else np.broadcast_to(np.asarray(pp, dtype=np.float64).reshape(-1, 2), (V, 2))
    return np.concatenate([render_ref.camera_table([cams2world[v]], [f[v]], shapes[v], None if p is None else p[v], near) for v in range(V)])


def world_points(x_out, cams2world, local_pointmaps):
    """list of float32 [n, 3]"""
    if local_pointmaps:
        return [cloud_ref.geotrf(np.asarray(c, dtype=F)[:3, :4], np.asarray(x['pts3d_local'], dtype=F).reshape(-1, 3)) for c, x in zip(cams2world, x_out)]
    return [np.asarray(x['pts3d'], dtype=F).reshape(-1, 3) for x in x_out]


def own_depth(world, conf, cam, thr):
    """float32 [n]: zc where the view measured something, 0 elsewhere"""
    with np.errstate(over='ignore', invalid='ignore'):
        xc, yc, zc = render_ref.camera_coords(world, cam)
        ok = (np.asarray(conf, dtype=F).reshape(-1) >= F(thr)) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc >= cam[15])
    return np.where(ok, zc, F(0)).astype(F)


def compare(zc, d, rel_tol):
    """the test of one (point, measured depth) pair, float32 arrays -> (agree, violate); neither: occluded"""
    zc, d = np.asarray(zc, dtype=F), np.asarray(d, dtype=F)
    with np.errstate(over='ignore', invalid='ignore'):
        tol = F(rel_tol) * d
        agree = np.abs(zc - d) <= tol
        violate = ~agree & ((d - zc) > tol)
    return agree, violate


def project(world, cam, H, W):
    """-> (inside bool [n], cell int64 [n] = py W + px (0 where not inside), zc float32 [n])"""
    f, cx, cy, near = cam[12], cam[13], cam[14], cam[15]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        xc, yc, zc = render_ref.camera_coords(world, cam)
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc >= near)
        zs = np.where(ok, zc, F(1))
        u = (render_ref.quotient(f * xc, zs) + cx).astype(F)
        v = (render_ref.quotient(f * yc, zs) + cy).astype(F)
        ok &= (np.abs(u) <= LIM) & (np.abs(v) <= LIM)                                               # a NaN fails
        px = np.floor(np.where(ok, u, F(0)) + F(0.5)).astype(np.int64)
        py = np.floor(np.where(ok, v, F(0)) + F(0.5)).astype(np.int64)
    inside = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    return inside, np.where(inside, py * W + px, 0), zc


def consistency(x_out, cams2world, focals, min_conf_thr=3.0, rel_tol=0.03, pan=None, local_pointmaps=False, pp=None, near=1e-3):
    """x_out: list of dict(pts3d, pts3d_local [H,W,3], conf [H,W]) float32 arrays; pan: list of int [H,W] or None.
    -> dict(agree, violate int32 [N], same_label int32 [N] or None, depth float32 [N])"""
    shapes = [tuple(x['conf'].shape) for x in x_out]
    V = len(shapes)
    tab = camera_tables(cams2world, focals, shapes, pp, near)
    world = world_points(x_out, cams2world, local_pointmaps)
    depth = [own_depth(world[v], x_out[v]['conf'], tab[v], min_conf_thr) for v in range(V)]
    labels = None if pan is None else [np.asarray(p).reshape(-1).astype(np.int32) for p in pan]
    agree, violate, same = [], [], []
    for i in range(V):
        live = depth[i] != 0
        a, b, s = (np.zeros(len(depth[i]), dtype=np.int32) for _ in range(3))
        for j in range(V):
            if j == i:
                continue
            H, W = shapes[j]
            inside, cell, zc = project(world[i], tab[j], H, W)
            d = np.where(inside, depth[j][cell], F(0)).astype(F)
            seen = live & inside & (d != 0)
            ag, vi = compare(zc, d, rel_tol)
            a += seen & ag
            b += seen & vi
            if labels is not None:
                s += seen & ag & (labels[i] > 0) & (labels[j][cell] == labels[i])
        agree.append(a); violate.append(b); same.append(s)
    return {'agree': np.concatenate(agree), 'violate': np.concatenate(violate), 'same_label': None if pan is None else np.concatenate(same),
            'depth': np.concatenate(depth)}


def keep(res, min_views=1, max_violations=0):
    return (res['agree'] >= min_views) & (res['violate'] <= max_violations)


# ---------------------------------------------------------------- the closed-form scenes
PLANE_SHAPE, PLANE_F, PLANE_PP, PLANE_Z = (24, 32), 64.0, (16.0, 12.0), 2.0
PLANE_TX = (0.0, 0.25, -0.5, 0.75)
PATCH = (slice(6, 14), slice(10, 20))                                                              # rows, columns of view 0's floaters


def plane_scene(floaters=False):
    """The plane z = 2 seen by four 24 x 32 views with identity rotation, f = 64, pp = (16, 12) and translations t_x of PLANE_TX: every quantity is
    exact in float32, and pixel x of view i lands on pixel x + 32 (t_i - t_j) of view j.  With `floaters` the PATCH of view 0 sits at half depth
    (z = 1, on the same rays): those pixels land on x + 64 (t_0 - t_j).  Confidence 5 everywhere; panoptic id 1 + (x // 8) of the pixel's WORLD column
    band, so that agreeing pairs of the plane carry equal ids.  -> (x_out, cams2world, focals, pan)"""
    H, W = PLANE_SHAPE
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    x_out, cams, pan = [], [], []
    for v, tx in enumerate(PLANE_TX):
        z = np.full((H, W), PLANE_Z)
        if floaters and v == 0:
            z[PATCH] = PLANE_Z / 2
        loc = np.stack([(xs - PLANE_PP[0]) * z / PLANE_F, (ys - PLANE_PP[1]) * z / PLANE_F, z], axis=-1)
        c = np.eye(4)
        c[0, 3] = tx
        pts = loc + np.array([tx, 0.0, 0.0])
        assert np.array_equal(loc.astype(F).astype(np.float64), loc) and np.array_equal(pts.astype(F).astype(np.float64), pts)
        x_out.append({'pts3d': pts.astype(F), 'pts3d_local': loc.astype(F), 'conf': np.full((H, W), 5.0, dtype=F)})
        cams.append(c)
        pan.append((1 + np.floor((xs + 32 * tx) / 8)).astype(np.int32) + 10)
    return x_out, cams, [PLANE_F] * len(PLANE_TX), pan


def plane_closed_form(floaters=False):
    """(agree, violate) int32 [N] of plane_scene by counting, no projection: see its docstring"""
    H, W = PLANE_SHAPE
    V = len(PLANE_TX)
    agree, violate = np.zeros((V, H, W), dtype=np.int32), np.zeros((V, H, W), dtype=np.int32)
    patch = np.zeros((H, W), dtype=bool)
    if floaters:
        patch[PATCH] = True
    for i in range(V):
        for j in range(V):
            if j == i:
                continue
            for y in range(H):
                for x in range(W):
                    fl = i == 0 and patch[y, x]
                    xj = x + (64 if fl else 32) * (PLANE_TX[i] - PLANE_TX[j])
                    assert xj == int(xj)
                    xj = int(xj)
                    if not 0 <= xj < W:
                        continue                                                                   # unseen by j
                    if fl:
                        violate[i, y, x] += 1                                                      # z = 1 in front of j's z = 2
                    elif j == 0 and patch[y, xj]:
                        pass                                                                       # z = 2 behind view 0's floater at z = 1: occluded
                    else:
                        agree[i, y, x] += 1
    return agree.reshape(-1), violate.reshape(-1)


def _ray_view(H, W, f, pp, z, tx=0.0):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (H, W))
    loc = np.stack([(xs - pp[0]) * z / f, (ys - pp[1]) * z / f, z], axis=-1).astype(F)
    pts = loc.copy()
    pts[..., 0] += F(tx)
    return {'pts3d': pts, 'pts3d_local': loc, 'conf': np.full((H, W), 5.0, dtype=F)}


def edge_scene(zs):
    """two 2 x 4 views at ONE pose (identity, f = 64, pp = (2, 1)): view 1 is the plane z = 2, view 0 the same but for its first row, whose four pixels
    sit on their own rays at the depths `zs` - each lands on its own pixel of view 1 and meets d = 2 there.  -> (x_out, cams2world, focals)"""
    z0 = np.full((2, 4), PLANE_Z)
    z0[0] = np.asarray(zs, dtype=F)
    return [_ray_view(2, 4, 64.0, (2.0, 1.0), z0), _ray_view(2, 4, 64.0, (2.0, 1.0), PLANE_Z)], [np.eye(4), np.eye(4)], [64.0, 64.0]


def border_scene():
    """two 6 x 8 views at one pose (identity, f = 64, pp = (4, 3)), both the plane z = 2; eight pixels of view 0 are moved, at z = 2, to the projections
    u = 7.5 (rounds onto column W = 8: out), just below it (column 7: in), -0.5 (column 0: in) and just below that (column -1: out), and the same in v
    with rows H = 6, 5, 0, -1.  At z = 2 and f = 64, u = 32 X + 4 and v = 32 Y + 3 exactly.  -> (x_out, cams2world, focals, the flat indices of the
    eight pixels in view 0, whether each is inside)"""
    H, W, pp = 6, 8, (4.0, 3.0)
    a, b = _ray_view(H, W, 64.0, pp, PLANE_Z), _ray_view(H, W, 64.0, pp, PLANE_Z)
    lo = lambda t: F(F(t) - F(2.0 ** -21))                                      # one ulp of [4, 8) below: every step of the projection stays exact
    us = [(F(7.5), F(3.0), False), (lo(7.5), F(3.0), True), (F(-0.5), F(3.0), True), (lo(-0.5), F(3.0), False),
          (F(4.0), F(5.5), False), (F(4.0), lo(5.5), True), (F(4.0), F(-0.5), True), (F(4.0), lo(-0.5), False)]
    idx = []
    for k, (u, v, _) in enumerate(us):
        y, x = 1 + k // 4, 1 + k % 4
        p = np.array([(u - F(4.0)) / F(32.0), (v - F(3.0)) / F(32.0), F(2.0)], dtype=F)
        a['pts3d'][y, x] = p
        a['pts3d_local'][y, x] = p
        idx.append(y * W + x)
    return [a, b], [np.eye(4), np.eye(4)], [64.0, 64.0], idx, [s for _, _, s in us]


# ---------------------------------------------------------------- a seeded scene for the GPU tests
def _rotation(rng, deg):
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg) * rng.uniform(0.3, 1.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rotated_scene(shapes, seed=0, deg=12.0, spread=0.35):
    """Views of a bumpy wall around z = 2 from rotated, translated cameras near the origin: per pixel a ray of its own camera times a seeded depth in
    2 (1 +- spread), so that pairs agree, violate and occlude in comparable numbers at rel_tol ~ 0.1; pts3d is the world-frame point plus a little
    seeded noise (so the two `local_pointmaps` modes differ); confidences exp-like (> 1); panoptic ids 0 .. 3 in blocks of world position.
    -> (x_out, cams2world, focals, pan)"""
    rng = np.random.default_rng(seed)
    x_out, cams, focals, pan = [], [], [], []
    for H, W in shapes:
        f = 0.9 * max(H, W)
        c = np.eye(4)
        c[:3, :3], c[:3, 3] = _rotation(rng, deg), rng.uniform(-0.4, 0.4, 3) * np.array([1, 1, 0.3])
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        z = PLANE_Z * (1 + spread * rng.uniform(-1, 1, (H, W)) * (rng.uniform(0, 1, (H, W)) < 0.5))
        loc = np.stack([(xs - W / 2) * z / f, (ys - H / 2) * z / f, z], axis=-1).astype(F)
        c32 = c.astype(F)
        wpt = cloud_ref.geotrf(c32[:3, :4], loc.reshape(-1, 3)).reshape(H, W, 3)
        pts = (wpt + (rng.standard_normal((H, W, 3)) * 1e-3).astype(F)).astype(F)
        conf = (F(1.0) + np.exp(rng.standard_normal((H, W)).astype(F))).astype(F)
        ids = ((np.floor(wpt[..., 0] * 2) + np.floor(wpt[..., 1] * 2)).astype(np.int64) % 4).astype(np.int32)
        x_out.append({'pts3d': pts, 'pts3d_local': loc, 'conf': conf})
        cams.append(c32.astype(np.float64))
        focals.append(float(f))
        pan.append(ids)
    return x_out, cams, focals, pan
