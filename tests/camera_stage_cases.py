"""Shared by tests/test_hip_camera_stages.py (GPU) and tests/test_camera_stage_checks.py (CPU): constructed cases that hold the point splatter
(csrc/render.hip) and the triangle rasteriser (csrc/mesh.hip) to their contract at its DECISION EDGES - the pixel rules, the inclusive near / far / limit
tests, the top-left rule, the tie rules, the launch and path thresholds - where the seeded room scenes of test_hip_render.py / test_hip_mesh.py hold no
sample.  Nothing here imports the code under test.

The references are the yardsticks themselves: render_ref.splat / resolve and mesh_ref.setup / raster / resolve, per camera; the area filter is a few lines
of numpy here (`area_ref`).  Every comparison is bit for bit.  Most cases use the PIXEL CAMERA - identity pose, focal 1 (or another power of two),
principal point 0 - and points at zc = 1 or a power of two, so u = x / zc is exact in fp32 and what a case holds can be read off its numbers; every
group adds a seeded rotated pose, where the rounding order of the world -> camera step matters as well.

`splat_v`, `setup_v`, `raster_v`, `resolve_v` and `area_ref` restate the yardsticks' steps with one PLANTED MISTAKE each (`variant=`); without a variant
they equal the yardsticks on every case (tests/test_camera_stage_checks.py).  CAUGHT names, per mistake, the cases whose output it changes."""
import functools

import numpy as np

import mesh_ref as M
import render_ref as R
from geom_stage_cases import same_bits, first_difference, f32_bits, from_bits      # noqa: F401 (re-exported for the two test modules)

F = np.float32
U64 = np.uint64
EMPTY = R.EMPTY
LOW = U64(0xFFFFFFFF)
NEAR_S = F(0.5)                             # the splat cases' near plane unless a case says otherwise


def below(x):
    return np.nextafter(F(x), F(-np.inf))


def above(x):
    return np.nextafter(F(x), F(np.inf))


def bits1(x):
    """the bit pattern of one float32, as a Python int"""
    return int(f32_bits(x).reshape(-1)[0])


def key(depth, row):
    """(bits(depth) << 32) | row"""
    return (U64(bits1(depth)) << U64(32)) | U64(row)


def pose(seed, scale=1.0):
    """a seeded camera-to-world matrix: a proper rotation and a translation"""
    g = np.random.Generator(np.random.PCG64(seed))
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c = np.eye(4)
    c[:3, :3], c[:3, 3] = q, g.standard_normal(3) * scale
    return c


def to_world(local, c2w):
    """camera-frame points moved to the world in float64, rounded to float32: the camera sees them near where they were, after roundings of its own"""
    return (np.asarray(local, dtype=np.float64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(F)


def cam_row(tail, c2w=None):
    """one row of a device camera table, written by hand: [R^T | -R^T t] (the identity without a pose; render_ref.camera_table's float64 recipe with
    one), then `tail` = (f, cx, cy, near) for the splatter or (fx, fy, cx, cy) for the rasteriser"""
    row = np.zeros(16, dtype=F)
    if c2w is None:
        row[[0, 5, 10]] = 1
    else:
        row[:12] = R.camera_table([c2w], 1.0, (1, 1))[0, :12]
    row[12:] = tail
    return row


PIXEL_S = cam_row((1, 0, 0, NEAR_S))        # splatter: u = x / zc, v = y / zc
PIXEL_M = cam_row((1, 1, 0, 0))             # rasteriser: the same
PIXEL_S_NEG = np.where(PIXEL_S == 0, F(-0.0), PIXEL_S)      # ... with every zero of the row a -0.0: the only pose under which u = -0.0 can come out (x = -0.0, y, z > 0)


def soup_points(seed, n, H, W, f, zlo=2.0, zhi=6.0):
    """n seeded camera-frame points that project about the H x W image of a camera with focal f and the principal point at its centre"""
    g = np.random.Generator(np.random.PCG64(seed))
    z = g.uniform(zlo, zhi, n)
    return np.stack([g.uniform(-0.6, 0.6, n) * W * z / f, g.uniform(-0.6, 0.6, n) * H * z / f, z], axis=1)


# ================================================================================================================================ the splatter
def splat_v(points, cam, H, W, half_size, radius, max_radius, variant=None):
    """render_ref.splat's steps 1 - 5 -> zbuf uint64 [H * W], with one planted mistake:
      near_gt zc > near | lim_lt |u| < 2^20 | trunc truncation for floor | foot_f64 the footprint product in fp64, not rounded to fp32 | foot_ceil ceil for
      floor in the footprint | radius_replaces a non-zero radius replaces the point-size radius | int_before_clamp the footprint quotient converted to
      int32 before the clamp (+inf becomes INT_MIN) | tie_larger_row equal depths go to the larger row"""
    f, cx, cy, near = cam[12], cam[13], cam[14], cam[15]
    half_size = F(half_size)
    zbuf = np.full(H * W, EMPTY, dtype=U64)
    with np.errstate(all='ignore'):
        xc, yc, zc = R.camera_coords(points, cam)
        keep = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & ((zc > near) if variant == 'near_gt' else (zc >= near))
        rows = np.nonzero(keep)[0]
        xc, yc, zc = xc[keep], yc[keep], zc[keep]
        u = (R.quotient(f * xc, zc) + cx).astype(F)
        v = (R.quotient(f * yc, zc) + cy).astype(F)
        ok = ((np.abs(u) < R.LIM) & (np.abs(v) < R.LIM)) if variant == 'lim_lt' else ((np.abs(u) <= R.LIM) & (np.abs(v) <= R.LIM))
        rows, zc, u, v = rows[ok], zc[ok], u[ok], v[ok]
        rnd = np.trunc if variant == 'trunc' else np.floor
        px, py = rnd(u).astype(np.int64), rnd(v).astype(np.int64)
        prod = (np.float64(f) * np.float64(half_size)) if variant == 'foot_f64' else np.float64(F(f * half_size))
        q = (np.ceil if variant == 'foot_ceil' else np.floor)((prod / zc.astype(np.float64)).astype(F))
        if variant == 'int_before_clamp':
            rs = np.minimum(np.where(np.isfinite(q) & (q < 2.0 ** 31), q, -2.0 ** 31).astype(np.int64), max_radius)
        else:
            rs = np.minimum(q, F(max_radius)).astype(np.int64)
    r = np.minimum(max_radius, np.maximum(radius, rs))
    if variant == 'radius_replaces' and radius > 0:
        r = np.full_like(r, min(max_radius, radius))
    low = rows.astype(U64)
    if variant == 'tie_larger_row':
        low = LOW - low
    k = (np.ascontiguousarray(zc).view(np.uint32).astype(U64) << U64(32)) | low
    top = int(r.max()) if len(r) else -1
    for dy in range(-top, top + 1):
        for dx in range(-top, top + 1):
            xx, yy = px + dx, py + dy
            m = (r >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.minimum.at(zbuf, (yy * W + xx)[m], k[m])
    if variant == 'tie_larger_row':
        hit = zbuf != EMPTY
        zbuf[hit] = (zbuf[hit] & ~LOW) | (LOW - (zbuf[hit] & LOW))
    return zbuf


def S(points, cams, H, W, half=0.0, radius=0, max_radius=16):
    return dict(points=np.ascontiguousarray(points, dtype=F).reshape(-1, 3), cams=np.ascontiguousarray(cams, dtype=F).reshape(-1, 16), H=H, W=W, half=F(half),
                radius=radius, max_radius=max_radius)


def splat_zbuf(case, variant=None):
    """uint64 [B, H * W]: the yardstick (render_ref.splat) without a variant, splat_v with one"""
    args = (case['H'], case['W'], case['half'], case['radius'], case['max_radius'])
    if variant is None:
        return np.stack([R.splat(case['points'], cam, *args)[0] for cam in case['cams']])
    return np.stack([splat_v(case['points'], cam, *args, variant=variant) for cam in case['cams']])


def cloud_fields(M_):
    """rgb, colors float32 [M, 3] and pan int32 [M] that name their row: a gather from the wrong row shows in every field"""
    r = np.arange(M_, dtype=np.float64)
    return np.stack([r + 0.25, -r - 0.5, r * 3 + 0.125], axis=1).astype(F), np.stack([r * 2 + 1, r + 0.75, -r * 5 - 1], axis=1).astype(F), (r + 1).astype(np.int32)


U_EDGE = lambda n: [F(3), below(3), F(-0.0), F(-0.5), F(n), below(n)]          # an integer and one ulp below it, -0.0, inside (-1, 0), the image's edge


def _rotated_splat(seed, H, W, **kw):
    c2w = pose(seed)
    return S(to_world(soup_points(seed, 300, H, W, 16.0), c2w), cam_row((16, W / 2, H / 2, 0.25), c2w), H, W, **kw)


# FOOT_F64: f, half_size and zc for which floor((f half_size) / zc) is 2 with the product rounded to fp32 (it rounds UP, and zc is half of it) and 1 with
# the exact product; found by a search over seeded fp32 pairs and pinned (asserted in test_camera_stage_checks.py)
FOOT_F64 = (F(12.094573), F(0.09752318))


@functools.lru_cache(maxsize=None)
def splat_cases():
    """group -> {name: case}"""
    c = {g: {} for g in ('pixel', 'cull', 'limit', 'footprint', 'depth', 'launch')}
    # ---- pixel rule: 24 x 8 (u) and 8 x 24 (v); six points at zc = 1, three rows (columns) apart, so that at radius 1 no footprint meets another
    for r in (0, 1):
        pu = [(u, 1.5 + 3 * k, 1) for k, u in enumerate(U_EDGE(8))]
        pv = [(1.5 + 3 * k, v, 1) for k, v in enumerate(U_EDGE(8))]
        c['pixel']['u_r%d' % r] = S(pu, PIXEL_S_NEG, 24, 8, radius=r)
        c['pixel']['v_r%d' % r] = S(pv, PIXEL_S_NEG, 8, 24, radius=r)
    c['pixel']['rotated'] = _rotated_splat(11, 24, 32)
    # ---- cull: near = 0.5.  (1, 1, 0.5) -> pixel (2, 2), kept; one ulp nearer -> pixel (2, 4) if it were kept
    nb = below(NEAR_S)
    big = F(3e38)
    cull = [(1, 1, NEAR_S), (2 * nb, nb, nb), (0, 0, np.inf), (0, 0, -np.inf), (0, 0, np.nan), (0.5, 0.5, -1), (np.nan, 0.5, 1), (0.5, np.inf, 1),
            (-np.inf, 0.5, 1), (0.5, np.nan, 1), (big, big, 1), (5.5, 3.5, 1), (0, 0, 0.0)]
    c2w = pose(12)
    w = cam_row((1, 0, 0, NEAR_S), c2w)
    sign = np.where(w[:3] < 0, -1.0, 1.0)                                      # finite, and the three products of xc have one sign: their sum overflows ...
    cull[10] = tuple(big * sign * (1 if w[8:11].astype(np.float64) @ sign > 0 else -1))      # ... while zc stays finite and in front of the rotated camera
    c['cull']['planes_and_non_finite'] = S(cull, [PIXEL_S, cam_row((1, 0, 0, NEAR_S), c2w)], 6, 8)
    c['cull']['rotated'] = S(np.concatenate([to_world(soup_points(12, 200, 12, 16, 8.0, 0.2, 3.0), c2w), np.asarray(cull, dtype=F)]), cam_row((8, 8, 6, 1.0), c2w), 12, 16,
                             radius=1)
    # ---- limit: u == 2^20 lands in column 2^20 of a 1 x (2^20 + 2) image; the next fp32 (2^20 + 1/8) is dropped although floor(u) is that column too
    n = 2 ** 20
    c['limit']['u'] = S([(n, 0.5, 1), (above(n), 0.5, 1), (7, 0.5, 1), (-n, 0.5, 1)], PIXEL_S, 1, n + 2)
    c['limit']['v'] = S([(0.5, n, 1), (0.5, above(n), 1), (0.5, 7, 1), (0.5, -n, 1)], PIXEL_S, n + 2, 1)
    c['limit']['rotated'] = _rotated_splat(13, 6, 8)
    # ---- footprint: 41 x 41, f = 16, the point at pixel (20, 20).  (f half) / zc = 8 / zc
    cam = cam_row((16, 20.5, 20.5, 2.0 ** -126))
    fp = lambda z, **kw: S([(0, 0, z)], cam, 41, 41, **kw)
    c['footprint']['quotient_integer'] = fp(2, half=0.5)                                  # 8 / 2 = 4 exactly: r = 4
    c['footprint']['quotient_below_integer'] = fp(2, half=below(0.5))                     # 16 below(0.5) / 2 = below(4), every step exact: r = 3
    c['footprint']['radius_below_size'] = fp(2, half=0.5, radius=2)                       # max(2, 4) = 4
    c['footprint']['radius_above_size'] = fp(2, half=0.5, radius=6)                       # max(6, 4) = 6
    c['footprint']['max_below_radius'] = fp(2, half=0.5, radius=5, max_radius=3)          # min(3, max(5, 4)) = 3
    c['footprint']['quotient_inf'] = fp(2.0 ** -126, half=0.5)                            # 8 / 2^-126 = 2^129 -> +inf: r = max_radius = 16
    c['footprint']['half_zero'] = fp(2, half=0.0, radius=1)                               # floor(0 / zc) = 0: r = radius
    c['footprint']['clipped_on_four_sides'] = S([(0, 0, 2.0 ** -126)], cam_row((16, 3.5, 2.5, 2.0 ** -126)), 5, 7, half=0.5)     # r = 16 on 5 x 7
    f64f, f64h = FOOT_F64
    c['footprint']['product_fp32_not_fp64'] = S([(0, 0, F(f64f * f64h) / F(2))], cam_row((f64f, 20.5, 20.5, 2.0 ** -126)), 41, 41, half=f64h)
    c['footprint']['rotated'] = _rotated_splat(14, 24, 32, half=0.3, radius=1, max_radius=5)
    # ---- depth and ties, 8 x 8: rows 3 and 300 (two workgroups) hold one point; row 5 is one ulp deeper than row 6; rows 1, 3, 4 of the last are one point
    p = np.tile(np.asarray([[0.5, 0.5, -1]], dtype=F), (301, 1))
    p[3] = p[300] = (2.5, 2.5, 1)
    p[5], p[6] = (5.5 * above(1), 2.5 * above(1), above(1)), (5.5, 2.5, 1)
    c['depth']['rows_3_and_300'] = S(p, PIXEL_S, 8, 8)
    c['depth']['rows_1_3_4'] = S([(90, 90, 5), (13.5, 10.5, 3), (-90, 90, 5), (13.5, 10.5, 3), (13.5, 10.5, 3)], PIXEL_S, 8, 8, radius=1)
    c['depth']['rotated'] = _rotated_splat(15, 8, 8, radius=3)
    # ---- launch edges
    for m in (1, 255, 256, 257):
        p = np.tile(np.asarray([[0.5, 0.5, -1]], dtype=F), (m, 1))
        p[m - 1] = (2.5, 1.5, 1)
        c['launch']['M_%d' % m] = S(p, PIXEL_S, 6, 8)
    c2w = [pose(16), pose(17), np.eye(4)]
    pts = np.concatenate([to_world(soup_points(16 + k, 100, 12, 16, 8.0), c2w[k]) for k in range(3)])
    c['launch']['three_cameras'] = S(pts, [cam_row((8, 8, 6, 3.0), c2w[0]), cam_row((16, 7, 5, 0.5), c2w[1]), cam_row((4, 9, 6.5, 4.0), c2w[2])], 12, 16, radius=1)
    c['launch']['rotated'] = _rotated_splat(18, 37, 51, radius=2)
    return c


MANY_B = 65535


def many_cameras():
    """65 535 cameras of 1 x 1 pixel over three points (2 k 2^k, 0.5 2^k, 2^k): u = 2 k + cx, v = 0.5.  Camera b has cx = -2 (b mod 3) and near = 2^((b mod 5) - 2): it sees
    point b mod 3 alone (the other two have u = +-2, +-4) unless that point is nearer than its near plane.  -> (case, zbuf uint64 [B, 1] written out from this rule;
    the check module holds it against render_ref.splat on a sample of the cameras)"""
    b = np.arange(MANY_B)
    k = b % 3
    near = (2.0 ** (b % 5 - 2)).astype(F)
    cams = np.zeros((MANY_B, 16), dtype=F)
    cams[:, [0, 5, 10]] = 1
    cams[:, 12], cams[:, 13], cams[:, 15] = 1, -2.0 * k, near
    z = (2.0 ** k).astype(F)
    want = np.where(z >= near, (z.view(np.uint32).astype(U64) << U64(32)) | k.astype(U64), EMPTY)
    return S([(2 * i * 2.0 ** i, 0.5 * 2.0 ** i, 2.0 ** i) for i in range(3)], cams, 1, 1), want.reshape(MANY_B, 1)


RESOLVE_M = 10


def render_resolve_case(npix, seed=0):
    """a hand-made z-buffer of npix cells over a cloud of 10 rows: random valid keys with arbitrary depth bits, then the cells the contract names"""
    g = np.random.Generator(np.random.PCG64(seed + npix))
    z = (g.integers(0, 2 ** 32, npix, dtype=np.uint64) << U64(32)) | g.integers(0, RESOLVE_M, npix, dtype=np.uint64)
    z[0] = EMPTY
    z[1] = key(1.5, RESOLVE_M - 1)
    z[2] = key(1.5, RESOLVE_M)                                                 # the guard: a row >= M is an empty cell
    z[3] = key(1.5, 2 ** 32 - 1)
    z[4] = (U64(0x7FC00001) << U64(32)) | U64(4)                               # a NaN's bits come back as they are
    z[5] = (U64(0xFFFFFFFF) << U64(32)) | U64(5)
    z[6] = (U64(0x80000000) << U64(32)) | U64(0)                               # -0.0
    z[npix - 1] = key(2.0, RESOLVE_M - 1)
    z[npix - 2] = EMPTY
    return z


# ================================================================================================================================ the rasteriser
def setup_v(vertices, faces, cam, H, W, near, variant=None):
    """mesh_ref.snap and mesh_ref.setup (steps 2, 3 and the bounding box), with one planted mistake:
      zc_near_gt zc > near | lim_lt |u| < 2^14 | snap_half_up floor(x + 0.5) | snap_half_away | all_inclusive, all_exclusive, bottom_right, no_top_edge the
      coverage rule | box_in j0 / i0 one pixel too far in ((lo + 128) >> 8)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Nv = len(vertices)
    with np.errstate(all='ignore'):
        xc, yc, zc = R.camera_coords(vertices, cam)
        u = (R.quotient(cam[12] * xc, zc) + cam[14]).astype(F)
        v = (R.quotient(cam[13] * yc, zc) + cam[15]).astype(F)
        lim = ((np.abs(u) < M.LIM) & (np.abs(v) < M.LIM)) if variant == 'lim_lt' else ((np.abs(u) <= M.LIM) & (np.abs(v) <= M.LIM))
        usable = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & np.isfinite(u) & np.isfinite(v) & ((zc > F(near)) if variant == 'zc_near_gt' else (zc >= F(near))) & lim
        snap = {'snap_half_up': lambda a: np.floor(a.astype(np.float64) + 0.5), 'snap_half_away': lambda a: np.sign(a) * np.floor(np.abs(a.astype(np.float64)) + 0.5)}.get(variant, np.rint)
        X = np.where(usable, snap(np.where(usable, u, 0) * F(256)), 0).astype(np.int64)
        Y = np.where(usable, snap(np.where(usable, v, 0) * F(256)), 0).astype(np.int64)
    inside = ((faces >= 0) & (faces < Nv)).all(axis=1)
    idx = np.where(inside[:, None], faces, 0)
    ok = inside & usable[idx].all(axis=1)
    fx, fy, fz = X[idx], Y[idx], zc[idx]
    A = (fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fy[:, 1] - fy[:, 0]) * (fx[:, 2] - fx[:, 0])
    ok &= A != 0
    swapped = A < 0
    order = np.where(swapped[:, None], [0, 2, 1], [0, 1, 2])
    fx, fy, fz = (np.take_along_axis(t, order, axis=1) for t in (fx, fy, fz))
    A = np.abs(A)
    a, b = [c[0] for c in M.CORNERS], [c[1] for c in M.CORNERS]
    dx, dy = fx[:, b] - fx[:, a], fy[:, b] - fy[:, a]
    least = {'all_inclusive': np.zeros_like(dx), 'all_exclusive': np.ones_like(dx), 'bottom_right': np.where((dy > 0) | ((dy == 0) & (dx < 0)), 0, 1),
             'no_top_edge': np.where(dy < 0, 0, 1)}.get(variant, np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1))
    lo = 128 if variant == 'box_in' else 127
    j0, j1 = np.maximum((fx.min(axis=1) + lo) >> 8, 0), np.minimum((fx.max(axis=1) - 128) >> 8, W - 1)
    i0, i1 = np.maximum((fy.min(axis=1) + lo) >> 8, 0), np.minimum((fy.max(axis=1) - 128) >> 8, H - 1)
    ok &= (j0 <= j1) & (i0 <= i1)
    box = np.where(ok, (j1 - j0 + 1) * (i1 - i0 + 1), 0)
    with np.errstate(all='ignore'):
        q = 1.0 / fz.astype(np.float64)
    return dict(ok=ok, usable=inside & usable[idx].all(axis=1), X=fx, Y=fy, xa=fx[:, a], ya=fy[:, a], dx=dx, dy=dy, least=least, A=A, q=q, swapped=swapped,
                j0=j0, j1=j1, i0=i0, i1=i1, box=box)


def raster_v(s, H, W, near, far, variant=None):
    """mesh_ref.raster (steps 4 - 6) -> zbuf uint64 [H * W], with one planted mistake:
      depth_near_gt depth > near | depth_far_lt depth < far | assoc_other s = E0 q0 + (E1 q1 + E2 q2) | tie_larger_face equal depths go to the larger face"""
    zbuf = np.full(H * W, EMPTY, dtype=U64)
    for f in np.nonzero(s['ok'])[0]:
        ii, jj = np.arange(s['i0'][f], s['i1'][f] + 1)[:, None], np.arange(s['j0'][f], s['j1'][f] + 1)[None, :]
        E = M.edges(s, f, ii, jj)
        cov = (E[0] >= s['least'][f, 0]) & (E[1] >= s['least'][f, 1]) & (E[2] >= s['least'][f, 2])
        with np.errstate(all='ignore'):
            q = s['q'][f]
            e = [E[k].astype(np.float64) * q[k] for k in range(3)]
            t = (e[0] + (e[1] + e[2])) if variant == 'assoc_other' else ((e[0] + e[1]) + e[2])
            depth = (np.float64(s['A'][f]) / t).astype(F)
            lo = (depth > F(near)) if variant == 'depth_near_gt' else (depth >= F(near))
            hi = (depth < F(far)) if variant == 'depth_far_lt' else (depth <= F(far))
            keep = cov & np.isfinite(depth) & lo & hi
        low = (LOW - U64(f)) if variant == 'tie_larger_face' else U64(f)
        np.minimum.at(zbuf, (ii * W + jj)[keep], (np.ascontiguousarray(depth[keep]).view(np.uint32).astype(U64) << U64(32)) | low)
    if variant == 'tie_larger_face':
        hit = zbuf != EMPTY
        zbuf[hit] = (zbuf[hit] & ~LOW) | (LOW - (zbuf[hit] & LOW))
    return zbuf


def resolve_v(zbuf, s, faces, H, W, vertex_ids=None, face_ids=None, variant=None):
    """mesh_ref.resolve (step 7) -> (face, depth, pan), with one planted mistake:
      corner_unswapped the E_k taken in the order after the exchange of corners 1 and 2, not as listed | tie_last_corner ties go to the last corner"""
    if variant is None:
        return M.resolve(zbuf, s, faces, H, W, vertex_ids, face_ids)[:3]
    low = zbuf & LOW
    hit = (zbuf != EMPTY) & (low < U64(len(s['ok'])))
    face = np.where(hit, low, U64(0)).astype(np.int64)
    depth = np.where(hit, (zbuf >> U64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    pix = np.arange(H * W)
    E = M.edges(s, face, pix // W, pix % W)
    sw = s['swapped'][face] & (variant != 'corner_unswapped')
    listed = [E[0], np.where(sw, E[2], E[1]), np.where(sw, E[1], E[2])]
    best = np.maximum(np.maximum(listed[0], listed[1]), listed[2])
    if variant == 'tie_last_corner':
        pos = np.where(listed[2] == best, 2, np.where(listed[1] == best, 1, 0))
    else:
        pos = np.where(listed[0] == best, 0, np.where(listed[1] == best, 1, 2))
    pan = np.zeros(H * W, dtype=np.int32)
    if face_ids is not None:
        pan = np.where(hit, np.asarray(face_ids, dtype=np.int32)[face], 0).astype(np.int32)
    elif vertex_ids is not None:
        seen = hit & s['ok'][face]
        corner = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face, pos]
        pan = np.where(seen, np.asarray(vertex_ids, dtype=np.int32)[np.where(seen, corner, 0)], 0).astype(np.int32)
    return np.where(hit, face, -1), depth, pan


SETUP_VARIANTS = ('zc_near_gt', 'lim_lt', 'snap_half_up', 'snap_half_away', 'all_inclusive', 'all_exclusive', 'bottom_right', 'no_top_edge', 'box_in')
RASTER_VARIANTS = ('depth_near_gt', 'depth_far_lt', 'assoc_other', 'tie_larger_face')
RESOLVE_VARIANTS = ('corner_unswapped', 'tie_last_corner')


def T(vertices, faces, cams=PIXEL_M, H=12, W=16, near=0.5, far=10.0, vertex_ids=None, face_ids=None, capacities=(None,)):
    """capacities: the big_capacity values the GPU test runs the case with (None: one entry per (camera, face))"""
    vertices = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    ids = lambda t: None if t is None else np.ascontiguousarray(t, dtype=np.int32)
    return dict(vertices=vertices, faces=faces, cams=np.ascontiguousarray(cams, dtype=F).reshape(-1, 16), H=H, W=W, near=F(near), far=F(far), vertex_ids=ids(vertex_ids),
                face_ids=ids(face_ids), capacities=tuple(capacities))


def mesh_setups(case, variant=None):
    v = variant if variant in SETUP_VARIANTS else None
    if v is None:
        return [M.setup(case['vertices'], case['faces'], cam, case['H'], case['W'], case['near']) for cam in case['cams']]
    return [setup_v(case['vertices'], case['faces'], cam, case['H'], case['W'], case['near'], v) for cam in case['cams']]


def mesh_zbuf(case, variant=None, setups=None):
    """uint64 [B, H * W]: the yardstick (mesh_ref.setup, mesh_ref.raster) without a variant"""
    setups = mesh_setups(case, variant) if setups is None else setups
    if variant is None:
        return np.stack([M.raster(s, case['H'], case['W'], case['near'], case['far'])[0] for s in setups])
    return np.stack([raster_v(s, case['H'], case['W'], case['near'], case['far'], variant if variant in RASTER_VARIANTS else None) for s in setups])


def mesh_resolved(case, zbuf, kind, variant=None, setups=None):
    """kind 'vertex' / 'face' / 'none': which of the case's ids go in -> (face int64, depth float32, pan int32), each [B, H * W]; the setups are the
    yardstick's (a resolve variant changes step 7 alone)"""
    setups = mesh_setups(case) if setups is None else setups
    vid = case['vertex_ids'] if kind == 'vertex' else None
    fid = case['face_ids'] if kind == 'face' else None
    out = [resolve_v(z, s, case['faces'], case['H'], case['W'], vid, fid, variant if variant in RESOLVE_VARIANTS else None) for z, s in zip(zbuf, setups)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def inside_quad(quad, H, W):
    """exact, in integers (coordinates x 4): +1 strictly inside the convex quad, 0 on its boundary, -1 outside, per pixel centre"""
    q = np.rint(np.asarray(quad) * 4).astype(np.int64)
    py, px = np.meshgrid(4 * np.arange(H) + 2, 4 * np.arange(W) + 2, indexing='ij')
    sides = []
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        sides.append((b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0]))
    s = np.stack(sides)
    if sum(q[k][0] * q[(k + 1) % 4][1] - q[(k + 1) % 4][0] * q[k][1] for k in range(4)) < 0:
        s = -s                                                                 # the other orientation
    return np.where((s > 0).all(axis=0), 1, np.where((s >= 0).all(axis=0), 0, -1))


QUADS = [
    [(2.5, 2.5), (9.5, 2.5), (9.5, 7.5), (2.5, 7.5)],                          # every edge through pixel centres, both diagonals too (a 7 x 5 box: one is not)
    [(3.5, 1.5), (8.5, 1.5), (8.5, 6.5), (3.5, 6.5)],                          # a square: both diagonals through pixel centres
    [(1.0, 1.0), (12.0, 2.0), (11.0, 9.0), (2.0, 8.0)],
    [(4.5, 0.5), (10.5, 4.5), (6.5, 10.5), (0.5, 6.5)],                        # a tilted square, corners on pixel centres
    [(2.25, 3.75), (11.75, 1.25), (13.5, 8.5), (3.5, 9.75)],
]
QUAD_SHAPE = (12, 16)


def quad_faces(reverse, diagonal):
    faces = [(0, 1, 2), (0, 2, 3)] if diagonal == 0 else [(1, 2, 3), (1, 3, 0)]
    return [f[::-1] for f in faces] if reverse else faces


STRIP_XS, STRIP_YS = [1.5, 5.5, 9.5, 13.5], [1.5, 5.5, 9.5]


def strip():
    """the 2 x 3 strip of split quads whose shared edges run through pixel centres -> (vertices, faces)"""
    verts = np.array([(x, y, 1.0) for y in STRIP_YS for x in STRIP_XS], dtype=F)
    k = lambda r, c: r * 4 + c
    faces = []
    for r in range(2):
        for c in range(3):
            a, b, d, e = k(r, c), k(r, c + 1), k(r + 1, c + 1), k(r + 1, c)
            faces += [(a, b, d), (a, d, e)] if (r + c) % 2 else [(b, d, e), (b, e, a)]
    return verts, faces


def uv(points, z=1.0):
    """vertices at depth z that the pixel camera sees at the listed (u, v); z a scalar or one per point.  Exact for the dyadic numbers used here"""
    p = np.asarray(points, dtype=np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(p),))
    return np.stack([p[:, 0] * z, p[:, 1] * z, z], axis=1).astype(F)


def soup_mesh(seed, n, H, W, f):
    """n seeded camera-frame triangles of a few pixels each -> (vertices [3 n, 3], faces [n, 3])"""
    g = np.random.Generator(np.random.PCG64(seed))
    centre = soup_points(seed, n, H, W, f)
    v = centre[:, None, :] + g.uniform(-1, 1, (n, 3, 3)) * [0.15 * W / f * 3, 0.15 * H / f * 3, 0.5]
    return v.reshape(-1, 3), np.arange(3 * n).reshape(n, 3)


def _rotated_mesh(seed, H, W, n=60, **kw):
    c2w = pose(seed)
    v, f = soup_mesh(seed, n, H, W, 16.0)
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    return T(to_world(v, c2w), f, cam_row((16, 15.5, W / 2, H / 2), c2w), H, W, vertex_ids=g.integers(1, 50, len(v)), face_ids=g.integers(1, 50, len(f)), **kw)


# SNAP: per class of half-way vertex the triangle (in 1/256 pixel: A's X is the half-way coordinate, everything else an integer) whose coverage of the
# 4 x 4 image changes when A snaps by another rule; found by a search over B's X and pinned.  256 u = k + 0.5 at u = (2 k + 1) / 512.
SNAP = {                                   # name: (u of A as a multiple of 1 / 512, (B, D) in 1 / 256 pixel); A's v is 0
    'positive_even': (257, ((640, 256), (900, 0))),
    'negative_odd': (-255, ((384, 256), (900, 0))),
    'negative_even': (-257, ((385, 256), (900, 0))),
}

# ASSOC: a tilted face, corners in 1/256 pixel with their zc, built so that at the pixel ASSOC_PIXEL the two associations of s part: there E0 = 2^20 and
# A = 17 631 603 (odd, 25 bits, 3 mod 4), so A / (E0 q0) = A 2^-20 lies half-way between two fp32 values and rounds to the even one above; E1 q1 and E2 q2
# are 0.39 and 0.29 of the last place of E0 q0 - (E0 q0 + E1 q1) + E2 q2 stays E0 q0 while E0 q0 + (E1 q1 + E2 q2) is one place larger, and the quotient
# falls below the half-way point
ASSOC = [((283, 284), 1.0), ((7808, 6281), 2.0 ** 56), ((6784, 7808), 2.0 ** 57)]
ASSOC_PIXEL, ASSOC_SHAPE, ASSOC_FAR = (26, 26), (32, 32), 2.0 ** 100

TIE_TRIANGLE = [(1.5, 2.0), (9.5, 2.0), (5.5, 10.0)]                           # symmetric about the pixel centres u = 5.5
TIE_LISTINGS = ([(0, 1, 2)], [(1, 0, 2)], [(2, 1, 0)], [(2, 0, 1)])
PATH_BOXES = {'8x8': [(10.25, 5.25), (17.75, 5.25), (10.25, 12.75)], '13x5': [(20.25, 5.25), (32.75, 5.25), (20.25, 9.75)],
              '5x13': [(40.25, 5.25), (44.75, 5.25), (40.25, 17.75)], '7x10': [(50.25, 5.25), (56.75, 5.25), (50.25, 14.75)],
              '65x1': [(-70, 30.25), (65.25, 30.25), (65.25, 30.75)], '1x65': [(68.25, -70), (68.25, 65.25), (68.75, 65.25)]}
PATH_PIXELS = {'8x8': 64, '13x5': 65, '5x13': 65, '7x10': 70, '65x1': 65, '1x65': 65}
STRIDE_H, STRIDE_W, STRIDE_B = 2049, 65, 5
BIG_WAVES = 8192                            # MS_BIG_BLOCKS x 4 waves: the wave path strides its list beyond this many entries


@functools.lru_cache(maxsize=None)
def mesh_cases():
    """group -> {name: case}"""
    c = {g: {} for g in ('topleft', 'snap', 'planes', 'limit', 'bad', 'corner', 'depth', 'duplicate', 'paths', 'launch')}
    # ---- the top-left rule
    for qi, quad in enumerate(QUADS):
        for reverse in (False, True):
            for diagonal in (0, 1):
                c['topleft']['quad%d_%s_d%d' % (qi, 'rev' if reverse else 'fwd', diagonal)] = T(uv(quad), quad_faces(reverse, diagonal), face_ids=[5, 6])
    v, f = strip()
    c['topleft']['strip'] = T(v, f, face_ids=np.arange(1, len(f) + 1))
    c['topleft']['rotated'] = _rotated_mesh(21, 24, 32)
    # ---- snap
    for name, (ua, (b, d)) in SNAP.items():
        c['snap'][name] = T(uv([(ua / 512, 0), (b[0] / 256, b[1] / 256), (d[0] / 256, d[1] / 256)]), [(0, 1, 2)], H=4, W=4, face_ids=[3])
    c['snap']['rotated'] = _rotated_mesh(22, 12, 16)
    # ---- planes: near = 0.5, far = 8.  A corner on the pixel centre (2.5, 2.5) with a top and a left edge is covered, and its depth there is its own zc
    tri = [(2.5, 2.5), (9.5, 2.5), (2.5, 7.5)]
    pl = lambda z, **kw: T(uv(tri, z), [(0, 1, 2)], near=0.5, far=8.0, face_ids=[9], **kw)
    c['planes']['at_near'], c['planes']['at_far'] = pl(0.5), pl(8.0)
    c['planes']['beyond_near'], c['planes']['beyond_far'] = pl(below(0.5)), pl(above(8.0))
    c['planes']['corner_at_near'], c['planes']['corner_at_far'] = pl([0.5, 1.0, 2.0]), pl([8.0, 4.0, 2.0])
    c['planes']['corner_below_near'] = pl([below(0.5), 1.0, 2.0])
    c['planes']['rotated'] = _rotated_mesh(23, 24, 32, near=3.0, far=4.5)
    # ---- limit: a vertex at u == 2^14 is usable, the next fp32 is not and the face goes whole
    n = 2 ** 14
    lim = lambda top: T(uv([(top, 0), (n - 8, 0), (n - 8, 4)]), [(0, 1, 2)], H=1, W=n + 2, face_ids=[4])
    c['limit']['at'], c['limit']['beyond'] = lim(n), lim(above(n))
    lim = lambda top: T(uv([(0, top), (0, n - 8), (4, n - 8)]), [(0, 1, 2)], H=n + 2, W=1, face_ids=[4])
    c['limit']['at_v'], c['limit']['beyond_v'] = lim(n), lim(above(n))
    c['limit']['rotated'] = _rotated_mesh(24, 6, 8)
    # ---- bad faces next to a good one
    v = np.concatenate([uv([(2, 2), (10, 2), (2, 10)]), [(np.nan, 0, 1), (np.inf, 1, 1), (4, 4, 0.4)], uv([(1, 1), (2, 2), (3, 3 + 1 / 1024)])]).astype(F)
    bad = [(0, 1, 3), (0, 1, 4), (0, 1, -1), (0, 1, len(v)), (0, 0, 1), (6, 7, 8), (0, 1, 5), (0, 1, 2)]
    c['bad']['every_kind'] = T(v, bad, face_ids=np.arange(1, len(bad) + 1), vertex_ids=np.arange(1, len(v) + 1))
    c['bad']['rotated'] = _rotated_mesh(25, 12, 16)
    # ---- the nearest corner
    for k, faces in enumerate(TIE_LISTINGS):
        c['corner']['tie_listing%d' % k] = T(uv(TIE_TRIANGLE), faces, vertex_ids=[10, 20, 30], face_ids=[7])
    c['corner']['clockwise_no_tie'] = T(uv([(1.25, 1.0), (3.75, 10.25), (14.0, 2.5)]), [(0, 1, 2)], vertex_ids=[10, 20, 30], face_ids=[7])
    c['corner']['rotated'] = _rotated_mesh(26, 24, 32)
    # ---- depth: the association of the three-term sum
    av = uv([(x / 256, y / 256) for (x, y), z in ASSOC], [z for p, z in ASSOC])
    for name, faces in (('assoc_listed', [(0, 1, 2)]), ('assoc_swapped', [(0, 2, 1)])):
        c['depth'][name] = T(av, faces, H=ASSOC_SHAPE[0], W=ASSOC_SHAPE[1], near=0.5, far=ASSOC_FAR, face_ids=[1])
    c['depth']['rotated'] = _rotated_mesh(27, 12, 16, n=20)
    # ---- duplicates: faces 2 and 300 (two workgroups) are one triangle; every other face repeats a corner
    f = np.zeros((301, 3), dtype=np.int64)
    f[2] = f[300] = (0, 1, 2)
    c['duplicate']['faces_2_and_300'] = T(uv(tri), f, face_ids=np.arange(1, 302))
    r = _rotated_mesh(28, 12, 16, n=20)                                        # every face of the soup fourteen times, 280 faces: the copies meet across workgroups
    c['duplicate']['rotated'] = T(r['vertices'], np.tile(r['faces'], (14, 1)), r['cams'], 12, 16, face_ids=np.arange(1, 281))
    # ---- the two paths, 72 x 72: one face per box, and one larger than the image behind them all
    v = np.concatenate([uv(p) for p in PATH_BOXES.values()] + [uv([(-100, -100), (300, -100), (-100, 300)], 4.0)])
    nbig = sum(n > 64 for n in PATH_PIXELS.values()) + 1
    c['paths']['boxes'] = T(v, np.arange(len(v)).reshape(-1, 3), H=72, W=72, face_ids=np.arange(1, len(v) // 3 + 1), capacities=(nbig, nbig - 1, 0, 1, None))
    c['paths']['rotated'] = _rotated_mesh(29, 48, 64, n=40, capacities=(None, 0, 3))
    # ---- launch edges: the last face alone is visible
    for nf in (1, 255, 256, 257):
        f = np.zeros((nf, 3), dtype=np.int64)
        f[nf - 1] = (0, 1, 2)
        c['launch']['Nf_%d' % nf] = T(uv(tri), f, face_ids=np.arange(1, nf + 1))
    c2w = [pose(30), pose(31), np.eye(4)]
    parts = [soup_mesh(30 + k, 30, 24, 32, 16.0) for k in range(3)]
    v = np.concatenate([to_world(p[0], c2w[k]) for k, p in enumerate(parts)])
    g = np.random.Generator(np.random.PCG64(30))
    c['launch']['three_cameras'] = T(v, np.arange(len(v)).reshape(-1, 3), [cam_row((16, 15, 16, 12), c2w[0]), cam_row((12, 17.5, 15.25, 11.5), c2w[1]), cam_row((20, 16, 17, 13), c2w[2])],
                                     24, 32, near=0.5, far=10.0, vertex_ids=g.integers(1, 50, len(v)), face_ids=g.integers(1, 50, len(v) // 3))
    c['launch']['rotated'] = _rotated_mesh(32, 37, 51)
    return c


@functools.lru_cache(maxsize=None)
def stride_case():
    """2 049 x 65, five cameras, one sliver face per image row with a 65 x 1 bounding box: 10 245 (camera, face) entries of 65 pixels each, every one the
    only face of its row in its camera - an entry the wave path skipped or took twice from another slot leaves an empty or a wrong row"""
    i = np.arange(STRIDE_H, dtype=np.float64)
    v = np.stack([np.stack([np.full_like(i, -70), i + 0.25], 1), np.stack([np.full_like(i, 65.25), i + 0.25], 1), np.stack([np.full_like(i, 65.25), i + 0.75], 1)], axis=1)
    cams = [cam_row((1, 1, b / 8, b / 32)) for b in range(STRIDE_B)]           # u + b / 8, v + b / 32: the box stays 65 x 1
    n = STRIDE_H * STRIDE_B
    return T(uv(v.reshape(-1, 2)), np.arange(3 * STRIDE_H).reshape(-1, 3), cams, STRIDE_H, STRIDE_W, face_ids=np.arange(1, STRIDE_H + 1), capacities=(n, BIG_WAVES))


def mesh_resolve_case():
    """hand-made z-buffers for two cameras of 5 x 7 = 35 pixels: cell 34 is camera 0's last pixel and cell 35 camera 1's first, with one key in both"""
    v = np.concatenate([uv([(0.25, 0.25), (6.75, 0.5), (3.0, 4.75)]), uv([(1, 1), (5, 1), (1, 4)], 0.4), uv([(1, 1), (5, 1), (3, 4)], 2.0)])
    faces = [(0, 1, 2), (3, 4, 5), (6, 8, 7)]                                  # face 1 is nearer than near in both cameras: it leaves no trace
    case = T(v, faces, [PIXEL_M, cam_row((1, 1, -3.5, 1.5))], 5, 7, near=0.5, far=10.0, vertex_ids=np.arange(11, 20), face_ids=[101, 102, 103])
    z = np.full((2, 35), EMPTY, dtype=U64)
    z[0, 34] = z[1, 0] = key(1.0, 0)                                           # the camera boundary at p / (H W)
    z[0, 0], z[1, 34] = key(1.0, 0), key(1.0, 0)
    z[0, 1] = key(1.25, 3)                                                     # the guard: face == Nf is an empty cell
    z[0, 2] = key(1.25, 2 ** 32 - 1)
    z[0, 3], z[1, 3] = key(0.75, 1), key(0.75, 1)                              # an unusable face under vertex_ids: id 0, face and depth from the key
    z[0, 10], z[1, 10] = key(2.0, 2), key(2.0, 2)                              # a swapped face
    z[1, 17] = (U64(0x7FC00001) << U64(32)) | U64(2)
    return case, z


# ================================================================================================================================ the area filter
def area_ref(pan, id2row, S_, min_area, variant=None):
    """step 8 over id2row directly: pan int32 [B, hw] -> (counts int32 [B, S], out int32 [B, hw]).  variant 'drop_cross_camera_run': a run of one row
    over adjacent pixels of one 64-lane wave that crosses a camera boundary is not counted (the key of the wave merge without its camera)"""
    pan, id2row = np.asarray(pan, dtype=np.int32), np.asarray(id2row, dtype=np.int32)
    B, hw = pan.shape
    ntab = len(id2row)
    inside = (pan > 0) & (pan < ntab)
    row = np.where(inside, id2row[np.where(inside, pan, 0)], -1)
    row = np.where((row >= 0) & (row < S_), row, -1)
    counts = np.zeros((B, S_), dtype=np.int32)
    flat = row.reshape(-1)
    p = 0
    while p < len(flat):
        e = p + 1
        while e < len(flat) and e // 64 == p // 64 and flat[e] == flat[p] and (variant == 'drop_cross_camera_run' or e // hw == p // hw):
            e += 1
        if flat[p] >= 0 and (e - 1) // hw == p // hw:
            counts[p // hw, flat[p]] += e - p
        p = e
    out = np.where((row >= 0) & (np.take_along_axis(counts, np.maximum(row, 0), axis=1) >= min_area), pan, 0).astype(np.int32)
    return counts, out


AREA_HW = 100
AREA_NTAB, AREA_S = 12, 4
AREA_ID2ROW = np.asarray([2, 0, 1, 2, 3, -1, AREA_S, 0, -5, 1, 3, 2], dtype=np.int32)     # id 0's entry is never read; id 5 -> -1, id 6 -> S, id 8 -> -5; 1 and 7, 2 and 9 share rows
AREA_MIN = 40


def area_cases():
    """name -> pan int32 [B, 100] (hw = 100 is no multiple of 64: cameras begin inside waves)"""
    c = {}
    runs = np.zeros((8, AREA_HW), dtype=np.int32).reshape(-1)
    at = 3
    for n, i in ((63, 1), (64, 2), (65, 3), (257, 4), (40, 10), (39, 11)):      # runs across wave (64), workgroup (256) and camera (100) edges
        runs[at:at + n] = i
        at += n + 2
    c['runs'] = runs.reshape(8, AREA_HW)
    cross = np.zeros((3, AREA_HW), dtype=np.int32)
    cross[0, 70:], cross[1, :20] = 3, 3                                         # pixels 70 .. 119 of the flat map: one run inside the wave 64 .. 127, two cameras
    cross[1, 60:], cross[2, :28] = 1, 7                                         # ids 1 and 7 share row 0: the key changes at the boundary, the row does not
    c['across_a_camera'] = cross
    g = np.random.Generator(np.random.PCG64(40))
    ids = np.asarray([0, -1, -(2 ** 31), AREA_NTAB - 1, AREA_NTAB, 2 ** 31 - 1, 2 ** 24, 5, 6, 8, 1, 2, 9], dtype=np.int64)
    c['ids'] = ids[g.integers(0, len(ids), (5, AREA_HW))].astype(np.int32)
    exact = np.zeros((2, AREA_HW), dtype=np.int32)
    exact[0, 10:10 + AREA_MIN], exact[1, 50:50 + AREA_MIN - 1] = 4, 4          # a count of exactly min_area, and one less
    exact[0, 60:80], exact[0, 80:100] = 1, 7                                   # 20 + 20 pixels of two ids that share a row: together they reach min_area
    c['exactly_min_area'] = exact
    return c


# ================================================================================================================================ the planted mistakes
# (stage, mistake) -> the cases 'group/name' whose output it changes; asserted one by one in tests/test_camera_stage_checks.py
CAUGHT = {
    # the splatter
    ('splat', 'near_gt'): ['cull/planes_and_non_finite'],
    ('splat', 'lim_lt'): ['limit/u', 'limit/v'],
    ('splat', 'foot_f64'): ['footprint/product_fp32_not_fp64'],
    ('splat', 'radius_replaces'): ['footprint/radius_below_size'],
    ('splat', 'int_before_clamp'): ['footprint/quotient_inf', 'footprint/clipped_on_four_sides'],
    ('splat', 'trunc'): ['pixel/u_r0', 'pixel/v_r0', 'pixel/u_r1', 'pixel/v_r1'],
    ('splat', 'foot_ceil'): ['footprint/quotient_below_integer'],
    ('splat', 'tie_larger_row'): ['depth/rows_3_and_300', 'depth/rows_1_3_4'],
    # the rasteriser
    ('mesh', 'depth_near_gt'): ['planes/at_near', 'planes/corner_at_near'],
    ('mesh', 'depth_far_lt'): ['planes/at_far', 'planes/corner_at_far'],
    ('mesh', 'zc_near_gt'): ['planes/at_near', 'planes/corner_at_near'],
    ('mesh', 'lim_lt'): ['limit/at', 'limit/at_v'],
    ('mesh_resolve', 'corner_unswapped'): ['corner/clockwise_no_tie'],
    ('mesh', 'assoc_other'): ['depth/assoc_listed', 'depth/assoc_swapped'],
    ('mesh', 'snap_half_up'): ['snap/positive_even', 'snap/negative_odd'],
    ('mesh', 'snap_half_away'): ['snap/positive_even', 'snap/negative_even'],
    ('mesh', 'all_inclusive'): ['topleft/strip', 'topleft/quad0_fwd_d0'],
    ('mesh', 'all_exclusive'): ['topleft/strip', 'topleft/quad0_fwd_d0'],
    ('mesh', 'bottom_right'): ['topleft/strip', 'topleft/quad0_fwd_d0'],
    ('mesh', 'no_top_edge'): ['topleft/strip', 'topleft/quad0_fwd_d0'],
    ('mesh_resolve', 'tie_last_corner'): ['corner/tie_listing0', 'corner/tie_listing1', 'corner/tie_listing2', 'corner/tie_listing3'],
    ('mesh', 'box_in'): ['topleft/strip', 'topleft/quad0_fwd_d0'],
    ('mesh', 'tie_larger_face'): ['duplicate/faces_2_and_300'],
    ('area', 'drop_cross_camera_run'): ['across_a_camera'],
}

# What the scenes of the existing GPU tests (mesh_ref.scene() at its three shapes with vertex_ids; the `mixed` cloud from the novel cameras and view 0 at
# radius 0, 1, 3 and point_size = voxel_size) did with these mistakes before the cases of this module existed, measured once on the restatements alone (the
# reruns take minutes: they are recorded here, not repeated): True = some cell differed.
SCENES_CAUGHT = {
    ('mesh', 'snap_half_up'): True, ('mesh', 'all_inclusive'): True, ('mesh', 'all_exclusive'): True, ('mesh', 'bottom_right'): True, ('mesh', 'no_top_edge'): True,
    ('mesh_resolve', 'tie_last_corner'): True, ('splat', 'trunc'): True, ('splat', 'foot_ceil'): True,
    ('mesh', 'depth_near_gt'): False, ('mesh', 'depth_far_lt'): False, ('mesh', 'zc_near_gt'): False, ('mesh', 'lim_lt'): False, ('mesh_resolve', 'corner_unswapped'): False,
    ('mesh', 'assoc_other'): False, ('splat', 'near_gt'): False, ('splat', 'lim_lt'): False, ('splat', 'foot_f64'): False, ('splat', 'radius_replaces'): False,
    ('splat', 'int_before_clamp'): False,
}


def gap_table():
    """[(stage, mistake, what the existing scenes did with it - True, False or None where it was not measured -, the cases that catch it now)]"""
    return [(stage, name, SCENES_CAUGHT.get((stage, name)), cases) for (stage, name), cases in sorted(CAUGHT.items())]
