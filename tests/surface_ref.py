"""numpy restatement of the surface mesh of the pointmap grids (the surface section of include/panst3r_hip.h), the yardstick of csrc/surface.hip.

Own code, no counterpart in the reference: [restated, parity unpinned].  The stage is integer work and float32 compares (one float32 subtraction per
diagonal, one float32 product per triangle), which elementwise float32 numpy performs exactly as the contract orders them, so the comparison with the
GPU is bit for bit.  Also here: the generated scene of the tests (`scene`), the plane of the hole count (`plane_scene`) and the islands by iterated
minimum-label propagation."""
import numpy as np

import cloud_ref
import mesh_ref

F = np.float32
TRI = np.array([[0, 2, 3], [0, 3, 1], [0, 2, 1], [1, 2, 3]])                   # corners a b c d = 0 1 2 3: (a,c,d), (a,d,b), (a,c,b), (b,c,d)
ACD, ADB, ACB, BCD = 0, 1, 2, 3


def depth_bound(max_depth_ratio):
    """k = float32(1 + max_depth_ratio) taken in double; None: no cut (+inf)"""
    return F(np.inf) if max_depth_ratio is None else F(1.0 + float(max_depth_ratio))


def row_table(index, N):
    """step 1: the cloud row of every scene pixel, -1 where the pixel was filtered out"""
    row = np.full(N, -1, dtype=np.int32)
    row[np.asarray(index, dtype=np.int64)] = np.arange(len(index), dtype=np.int32)
    return row


def mesh(index, vertex_ids, shapes, depths, max_depth_ratio=0.1, force_diagonal=None):
    """steps 1 - 5.  index int64 [M], vertex_ids int32 [M]: the cloud's; shapes [(H, W)]; depths: per view the float32 [H, W] third component of
    pts3d_local.  force_diagonal 'ad' / 'bc' overrides the diagonal rule (for the property tests only).
    -> dict(faces int32 [F,3], face_ids int32 [F], quad int64 [F]) and, about the run itself, per quad of the scene in order: corners (how many are
    present), present [Q,4], bc (diagonal b-c chosen), tie (four corners, equal |dz|), and per candidate [Q,2]: has, keep, zmin, zmax, bound (= zmin * k)."""
    vertex_ids = np.asarray(vertex_ids, dtype=np.int32)
    k = depth_bound(max_depth_ratio)
    row = row_table(index, sum(h * w for h, w in shapes))
    out = {n: [] for n in ('faces', 'face_ids', 'quad', 'corners', 'present', 'bc', 'tie', 'has', 'keep', 'zmin', 'zmax', 'bound')}
    off = 0
    for (H, W), depth in zip(shapes, depths):
        o, off = off, off + H * W
        if H < 2 or W < 2:
            continue
        r = row[o:o + H * W].reshape(H, W)
        z = np.where(r >= 0, np.asarray(depth, dtype=F).reshape(H, W), F(0))
        R = np.stack([r[:-1, :-1], r[:-1, 1:], r[1:, :-1], r[1:, 1:]], axis=-1).reshape(-1, 4)           # a b c d per quad, raster order
        Z = np.stack([z[:-1, :-1], z[:-1, 1:], z[1:, :-1], z[1:, 1:]], axis=-1).reshape(-1, 4)
        present = R >= 0
        n = present.sum(axis=1)
        with np.errstate(invalid='ignore', over='ignore'):
            bc = np.abs(Z[:, 1] - Z[:, 2]) < np.abs(Z[:, 0] - Z[:, 3])          # a tie or a NaN: a-d
            tie = (np.abs(Z[:, 1] - Z[:, 2]) == np.abs(Z[:, 0] - Z[:, 3])) & (n == 4)
        if force_diagonal is not None:
            bc = np.full(len(R), force_diagonal == 'bc')
        three = np.where(~present[:, 3], ACB, np.where(~present[:, 0], BCD, np.where(~present[:, 1], ACD, ADB)))
        code = np.stack([np.where(n == 4, np.where(bc, ACB, ACD), three), np.where(bc, BCD, ADB)], axis=1)   # [Q, 2]
        has = np.stack([n >= 3, n == 4], axis=1)
        corners = TRI[code]                                                    # [Q, 2, 3]
        tr = np.take_along_axis(R[:, None, :], corners, axis=2)
        tz = np.take_along_axis(Z[:, None, :], corners, axis=2)
        with np.errstate(invalid='ignore', over='ignore'):
            zmin, zmax = np.minimum.reduce(tz, axis=2), np.maximum.reduce(tz, axis=2)                    # a NaN propagates: both compares fail
            bound = (zmin * k).astype(F)
            keep = has & (zmin > 0) & (zmax <= bound)
        ids = vertex_ids[np.where(tr >= 0, tr, 0)]
        fid = np.where((ids[..., 0] == ids[..., 1]) | (ids[..., 0] == ids[..., 2]), ids[..., 0], np.where(ids[..., 1] == ids[..., 2], ids[..., 1], 0))
        yy, xx = np.divmod(np.arange(len(R), dtype=np.int64), W - 1)
        q = np.broadcast_to((o + yy * W + xx)[:, None], keep.shape)
        out['faces'].append(tr[keep]); out['face_ids'].append(fid[keep]); out['quad'].append(q[keep])
        for name, val in (('corners', n), ('present', present), ('bc', bc & (n == 4)), ('tie', tie), ('has', has), ('keep', keep), ('zmin', zmin), ('zmax', zmax), ('bound', bound)):
            out[name].append(val)
    cat = lambda name, shape, dt: np.concatenate(out[name]).astype(dt) if out[name] else np.zeros(shape, dtype=dt)
    return {'faces': cat('faces', (0, 3), np.int32), 'face_ids': cat('face_ids', (0,), np.int32), 'quad': cat('quad', (0,), np.int64),
            'corners': cat('corners', (0,), np.int64), 'present': cat('present', (0, 4), bool), 'bc': cat('bc', (0,), bool), 'tie': cat('tie', (0,), bool), 'has': cat('has', (0, 2), bool),
            'keep': cat('keep', (0, 2), bool), 'zmin': cat('zmin', (0, 2), F), 'zmax': cat('zmax', (0, 2), F), 'bound': cat('bound', (0, 2), F)}


def face_component(faces, M):
    """step 6: int32 [F], the smallest vertex row of every face's component.  Iterated minimum-label propagation: every vertex starts with its own row,
    every face gives its three vertices the smallest of their labels, and a vertex takes the label of its label (label[v] <= v is a row of the same
    component), until nothing changes."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.arange(M, dtype=np.int64)
    while len(faces):
        m = label[faces].min(axis=1)
        new = label.copy()
        for j in range(3):
            np.minimum.at(new, faces[:, j], m)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    return label[faces[:, 0]].astype(np.int32) if len(faces) else np.zeros(0, dtype=np.int32)


def drop_small(m, M, min_faces):
    """the faces whose component has at least min_faces faces, order kept -> dict(faces, face_ids, quad)"""
    comp = face_component(m['faces'], M)
    keep = np.bincount(comp, minlength=max(M, 1))[comp] >= min_faces
    return {k: m[k][keep] for k in ('faces', 'face_ids', 'quad')}


def render(vertices, m, cams2world, focals, shape, **kw):
    """the restated mesh through the restated rasteriser"""
    return mesh_ref.render(vertices, m['faces'].astype(np.int64), cams2world, focals, shape, face_ids=m['face_ids'], **kw)


def winding_z(local, faces):
    """z of (v1 - v0) x (v2 - v0) per face in the camera frame of `local` [M, 3] (float64)"""
    p = np.asarray(local, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]


# ---------------------------------------------------------------- the scenes of the tests
def focal_of(shape):
    return 0.8 * shape[1]


def backproject(z, focal):
    """pts3d_local [H, W, 3] float32 of a depth map through a pinhole with the principal point (W / 2, H / 2), pixel centres at + 0.5"""
    H, W = z.shape
    y, x = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing='ij')
    with np.errstate(invalid='ignore'):
        X = ((x + F(0.5) - F(W / 2)) * z / F(focal)).astype(F)
        Y = ((y + F(0.5) - F(H / 2)) * z / F(focal)).astype(F)
    return np.stack([X, Y, z.astype(F)], axis=-1)


def _pose(axis, deg, t):
    c = np.eye(4, dtype=F)
    c[:3, :3] = mesh_ref._rot(axis, deg).astype(F)                         # axis: 0, 1 or 2
    c[:3, 3] = t
    return c


def _views_to_scene(zs, confs, pans, cams, nseg):
    from panst3r_amd.synthetic import synth_image
    x_out, imgs = [], []
    for v, (z, conf, c) in enumerate(zip(zs, confs, cams)):
        loc = backproject(z, focal_of(z.shape))
        with np.errstate(invalid='ignore'):
            pts = cloud_ref.geotrf(c, loc.reshape(-1, 3)).reshape(loc.shape)
        x_out.append({'pts3d': pts, 'pts3d_local': loc, 'conf': conf.astype(F)})
        imgs.append(synth_image(v, *z.shape).numpy())
    info = [{'id': i, 'query_id': i - 1, 'category_id': i % 5} for i in range(1, nseg + 1)]
    return x_out, imgs, [p.astype(np.int32) for p in pans], info, cams


SHAPES = [(6, 9), (17, 23), (64, 65), (2, 2)]
THR, THR_WITHOUT_VIEW0 = 1.0, 3.0                                             # kept pixels of view 0 have confidence 2, of the other views 5, dropped ones 0
NSEG = 24
EQ = F(F(1.0) * F(1.1))                                                        # zmin * k for zmin = 1 at the default ratio


def scene(seed=0):
    """Four views, SHAPES, everything the GPU comparison is meant to decide placed by hand (tests/test_hip_surface.py lists and checks the conditions):
    view 0  a constant depth, all kept: every diagonal a tie.  Its confidence is 2: THR_WITHOUT_VIEW0 leaves it without a point.
    view 1  rows 0 - 8 dropped except for small marked groups of pixels (`marks`: name -> (y, x) of the group's first pixel), rows 10 - 16 a kept patch.
    view 2  the large patch: smooth depth plus noise, a depth step at x = 40, seeded drops of 8 % of the pixels.
    view 3  2 x 2, one pixel dropped, one of the rest five times as deep: points, but no face.
    -> (x_out, imgs, pan, segments_info, cams2world) as cloud_ref.synthetic_scene returns them, and marks."""
    g = np.random.Generator(np.random.PCG64(seed))
    zs = [np.full(s, 3.0, dtype=F) for s in SHAPES]
    confs = [np.full(SHAPES[0], 2.0, dtype=F)] + [np.zeros(s, dtype=F) for s in SHAPES[1:]]
    pans = [np.full(s, 2, dtype=np.int32) for s in SHAPES]
    pans[0][:, 5:] = 1
    # view 1: the marked groups
    z, conf, pan, marks = zs[1], confs[1], pans[1], {}
    z[:] = 1.0

    def put(name, y, x, pixels, depth=None):
        marks[name] = (y, x)
        for j, (dy, dx) in enumerate(pixels):
            conf[y + dy, x + dx] = 5.0
            if depth is not None:
                z[y + dy, x + dx] = depth[j]
    ell, block = [(0, 0), (0, 1), (1, 0)], [(0, 0), (0, 1), (1, 0), (1, 1)]      # a, b, c (d missing); a, b, c, d
    put('island1', 0, 0, ell)
    put('island5', 0, 3, [(dy, dx) for dy in range(2) for dx in range(3)] + [(2, 0)])
    put('island6', 0, 7, [(dy, dx) for dy in range(2) for dx in range(4)])
    put('touch', 0, 12, [(0, 0), (0, 1), (1, 1), (2, 1), (2, 2)])              # two triangles that share the pixel (1, 13) and nothing else
    put('t0_cut', 0, 16, block, [1, 1, 2, 1])                                  # c deep: diagonal a-d, T0 = (a, c, d) cut, T1 = (a, d, b) kept
    put('t1_cut', 0, 19, block, [1, 2, 1, 1])                                  # b deep: T0 kept, T1 cut
    put('equal', 4, 0, ell, [1, 1, EQ])                                        # zmax == zmin * k: kept
    put('above', 4, 3, ell, [1, 1, np.nextafter(EQ, F(2))])                    # the next float32: cut
    put('zero', 4, 6, ell, [1, 1, 0])
    put('nan', 4, 9, ell, [1, 1, np.nan])
    put('nan_diagonal', 4, 12, block, [1, np.nan, 1, 1])                       # a NaN in the comparison: a-d; T1 = (a, d, b) cut by it
    put('void_ids', 4, 15, block)
    put('negative', 4, 18, ell, [1, 1, -1])
    put('bc', 4, 21, block, [1, 1, 1, 1.05])                                   # |z_b - z_c| = 0 < |z_a - z_d|: diagonal b-c
    pan[4:6, 15:17] = [[3, 4], [5, 6]]                                         # four ids in one quad: both faces void
    conf[10:, :] = 5.0
    z[10:, :] = (F(1.5) + F(0.01) * np.arange(23, dtype=F))[None, :]
    pan[10:, :] = (7 + np.arange(23) // 6)[None, :]                            # bands: faces with two equal ids at their borders
    # view 2
    H, W = SHAPES[2]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    zs[2] = (2.0 + 0.3 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.01 * g.standard_normal((H, W)) + (xx >= 40) * 1.0).astype(F)
    confs[2] = np.where(g.uniform(size=(H, W)) < 0.08, 0.0, 5.0).astype(F)
    pans[2] = (11 + (xx // 11) + 6 * (yy // 32)).astype(np.int32)
    pans[2][:3] = 0
    # view 3
    zs[3] = np.array([[1, 1], [5, 1]], dtype=F)
    confs[3] = np.array([[5, 5], [5, 0]], dtype=F)
    cams = [_pose(1, 0, (0, 0, 0)), _pose(1, 12, (0.4, 0, 0.1)), _pose(0, -8, (-0.3, 0.2, 0)), _pose(2, 30, (0, -0.5, 0.2))]
    return _views_to_scene(zs, confs, pans, cams, NSEG) + (marks,)


def plane_scene(shape=(24, 32), depth=2.0):
    """one fronto-parallel plane at `depth`, every pixel kept, a panoptic map of vertical bands, the camera at the origin"""
    z = np.full(shape, depth, dtype=F)
    pan = (1 + np.arange(shape[1]) // 8)[None, :].repeat(shape[0], axis=0)
    return _views_to_scene([z], [np.full(shape, 5.0, dtype=F)], [pan], [np.eye(4, dtype=F)], 4)


def grid_scene(h, w, seed=1):
    """one fully kept h x w view with a smooth depth (property tests of the restatement)"""
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    z = (2.0 + 0.02 * xx + 0.015 * yy + 0.004 * g.standard_normal((h, w))).astype(F)
    return _views_to_scene([z], [np.full((h, w), 5.0, dtype=F)], [np.ones((h, w), dtype=np.int32)], [np.eye(4, dtype=F)], 1)


STRIP_SHAPE, STRIP_DROP = (2, 258), (0, 0, 1, 1, 0, 1, 1, 0)


def strip_scene():
    """one 2 x 258 view: 257 quads in raster order, so the quad kernels' 256-quad workgroups are one full workgroup and one that holds a single quad.
    The top row is kept; bottom pixel x is dropped where STRIP_DROP[x mod 8] is set, so quad x has 4 - drop[x] - drop[x + 1] corners and yields
    2, 1, 0, 1, 1, 0, 1, 2 faces for x mod 8 = 0 .. 7: before and after every multiple of 8 - the 64-lane edges, and 256 from below - stand quads with
    0, 1 and 2 faces.  The depth stays inside the cut, the ids change every 16 pixels."""
    H, W = STRIP_SHAPE
    x = np.arange(W)
    z = np.broadcast_to((1.0 + 0.001 * (x % 7)).astype(F), (H, W)).copy()
    conf = np.full((H, W), 5.0, dtype=F)
    conf[1, np.asarray(STRIP_DROP, dtype=bool)[x % 8]] = 0.0
    pan = np.broadcast_to(1 + x // 16, (H, W)).astype(np.int32)
    return _views_to_scene([z], [conf], [pan], [np.eye(4, dtype=F)], 17)


def of_scene(sc, thr, max_depth_ratio=0.1, force_diagonal=None):
    """(cloud, mesh) of a scene tuple by the two restatements"""
    x_out, imgs, pan, info, cams = sc[:5]
    from panst3r_amd.engine import default_colors
    with np.errstate(invalid='ignore'):
        c = cloud_ref.cloud(x_out, imgs, pan, info, cams, min_conf_thr=thr, colors=default_colors(len(info) + 1))
    shapes = [x['conf'].shape for x in x_out]
    return c, mesh(c['index'], c['pan'], shapes, [x['pts3d_local'][..., 2] for x in x_out], max_depth_ratio, force_diagonal)
