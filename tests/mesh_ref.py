"""numpy restatement of the z-buffered triangle rasterisation of a labelled mesh (panst3r_amd/engine/mesh.py, csrc/mesh.hip), the yardstick the kernels are
held to bit for bit, and the generated scene the mesh tests share.

Written from the contract (the reference renders through pyrender / OpenGL, which cannot run here).  The steps of the mesh section of
include/panst3r_hip.h:
  1 camera    float64 on the host: the rows of [R^T | -R^T t] as render_ref.camera_table rounds them, then fx fy cx cy.
  2 vertex    xc, yc, zc in float32 as render_ref.camera_coords; u = float32(float64(fx xc) / float64(zc)) + cx, v likewise; unusable if any of the
              five is not finite, zc < near, |u| or |v| > 2^14; X = rint(u 256), Y = rint(v 256) (np.rint: half to even).
  3 face      left out with an unusable vertex or an index outside [0, Nv); A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in int64, A == 0 drops the face,
              A < 0 exchanges corners 1 and 2.
  4 coverage  P = (256 j + 128, 256 i + 128); E_k = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa) for (a, b) = (1, 2), (2, 0), (0, 1); covered iff every E_k > 0
              or E_k == 0 on a top or left edge (dy < 0, or dy == 0 and dx > 0).  Only the pixels of the clipped bounding box are tested.
  5 depth     q_k = 1.0 / float64(zc_k); s = (E0 q0 + E1 q1) + E2 q2; depth = float32(float64(A) / s); left out if not finite, < near or > far.
  6 z-buffer  key = (uint64(bits(depth)) << 32) | face; np.minimum.at into a uint64 buffer of all ones.
  7 resolve   empty, or a key whose face is >= Nf: face -1, depth 0, id 0; face_ids[face], or vertex_ids of the corner with the largest E_k (ties: the
              lowest listed position; a face that is not rasterised in this camera: id 0).
  8 area      per (camera, listed id) pixel counts; an id that is not listed or has fewer than min_area pixels in its camera becomes 0.
Elementwise numpy rounds every float32 / float64 operation on its own, which is what the kernels promise; int64 arithmetic and the minimum are exact."""
import numpy as np

import render_ref as R

F = np.float32
LIM = F(2 ** 14)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
CORNERS = ((1, 2), (2, 0), (0, 1))


def camera_table(cams2world, focals, shape, pp=None):
    """float32 [B, 16] of step 1: W00 W01 W02 s0 W10 W11 W12 s1 W20 W21 W22 s2 fx fy cx cy"""
    H, W = shape
    tab = R.camera_table(cams2world, 1.0, shape, None, 1.0)                  # the twelve world-to-camera numbers, rounded as the render contract's
    B = len(tab)
    f = np.asarray(focals, dtype=np.float64)
    f = np.broadcast_to(f, (B, 2)) if f.ndim == 2 else np.broadcast_to(f.reshape(-1, 1), (B, 2))
    p = np.broadcast_to(np.asarray([W / 2, H / 2] if pp is None else pp, dtype=np.float64).reshape(-1, 2), (B, 2))
    tab[:, 12:14], tab[:, 14:16] = f, p
    return tab


def snap(vertices, cam, near):
    """step 2 for one camera -> usable bool [Nv], X, Y int64 [Nv] (0 where unusable), zc float32 [Nv]"""
    with np.errstate(all='ignore'):
        xc, yc, zc = R.camera_coords(vertices, cam)
        u = (R.quotient(cam[12] * xc, zc) + cam[14]).astype(F)
        v = (R.quotient(cam[13] * yc, zc) + cam[15]).astype(F)
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & np.isfinite(u) & np.isfinite(v) & (zc >= F(near)) & (np.abs(u) <= LIM) & (np.abs(v) <= LIM)
        X = np.where(ok, np.rint(np.where(ok, u, 0) * F(256)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, v, 0) * F(256)), 0).astype(np.int64)
    return ok, X, Y, zc


def setup(vertices, faces, cam, H, W, near):
    """steps 2 and 3 and the clipped bounding box of every face for one camera -> dict of [Nf, ...] arrays; `ok`: the face is rasterised, `box`: the pixels
    of its bounding box (0 where not ok)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Nv = len(vertices)
    usable, X, Y, zc = snap(vertices, cam, near)
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
    a, b = [c[0] for c in CORNERS], [c[1] for c in CORNERS]
    dx, dy = fx[:, b] - fx[:, a], fy[:, b] - fy[:, a]
    least = np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1)
    j0, j1 = np.maximum((fx.min(axis=1) + 127) >> 8, 0), np.minimum((fx.max(axis=1) - 128) >> 8, W - 1)
    i0, i1 = np.maximum((fy.min(axis=1) + 127) >> 8, 0), np.minimum((fy.max(axis=1) - 128) >> 8, H - 1)
    ok &= (j0 <= j1) & (i0 <= i1)
    box = np.where(ok, (j1 - j0 + 1) * (i1 - i0 + 1), 0)
    with np.errstate(all='ignore'):
        q = 1.0 / fz.astype(np.float64)
    return dict(ok=ok, usable=inside & usable[idx].all(axis=1), X=fx, Y=fy, xa=fx[:, a], ya=fy[:, a], dx=dx, dy=dy, least=least, A=A, q=q, swapped=swapped,
                j0=j0, j1=j1, i0=i0, i1=i1, box=box)


def edges(s, f, i, j):
    """E_k of face(s) f at the pixel(s) (i, j), broadcast: a list of three int64 arrays"""
    px, py = 256 * np.asarray(j, dtype=np.int64) + 128, 256 * np.asarray(i, dtype=np.int64) + 128
    return [s['dx'][f, k] * (py - s['ya'][f, k]) - s['dy'][f, k] * (px - s['xa'][f, k]) for k in range(3)]


def raster(s, H, W, near, far):
    """steps 4 - 6 for one camera from setup()'s arrays -> (zbuf uint64 [H * W], candidates int64 [H * W])"""
    zbuf, cand = np.full(H * W, EMPTY, dtype=np.uint64), np.zeros(H * W, dtype=np.int64)
    for f in np.nonzero(s['ok'])[0]:
        ii, jj = np.arange(s['i0'][f], s['i1'][f] + 1)[:, None], np.arange(s['j0'][f], s['j1'][f] + 1)[None, :]
        E = edges(s, f, ii, jj)
        cov = (E[0] >= s['least'][f, 0]) & (E[1] >= s['least'][f, 1]) & (E[2] >= s['least'][f, 2])
        with np.errstate(all='ignore'):
            q = s['q'][f]
            t = (E[0].astype(np.float64) * q[0] + E[1].astype(np.float64) * q[1]) + E[2].astype(np.float64) * q[2]
            depth = (np.float64(s['A'][f]) / t).astype(F)
            keep = cov & np.isfinite(depth) & (depth >= F(near)) & (depth <= F(far))
        cell = (ii * W + jj)[keep]
        key = (np.ascontiguousarray(depth[keep]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        np.minimum.at(zbuf, cell, key)
        cand[cell] += 1                                                        # (a face reaches a cell once)
    return zbuf, cand


def resolve(zbuf, s, faces, H, W, vertex_ids=None, face_ids=None):
    """step 7 for one camera -> (face int64, depth float32, pan int32, ties) flat [H * W]; ties = the hit pixels whose largest E_k is shared"""
    low = zbuf & np.uint64(0xFFFFFFFF)
    hit = (zbuf != EMPTY) & (low < np.uint64(len(s['ok'])))                  # a key that names a face >= Nf is an empty cell
    face = np.where(hit, low, np.uint64(0)).astype(np.int64)
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32).view(F), F(0)).astype(F)
    pan, ties = np.zeros(H * W, dtype=np.int32), np.zeros(H * W, dtype=bool)
    pix = np.arange(H * W)
    E = edges(s, face, pix // W, pix % W)
    sw = s['swapped'][face]
    listed = [E[0], np.where(sw, E[2], E[1]), np.where(sw, E[1], E[2])]       # by position in `faces`
    best = np.maximum(np.maximum(listed[0], listed[1]), listed[2])
    pos = np.where(listed[0] == best, 0, np.where(listed[1] == best, 1, 2))
    ties = hit & (sum((e == best).astype(int) for e in listed) >= 2)
    if face_ids is not None:
        pan = np.where(hit, np.asarray(face_ids, dtype=np.int32)[face], 0).astype(np.int32)
    elif vertex_ids is not None:
        seen = hit & s['ok'][face]                                             # a face that leaves no trace in this camera: id 0, face and depth from the key
        corner = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face, pos]
        pan = np.where(seen, np.asarray(vertex_ids, dtype=np.int32)[np.where(seen, corner, 0)], 0).astype(np.int32)
    return np.where(hit, face, -1), depth, pan, ties


def render(vertices, faces, cams2world, focals, shape, vertex_ids=None, face_ids=None, pp=None, near=0.05, far=20.0):
    """-> dict(depth [B,H,W] float32, face [B,H,W] int64, pan [B,H,W] int32) and, about the run itself, candidates [B,H,W] int64, ties [B,H,W] bool,
    box [B,Nf] int64 (the bounding-box pixels of every rasterised face, 0 for one left out), usable [B,Nf] bool (no unusable vertex, no bad index)"""
    H, W = shape
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    out = {k: [] for k in ('depth', 'face', 'pan', 'candidates', 'ties', 'box', 'usable')}
    for cam in camera_table(cams2world, focals, shape, pp):
        s = setup(vertices, faces, cam, H, W, near)
        zbuf, cand = raster(s, H, W, near, far)
        face, depth, pan, ties = resolve(zbuf, s, faces, H, W, vertex_ids, face_ids)
        for k, v in (('depth', depth), ('face', face), ('pan', pan), ('candidates', cand), ('ties', ties)):
            out[k].append(v.reshape(H, W))
        out['box'].append(s['box'])
        out['usable'].append(s['usable'])
    return {k: np.stack(v) for k, v in out.items()}


def area_filter(pan, ids, min_area):
    """step 8: pan int32 [B,H,W], the listed ids in row order -> (filtered maps, counts int32 [B, S])"""
    pan = np.asarray(pan, dtype=np.int32)
    counts = np.stack([(pan == i).reshape(len(pan), -1).sum(axis=1) for i in ids], axis=1).astype(np.int32) if len(ids) else np.zeros((len(pan), 0), np.int32)
    out = np.zeros_like(pan)
    for s, i in enumerate(ids):
        if i > 0:
            m = (pan == i) & (counts[:, s] >= min_area)[:, None, None]
            out[m] = i
    return out, counts


def ground_truth(vertices, faces, vertex_ids, segments, cameras, min_area=50, near=0.05, far=20.0):
    """engine.mesh.ground_truth_maps: cameras are dicts with cam2world, fx, fy, cx, cy, height, width -> (maps, segments, depths, counts per camera)"""
    ids = [int(s['id']) for s in segments]
    maps, depths, counts = [], [], []
    for c in cameras:
        r = render(vertices, faces, [c['cam2world']], [[c['fx'], c['fy']]], (c['height'], c['width']), vertex_ids=vertex_ids, pp=[c['cx'], c['cy']], near=near, far=far)
        m, n = area_filter(r['pan'], ids, min_area)
        maps.append(m[0]); depths.append(r['depth'][0]); counts.append(n[0])
    area = np.where(np.stack(counts) >= min_area, np.stack(counts), 0).sum(axis=0) if ids else np.zeros(0, int)
    segs = [{'id': i, 'category_id': int(s['category_id'] if 'category_id' in s else s['class_id']), 'area': int(a)} for i, s, a in zip(ids, segments, area) if a > 0]
    return maps, segs, depths, counts


# ---------------------------------------------------------------- the generated scene of the mesh tests
def _grid(p0, du, dv, n):
    """(n + 1)^2 vertices p0 + a du + b dv and the 2 n^2 triangles of the tessellated parallelogram"""
    a, b = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing='ij')
    v = np.asarray(p0, float) + a[..., None] * np.asarray(du, float) + b[..., None] * np.asarray(dv, float)
    k = lambda i, j: i * (n + 1) + j
    f = [t for i in range(n) for j in range(n) for t in ((k(i, j), k(i + 1, j), k(i + 1, j + 1)), (k(i, j), k(i + 1, j + 1), k(i, j + 1)))]
    return v.reshape(-1, 3), np.array(f, dtype=np.int64)


def _box(centre, size, n):
    c, h = np.asarray(centre, float), np.asarray(size, float) / 2
    parts = []
    for ax in range(3):
        u, w = np.eye(3)[(ax + 1) % 3] * 2 * h[(ax + 1) % 3], np.eye(3)[(ax + 2) % 3] * 2 * h[(ax + 2) % 3]
        for sgn in (-1, 1):
            parts.append(_grid(c + sgn * np.eye(3)[ax] * h[ax] - u / 2 - w / 2, u, w, n))
    return parts


def _rot(axis, deg):
    a, c, s = np.eye(3)[axis], np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


CLS_SEP, WALL, FLOOR, THING, MARK = 256, 1, 2, 3, 4
UNLISTED = 999                                                                 # the ceiling's id: in no segment list


def scene(seed=0, n_wall=16, n_ceiling=4):
    """A box room x in [-4, 4], y in [-2, 1.5] (y points down: the floor is y = 1.5), z in [-3, 5] around the origin, in the frame of camera 0 (identity):
    four tessellated walls (their vertices jittered inside their planes by the seed), a coarse ceiling, a floor of two triangles in front of camera 0, two labelled boxes, marker
    faces in front of camera 0 placed by pixel (for the 48 x 64 image with focal 32), and the deliberately bad faces.  -> dict"""
    rng = np.random.default_rng(seed)
    parts, ids, names = [], [], []

    def add(part, pid, name):
        parts.append(part); ids.append(pid); names.append(name)
    x0, x1, y0, y1, z0, z1 = -4.0, 4.0, -2.0, 1.5, -3.0, 5.0
    walls = {'front': ((x0, y0, z1), (x1 - x0, 0, 0), (0, y1 - y0, 0)), 'back': ((x0, y0, z0), (x1 - x0, 0, 0), (0, y1 - y0, 0)),
             'left': ((x0, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0)), 'right': ((x1, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0))}
    inst = 1
    segments = []
    for name, (p0, du, dv) in walls.items():
        v, f = _grid(p0, du, dv, n_wall)
        inner = np.ones((n_wall + 1, n_wall + 1), bool)
        inner[[0, -1], :] = inner[:, [0, -1]] = False
        jit = rng.uniform(-0.3, 0.3, (len(v), 2)) / n_wall
        v = v + inner.reshape(-1, 1) * (jit[:, :1] * np.asarray(du, float) + jit[:, 1:] * np.asarray(dv, float))
        add((v, f), inst * CLS_SEP + WALL, name)
        segments.append({'id': inst * CLS_SEP + WALL, 'category_id': WALL})
        inst += 1
    add(_grid((x0, y0, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0), n_ceiling), UNLISTED, 'ceiling')          # coarse: faces of hundreds of pixels
    # two triangles that fill the lower part of camera 0's image.  The floor starts in front of that camera (z = 0.1): a face with a vertex behind the
    # near plane is left out whole, so a floor under the camera would not be seen from it
    add(_grid((x0, y1, 0.1), (x1 - x0, 0, 0), (0, 0, z1 - 0.1), 1), inst * CLS_SEP + FLOOR, 'floor')
    segments.append({'id': inst * CLS_SEP + FLOOR, 'category_id': FLOOR})
    inst += 1
    for name, centre, size in (('box_a', (-1.5, 0.9, 3.5), (1.0, 1.2, 1.0)), ('box_b', (1.5, 1.375, 3.0), (0.25, 0.25, 0.25))):
        for part in _box(centre, size, 3 if name == 'box_a' else 1):
            add(part, inst * CLS_SEP + THING, name)
        segments.append({'id': inst * CLS_SEP + THING, 'class_id': THING})   # (the reference's key, accepted as an alias)
        inst += 1
    # marker faces at z = 2 in front of camera 0, corners given as pixels (u, v) of the 48 x 64 image, focal 32, principal point (32, 24): x = (u - 32) /
    # 16, y = (v - 24) / 16 are exact in float32, so are u and v
    pix = lambda u, v: ((u - 32) / 16, (v - 24) / 16, 2.0)
    markers = {'box64': [(10.25, 5.25), (17.75, 5.25), (10.25, 12.75)],        # an 8 x 8 bounding box: exactly MESH_LANE_PIXELS
               'box65': [(20.25, 5.25), (24.75, 5.25), (20.25, 17.75)],        # 5 x 13: one more
               'tie': [(40.5, 10.0), (44.5, 10.0), (42.5, 14.0)]}              # symmetric about the pixel centres u = 42.5: corners 0 and 1 tie there
    special = {}
    for name, uv in markers.items():
        v = np.array([pix(*p) for p in uv])
        pid = [(inst + k) * CLS_SEP + MARK for k in range(3)] if name == 'tie' else [inst * CLS_SEP + MARK] * 3
        add((v, np.array([[0, 1, 2]])), pid, name)
        for p in sorted(set(pid)):
            segments.append({'id': p, 'category_id': MARK})
        inst += len(set(pid))
    verts, faces, vids, fids, first_face = [], [], [], [], {}
    nv = 0
    for (v, f), pid, name in zip(parts, ids, names):
        first_face.setdefault(name, sum(len(x) for x in faces))
        verts.append(v); faces.append(f + nv)
        vids.append(np.broadcast_to(np.asarray(pid), (len(v),)) if np.ndim(pid) == 0 else np.asarray(pid))
        fids.append(np.full(len(f), np.min(pid)))
        nv += len(v)
    verts, faces, vids, fids = np.concatenate(verts).astype(F), np.concatenate(faces), np.concatenate(vids).astype(np.int32), np.concatenate(fids).astype(np.int32)
    for name in markers:
        special[name] = first_face[name]
    # the deliberately bad faces, appended: their rows are in `special`
    box_a = first_face['box_a'] + 0                                            # the first face of box_a's -x ... side; the duplicate is of a camera-facing one below
    extra_v = np.array([[np.nan, 0.0, 2.0], [0.0, -0.5, 0.01], [0.3, -0.5, 1.0], [-0.3, -0.5, 1.0]], dtype=F)
    nan_v, near_v = nv, nv + 1
    a, b, c = faces[box_a]
    bad = {'degenerate': (a, a, b), 'nan': (nan_v, a, b), 'index_high': (nv + len(extra_v), a, b), 'index_negative': (-1, a, b),
           'near': (near_v, near_v + 1, near_v + 2)}
    # the duplicate: a face of box_a whose three vertices have z = 3 (the side towards camera 0)
    front = [k for k in range(first_face['box_a'], first_face['box_b']) if (verts[faces[k], 2] == F(3.0)).all()]
    bad['duplicate'] = tuple(faces[front[4]])
    special['original'] = front[4]
    for name, f in bad.items():
        special[name] = len(faces)
        faces = np.concatenate([faces, np.array([f], dtype=np.int64)])
        fids = np.concatenate([fids, fids[box_a:box_a + 1]])
    verts = np.concatenate([verts, extra_v])
    vids = np.concatenate([vids, np.full(len(extra_v), vids[faces[box_a][0]], dtype=np.int32)])
    cams = []
    for Rm, t in ((np.eye(3), (0, 0, 0)), (_rot(1, 30), (1.0, 0.0, 0.5)), (_rot(0, -25) @ _rot(1, -40), (-1.0, -0.5, 1.0)),
                  (np.eye(3), (0.0, -0.5, -12.0)), (_rot(1, 180), (0.0, 0.0, -12.0))):      # 0 - 2 inside, 3 outside looking at the room, 4 outside looking away
        c = np.eye(4)
        c[:3, :3], c[:3, 3] = Rm, t
        cams.append(c)
    return dict(vertices=verts, faces=faces, vertex_ids=vids, face_ids=fids, segments=segments, cams=cams, special=special)


def focal_of(shape):
    return shape[1] / 2                                                        # 32 for the 48 x 64 image the markers are placed for


def camera_dicts(cams, shapes, aniso=1.0):
    """one dict per camera with cam2world, fx, fy = aniso fx, cx, cy, height, width; shapes: one (H, W) per camera"""
    return [{'cam2world': c, 'fx': focal_of(s), 'fy': aniso * focal_of(s), 'cx': s[1] / 2, 'cy': s[0] / 2, 'height': s[0], 'width': s[1]} for c, s in zip(cams, shapes)]
