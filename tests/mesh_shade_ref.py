"""numpy restatement of the mesh shading contract (include/panst3r_hip.h, the mesh shading section; panst3r_amd/engine/shade.py, csrc/mesh_normals.hip and
pst_mesh_interp of csrc/mesh.hip), the yardstick the kernels are held to bit for bit.  It does not go through the engine: it builds on mesh_ref.setup and
mesh_ref.edges, the restated rasteriser.

  normals   1 valid face: three indices in [0, Nv), nine finite coordinates.  2 c = e1 x e2 in float64, every product and difference rounded on its own.
            3 sh = 51 - 2 ex, ex = frexp's exponent of the largest axis extent of the finite coordinates (0 for no extent).  4 q = int64(rint(ldexp(c, sh))),
            hi = q >> 26, lo = q & (2^26 - 1).  5 int64 sums per (vertex, axis, limb) - np.add.at, exact.  7 S = float64(hi) 2^26 + float64(lo),
            len2 = (Sx Sx + Sy Sy) + Sz Sz, n = float32(S / sqrt_heron(len2)), 0 for len2 == 0.  8 sqrt_heron: six Heron steps from 1.0 on r in [0.5, 2).
  interp    9 hit: 0 <= f < Nf, the face is rasterised in the pixel's camera, the pixel is covered.  10 w_k = float64(E_k) q_k, s = (w0 + w1) + w2; set-up
            corner k = listed position k, 1 and 2 exchanged after a swap.  11 out = float32(((w0 a0 + w1 a1) + w2 a2) / s).  12 shade: N (smooth: the
            weighted normals, no division; flat: c of the corners as listed) rotated by the camera's rows, the view ray through the pixel centre,
            float32(|dot| / sqrt_heron(nn dd)), 0 when nn dd is zero or not finite.  A miss: fill, shade 0.
Elementwise numpy rounds every float64 operation on its own, which is what the kernels promise.

`variant=` plants ONE mistake at a time (tests/test_mesh_shade_host.py shows a case that each one changes):
  'no_swap' attributes and normals do not follow the corner exchange     'assoc'  w0 a0 + (w1 a1 + w2 a2)
  'affine'  screen-space weights E_k / A                                 'trunc'  hi by truncation towards zero instead of floor
  'unit'    unweighted (unit) face normals                               'heron5' five Heron steps
  'no_coverage' the coverage test dropped"""
import math

import numpy as np

import mesh_ref as M

F = np.float32
VARIANTS = ('no_swap', 'assoc', 'affine', 'trunc', 'unit', 'heron5', 'no_coverage')
LIMB = 26
MASK = np.int64((1 << LIMB) - 1)
UNIT_SHIFT = 40                                                                # the 'unit' variant's scale: its vectors have length 1


def sqrt_heron(x, steps=6):
    """step 8 for float64 x > 0 (elementwise)"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    e2 = e - (e & 1)
    r = np.ldexp(x, -e2)
    s = np.ones_like(r)
    for _ in range(steps):
        s = 0.5 * (s + r / s)
    return np.ldexp(s, e2 // 2)


def _steps(variant):
    return 5 if variant == 'heron5' else 6


def valid_faces(vertices, faces):
    """step 1 -> (valid bool [Nf], indices with 0 in the rows that are not valid)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    inside = ((faces >= 0) & (faces < len(vertices))).all(axis=1)
    idx = np.where(inside[:, None], faces, 0)
    valid = inside & np.isfinite(vertices[idx]).all(axis=(1, 2))
    return valid, np.where(valid[:, None], faces, 0)


def face_vectors(vertices, idx):
    """step 2 for the faces idx int64 [n, 3] -> float64 [n, 3]"""
    v = vertices[idx].astype(np.float64)
    with np.errstate(all='ignore'):
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def shift(vertices):
    """step 3"""
    D = 0.0
    for a in range(3):
        x = vertices[:, a][np.isfinite(vertices[:, a])]
        if len(x):
            D = max(D, float(np.float64(x.max()) - np.float64(x.min())))
    return 51 - 2 * math.frexp(D)[1] if D > 0 else 0


def accumulate(vertices, faces, sh=None, variant=None):
    """steps 1 - 5 -> acc int64 [Nv, 3, 2]"""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    valid, idx = valid_faces(vertices, faces)
    idx = idx[valid]
    c = face_vectors(vertices, idx)
    sh = shift(vertices) if sh is None else sh
    if variant == 'unit':
        length = np.sqrt((c * c).sum(axis=1, keepdims=True))
        c, sh = np.where(length > 0, c / np.where(length > 0, length, 1), 0.0), UNIT_SHIFT
    q = np.rint(np.ldexp(c, sh)).astype(np.int64)
    assert (np.abs(q) < 2 ** 52).all()
    hi = (np.trunc(q / 2.0 ** LIMB)).astype(np.int64) if variant == 'trunc' else q >> LIMB
    lo = q & MASK
    acc = np.zeros((len(vertices), 3, 2), dtype=np.int64)
    for k in range(3):
        np.add.at(acc[:, :, 0], idx[:, k], hi)
        np.add.at(acc[:, :, 1], idx[:, k], lo)
    return acc


def finish(acc, variant=None):
    """step 7 -> float32 [Nv, 3]"""
    S = acc[:, :, 0].astype(np.float64) * 67108864.0 + acc[:, :, 1].astype(np.float64)
    len2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
    some = len2 != 0
    length = sqrt_heron(np.where(some, len2, 1.0), _steps(variant))
    return np.where(some[:, None], S / length[:, None], 0.0).astype(F)


def normals(vertices, faces, variant=None):
    """engine.shade.vertex_normals -> float32 [Nv, 3]"""
    return finish(accumulate(vertices, faces, None, variant), variant)


def _blend(w, a, variant):
    """(w0 a0 + w1 a1) + w2 a2 for w: three float64 [n], a: float64 [n, 3 corners, C] -> [n, C]"""
    t = [w[k][:, None] * a[:, k] for k in range(3)]
    return t[0] + (t[1] + t[2]) if variant == 'assoc' else (t[0] + t[1]) + t[2]


def interp(face_map, vertices, faces, cams, near, attr=None, fill=0.0, shade_mode=0, normals=None, variant=None):
    """pst_mesh_interp over face_map int64 [B, H, W] with the camera table cams float32 [B, 16] (mesh_ref.camera_table) ->
    dict(attr float32 [B, H, W, C] or None, shade float32 [B, H, W] or None, hit bool [B, H, W])"""
    face_map = np.asarray(face_map, dtype=np.int64)
    B, H, W = face_map.shape
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Nf = len(faces)
    safe = np.where(((faces >= 0) & (faces < len(vertices))).all(axis=1)[:, None], faces, 0)
    out_attr = None if attr is None else np.empty((B, H, W, attr.shape[1]), dtype=F)
    out_shade = None if shade_mode == 0 else np.empty((B, H, W), dtype=F)
    hits = np.zeros((B, H, W), dtype=bool)
    ii, jj = (x.reshape(-1) for x in np.meshgrid(np.arange(H), np.arange(W), indexing='ij'))
    for b in range(B):
        cam = np.asarray(cams[b], dtype=F)
        s = M.setup(vertices, faces, cam, H, W, near)
        f = face_map[b].reshape(-1)
        inrange = (f >= 0) & (f < Nf)
        fi = np.where(inrange, f, 0)
        E = M.edges(s, fi, ii, jj)
        hit = inrange & s['ok'][fi]
        if variant != 'no_coverage':
            hit &= (ii >= s['i0'][fi]) & (ii <= s['i1'][fi]) & (jj >= s['j0'][fi]) & (jj <= s['j1'][fi])
            hit &= (E[0] >= s['least'][fi, 0]) & (E[1] >= s['least'][fi, 1]) & (E[2] >= s['least'][fi, 2])
        with np.errstate(all='ignore'):
            if variant == 'affine':
                w = [E[k].astype(np.float64) / s['A'][fi].astype(np.float64) for k in range(3)]
            else:
                w = [E[k].astype(np.float64) * s['q'][fi, k] for k in range(3)]
            ssum = (w[0] + w[1]) + w[2]
            order = np.where(s['swapped'][fi][:, None] & (variant != 'no_swap'), [0, 2, 1], [0, 1, 2])
            vid = np.take_along_axis(safe[fi], order, axis=1)                  # the vertex at set-up corner k
            if attr is not None:
                a = np.asarray(attr, dtype=F)[vid].astype(np.float64)
                val = (_blend(w, a, variant) / ssum[:, None]).astype(F)
                out_attr[b] = np.where(hit[:, None], val, F(fill)).reshape(H, W, -1)
            if shade_mode != 0:
                if shade_mode == 2:
                    N = _blend(w, np.asarray(normals, dtype=F)[vid].astype(np.float64), variant)
                else:
                    N = face_vectors(vertices, safe[fi])
                c = cam.astype(np.float64)
                n = [(c[4 * r] * N[:, 0] + c[4 * r + 1] * N[:, 1]) + c[4 * r + 2] * N[:, 2] for r in range(3)]
                d0, d1 = ((jj.astype(np.float64) + 0.5) - c[14]) / c[12], ((ii.astype(np.float64) + 0.5) - c[15]) / c[13]
                dot = (n[0] * d0 + n[1] * d1) + n[2]
                nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                dd = (d0 * d0 + d1 * d1) + 1.0
                x = nn * dd
                good = np.isfinite(x) & (x > 0)
                val = (np.abs(dot) / sqrt_heron(np.where(good, x, 1.0), _steps(variant))).astype(F)
                out_shade[b] = np.where(hit & good, val, F(0)).reshape(H, W)
        hits[b] = hit.reshape(H, W)
    return dict(attr=out_attr, shade=out_shade, hit=hits)


def colors_u8(c):
    """engine.cloud.ply_colors_u8: uchar = floor(clip(c, 0, 1) * 255 + 0.5) in float32"""
    c = np.clip(np.asarray(c, dtype=F), F(0), F(1))
    return np.floor(c * F(255) + F(0.5)).astype(np.uint8)


def render_color(face_map, vertices, faces, cams, near, colors, shading='smooth', ambient=0.3, background=(0, 0, 0)):
    """PanopticMesh.render_color from the rendered face map -> uint8 [B, H, W, 3]"""
    mode = {'smooth': 2, 'flat': 1, None: 0}[shading]
    r = interp(face_map, vertices, faces, cams, near, attr=np.asarray(colors, dtype=F), fill=0.0, shade_mode=mode,
               normals=normals(vertices, faces) if mode == 2 else None)
    col = r['attr']
    if mode:
        light = (r['shade'] * F(1.0 - float(ambient))).astype(F) + F(float(ambient))
        col = (col * light[..., None]).astype(F)
    hit = np.asarray(face_map) >= 0
    return np.where(hit[..., None], colors_u8(col), colors_u8(np.asarray(background, dtype=F)))
