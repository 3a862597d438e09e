"""numpy restatement of the panoptic point cloud (reference tools/demo_panst3r.py:279-300, 351-352, 622-687), the yardstick of csrc/cloud.hip.

Own code: the demo module cannot be imported (gradio / viser / roma at its top) and dust3r's `geotrf` / `rgb` are not vendored, so nothing here is
pinned to the reference's output - the semantics are restated from its lines and the ARITHMETIC ORDER is the one include/panst3r_hip.h fixes:
elementwise float32 numpy rounds every product and every sum on its own, which is exactly what the kernel promises, so the comparison is bit for bit.
"""
import numpy as np

F = np.float32


def geotrf(c2w, pts):
    """x' = ((R00 x + R01 y) + R02 z) + t0 ..., float32, each operation rounded on its own.  pts [n, 3]"""
    c = np.asarray(c2w, dtype=F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((c[r, 0] * x + c[r, 1] * y) + c[r, 2] * z) + c[r, 3] for r in range(3)], axis=1).astype(F)


def blend(rgb, pan_vis, opacity):
    """w1 * rgb + w2 * pan_vis with w1 = float32(1 - opacity) (taken in double), w2 = float32(opacity)"""
    w1, w2 = F(1.0 - float(opacity)), F(float(opacity))
    return (w1 * rgb + w2 * pan_vis).astype(F)


def median_two_stat(x):
    """the kernel's form of np.median for float32: the middle order statistic (odd), (a + b) * 0.5f of the two middle ones (even).  The order is the
    total one of include/panst3r_hip.h: -0.0 below +0.0 (np.sort leaves equal zeros where it finds them).  NaN for an axis that holds a NaN, as
    np.median, and for no values at all.  The sum and the product are plain float32 operations: subnormals are kept, an overflowing sum is inf."""
    x = np.asarray(x, dtype=F).reshape(-1)
    if len(x) == 0 or np.isnan(x).any():
        return F(np.nan)
    s = x[np.lexsort((~np.signbit(x), x))]
    n = len(s)
    return s[n // 2] if n % 2 else F(F(s[n // 2 - 1] + s[n // 2]) * F(0.5))


def cloud(x_out, imgs, pan, segments_info, cams2world, min_conf_thr=3.0, opacity=0.5, colors=None, local_pointmaps=False):
    """x_out: list of dict(pts3d, pts3d_local [H,W,3], conf [H,W]) float32 arrays; imgs [3,H,W] in [-1,1]; pan int [H,W]; colors [n_ids,3].
    Returns dict(points, points_local, rgb, pan, colors, index, segments)."""
    conf = np.concatenate([np.asarray(x['conf'], dtype=F).reshape(-1) for x in x_out])
    pts = np.concatenate([np.asarray(x['pts3d'], dtype=F).reshape(-1, 3) for x in x_out])
    loc = np.concatenate([geotrf(c, np.asarray(x['pts3d_local'], dtype=F).reshape(-1, 3)) for c, x in zip(cams2world, x_out)])
    rgb = np.concatenate([(np.asarray(i, dtype=F) * F(0.5) + F(0.5)).transpose(1, 2, 0).reshape(-1, 3) for i in imgs])
    pan_f = np.concatenate([np.asarray(p).reshape(-1) for p in pan]).astype(np.int32)
    colors = np.asarray(colors, dtype=F).reshape(-1, 3)
    m = conf >= F(min_conf_thr)
    idx = np.nonzero(m)[0].astype(np.int64)
    pts, loc, rgb, pan_f = pts[m], loc[m], rgb[m], pan_f[m]
    known = (pan_f > 0) & (pan_f < len(colors))
    pan_vis = np.zeros((len(pan_f), 3), dtype=F)
    pan_vis[known] = colors[pan_f[known]]
    segments = []
    for seg in segments_info:
        sel = pan_f == seg['id']
        if not np.any(sel):
            continue
        segments.append({'id': seg['id'], 'query_id': seg.get('query_id'), 'category_id': seg.get('category_id'), 'count': int(sel.sum()),
                         'median': np.median(loc[sel], axis=0)})
    return {'points': loc if local_pointmaps else pts, 'points_local': loc, 'rgb': rgb, 'pan': pan_f, 'colors': blend(rgb, pan_vis, opacity), 'index': idx,
            'segments': segments}


def frusta(shapes, focals, cams2world):
    """fov = 2 atan2(H / 2, focal), aspect = W / H, position (demo :669-683); the quaternion is checked against known rotations instead"""
    return [{'fov': 2 * np.arctan2(H / 2, f), 'aspect': W / H, 'position': np.asarray(c, dtype=np.float64)[:3, 3]} for (H, W), f, c in zip(shapes, focals, cams2world)]


def synthetic_scene(shapes, seed=0, nseg=60):
    """A seeded scene for the GPU tests and tools/cloud_bench.py: pointmaps, confidences (exp-like, > 1) and cameras from a numpy generator, images
    from synthetic.synth_image, and a panoptic map of `nseg` segments of very unequal size.  Segment 1 is a single pixel of view 0, segment 2 an
    even number of pixels (a 2 x 3 patch), segment 3 a patch whose confidence is forced below every threshold used (1.0); segment nseg + 1 is
    listed in segments_info but never drawn.  Returns (x_out, imgs, pan, segments_info, cams2world) as numpy arrays."""
    from panst3r_amd.synthetic import synth_image
    g = np.random.Generator(np.random.PCG64(seed))
    x_out, imgs, pan, cams = [], [], [], []
    cuts = np.sort(g.uniform(0, 1, nseg - 4)) ** 2            # unequal band widths
    for v, (H, W) in enumerate(shapes):
        pts = g.standard_normal((H, W, 3)).astype(F) * F(2.0)
        loc = g.standard_normal((H, W, 3)).astype(F) * F(2.0)
        conf = (F(1.0) + np.exp(g.standard_normal((H, W)).astype(F))).astype(F)
        # bands of columns, shifted per view; ids 4 .. nseg, 0 = void in the first rows
        col = (np.arange(W) / W + 0.37 * v) % 1.0
        band = (np.searchsorted(cuts, col) + 4).astype(np.int32)
        p = np.broadcast_to(band[None, :], (H, W)).copy()
        p[: max(1, H // 16)] = 0
        if v == 0:
            p[p == 1] = 0
            p[H // 2, W // 2] = 1
            p[H // 2 + 2: H // 2 + 4, 2:5] = 2
            p[H - 4: H - 1, 1:9] = 3
            conf[H // 2, W // 2] = 50.0
            conf[H // 2 + 2: H // 2 + 4, 2:5] = 50.0
            conf[H - 4: H - 1, 1:9] = 1.0
        a = g.standard_normal((3, 3))
        q, _ = np.linalg.qr(a)
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c = np.eye(4, dtype=F)
        c[:3, :3], c[:3, 3] = q.astype(F), g.standard_normal(3).astype(F)
        x_out.append({'pts3d': pts, 'pts3d_local': loc, 'conf': conf})
        imgs.append(synth_image(v, H, W).numpy())
        pan.append(p)
        cams.append(c)
    segments_info = [{'id': i, 'query_id': i - 1, 'category_id': i % 7} for i in range(1, nseg + 2)]
    return x_out, imgs, pan, segments_info, cams
