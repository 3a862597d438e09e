"""numpy restatement of the voxel fusion of the point cloud (panst3r_amd/engine/voxels.py, csrc/voxel.hip), the yardstick the kernels are held to bit
for bit, and a seeded scene whose views really overlap in 3-D.

Own design (the reference has no such stage).  The five steps of the contract in include/panst3r_hip.h:
  1 cell      inv = float32(1 / float64(voxel_size)); t = p * inv in float32; c = floor(t).  A point with a non-finite coordinate or |c| >= 2^20 on an
              axis is left out (counted in `dropped`).
  2 position  q = int(floor((t - c) * 65536)) in float32 (the difference is one rounded operation: exact for t >= 0, correctly rounded for t < 0, where it
              can reach 1 and q = 65536; the product is exact), summed per voxel and axis as integers;
              pos = float32((float64(c) + float64(sum) / float64(count) * 2^-16) * float64(voxel_size)), every float64 operation rounded on its own.
  3 colour    u = floor(clip(rgb, 0, 1) * 255 + 0.5) in float32 (NaN -> 0), summed as integers; mean = float32(float64(sum) / float64(count) / 255.0);
              colour = w1 * mean + w2 * table[pan], as the cloud blends.
  4 vote      one vote per point for its id; ids <= 0 and ids that are not in the segment table are void; the non-void id with the most votes wins, ties
              to the smallest id; only void votes: id 0, votes = their number.
  5 order     voxels by their smallest member row (np.unique's first index, re-sorted).
Elementwise numpy rounds every operation on its own, which is what the kernels promise; the sums are integers, exact in any order."""
import numpy as np

import cloud_ref

F = np.float32
LIM = 1 << 20


def cells(points, voxel_size):
    """(t, c float32 [M, 3], keep bool [M]) of step 1"""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    with np.errstate(over='ignore', invalid='ignore'):
        inv = F(1.0 / float(voxel_size))
        t = (p * inv).astype(F)
        c = np.floor(t)
        keep = np.isfinite(p).all(axis=1) & (np.abs(c) < F(LIM)).all(axis=1)
    return t, c, keep


def voxelize(points, rgb, pan, index, segment_ids, voxel_size, colors, opacity=0.5):
    """points, rgb [M, 3] float32, pan [M] int, index [M] int64, segment_ids: the ids of the segment table, colors [n_ids, 3].  Returns dict(points, rgb,
    pan, colors, count, votes, first_index, point_voxel, dropped)."""
    vs = float(voxel_size)
    rgb, pan, index = np.asarray(rgb, dtype=F).reshape(-1, 3), np.asarray(pan).reshape(-1).astype(np.int32), np.asarray(index).reshape(-1).astype(np.int64)
    colors = np.asarray(colors, dtype=F).reshape(-1, 3)
    M = len(pan)
    t, c, keep = cells(points, vs)
    rows = np.nonzero(keep)[0]
    t, c = t[keep], c[keep]
    ci = c.astype(np.int64) + LIM
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    with np.errstate(invalid='ignore'):
        q = np.floor(((t - c).astype(F) * F(65536)).astype(F)).astype(np.int64)                     # step 2
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')                                                          # step 5
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    vox = rank[inverse.reshape(-1)]
    Mv = len(first)
    first_row = rows[first[order]] if Mv else np.zeros(0, dtype=np.int64)
    count = np.bincount(vox, minlength=Mv).astype(np.int64)
    isum = lambda v: np.stack([np.bincount(vox, weights=v[:, a].astype(np.float64), minlength=Mv) for a in range(3)], axis=1) if Mv else np.zeros((0, 3))
    qsum = isum(q)                                                                                    # integers below 2^53: exact in float64
    cnt = count.astype(np.float64)[:, None]
    cf = c[first[order]].astype(np.float64) if Mv else np.zeros((0, 3))
    pos = ((cf + (qsum / cnt) * np.float64(2.0 ** -16)) * np.float64(vs)).astype(F)
    g = rgb[keep]
    g = np.where(np.isnan(g), F(0), g)
    u = np.floor((np.clip(g, F(0), F(1)) * F(255) + F(0.5)).astype(F)).astype(np.int64)           # step 3
    mean = ((isum(u) / cnt) / np.float64(255.0)).astype(F)
    # step 4
    ntab = max([int(i) for i in segment_ids] + [0]) + 1
    in_table = np.zeros(ntab, dtype=bool)
    in_table[[int(i) for i in segment_ids]] = True
    pk = pan[keep].astype(np.int64)
    valid = (pk > 0) & (pk < ntab)
    valid[valid] = in_table[pk[valid]]
    vpan, votes = np.zeros(Mv, dtype=np.int32), count.astype(np.int32).copy()
    if valid.any():
        pairs, n = np.unique(vox[valid] * ntab + pk[valid], return_counts=True)
        pv, pid = pairs // ntab, pairs % ntab
        o = np.lexsort((pid, -n, pv))                                                                 # by voxel, then most votes, then smallest id
        head = np.ones(len(o), dtype=bool)
        head[1:] = pv[o][1:] != pv[o][:-1]
        w = o[head]
        vpan[pv[w]] = pid[w].astype(np.int32)
        votes[pv[w]] = n[w].astype(np.int32)
    known = (vpan > 0) & (vpan < len(colors))
    vis = np.zeros((Mv, 3), dtype=F)
    vis[known] = colors[vpan[known]]
    point_voxel = np.full(M, -1, dtype=np.int32)
    point_voxel[rows] = vox.astype(np.int32)
    return {'points': pos, 'rgb': mean, 'pan': vpan, 'colors': cloud_ref.blend(mean, vis, opacity), 'count': count.astype(np.int32), 'votes': votes,
            'first_index': index[first_row], 'point_voxel': point_voxel, 'dropped': int(M - len(rows))}


def segments(vox, segments_info):
    """the voxel cloud's segment table: per listed segment with a voxel, the number of voxels and np.median of their positions"""
    out = []
    for seg in segments_info:
        sel = vox['pan'] == seg['id']
        if sel.any():
            out.append({'id': seg['id'], 'query_id': seg.get('query_id'), 'category_id': seg.get('category_id'), 'count': int(sel.sum()),
                        'median': np.median(vox['points'][sel], axis=0)})
    return out


def point_labels(vox, pan):
    pv = vox['point_voxel']
    out = np.asarray(pan).astype(np.int32).copy()
    out[pv >= 0] = vox['pan'][pv[pv >= 0]]
    return out


def consistent_maps(vox, cloud, pan_maps):
    """cloud: dict(pan, index) of cloud_ref.cloud; pan_maps: the per-view input maps"""
    flat = np.concatenate([np.asarray(p).reshape(-1) for p in pan_maps]).astype(np.int32)
    flat[cloud['index']] = point_labels(vox, cloud['pan'])
    out, off = [], 0
    for p in pan_maps:
        out.append(flat[off:off + p.size].reshape(p.shape))
        off += p.size
    return out


# ---------------------------------------------------------------- a scene whose views overlap in 3-D
ROOM_LO, ROOM_HI = np.array([1.0, 1.0, 1.0]), np.array([9.0, 9.0, 5.0])       # all coordinates positive: one huge cell can hold the scene
BOXES = [((2.0, 2.5, 1.0), (3.5, 4.0, 2.5)), ((5.0, 5.5, 1.0), (7.0, 6.5, 2.0)), ((6.0, 2.0, 1.0), (7.0, 3.0, 3.5)), ((3.0, 6.0, 1.0), (4.5, 7.5, 1.8))]
N_LABELS = 6 + len(BOXES)                                                     # room faces 1 .. 6, boxes 7 ...


def _look_at(eye, target):
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    c = np.eye(4)
    c[:3, 0], c[:3, 1], c[:3, 2], c[:3, 3] = x, y, z, eye
    return c


def _cast(o, d):
    """nearest hit of the rays o + s d with the room (from inside) and the boxes (from outside) -> (distance, surface label)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / d
        a, b = (ROOM_LO - o) * inv, (ROOM_HI - o) * inv
        far = np.maximum(a, b)                                                # the room: where the ray leaves the slab intersection
        axis = np.argmin(far, axis=1)
        s = far[np.arange(len(d)), axis]
        label = 1 + 2 * axis + (d[np.arange(len(d)), axis] > 0)
        for k, (lo, hi) in enumerate(BOXES):
            a, b = (np.array(lo) - o) * inv, (np.array(hi) - o) * inv
            near, farb = np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
            hit = (near < farb) & (near > 0) & (near < s)
            s = np.where(hit, near, s)
            label = np.where(hit, 7 + k, label)
    return s, label.astype(np.int32)


def overlapping_scene(shapes, seed=0, flip=0.2, noise=2e-3):
    """Views of one room with boxes, from cameras on a circle under the ceiling that look at its middle: global pointmaps with seeded noise, local
    pointmaps, confidences (> 1, exp-like), images shaded per surface, per-view panoptic maps = the surface labels with a seeded fraction `flip` of
    pixels relabelled at random.  Returns (x_out, imgs, pan, segments_info, cams2world, clean) - `clean` the per-view labels without flips."""
    g = np.random.Generator(np.random.PCG64(seed))
    V = len(shapes)
    centre = (ROOM_LO + ROOM_HI) / 2 - np.array([0.0, 0.0, 1.2])
    x_out, imgs, pan, cams, clean = [], [], [], [], []
    for v, (H, W) in enumerate(shapes):
        ang = 2 * np.pi * v / V + 0.1
        eye = np.array([5.0 + 3.2 * np.cos(ang), 5.0 + 3.2 * np.sin(ang), 4.2])
        c2w = _look_at(eye, centre + g.uniform(-0.3, 0.3, 3))
        f = 0.55 * max(H, W)
        ys, xs = np.mgrid[0:H, 0:W]
        dc = np.stack([(xs + 0.5 - W / 2) / f, (ys + 0.5 - H / 2) / f, np.ones((H, W))], axis=-1).reshape(-1, 3)
        s, lab = _cast(np.broadcast_to(eye, dc.shape), dc @ c2w[:3, :3].T)
        loc = dc * s[:, None] + g.standard_normal(dc.shape) * noise
        c32 = c2w.astype(F)
        pts = cloud_ref.geotrf(c32, loc.astype(F))
        conf = (F(1.0) + np.exp(g.standard_normal(H * W).astype(F))).astype(F)
        shade = 0.35 + 0.06 * lab[:, None] * np.array([1.0, -0.7, 0.4]) + 0.05 * np.sin(pts * 3.0)
        img = (np.clip(shade, 0, 1) * 2 - 1).astype(F).reshape(H, W, 3).transpose(2, 0, 1).copy()
        noisy = lab.copy()
        sel = g.uniform(0, 1, H * W) < flip
        noisy[sel] = g.integers(1, N_LABELS + 1, int(sel.sum())).astype(np.int32)
        x_out.append({'pts3d': pts.reshape(H, W, 3), 'pts3d_local': loc.astype(F).reshape(H, W, 3), 'conf': conf.reshape(H, W)})
        imgs.append(img)
        pan.append(noisy.reshape(H, W))
        clean.append(lab.reshape(H, W))
        cams.append(c32)
    segments_info = [{'id': i, 'query_id': i - 1, 'category_id': i % 5} for i in range(1, N_LABELS + 1)]
    return x_out, imgs, pan, segments_info, cams, clean
