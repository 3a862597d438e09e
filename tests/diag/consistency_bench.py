#!/usr/bin/env python
"""Time the cross-view depth consistency (panst3r_amd.engine.view_consistency, csrc/consistency.hip) and record what the default floater filter does.

    consistency_bench.py               the two kernels at the benchmark's scene size, 50 views of 384x512 of voxel_ref.overlapping_scene (9.8 M pixels,
                                       4.8e8 pairs), with and without labels; device events around N launches after a warm-up, the series twice
    consistency_bench.py --views 200   the same at 200 views (39 M pixels, 7.8e9 pairs)
    consistency_bench.py --ref [K]     tests/consistency_ref.py (numpy) on the same 50-view inputs: the depth pass of every view, and the count pass of
                                       the first K (default: all 50) source views against all 49 targets, scaled to 50 sources: what the host would do
    consistency_bench.py --floaters    a synthetic room rasterised by ground_truth_maps from 12 cameras, a known share of pixels pushed toward the
                                       camera: how many of them, and how many true points, PanopticCloud.filter_consistent() removes at its defaults,
                                       and score_reconstruction(metric='surface') precision before and after

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`.
overlapping_scene puts pixel x at u = x + 0.5, the consistency stage at u = x: the principal point handed over is (W / 2 - 0.5, H / 2 - 0.5)."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import voxel_ref

H, W = 384, 512
N = 10
dev = 'cuda:0'


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv and len(sys.argv) > sys.argv.index(name) + 1 and sys.argv[sys.argv.index(name) + 1].isdigit() else default


def bench_scene(V):
    x, im, pan, info, cams = voxel_ref.overlapping_scene([(H, W)] * V, seed=4)[:5]
    return x, pan, [np.asarray(c, dtype=np.float64) for c in cams], [0.55 * W] * V, (W / 2 - 0.5, H / 2 - 0.5)


def floaters():
    from panst3r_amd.engine import ground_truth_maps, panoptic_point_cloud, score_reconstruction
    rng = np.random.default_rng(0)
    Hs, Ws, V, share = 192, 256, 12, 0.02
    f = 0.55 * Ws

    def grid(p0, du, dv, n):
        p0, du, dv = (np.asarray(a, dtype=np.float64) for a in (p0, du, dv))
        i, j = np.mgrid[0:n + 1, 0:n + 1]
        v = p0 + i.reshape(-1, 1) * du / n + j.reshape(-1, 1) * dv / n
        q = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
        return v, np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)])

    def box(lo, hi, n):
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        d = hi - lo
        out = []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for p0 in (lo, lo + np.eye(3)[a] * d[a]):
                out.append(grid(p0, np.eye(3)[b] * d[b], np.eye(3)[c] * d[c], n))
        return out
    parts = [(p, 1 + k) for k, p in enumerate(box(voxel_ref.ROOM_LO, voxel_ref.ROOM_HI, 24))]
    for k, (lo, hi) in enumerate(voxel_ref.BOXES):
        parts += [(p, 7 + k) for p in box(lo, hi, 6)]
    verts, faces, vids, nv = [], [], [], 0
    for (v, fc), pid in parts:
        verts.append(v); faces.append(fc + nv); vids.append(np.full(len(v), pid, dtype=np.int32)); nv += len(v)
    verts, faces, vids = np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32), np.concatenate(vids)
    segments = [{'id': i, 'category_id': i % 5} for i in range(1, voxel_ref.N_LABELS + 1)]
    centre = (voxel_ref.ROOM_LO + voxel_ref.ROOM_HI) / 2 - np.array([0.0, 0.0, 1.2])
    cams = [voxel_ref._look_at(np.array([5.0 + 3.2 * np.cos(a), 5.0 + 3.2 * np.sin(a), 4.2]), centre) for a in 2 * np.pi * np.arange(V) / V + 0.1]
    # pixel x at u = x (the pointmaps' convention): the rasteriser samples pixel centres x + 0.5, so its principal point is half a pixel further
    cameras = [{'cam2world': c, 'fx': f, 'fy': f, 'cx': Ws / 2 + 0.5, 'cy': Hs / 2 + 0.5, 'height': Hs, 'width': Ws} for c in cams]
    vd, fd = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    maps, _, depths = ground_truth_maps(vd, fd, vids, segments, cameras, min_area=0, near=0.05, far=30.0)
    ys, xs = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    x_out, imgs, injected = [], [], []
    for c, d in zip(cams, depths):
        d = d.cpu().numpy().astype(np.float64)
        hit = d > 0
        fl = hit & (rng.uniform(0, 1, d.shape) < share)
        z = np.where(fl, d * rng.uniform(0.4, 0.85, d.shape), d * (1 + 1e-3 * rng.standard_normal(d.shape)))
        loc = np.stack([(xs - Ws / 2) * z / f, (ys - Hs / 2) * z / f, z], -1)
        pts = loc @ c[:3, :3].T + c[:3, 3]
        x_out.append({'pts3d': torch.from_numpy(pts.astype(np.float32)).to(dev), 'pts3d_local': torch.from_numpy(loc.astype(np.float32)).to(dev),
                      'conf': torch.from_numpy(np.where(hit, 5.0, 1.0).astype(np.float32)).to(dev)})
        imgs.append(torch.zeros(3, Hs, Ws, device=dev))
        injected.append(fl.reshape(-1))
    injected = np.concatenate(injected)
    cloud = panoptic_point_cloud(x_out, imgs, None, maps, segments, [torch.from_numpy(c) for c in cams], [f] * V, min_conf_thr=3.0)
    filt = cloud.filter_consistent()
    idx, kept = cloud.index.cpu().numpy(), np.zeros(len(injected), dtype=bool)
    kept[filt.index.cpu().numpy()] = True
    live = np.zeros(len(injected), dtype=bool)
    live[idx] = True
    out = {'workload': 'floaters: %d views of %dx%d of a box room with %d boxes, %.0f %% of the measured pixels pushed to 0.4 .. 0.85 of their depth' % (V, Hs, Ws, len(voxel_ref.BOXES), 100 * share),
           'filter': 'filter_consistent() defaults: min_views=1, max_violations=0, rel_tol=0.03', 'points': int(live.sum()),
           'floaters': int((injected & live).sum()), 'floaters_removed': int((injected & live & ~kept).sum()),
           'true_points': int((~injected & live).sum()), 'true_points_removed': int((~injected & live & ~kept).sum())}
    for name, c in (('before', cloud), ('after', filt)):
        s = score_reconstruction(c, vd, fd, thresholds=(0.02, 0.05), spacing=0.05, metric='surface')
        out['precision_%s' % name] = [round(float(p), 5) for p in s['precision']]
        out['recall_%s' % name] = [round(float(p), 5) for p in s['recall']]
    print(json.dumps(out))


if '--floaters' in sys.argv:
    floaters()
    sys.exit(0)

V = arg('--views', 50)
t0 = time.perf_counter()
x, pan, cams, focals, pp = bench_scene(50 if '--ref' in sys.argv else V)
out = {'workload': 'view_consistency: %d views of %dx%d, every pixel measured, rel_tol 0.03' % (len(x), H, W), 'scene_s': round(time.perf_counter() - t0, 1)}
thr = float(min(v['conf'].min() for v in x))

if '--ref' in sys.argv:
    import consistency_ref as R
    K = arg('--ref', len(x))
    shapes = [(H, W)] * len(x)
    tab = R.camera_tables(cams, focals, shapes, pp)
    t0 = time.perf_counter()
    world = R.world_points(x, cams, False)
    depth = [R.own_depth(world[v], x[v]['conf'], tab[v], thr) for v in range(len(x))]
    out['ref_depth_s'] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    agree = violate = 0
    for i in range(K):
        for j in range(len(x)):
            if j != i:
                inside, cell, zc = R.project(world[i], tab[j], H, W)
                d = np.where(inside, depth[j][cell], np.float32(0))
                ag, vi = R.compare(zc, d, 0.03)
                seen = inside & (d != 0)
                agree, violate = agree + int((seen & ag).sum()), violate + int((seen & vi).sum())
    s = time.perf_counter() - t0
    out.update(ref_count_sources=K, ref_count_s=round(s, 2), ref_count_scaled_to_all_sources_s=round(s * len(x) / K, 1), agree_pairs=agree, violate_pairs=violate)
    print(json.dumps(out))
    sys.exit(0)

from panst3r_amd import hip
from panst3r_amd.engine.consistency import own_camera_table
views = [(torch.from_numpy(v['conf']).to(dev), torch.from_numpy(v['pts3d']).to(dev), torch.from_numpy(v['pts3d_local']).to(dev),
          torch.from_numpy(np.ascontiguousarray(p)).to(dev)) for v, p in zip(x, pan)]
shapes = [(H, W)] * V
c34 = [np.asarray(c, dtype=np.float32)[:3, :4] for c in cams]
table, camd, dims, nwg, NP = hip.consist_view_table(views, c34, own_camera_table(cams, focals, shapes, pp), shapes, dev)
plain, _, _, _, _ = hip.consist_view_table([v[:3] + (None,) for v in views], c34, own_camera_table(cams, focals, shapes, pp), shapes, dev)
depth = torch.empty(NP, dtype=torch.float32, device=dev)
agree, violate, same = (torch.empty(NP, dtype=torch.int32, device=dev) for _ in range(3))
out.update(pixels=NP, pairs=NP * (V - 1))
runs = {'depth': lambda: hip.consist_depth(table, camd, V, nwg, thr, False, depth),
        'depth_local': lambda: hip.consist_depth(table, camd, V, nwg, thr, True, depth),
        'count': lambda: hip.consist_count(plain, camd, dims, V, nwg, 0.03, False, depth, agree, violate, None),
        'count_labels': lambda: hip.consist_count(table, camd, dims, V, nwg, 0.03, False, depth, agree, violate, same)}
n = N if V <= 50 else 3
for fn in runs.values():
    fn()                                                                      # warm-up
torch.cuda.synchronize()
runs['depth']()                                                               # the counts below read the depth of the global pointmaps
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for name in ('count', 'count_labels', 'depth_local', 'depth'):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            runs[name]()
        b.record()
        torch.cuda.synchronize()
        out.setdefault('ms_' + name, []).append(round(a.elapsed_time(b) / n, 4))
seen = (depth != 0)
out.update(measured_share=round(float(seen.float().mean()), 4), agree_mean=round(float(agree.float().mean()), 3), violate_mean=round(float(violate.float().mean()), 3),
           same_label_mean=round(float(same.float().mean()), 3), keep_share=round(float(((agree >= 1) & (violate == 0)).float().mean()), 4))
print(json.dumps(out))
