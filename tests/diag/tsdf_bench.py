#!/usr/bin/env python
"""Time the fused TSDF surface (panst3r_amd.engine.fuse_surface, csrc/tsdf.hip) and record what it does to a reconstruction's score.

    tsdf_bench.py [--voxel MM]         the kernels of one fusion, one by one, at the benchmark's scene size: 50 views of 384x512 of
                                       voxel_ref.overlapping_scene (9.8 M pixels) at a voxel size of MM millimetres (default 50), band 2; device
                                       events around N launches after a warm-up, the series twice; the memory of the node table
    tsdf_bench.py --ref [--voxel MM]   tests/tsdf_ref.py (numpy) on the same inputs - the voxels' cells, counts, ids and colours come from the device,
                                       the restatement of THIS stage is timed
    tsdf_bench.py --floaters           consistency_bench.py --floaters' room (12 views of 192x256, 2 % of the pixels pushed toward the camera):
                                       score_reconstruction(metric='surface') of the raw cloud, the f9 mesh (cloud.mesh()) and the fused mesh

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`, no
retries.  overlapping_scene puts pixel x at u = x + 0.5, the stage at u = x: the principal point handed over is (W / 2 - 0.5, H / 2 - 0.5)."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import voxel_ref

H, W, V = 384, 512, 50
N = 10
BAND = 2
dev = 'cuda:0'


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv and len(sys.argv) > sys.argv.index(name) + 1 and sys.argv[sys.argv.index(name) + 1].isdigit() else default


def put(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def floaters():
    """the room of consistency_bench.py --floaters, built the same way"""
    from panst3r_amd.engine import ground_truth_maps, panoptic_point_cloud, score_reconstruction
    rng = np.random.default_rng(0)
    Hs, Ws, Vs, share = 192, 256, 12, 0.02
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
        return [grid(p0, np.eye(3)[(a + 1) % 3] * d[(a + 1) % 3], np.eye(3)[(a + 2) % 3] * d[(a + 2) % 3], n)
                for a in range(3) for p0 in (lo, lo + np.eye(3)[a] * d[a])]
    parts = [(p, 1 + k) for k, p in enumerate(box(voxel_ref.ROOM_LO, voxel_ref.ROOM_HI, 24))]
    for k, (lo, hi) in enumerate(voxel_ref.BOXES):
        parts += [(p, 7 + k) for p in box(lo, hi, 6)]
    verts, faces, vids, nv = [], [], [], 0
    for (v, fc), pid in parts:
        verts.append(v); faces.append(fc + nv); vids.append(np.full(len(v), pid, dtype=np.int32)); nv += len(v)
    verts, faces, vids = np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32), np.concatenate(vids)
    segments = [{'id': i, 'category_id': i % 5} for i in range(1, voxel_ref.N_LABELS + 1)]
    centre = (voxel_ref.ROOM_LO + voxel_ref.ROOM_HI) / 2 - np.array([0.0, 0.0, 1.2])
    cams = [voxel_ref._look_at(np.array([5.0 + 3.2 * np.cos(a), 5.0 + 3.2 * np.sin(a), 4.2]), centre) for a in 2 * np.pi * np.arange(Vs) / Vs + 0.1]
    cameras = [{'cam2world': c, 'fx': f, 'fy': f, 'cx': Ws / 2 + 0.5, 'cy': Hs / 2 + 0.5, 'height': Hs, 'width': Ws} for c in cams]
    vd, fd = put(verts), put(faces)
    maps, _, depths = ground_truth_maps(vd, fd, vids, segments, cameras, min_area=0, near=0.05, far=30.0)
    ys, xs = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    x_out, imgs = [], []
    for c, d in zip(cams, depths):
        d = d.cpu().numpy().astype(np.float64)
        hit = d > 0
        fl = hit & (rng.uniform(0, 1, d.shape) < share)
        z = np.where(fl, d * rng.uniform(0.4, 0.85, d.shape), d * (1 + 1e-3 * rng.standard_normal(d.shape)))
        loc = np.stack([(xs - Ws / 2) * z / f, (ys - Hs / 2) * z / f, z], -1)
        pts = loc @ c[:3, :3].T + c[:3, 3]
        x_out.append({'pts3d': put(pts.astype(np.float32)), 'pts3d_local': put(loc.astype(np.float32)), 'conf': put(np.where(hit, 5.0, 1.0).astype(np.float32))})
        imgs.append(torch.zeros(3, Hs, Ws, device=dev))
    cloud = panoptic_point_cloud(x_out, imgs, None, maps, segments, [torch.from_numpy(c) for c in cams], [f] * Vs, min_conf_thr=3.0)
    vs = arg('--voxel', 50) / 1000.0
    fused = cloud.fused_mesh(vs, band=BAND)
    out = {'workload': 'floaters: %d views of %dx%d of a box room with %d boxes, %.0f %% of the measured pixels pushed to 0.4 .. 0.85 of their depth' % (Vs, Hs, Ws, len(voxel_ref.BOXES), 100 * share),
           'score': "score_reconstruction(metric='surface', thresholds=(0.02, 0.05), spacing=0.05)", 'voxel_size': vs, 'band': BAND, 'points': len(cloud),
           'f9_faces': None, 'fused_faces': len(fused), 'fused_stats': fused.tsdf_stats}
    f9 = cloud.mesh()
    out['f9_faces'] = len(f9)
    for name, pred in (('cloud', cloud), ('f9_mesh', f9), ('fused_mesh', fused)):
        s = score_reconstruction(pred, vd, fd, thresholds=(0.02, 0.05), spacing=0.05, metric='surface')
        out[name] = {'fscore': [round(float(p), 5) for p in s['fscore']], 'precision': [round(float(p), 5) for p in s['precision']],
                     'recall': [round(float(p), 5) for p in s['recall']], 'accuracy_mean': round(float(s['accuracy_mean']), 5), 'completeness_mean': round(float(s['completeness_mean']), 5)}
    print(json.dumps(out))


if '--floaters' in sys.argv:
    floaters()
    sys.exit(0)

from panst3r_amd import hip
from panst3r_amd.engine import panoptic_point_cloud
from panst3r_amd.engine.consistency import own_camera_table

vs = arg('--voxel', 50) / 1000.0
t0 = time.perf_counter()
x, im, pan, info, cams = voxel_ref.overlapping_scene([(H, W)] * V, seed=4)[:5]
cams = [np.asarray(c, dtype=np.float64) for c in cams]
focals, pp = [0.55 * W] * V, (W / 2 - 0.5, H / 2 - 0.5)
out = {'workload': 'fuse_surface: %d views of %dx%d, every pixel measured, voxel size %g, band %d' % (V, H, W, vs, BAND), 'scene_s': round(time.perf_counter() - t0, 1)}
thr = float(min(v['conf'].min() for v in x))
cloud = panoptic_point_cloud([{k: put(v) for k, v in d.items()} for d in x], [put(i) for i in im], None, [put(p) for p in pan], info,
                             [torch.from_numpy(c) for c in cams], focals, min_conf_thr=thr)
vox = cloud.voxelize(vs)
Mv = len(vox)
out.update(points=len(cloud), voxels=Mv, pairs=hip.tsdf_pairs(Mv, BAND), table_slots=hip.tsdf_capacity(Mv, BAND), table_MiB=round(hip.tsdf_table_bytes(Mv, BAND) / 2 ** 20, 1))

if '--ref' in sys.argv:
    import tsdf_ref as T
    cells, count, vpan, vcol = (t.cpu().numpy() for t in (vox.cells, vox.count, vox.pan, vox.colors))
    t0 = time.perf_counter()
    r = T.fuse(cells, count, vpan, vcol, x, cams, focals, vs, min_conf_thr=thr, band=BAND, pp=pp)
    out.update(ref_fuse_s=round(time.perf_counter() - t0, 1), stats=r['stats'], faces=len(r['faces']))
    print(json.dumps(out))
    sys.exit(0)

# the steps of engine.tsdf.fuse_surface, one launch each
src = cloud._source
shapes = src.shapes
table, camd, dims, vwg, NP = hip.consist_view_table([(c, p, l, None) for c, p, l, _, _ in src.views], src.c34, own_camera_table(cams, focals, shapes, pp), shapes, dev)
depth = torch.empty(NP, dtype=torch.float32, device=dev)
hip.consist_depth(table, camd, V, vwg, thr, False, depth)
cells = vox.cells.contiguous()
e = lambda *s, dtype=torch.int32: torch.empty(*s, dtype=dtype, device=dev)
P = hip.tsdf_pairs(Mv, BAND)
pwg, pcounts, pbase = hip.scan_buffers(dev, P)


def table_build():
    ws = hip.tsdf_workspace(Mv, BAND, dev)
    hip.tsdf_insert(cells, BAND, ws)
    return ws


ws = table_build()
hip.voxel_count(ws, pcounts); hip.cloud_scan(pcounts, pbase); hip.voxel_rank(ws, pbase)
Nn = int(pbase[pwg])
nodes, voxel_row, sdf, weight, cell_vertex, face_mask = e(Nn, 3), torch.full((Nn,), -1, dtype=torch.int32, device=dev), e(Nn, dtype=torch.float32), e(Nn), e(Nn), e(Nn)
nwg, counts, base = hip.scan_buffers(dev, Nn)
fbase = torch.empty_like(base)
vs32 = float(np.float32(vs))
hip.tsdf_nodes(cells, BAND, Nn, ws, nodes, voxel_row)
hip.tsdf_integrate(nodes, vs32, BAND, table, camd, dims, V, depth, sdf, weight)
hip.tsdf_cells(nodes, ws, sdf, weight, 1, cell_vertex, counts)
hip.cloud_scan(counts, base)
Nv = int(base[nwg])
flags = cell_vertex.clone()
vertices, vertex_ids, colors = e(Nv, 3, dtype=torch.float32), e(Nv), e(Nv, 3, dtype=torch.float32)
vcount, vpan, vcol = vox.count.contiguous(), vox.pan.contiguous(), vox.colors.float().contiguous()


def run_vertices():
    cell_vertex.copy_(flags)                                                  # the kernel turns the flags into vertex rows in place
    hip.tsdf_vertices(nodes, ws, sdf, weight, 1, voxel_row, vcount, vpan, vcol, vs32, base, cell_vertex, vertices, vertex_ids, colors)


run_vertices()
hip.tsdf_face_count(nodes, ws, sdf, weight, 1, cell_vertex, face_mask, counts)
hip.cloud_scan(counts, fbase)
Fn = int(fbase[nwg])
faces, face_ids, edge = e(6 * Nv, 3), e(6 * Nv), e(6 * Nv, dtype=torch.int64)
out.update(nodes=Nn, node_view_pairs=Nn * V, valid_nodes=int((weight >= 1).sum()), vertices=Nv, faces=Fn)
runs = {'insert_with_table_fill': table_build,
        'rank': lambda: (hip.voxel_count(ws, pcounts), hip.cloud_scan(pcounts, pbase), hip.voxel_rank(ws, pbase)),
        'nodes': lambda: hip.tsdf_nodes(cells, BAND, Nn, ws, nodes, voxel_row),
        'depth': lambda: hip.consist_depth(table, camd, V, vwg, thr, False, depth),
        'integrate': lambda: hip.tsdf_integrate(nodes, vs32, BAND, table, camd, dims, V, depth, sdf, weight),
        'cells': lambda: (hip.tsdf_cells(nodes, ws, sdf, weight, 1, flags, counts), hip.cloud_scan(counts, base)),
        'vertices_with_flag_copy': run_vertices,
        'face_count': lambda: (hip.tsdf_face_count(nodes, ws, sdf, weight, 1, cell_vertex, face_mask, counts), hip.cloud_scan(counts, fbase)),
        'face_emit': lambda: hip.tsdf_face_emit(nodes, ws, sdf, cell_vertex, face_mask, vertex_ids, fbase, faces, face_ids, edge),
        'fuse_surface': lambda: cloud.fused_mesh(vs, band=BAND, vox=vox, pp=pp)}
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for name, fn in runs.items():
        n = 3 if name in ('insert_with_table_fill', 'fuse_surface') else N
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.setdefault('ms_' + name, []).append(round(a.elapsed_time(b) / n, 4))
print(json.dumps(out))
