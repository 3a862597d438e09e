#!/usr/bin/env python
"""Time the mesh simplification (PanopticMesh.simplify, csrc/simplify.hip on top of the voxel kernels) at the benchmark scene's shape and record what
it does to the size of a mesh.

    simplify_bench.py           surface_bench.py's scene (50 views of 384x512, 9.8 M quads): `cloud.mesh()` -> `simplify` at 1, 2 and 5 cm, dedupe on
                                (and off at 1 and 5 cm); device events around N whole calls after a warm-up, the series twice; vertex and face counts
                                before and after, the PLY sizes (header + 19 bytes per vertex + 17 per face, as write_ply packs them), and
                                `mesh.render` of the same 16 turntable cameras on the unsimplified and on every simplified mesh, in this process
    simplify_bench.py --fused   tsdf_bench.py's scene (voxel_ref.overlapping_scene, 50 views of 384x512): `cloud.fused_mesh(0.05, band=2)` ->
                                `simplify` at 10 and 20 cm, the same way
    simplify_bench.py --ref     tests/simplify_ref.py (numpy) on the first scene's mesh at 5 cm

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, math, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from panst3r_amd.engine import panoptic_point_cloud, orbit_cameras

V, H, W = 50, 384, 512
FOCAL, THR, N = 0.8 * W, 1.3, 5
dev = 'cuda:0'


def surface_scene():
    """the scene of surface_bench.py, built the same way"""
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing='ij')
    x_out, imgs, pan, cams = [], [], [], []
    for v in range(V):
        z = 2.0 + 0.5 * torch.sin(xx / 40 + v) * torch.cos(yy / 30) + 0.8 * (xx > 200 + 3 * v)
        local = torch.stack([(xx + 0.5 - W / 2) * z / FOCAL, (yy + 0.5 - H / 2) * z / FOCAL, z], dim=-1)
        a = math.radians(7.2 * v)
        c = torch.eye(4)
        c[:3, :3] = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        c[:3, 3] = torch.tensor([0.1 * v, 0.0, -0.05 * v])
        cd = c.to(dev)
        x_out.append({'pts3d': local @ cd[:3, :3].T + cd[:3, 3], 'pts3d_local': local, 'conf': 1 + torch.exp(torch.randn(H, W, device=dev, generator=g))})
        imgs.append(torch.rand(3, H, W, device=dev, generator=g) * 2 - 1)
        pan.append((1 + (xx // 64) + 8 * (yy // 128)).to(torch.int32))
        cams.append(c)
    info = [{'id': i, 'query_id': i - 1, 'category_id': i % 7} for i in range(1, 25)]
    cloud = panoptic_point_cloud(x_out, imgs, None, pan, info, cams, [FOCAL] * V, min_conf_thr=THR)
    return cloud.mesh(), orbit_cameras((0.0, 0.0, 2.0), 1.0, 16, 0.2, up=(0, -1, 0)), FOCAL          # the scene's frame has y pointing down


def fused_scene():
    """the scene of tsdf_bench.py, built the same way, fused at 5 cm"""
    import voxel_ref
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, im, pan, info, cams = voxel_ref.overlapping_scene([(H, W)] * V, seed=4)[:5]
    cams = [np.asarray(c, dtype=np.float64) for c in cams]
    focals, pp = [0.55 * W] * V, (W / 2 - 0.5, H / 2 - 0.5)
    thr = float(min(v['conf'].min() for v in x))
    cloud = panoptic_point_cloud([{k: put(v) for k, v in d.items()} for d in x], [put(i) for i in im], None, [put(p) for p in pan], info,
                                 [torch.from_numpy(c) for c in cams], focals, min_conf_thr=thr)
    centre = (voxel_ref.ROOM_LO + voxel_ref.ROOM_HI) / 2
    return cloud.fused_mesh(0.05, band=2, pp=pp), orbit_cameras(tuple(centre), 2.5, 16, 0.3, up=(0, 0, 1)), 0.55 * W


def ply_bytes(mesh):
    M, F = int(mesh.vertices.shape[0]), len(mesh)
    header = ('ply\nformat binary_little_endian 1.0\ncomment panst3r_amd panoptic surface mesh\nelement vertex %d\nproperty float x\nproperty float y\n'
              'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nelement face %d\n'
              'property list uchar int vertex_indices\nproperty int label\nend_header\n' % (M, F))
    return len(header) + 19 * M + 17 * F


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 4), r


t0 = time.perf_counter()
fused = '--fused' in sys.argv
mesh, turntable, focal = fused_scene() if fused else surface_scene()
torch.cuda.synchronize()
out = {'workload': ('fused_mesh(0.05, band=2) of 50 views of 384x512 (overlapping_scene)' if fused else 'cloud.mesh() of 50 views of 384x512 (surface_bench scene)'),
       'scene_s': round(time.perf_counter() - t0, 1), 'vertices': int(mesh.vertices.shape[0]), 'faces': len(mesh), 'ply_bytes': ply_bytes(mesh)}

if '--ref' in sys.argv:
    import simplify_ref as S
    arrays = [t.cpu().numpy() for t in (mesh.vertices, mesh.colors, mesh.vertex_ids, mesh.faces, mesh.quad)]
    t0 = time.perf_counter()
    r = S.simplify(*arrays, [int(s['id']) for s in mesh.segments], 0.05)
    out.update(simplify_ref_5cm_s=round(time.perf_counter() - t0, 1), stats=r['stats'])
    print(json.dumps(out))
    sys.exit(0)

cases = [(0.10, True), (0.20, True)] if fused else [(0.01, True), (0.01, False), (0.02, True), (0.05, True), (0.05, False)]
results = {}
for cell, dedupe in cases:
    try:
        results[(cell, dedupe)] = mesh.simplify(cell, dedupe=dedupe)             # the warm-up
    except ValueError as e:                                                     # the 2^21 cap of dedupe at a small cell: on record, not timed
        out['simplify_%gcm_dedupe_%d' % (100 * cell, dedupe)] = {'refused': str(e)}
torch.cuda.synchronize()
for rep in range(2):                                                            # the whole series twice: the spread between the two is the noise
    for (cell, dedupe), small in results.items():
        ms, _ = timed(lambda: mesh.simplify(cell, dedupe=dedupe), N)
        row = out.setdefault('simplify_%gcm_dedupe_%d' % (100 * cell, dedupe), {'stats': small.simplify_stats, 'ply_bytes': ply_bytes(small), 'ms': []})
        row['ms'].append(ms)
mesh.render(turntable, focal, (H, W))
torch.cuda.synchronize()
ms, r = timed(lambda: mesh.render(turntable, focal, (H, W)), 2)
out['ms_render_16_cameras'], out['hit_share'] = ms, round(float(r.hit.float().mean()), 4)
for (cell, dedupe), small in results.items():
    small.render(turntable, focal, (H, W))
    torch.cuda.synchronize()
    ms, r = timed(lambda: small.render(turntable, focal, (H, W)), 2)
    row = out['simplify_%gcm_dedupe_%d' % (100 * cell, dedupe)]
    row['ms_render_16_cameras'], row['hit_share'] = ms, round(float(r.hit.float().mean()), 4)
print(json.dumps(out))
