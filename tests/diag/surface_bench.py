#!/usr/bin/env python
"""Time the surface mesh of the pointmap grids (panst3r_amd.engine.panoptic_mesh, PanopticMesh.drop_small) at the benchmark scene's shape: 50 views of
384x512 synthetic pointmaps (a smooth depth with a step per view, 88 % of the pixels kept), 9.8 M quads.

    surface_bench.py         device events around N whole `cloud.mesh()` calls and N whole `mesh.drop_small(64)` calls (the islands labelled again in
                             every call) after a warm-up, the series twice; then one `mesh.render` of 16 novel cameras at 384x512
    surface_bench.py --ref   tests/surface_ref.py (numpy) on the same cloud: the triangulation of the whole scene, the islands of its first REF_VIEWS views

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, math, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from panst3r_amd.engine import panoptic_point_cloud, orbit_cameras, PanopticMesh

V, H, W = 50, 384, 512
FOCAL, THR, MIN_FACES, N, REF_VIEWS = 0.8 * W, 1.3, 64, 10, 4
dev = 'cuda:0'


def make_scene():
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
    return x_out, imgs, pan, info, cams


t0 = time.perf_counter()
x_out, imgs, pan, info, cams = make_scene()
cloud = panoptic_point_cloud(x_out, imgs, None, pan, info, cams, [FOCAL] * V, min_conf_thr=THR)
torch.cuda.synchronize()
out = {'workload': 'panoptic_mesh: %d views of %dx%d, %d quads, %d of %d pixels kept' % (V, H, W, V * (H - 1) * (W - 1), len(cloud), V * H * W),
       'scene_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    import surface_ref as S
    index, ids = cloud.index.cpu().numpy(), cloud.pan.cpu().numpy()
    depths = [x['pts3d_local'][..., 2].cpu().numpy() for x in x_out]
    t0 = time.perf_counter()
    m = S.mesh(index, ids, [(H, W)] * V, depths)
    out['surface_ref_mesh_s'], out['faces'] = round(time.perf_counter() - t0, 2), len(m['faces'])
    few = index < REF_VIEWS * H * W                                            # the first views alone: their rows are the first rows of the cloud
    m = S.mesh(index[few], ids[few], [(H, W)] * REF_VIEWS, depths[:REF_VIEWS])
    t0 = time.perf_counter()
    d = S.drop_small(m, int(few.sum()), MIN_FACES)
    out['surface_ref_drop_small_%d_views_s' % REF_VIEWS] = round(time.perf_counter() - t0, 2)
    out['faces_%d_views' % REF_VIEWS], out['kept_%d_views' % REF_VIEWS] = len(m['faces']), len(d['faces'])
    print(json.dumps(out))
    sys.exit(0)


def run_mesh(n):
    for _ in range(n):
        m = cloud.mesh()
    return m


def run_drop(mesh, n):
    for _ in range(n):
        fresh = PanopticMesh(mesh.vertices, mesh.faces, mesh.face_ids, mesh.vertex_ids, mesh.colors, mesh.quad, mesh.view_offsets, mesh.segments, mesh.cameras)
        d = fresh.drop_small(MIN_FACES)                                        # a fresh mesh on the same tensors labels its islands again: the whole call is timed
    return d


mesh = run_mesh(2)
kept = run_drop(mesh, 2)
torch.cuda.synchronize()
out['faces'], out['faces_after_drop_small_%d' % MIN_FACES] = len(mesh), len(kept)
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for name, fn in (('ms_panoptic_mesh', lambda: run_mesh(N)), ('ms_drop_small', lambda: run_drop(mesh, N))):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.setdefault(name, []).append(round(a.elapsed_time(b) / N, 4))
turntable = orbit_cameras((0.0, 0.0, 2.0), 1.0, 16, 0.2, up=(0, -1, 0))        # the scene's frame has y pointing down
r = kept.render(turntable, FOCAL, (H, W))
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
r = kept.render(turntable, FOCAL, (H, W))
b.record()
torch.cuda.synchronize()
out['ms_render_16_cameras'], out['hit_share'] = round(a.elapsed_time(b), 4), round(float(r.hit.float().mean()), 4)
print(json.dumps(out))
