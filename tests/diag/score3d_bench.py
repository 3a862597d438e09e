#!/usr/bin/env python
"""Time the two primitives of the 3-D scores (panst3r_amd.engine.sample_mesh, nearest_points) and `score_reconstruction` at the benchmark scene's cloud
size: a box room of 8 x 3.5 x 8 m tessellated into 3 072 faces, sampled at spacing 0.0108 to 9.8 M ground-truth points, against 9.7 M predicted
points - the same surface sampled at 0.0109 and moved by noise of 1 cm.  The sampler is timed once more on the same room in 1 002 252 faces (289 x 289
tiles per wall), where the single-workgroup scan of the per-face counts takes 979 rounds instead of 3.

    score3d_bench.py         device events around N whole `sample_mesh` calls and N whole `nearest_points` calls (build, host sync, query) after a
                             warm-up, the series twice; then one `score_reconstruction`
    score3d_bench.py --ref   scipy.spatial.cKDTree on the same points and radius, same box: build and query (workers = the CPUs the job may use)

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from panst3r_amd.engine import sample_mesh, nearest_points, score_reconstruction
from panst3r_amd.engine.score3d import NearestIndex

GT_SPACING, PRED_SPACING, RADIUS, NOISE, N, TILES, FINE_TILES = 0.0108, 0.0109, 0.05, 0.01, 5, 16, 289
TAUS = (0.02, 0.05)
dev = 'cuda:0'


def room(n=TILES):
    """vertices [Nv,3], faces [Nf,3]: six walls of n x n quads, two triangles each"""
    x0, x1, y0, y1, z0, z1 = -4.0, 4.0, -2.0, 1.5, -3.0, 5.0
    walls = [((x0, y0, z1), (x1 - x0, 0, 0), (0, y1 - y0, 0)), ((x0, y0, z0), (x1 - x0, 0, 0), (0, y1 - y0, 0)), ((x0, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0)),
             ((x1, y0, z0), (0, 0, z1 - z0), (0, y1 - y0, 0)), ((x0, y0, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0)), ((x0, y1, z0), (x1 - x0, 0, 0), (0, 0, z1 - z0))]
    verts, faces, nv = [], [], 0
    for p0, du, dv in walls:
        a, b = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n, indexing='ij')
        verts.append((np.asarray(p0) + a[..., None] * np.asarray(du) + b[..., None] * np.asarray(dv)).reshape(-1, 3))
        k = lambda i, j: nv + i * (n + 1) + j
        faces.extend(t for i in range(n) for j in range(n) for t in ((k(i, j), k(i + 1, j), k(i + 1, j + 1)), (k(i, j), k(i + 1, j + 1), k(i, j + 1))))
        nv += (n + 1) ** 2
    return torch.tensor(np.concatenate(verts), dtype=torch.float32, device=dev), torch.tensor(faces, dtype=torch.int64, device=dev)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 3), r


verts, faces = room()
gt = sample_mesh(verts, faces, GT_SPACING)
pred = sample_mesh(verts, faces, PRED_SPACING).points
pred = pred + NOISE * torch.randn(pred.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
torch.cuda.synchronize()
out = {'workload': 'score3d: %d faces, %d ground-truth samples at spacing %g, %d predicted points, radius %g (radius / spacing %.2f)'
                   % (len(faces), len(gt), GT_SPACING, len(pred), RADIUS, RADIUS / GT_SPACING)}

if '--ref' in sys.argv:
    from scipy.spatial import cKDTree
    g, p = gt.points.cpu().numpy().astype(np.float64), pred.cpu().numpy().astype(np.float64)
    workers = int(os.environ.get('OMP_NUM_THREADS', '16'))
    t0 = time.perf_counter()
    tree = cKDTree(g)
    out['ckdtree_build_s'] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    d, i = tree.query(p, k=1, distance_upper_bound=RADIUS, workers=workers)
    out['ckdtree_query_s'], out['workers'], out['matched_share'] = round(time.perf_counter() - t0, 2), workers, round(float(np.isfinite(d).mean()), 4)
    print(json.dumps(out))
    sys.exit(0)

index = NearestIndex(gt.points, RADIUS, max_cell_points=1 << 20)               # the occupancy met, whatever the default guard says about it
out['max_cell_occupancy'], out['dropped_targets'] = index.max_occupancy, index.dropped
timed(lambda: sample_mesh(verts, faces, GT_SPACING), 2)
timed(lambda: nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20), 1)
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for name, fn, n in (('ms_sample_mesh', lambda: sample_mesh(verts, faces, GT_SPACING), N),
                        ('ms_nearest_points', lambda: nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20), N),
                        ('ms_nearest_build_only', lambda: NearestIndex(gt.points, RADIUS, max_cell_points=1 << 20), N)):
        out.setdefault(name, []).append(timed(fn, n)[0])
fine_v, fine_f = room(FINE_TILES)
fine = timed(lambda: sample_mesh(fine_v, fine_f, GT_SPACING), 2)[1]
out['fine_faces'], out['fine_samples'] = len(fine_f), len(fine)
out['ms_sample_mesh_fine'] = [timed(lambda: sample_mesh(fine_v, fine_f, GT_SPACING), N)[0] for rep in range(2)]
d2, row = nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20)
out['matched_share'] = round(float((row >= 0).float().mean()), 4)
ms, s = timed(lambda: score_reconstruction(pred, verts, faces, thresholds=TAUS, spacing=GT_SPACING, max_cell_points=1 << 20), 1)
out['ms_score_reconstruction'] = ms
out['scores'] = {k: s[k] for k in ('precision', 'recall', 'fscore', 'accuracy_mean', 'completeness_mean', 'chamfer', 'n_pred', 'n_gt')}
print(json.dumps(out))
