#!/usr/bin/env python
"""Time one fused point-to-plane ICP step against the triangles (panst3r_amd.hip.icp_plane_step: move, the mesh distance's list walk and the 38
float64 moments of the normal equations in one launch plus a one-block reduction) next to what it is made of and what it replaces, on the same
sources: one point-to-point `hip.icp_step` against the ground truth's samples, and one `MeshIndex.query` (d2 and face, no closest point).  The scene
is meshdist_bench.py's: the box room of 8 x 3.5 x 8 m, once in 3 072 faces and once in 1 002 252, against the 9.65 M predicted points of that bench -
the room's surface sampled at 0.0109 plus 1 cm of noise - displaced by icp_bench.py's rigid motion of 0.2 degrees and 1.5 cm, cells and radius 0.05.
Then one whole `icp_to_mesh` and one whole `refine_alignment` (point to point) from that start, and how far each ends from the known motion.

    icp_plane_bench.py   device events around N calls of each kind after a warm-up, the kinds alternating, the series twice (the spread between the two
                         values is the noise)

Prints one JSON line.  One process: on a shared GPU box run it under its own `timeout -k 10 SECONDS`."""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from panst3r_amd import hip
from panst3r_amd.engine import sample_mesh, refine_alignment, icp_to_mesh
from panst3r_amd.engine.meshdist import MeshIndex
from panst3r_amd.engine.score3d import NearestIndex

GT_SPACING, PRED_SPACING, RADIUS, MIN_DIST, NOISE, N, TILES, FINE_TILES = 0.0108, 0.0109, 0.05, 0.02, 0.01, 3, 16, 289
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
        i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
        k = lambda i, j: nv + i * (n + 1) + j
        faces.append(np.stack([np.stack([k(i, j), k(i + 1, j), k(i + 1, j + 1)], 1), np.stack([k(i, j), k(i + 1, j + 1), k(i, j + 1)], 1)], 1).reshape(-1, 3))
        nv += (n + 1) ** 2
    return torch.tensor(np.concatenate(verts), dtype=torch.float32, device=dev), torch.tensor(np.concatenate(faces), dtype=torch.int64, device=dev)


def rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 3), r


def corner_error(T):
    return float(np.abs((T - D)[:3] @ np.array([[4.0, 1.5, 5.0, 1.0]]).T).max())


verts, faces = room()
gt = sample_mesh(verts, faces, GT_SPACING)
pred = sample_mesh(verts, faces, PRED_SPACING).points
pred = pred + NOISE * torch.randn(pred.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
D = np.eye(4)
D[:3, :3], D[:3, 3] = rotation((1, 2, -0.5), 0.2), [0.009, -0.009, 0.008]
Di = torch.tensor(np.linalg.inv(D), dtype=torch.float32, device=dev)
away = (pred @ Di[:3, :3].T + Di[:3, 3]).contiguous()                           # the prediction in a frame of its own: D carries it back
torch.cuda.synchronize()
out = {'workload': 'icp_plane: %d sources, cells and radius %g, displaced by 0.2 degrees and %.1f cm; the room in %d and in %d faces; icp_step against %d '
                   'samples at spacing %g' % (len(away), RADIUS, 100 * float(np.linalg.norm(D[:3, 3])), len(faces), 6 * 2 * FINE_TILES ** 2, len(gt), GT_SPACING)}
A = np.eye(4)[:3].astype(np.float32)
C0 = np.zeros(3, dtype=np.float32)

points = NearestIndex(gt.points, RADIUS, max_cell_points=1 << 20)               # the occupancy met, whatever the default guard says about it
iws = hip.icp_workspace(len(away), dev)
pws = hip.icp_plane_workspace(len(away), dev)
to_points = lambda: hip.icp_step(away, A, points.targets, points.inv, points.r2, points.r2, points.ws, points.max_cell_points, iws)
timed(to_points, 1)
for name, (v, f) in (('coarse', (verts, faces)), ('fine', room(FINE_TILES))):
    index = MeshIndex(v, f, RADIUS, max_cell_faces=1 << 20)
    plane = lambda: hip.icp_plane_step(away, A, C0, index.vertices, index.faces, index.inv, index.r2, index.r2, index.ws, index.max_cell_faces, pws)
    query = lambda: (index.query(away, closest=False), index.check())
    mom = timed(plane, 1)[1].cpu().numpy()
    (d2, face, _), _ = timed(query, 1)[1]
    assert mom[0] == int((face >= 0).sum()) and abs(mom[37] - float(d2[face >= 0].double().sum())) <= 1e-9 * mom[37]      # the step's matches are the query's
    res = {'faces': len(f), 'pairs': index.pairs, 'longest_list': index.max_occupancy, 'matched': int(mom[0]), 'rmse': float(np.sqrt(mom[37] / mom[0])),
           'plane_rmse': float(np.sqrt(mom[36] / mom[0]))}
    for rep in range(2):                                                          # the whole series twice, the kinds alternating
        for key, fn in (('ms_plane_step', plane), ('ms_mesh_query_no_closest', query), ('ms_icp_step_points', to_points)):
            res.setdefault(key, []).append(timed(fn, N)[0])
    out[name] = res
    del index
kw = dict(max_dist=RADIUS, min_dist=MIN_DIST)
icp_to_mesh(away, verts, faces, iters=2, max_cell_faces=1 << 20, **kw)          # warm-up
ms, al = timed(lambda: icp_to_mesh(away, verts, faces, max_cell_faces=1 << 20, **kw), 1)
out['icp_to_mesh'] = {'ms': ms, 'iterations': al.iterations, 'reason': al.reason, 'first': al.history[0], 'last': al.history[-1],
                      'ms_per_iteration': round(ms / al.iterations, 3), 'corner_error_m': corner_error(al.transform.numpy())}
refine_alignment(away, verts, faces, spacing=GT_SPACING, iters=2, max_cell_points=1 << 20, **kw)
ms, al = timed(lambda: refine_alignment(away, verts, faces, spacing=GT_SPACING, max_cell_points=1 << 20, **kw), 1)
out['refine_alignment_points'] = {'ms': ms, 'iterations': al.iterations, 'reason': al.reason, 'first': al.history[0], 'last': al.history[-1],
                                  'ms_per_iteration': round(ms / al.iterations, 3), 'corner_error_m': corner_error(al.transform.numpy())}
print(json.dumps(out))
