#!/usr/bin/env python
"""Time the fused ICP step (panst3r_amd.hip.icp_step: move, search and the float64 moments in one launch plus a one-block reduction) against the same
step COMPOSED from the public calls that existed before it - a torch move, `NearestIndex.query`, a gather of the matched targets, the moments as
float64 reductions through torch - and a whole `refine_alignment`, on the scene of score3d_bench.py: a box room of 8 x 3.5 x 8 m in 3 072 faces,
sampled at spacing 0.0108 to 9.8 M ground-truth points, against 9.7 M predicted points - the same surface sampled at 0.0109 plus 1 cm of noise - here
displaced by a rigid motion of 0.2 degrees and 1.5 cm that the refinement has to find.

    icp_bench.py         device events around N steps of either kind after a warm-up, the two kinds alternating, the series twice (the spread between
                         the two values is the noise); then one `refine_alignment` (the sampling, the build, every step and its host sync)

Prints one JSON line.  One process: on a shared GPU box run it under its own `timeout -k 10 SECONDS`."""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from panst3r_amd import hip
from panst3r_amd.engine import sample_mesh, refine_alignment
from panst3r_amd.engine.score3d import NearestIndex

GT_SPACING, PRED_SPACING, RADIUS, MIN_DIST, NOISE, N, TILES = 0.0108, 0.0109, 0.05, 0.02, 0.01, 5, 16
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


verts, faces = room()
gt = sample_mesh(verts, faces, GT_SPACING)
pred = sample_mesh(verts, faces, PRED_SPACING).points
pred = pred + NOISE * torch.randn(pred.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
D = np.eye(4)
D[:3, :3], D[:3, 3] = rotation((1, 2, -0.5), 0.2), [0.009, -0.009, 0.008]
Di = torch.tensor(np.linalg.inv(D), dtype=torch.float32, device=dev)
away = (pred @ Di[:3, :3].T + Di[:3, 3]).contiguous()                           # the prediction in a frame of its own: D carries it back
torch.cuda.synchronize()
out = {'workload': 'icp: %d sources against %d targets (spacing %g), cells and radius %g (radius / spacing %.2f), displaced by 0.2 degrees and %.1f cm'
                   % (len(away), len(gt), GT_SPACING, RADIUS, RADIUS / GT_SPACING, 100 * float(np.linalg.norm(D[:3, 3])))}

index = NearestIndex(gt.points, RADIUS, max_cell_points=1 << 20)               # the occupancy met, whatever the default guard says about it
out['max_cell_occupancy'] = index.max_occupancy
iws = hip.icp_workspace(len(away), dev)
A = np.eye(4)[:3].astype(np.float32)
At = torch.tensor(A, device=dev)


def fused():
    return hip.icp_step(away, A, index.targets, index.inv, index.r2, index.r2, index.ws, index.max_cell_points, iws)


def composed():
    """the same 18 sums from the calls the parent had: 12 B per point written by the move, the query's d2 and row, a second scattered read of the
    matched targets, float64 temporaries for the products"""
    moved = (away @ At[:, :3].T + At[:, 3]).contiguous()
    d2, row = index.query(moved)
    hit = row >= 0
    h = hit.double()[:, None]
    x, y = away.double() * h, index.targets[row.clamp(min=0).long()].double() * h
    return torch.cat([hit.sum().double()[None], x.sum(0), y.sum(0), (y.T @ x).reshape(-1), (x * x).sum()[None],
                      torch.where(hit, d2, torch.zeros_like(d2)).double().sum()[None]])


fused_mom, composed_mom = timed(fused, 2)[1].cpu().numpy(), timed(composed, 2)[1].cpu().numpy()      # the warm-up; the two agree up to the order of the sums
out['matched'] = int(fused_mom[0])
out['moments_max_rel_diff'] = float(np.abs(fused_mom[:18] - composed_mom).max() / np.abs(composed_mom).max())
assert fused_mom[0] == composed_mom[0] and out['moments_max_rel_diff'] < 1e-9
for rep in range(2):                                                          # the whole series twice, the kinds alternating
    for name, fn in (('ms_icp_step_fused', fused), ('ms_icp_step_composed', composed)):
        out.setdefault(name, []).append(timed(fn, N)[0])
kw = dict(spacing=GT_SPACING, max_dist=RADIUS, min_dist=MIN_DIST, max_cell_points=1 << 20)
refine_alignment(away, verts, faces, iters=2, **kw)                           # warm-up
for rep in range(2):
    ms, al = timed(lambda: refine_alignment(away, verts, faces, **kw), 1)
    out.setdefault('ms_refine_alignment', []).append(ms)
T = al.transform.numpy()
out['refine'] = {'iterations': al.iterations, 'reason': al.reason, 'first': al.history[0], 'last': al.history[-1],
                 'ms_per_iteration': round(out['ms_refine_alignment'][-1] / al.iterations, 3),
                 'corner_error_m': float(np.abs((T - D)[:3] @ np.array([[4.0, 1.5, 5.0, 1.0]]).T).max())}
print(json.dumps(out))
