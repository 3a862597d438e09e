#!/usr/bin/env python
"""Time the exact point-to-mesh distance (panst3r_amd.engine.mesh_distance: the build of the index and the query) at the benchmark scene's cloud size:
the box room of score3d_bench.py, 8 x 3.5 x 8 m, once tessellated into 3 072 faces and once into 1 002 252 (289 x 289 tiles per wall), against the
9.65 M predicted points of that bench - the room's surface sampled at 0.0109 and moved by noise of 1 cm - at radius 0.05.  In the same run
`nearest_points` of the same points against the 9.8 M samples of the room at spacing 0.0108: how the point-to-point metric obtains the same number,
and the thing to compare with.

    meshdist_bench.py        device events around N whole `MeshIndex` builds and N whole queries (host syncs included) after a warm-up, the series twice;
                             per mesh the (face, cell) pairs, pairs per face, the longest cell list and the mean candidates per query

Prints one JSON line.  One process: on a shared GPU box run it under its own `timeout -k 10 SECONDS`."""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from panst3r_amd.engine import sample_mesh, nearest_points
from panst3r_amd.engine.meshdist import MeshIndex

GT_SPACING, PRED_SPACING, RADIUS, NOISE, N, TILES, FINE_TILES = 0.0108, 0.0109, 0.05, 0.01, 3, 16, 289
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


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 3), r


def candidates(index, points):
    """the mean number of faces a query evaluates = the length of its own cell's list, by looking every query's cell key up in the index's table (plain
    torch: a sort and a search; not timed)"""
    c = torch.floor(points * index.inv).long() + (1 << 20)
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    used = index.ws['keys'] >= 0
    tab, order = torch.sort(index.ws['keys'][used])
    cnt = index.ws['cell_count'][used][order].long()
    pos = torch.searchsorted(tab, key).clamp(max=len(tab) - 1)
    return float(torch.where(tab[pos] == key, cnt[pos], torch.zeros_like(key)).double().mean())


def query(index, points):
    out = index.query(points)
    index.check()
    return out


verts, faces = room()
gt = sample_mesh(verts, faces, GT_SPACING)
pred = sample_mesh(verts, faces, PRED_SPACING).points
pred = pred + NOISE * torch.randn(pred.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
torch.cuda.synchronize()
out = {'workload': 'meshdist: %d predicted points at radius %g against the room in %d and in %d faces; nearest_points against %d samples at spacing %g'
                   % (len(pred), RADIUS, len(faces), 6 * 2 * FINE_TILES ** 2, len(gt), GT_SPACING)}
for name, (v, f) in (('coarse', (verts, faces)), ('fine', room(FINE_TILES))):
    index = timed(lambda: MeshIndex(v, f, RADIUS, max_cell_faces=1 << 20), 1)[1]           # the warm-up; the occupancy met, whatever the default guard says
    d2, face, _ = query(index, pred)
    cnt = index.ws['cell_count']
    res = {'faces': len(f), 'pairs': index.pairs, 'pairs_per_face': round(index.pairs / len(f), 1), 'longest_list': index.max_occupancy,
           'cells': int((cnt > 0).sum()), 'dropped_faces': index.dropped_faces, 'matched_share': round(float((face >= 0).float().mean()), 4),
           'mean_distance': round(float(d2[face >= 0].double().sqrt().mean()), 6)}
    res['candidates_per_query'] = round(candidates(index, pred), 1)
    res['ms_build'], res['ms_query'], res['ms_query_no_closest'] = [], [], []
    for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
        res['ms_build'].append(timed(lambda: MeshIndex(v, f, RADIUS, max_cell_faces=1 << 20), N)[0])
        res['ms_query'].append(timed(lambda: query(index, pred), N)[0])
        res['ms_query_no_closest'].append(timed(lambda: (index.query(pred, closest=False), index.check()), N)[0])
    out[name] = res
    del index
timed(lambda: nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20), 1)
out['ms_nearest_points'] = [timed(lambda: nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20), N)[0] for rep in range(2)]
d2, row = nearest_points(pred, gt.points, RADIUS, max_cell_points=1 << 20)
out['nearest_points_mean_distance'] = round(float(d2[row >= 0].double().sqrt().mean()), 6)
print(json.dumps(out))
