"""Time of the voxel fusion of the point cloud (engine/voxels.py, csrc/voxel.hip) for the benchmark scene: 50 views of 384 x 512 of one room
(tests/voxel_ref.overlapping_scene), every point kept.

    python tools/voxel_bench.py [--views 50] [--runs 10] [--numpy] [--limit SECONDS] [--out FILE.json]

Per voxel size (all points in one voxel / in between / every point alone), with the in-wave key merge on and off: HIP-event time of each kernel
(warm, median of --runs, workspaces re-initialised outside the timed region), of the workspace initialisation, and the wall time of the whole
`voxelize_cloud` call (which ends in its one host sync); Mv / M and the PLY size.  Next to them the bytes the pass has to move at the least,
    read   M x (12 + 12 + 4) once for the cells, again for the sums      (points, rgb, pan)
    write  M x 4 (point_voxel) + Mv x 60 (the seven outputs)
and the GB/s that makes - the tables, the workspaces and their initialisation come on top of it and are what the comparison shows.
--numpy adds the wall time of the numpy restatement on the host.  The device part stops itself after --limit seconds."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from panst3r_amd import hip                                                        # noqa: E402
from panst3r_amd.engine import panoptic_point_cloud, default_colors, voxelize_cloud  # noqa: E402
import voxel_ref as R                                                              # noqa: E402

SIZES = {'one': 1024.0, 'mid': 0.05, 'alone': 1e-5}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernels(cloud, vs, merge, runs):
    """median HIP-event milliseconds of each step of one fusion"""
    dev = cloud.pan.device
    M = len(cloud)
    inv = float(np.float32(1.0 / vs))
    ids = [s['id'] for s in cloud.segments]
    row = np.full(max(ids) + 1, -1, dtype=np.int32)
    row[ids] = np.arange(len(ids))
    id2row = torch.from_numpy(row).to(dev)
    nwg = (M + hip.CLOUD_WG - 1) // hip.CLOUD_WG
    i32 = dict(dtype=torch.int32, device=dev)
    counts, base, pv = torch.empty(nwg, **i32), torch.empty(nwg + 1, **i32), torch.empty(M, **i32)
    f3 = lambda: torch.empty(M, 3, dtype=torch.float32, device=dev)
    o = (f3(), f3(), torch.empty(M, **i32), f3(), torch.empty(M, **i32), torch.empty(M, dtype=torch.int64, device=dev))
    ts = {k: [] for k in ('init', 'insert', 'count', 'scan', 'rank', 'accumulate', 'vote', 'emit')}
    for it in range(runs + 2):
        box = {}
        t = {'init': event_ms(lambda: box.update(ws=hip.voxel_workspace(M, dev)))}
        ws = box['ws']
        t['insert'] = event_ms(lambda: hip.voxel_insert(cloud.points, inv, ws, merge))
        t['count'] = event_ms(lambda: hip.voxel_count(ws, counts))
        t['scan'] = event_ms(lambda: hip.cloud_scan(counts, base))
        t['rank'] = event_ms(lambda: hip.voxel_rank(ws, base))
        t['accumulate'] = event_ms(lambda: hip.voxel_accumulate(cloud.points, cloud.rgb, cloud.pan, inv, id2row, ws, pv, merge))
        t['vote'] = event_ms(lambda: hip.voxel_vote(ws))
        t['emit'] = event_ms(lambda: hip.voxel_emit(cloud.points, cloud.index, base[nwg:], inv, vs, ws, cloud._source.colors, 0.5, 0.5, *o))
        assert int(ws['status'][0]) == 0
        if it >= 2:
            for k in ts:
                ts[k].append(t[k])
        del ws, box
    return {k: float(np.median(v)) for k, v in ts.items()}, int(base[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=50)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--numpy', action='store_true')
    ap.add_argument('--limit', type=int, default=420)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    signal.alarm(a.limit)                                                          # its own time limit: the process ends, nothing is retried
    dev = 'cuda:0'
    x, im, pan, info, cams, _ = R.overlapping_scene([(384, 512)] * a.views, seed=4)
    colors = default_colors(len(info) + 1)
    td = lambda v: torch.from_numpy(v).to(dev)
    cloud = panoptic_point_cloud([{k: td(v) for k, v in d.items()} for d in x], [td(i) for i in im], None, [td(p) for p in pan], info, [torch.from_numpy(c) for c in cams],
                                 min_conf_thr=0.0, colors=colors)
    M = len(cloud)
    out = {'views': a.views, 'points': M, 'runs': a.runs, 'device': torch.cuda.get_device_name(0), 'cases': {}}
    for name, vs in SIZES.items():
        case = {'voxel_size': vs}
        for merge in (1, 0):
            ms, Mv = kernels(cloud, vs, merge, a.runs)
            old, hip.VOXEL_MERGE = hip.VOXEL_MERGE, merge
            wall = []
            for _ in range(max(3, a.runs // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                v = voxelize_cloud(cloud, vs)
                wall.append((time.perf_counter() - t0) * 1e3)
            hip.VOXEL_MERGE = old
            nbytes = 2 * 28 * M + 4 * M + 60 * Mv
            total = sum(ms.values())
            case['merge' if merge else 'plain'] = {'kernel_ms': ms, 'kernels_total_ms': total, 'voxelize_cloud_wall_ms': float(np.median(wall)), 'min_bytes': nbytes,
                                                   'GBps_of_min_bytes': nbytes / total / 1e6}
        case['voxels'], case['voxels_per_point'] = Mv, Mv / M
        with tempfile.TemporaryDirectory() as d:
            case['ply_bytes'] = os.path.getsize(v.write_ply(os.path.join(d, 'v.ply')))
        out['cases'][name] = case
        print(name, json.dumps(case), flush=True)
    signal.alarm(0)
    with tempfile.TemporaryDirectory() as d:
        out['cloud_ply_bytes'] = os.path.getsize(cloud.write_ply(os.path.join(d, 'c.ply')))
    if a.numpy:
        c = {k: getattr(cloud, k).cpu().numpy() for k in ('points', 'rgb', 'pan', 'index')}
        for name, vs in SIZES.items():
            t0 = time.perf_counter()
            R.voxelize(c['points'], c['rgb'], c['pan'], c['index'], [s['id'] for s in cloud.segments], vs, colors)
            out['cases'][name]['numpy_wall_ms'] = (time.perf_counter() - t0) * 1e3
            print(name, 'numpy %.0f ms' % out['cases'][name]['numpy_wall_ms'], flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
