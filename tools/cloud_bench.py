"""Time of the panoptic point cloud (engine/cloud.py, csrc/cloud.hip) for the benchmark scene: 50 views of 384 x 512, about 60 segments.

    python tools/cloud_bench.py [--views 50] [--runs 20] [--numpy] [--out FILE.json]

Per threshold (keep nothing / about half / everything): HIP-event time of each kernel (warm, median of --runs), of the whole
`panoptic_point_cloud` call and of `rethreshold` alone (wall clock around the call, which ends in its one host sync), next to the bytes each
kernel has to move and the GB/s that makes:
    count    4 N                                            (conf)
    compact  4 N + 100 r N     (conf again; per kept point 12 + 12 + 12 + 4 read, 4 x 12 + 4 + 8 written)
    median   4 passes x (4 r N G + 12 L)                    (pan once per segment block G = ceil(S / 8), coordinates of the L non-void kept points)
--numpy adds the wall time of the numpy restatement on the host (what the demo pays per slider move), for orientation.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from panst3r_amd import hip                                           # noqa: E402
from panst3r_amd.engine.cloud import _Source, default_colors          # noqa: E402
import cloud_ref as R                                                 # noqa: E402


def timed(fn, runs):
    """median HIP-event milliseconds of fn() on the current stream, warm"""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=50)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--numpy', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = 'cuda:0'
    scene = R.synthetic_scene([(384, 512)] * a.views, seed=4, nseg=60)
    x, im, pan, info, cams = scene
    conf = np.concatenate([v['conf'].reshape(-1) for v in x])
    thr = {'none': float(conf.max()) * 2, 'half': float(np.sort(conf)[len(conf) // 2]), 'all': float(conf.min())}
    xd = [{k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in x]
    src = _Source(xd, [torch.from_numpy(i).to(dev) for i in im], None, [torch.from_numpy(p).to(dev) for p in pan], info, [torch.from_numpy(c) for c in cams],
                  None, default_colors(len(info) + 1), False)
    N, S, V = src.N, len(info), len(xd)
    G = (S + 7) // 8
    out = {'views': V, 'points': N, 'segments': S, 'runs': a.runs, 'device': torch.cuda.get_device_name(0), 'cases': {}}
    i32 = dict(dtype=torch.int32, device=dev)
    counts, base = torch.empty(src.nwg, **i32), torch.empty(src.nwg + 1, **i32)
    f3 = lambda: torch.empty(N, 3, dtype=torch.float32, device=dev)
    points, local, rgb, col = f3(), f3(), f3(), f3()
    pn, index = torch.empty(N, **i32), torch.empty(N, dtype=torch.int64, device=dev)
    count, median = torch.empty(S, **i32), torch.empty(S, 3, dtype=torch.float32, device=dev)
    for name, t in thr.items():
        k_count = lambda: hip.cloud_count(src.table, V, src.nwg, t, counts)
        k_scan = lambda: hip.cloud_scan(counts, base)
        k_compact = lambda: hip.cloud_compact(src.table, V, src.nwg, t, base, src.colors, 0.5, 0.5, points, local, rgb, pn, col, index)
        k_median = lambda: hip.cloud_segment_median(local, pn, base[src.nwg:], src.id2row, S, count, median)
        k_count(); k_scan(); k_compact(); k_median()
        M = int(base[-1])
        r = M / N
        L = int((pn[:M] > 0).sum())                                   # non-void kept points: the ones whose coordinates the median passes read
        ms = {'count': timed(k_count, a.runs), 'scan': timed(k_scan, a.runs), 'compact': timed(k_compact, a.runs), 'median': timed(k_median, a.runs)}
        nbytes = {'count': 4 * N, 'compact': 4 * N + 100 * M, 'median': 4 * (4 * M * G + 12 * L)}
        cloud = src.assemble(t, 0.5)
        wall = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cloud.rethreshold(t)
            wall.append((time.perf_counter() - t0) * 1e3)
        case = {'threshold': t, 'kept': M, 'keep_ratio': r, 'kernel_ms': ms, 'kernels_total_ms': sum(ms.values()), 'rethreshold_wall_ms': float(np.median(wall)),
                'bytes': nbytes, 'GBps': {k: nbytes[k] / ms[k] / 1e6 for k in nbytes}}
        if a.numpy:
            t0 = time.perf_counter()
            R.cloud(x, im, pan, info, cams, min_conf_thr=t, colors=default_colors(len(info) + 1))
            case['numpy_wall_ms'] = (time.perf_counter() - t0) * 1e3
        out['cases'][name] = case
        print(name, json.dumps(case), flush=True)
    from panst3r_amd.engine import panoptic_point_cloud
    torch.cuda.synchronize()
    wall = []
    for _ in range(max(3, a.runs // 4)):
        t0 = time.perf_counter()
        panoptic_point_cloud(xd, [v[3] for v in src.views], None, [v[4] for v in src.views], info, [torch.from_numpy(c) for c in cams],
                             min_conf_thr=thr['half'])
        wall.append((time.perf_counter() - t0) * 1e3)
    out['panoptic_point_cloud_wall_ms_half'] = float(np.median(wall))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
