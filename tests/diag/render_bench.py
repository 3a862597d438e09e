#!/usr/bin/env python
"""Time the GPU cloud renderer (panst3r_amd.engine.render_cloud) on the full-size case of tests/test_hip_render.py: the cloud of 50 views of 384x512 of
voxel_ref.overlapping_scene with every point kept (9.8 M points), rendered at 384x512 from cameras of a turntable inside the room.

    render_bench.py            render_cloud for 1 and 16 cameras at radius 0 and 1, with the relaxed-load pre-check and with a plain atomicMin on every
                               candidate, alternating; device events around N calls after a warm-up
    render_bench.py --ref      tests/render_ref.py (numpy, np.minimum.at) on the same cloud, one camera, radius 0 and 1: what the host would do
    render_bench.py --profile  three calls per setting and nothing else, to run under `rocprofv3 --kernel-trace --stats -d DIR -- python ...`

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import cloud_ref
import voxel_ref
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_point_cloud, default_colors, render_cloud, orbit_cameras

V, H, W = 50, 384, 512
SHAPE, FOCAL = (H, W), 0.55 * W
N = 10
t0 = time.perf_counter()
scene = voxel_ref.overlapping_scene([SHAPE] * V, seed=4)
x, im, pan, info, cams = scene[:5]
thr = float(min(v['conf'].min() for v in x))
colors = default_colors(len(info) + 1)
turntable = orbit_cameras((5.0, 5.0, 2.2), 3.0, 16, 1.5)
out = {'workload': 'render_cloud: %d views of %dx%d, every point kept, rendered at %dx%d' % (V, H, W, H, W), 'scene_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    import render_ref
    rc = cloud_ref.cloud(x, im, pan, info, cams, min_conf_thr=thr, colors=colors)
    out['points'] = len(rc['index'])
    for radius in (0, 1):
        t0 = time.perf_counter()
        r = render_ref.render(rc['points'], rc['rgb'], rc['colors'], rc['pan'], turntable[:1], FOCAL, SHAPE, radius=radius)
        out['render_ref_1cam_r%d_s' % radius] = round(time.perf_counter() - t0, 2)
        out['hit_share_r%d' % radius] = round(float((r['index'] >= 0).mean()), 4)
        out['candidates_r%d' % radius] = int(r['candidates'].sum())
    print(json.dumps(out))
    sys.exit(0)

dev = 'cuda:0'
xd = [{k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in x]
cloud = panoptic_point_cloud(xd, [torch.from_numpy(i).to(dev) for i in im], None, [torch.from_numpy(p).to(dev) for p in pan], info,
                             [torch.from_numpy(c) for c in cams], min_conf_thr=thr, colors=colors)
out['points'] = len(cloud)
settings = [(B, radius, pre) for B in (1, 16) for radius in (0, 1) for pre in (1, 0)]


def run(B, radius, pre, n):
    hip.RENDER_PRECHECK = pre
    for _ in range(n):
        r = render_cloud(cloud, turntable[:B], FOCAL, SHAPE, radius=radius)
    return r


if '--profile' in sys.argv:
    for B, radius, pre in settings:
        run(B, radius, pre, 3)
    torch.cuda.synchronize()
    out['calls_per_setting'], out['settings'] = 3, settings
    print(json.dumps(out))
    sys.exit(0)

for s in settings:
    run(*s, 2)                                                                # warm-up of every shape
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for B, radius, pre in settings:                                           # pre-check on / off next to each other
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = run(B, radius, pre, N)
        b.record()
        torch.cuda.synchronize()
        out.setdefault('ms_B%d_r%d_%s' % (B, radius, 'precheck' if pre else 'plain'), []).append(round(a.elapsed_time(b) / N, 4))
    out['hit_share_B%d' % B] = round(float(r.hit.float().mean()), 4)
print(json.dumps(out))
