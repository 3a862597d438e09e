#!/usr/bin/env python
"""Time the GPU mesh rasteriser (panst3r_amd.engine.render_mesh) on a room of about a million faces at 384x512: the generated scene of tests/mesh_ref.py
with its walls tessellated 360 x 360 (1.04 M faces, most of them a pixel or less, plus the coarse ceiling and the two floor triangles that take the
one-wave-per-face path), from cameras of a turntable inside the room.

    mesh_bench.py            render_mesh with vertex ids for 1 and 16 cameras, with the relaxed-load pre-check and with a plain atomicMin on every sample,
                             and with the list of large faces switched off (everything in the lane path), alternating; device events around N calls
    mesh_bench.py --ref      tests/mesh_ref.py (numpy) on the same mesh, one camera: what the host would do
    mesh_bench.py --profile  three calls per setting and nothing else, to run under `rocprofv3 --kernel-trace --stats -d DIR -- python ...`

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import mesh_ref
from panst3r_amd import hip
from panst3r_amd.engine import render_mesh, orbit_cameras

H, W = 384, 512
SHAPE, FOCAL = (H, W), 0.5 * W
N = 10
t0 = time.perf_counter()
scene = mesh_ref.scene(n_wall=360)
turntable = orbit_cameras((0.0, 0.0, 1.0), 1.5, 16, 0.3, up=(0, -1, 0))      # the room's frame has y pointing down
out = {'workload': 'render_mesh: %d faces, %d vertices, rendered at %dx%d' % (len(scene['faces']), len(scene['vertices']), H, W),
       'scene_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    t0 = time.perf_counter()
    r = mesh_ref.render(scene['vertices'], scene['faces'], turntable[:1], FOCAL, SHAPE, vertex_ids=scene['vertex_ids'])
    out['mesh_ref_1cam_s'] = round(time.perf_counter() - t0, 2)
    out['hit_share'] = round(float((r['face'] >= 0).mean()), 4)
    out['samples'] = int(r['candidates'].sum())
    out['faces_rasterised'], out['faces_above_lane_pixels'] = int((r['box'] > 0).sum()), int((r['box'] > hip.MESH_LANE_PIXELS).sum())
    print(json.dumps(out))
    sys.exit(0)

dev = 'cuda:0'
verts, faces, vid = (torch.from_numpy(np.ascontiguousarray(scene[k])).to(dev) for k in ('vertices', 'faces', 'vertex_ids'))
faces = torch.where((faces < 0) | (faces >= len(verts)), torch.full_like(faces, -1), faces).to(torch.int32)
CAP = hip.MESH_BIG_CAPACITY
settings = [(B, pre, cap) for B in (1, 16) for pre, cap in ((1, CAP), (0, CAP), (1, 0))]


def run(B, pre, cap, n):
    hip.MESH_PRECHECK, hip.MESH_BIG_CAPACITY = pre, cap
    for _ in range(n):
        r = render_mesh(verts, faces, turntable[:B], FOCAL, SHAPE, vertex_ids=vid)
    return r


if '--profile' in sys.argv:
    for s in settings:
        run(*s, 3)
    torch.cuda.synchronize()
    out['calls_per_setting'], out['settings'] = 3, settings
    print(json.dumps(out))
    sys.exit(0)

for s in settings:
    run(*s, 2)                                                                # warm-up of every shape
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for B, pre, cap in settings:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = run(B, pre, cap, N)
        b.record()
        torch.cuda.synchronize()
        out.setdefault('ms_B%d_%s_%s' % (B, 'precheck' if pre else 'plain', 'two_paths' if cap else 'lane_only'), []).append(round(a.elapsed_time(b) / N, 4))
    out['hit_share_B%d' % B] = round(float(r.hit.float().mean()), 4)
print(json.dumps(out))
