#!/usr/bin/env python
"""Time the mesh shading stage (f17) on the room of tests/diag/mesh_bench.py: the generated scene of tests/mesh_ref.py with its walls tessellated 360 x 360
(1.04 M faces), 16 turntable cameras of 384 x 512.

    shade_bench.py           engine.vertex_normals of the million-face mesh; colour and smooth shade (C = 3, one launch) over the face maps of the 16 cameras
                             - the engine call (camera table built and uploaded, outputs allocated) and hip.mesh_interp alone (pst_mesh_interp and its
                             operand checks) - next to render_mesh for the same cameras; device events around N calls, the series twice
    shade_bench.py --ref     tests/mesh_shade_ref.py (numpy) on the same mesh: normals(), and interp() for ONE camera's face map (from tests/mesh_ref.py)

Each prints one JSON line.  No time is a pass condition.  Every mode is one process: on a shared GPU box run each under its own
`timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import mesh_ref
import mesh_shade_ref
from panst3r_amd import hip
from panst3r_amd.engine import render_mesh, orbit_cameras, vertex_normals, mesh_camera_table
from panst3r_amd.engine.shade import color_and_shade

H, W = 384, 512
SHAPE, FOCAL, NEAR = (H, W), 0.5 * W, 0.05
N = 10
t0 = time.perf_counter()
scene = mesh_ref.scene(n_wall=360)
turntable = orbit_cameras((0.0, 0.0, 1.0), 1.5, 16, 0.3, up=(0, -1, 0))      # the room's frame has y pointing down
colors = np.random.default_rng(0).uniform(0, 1, (len(scene['vertices']), 3)).astype(np.float32)
out = {'workload': 'shade: %d faces, %d vertices, 16 cameras at %dx%d, C = 3 + smooth shade' % (len(scene['faces']), len(scene['vertices']), H, W),
       'scene_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    t0 = time.perf_counter()
    nrm = mesh_shade_ref.normals(scene['vertices'], scene['faces'])
    out['ref_normals_s'] = round(time.perf_counter() - t0, 2)
    r = mesh_ref.render(scene['vertices'], scene['faces'], turntable[:1], FOCAL, SHAPE)
    tab = mesh_ref.camera_table(turntable[:1], FOCAL, SHAPE)
    t0 = time.perf_counter()
    got = mesh_shade_ref.interp(r['face'], scene['vertices'], scene['faces'], tab, NEAR, attr=colors, shade_mode=2, normals=nrm)
    out['ref_interp_1cam_s'] = round(time.perf_counter() - t0, 2)
    out['hit_share'] = round(float(got['hit'].mean()), 4)
    print(json.dumps(out))
    sys.exit(0)

dev = 'cuda:0'
verts, faces, col = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene['vertices'], scene['faces'], colors))
faces = torch.where((faces < 0) | (faces >= len(verts)), torch.full_like(faces, -1), faces).to(torch.int32)


def timed(fn, n=N):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r = fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 4), r


steps = {'vertex_normals': lambda: vertex_normals(verts, faces), 'render_mesh_B16': lambda: render_mesh(verts, faces, turntable, FOCAL, SHAPE, near=NEAR)}
for fn in steps.values():
    fn()                                                                      # warm-up
nrm, views = steps['vertex_normals'](), steps['render_mesh_B16']()
steps['color_and_shade_B16_C3_smooth'] = lambda: color_and_shade(views, verts, faces, turntable, FOCAL, col, normals=nrm, near=NEAR)
cams = torch.from_numpy(mesh_camera_table(turntable, FOCAL, SHAPE)).to(dev)
out_attr, out_shade = steps['color_and_shade_B16_C3_smooth']()
steps['hip_mesh_interp_B16_C3_smooth'] = lambda: hip.mesh_interp(views.face, verts, faces, cams, NEAR, attr=col, fill=0.0, out_attr=out_attr,
                                                                 shade_mode=hip.MESH_SHADE_SMOOTH, normals=nrm, out_shade=out_shade)
steps['hip_mesh_interp_B16_C3_smooth']()
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for name, fn in steps.items():
        out.setdefault('ms_' + name, []).append(timed(fn)[0])
out['hit_share'] = round(float(views.hit.float().mean()), 4)
out['unit_normals_share'] = round(float((nrm.norm(dim=1) > 0.5).float().mean()), 4)
print(json.dumps(out))
