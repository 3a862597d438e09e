#!/usr/bin/env python
"""Time the connected components of the voxel cloud and the label despeckling (panst3r_amd.engine.voxel_components / clean_voxel_labels).

    vcc_bench.py CASE        CASE = scene05 | scene02: the 50-view 384x512 voxel_ref.overlapping_scene (seed 4, every pixel kept) fused at voxel 0.05 /
                             0.02; solid: a solid 128^3 block of one id, built by hand.  hip.VCC_MERGE 1 and 0 alternating: every entry point alone,
                             and the whole components() / clean_labels(4) call with its host sync; device events around N calls after a warm-up (the
                             whole calls: wall clock), the series twice
    vcc_bench.py CASE --ref  tests/vcc_ref.py (numpy) on the same voxels, on this machine's host: what the host would do

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import vcc_ref
import voxel_ref
from panst3r_amd import hip
from panst3r_amd.engine import VoxelCloud, default_colors, panoptic_point_cloud

V, H, W = 50, 384, 512
N = 10
CONN, MIN_VOXELS = 26, 4
case = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('-') else 'scene05'
dev = 'cuda:0'
t0 = time.perf_counter()
if case in ('scene05', 'scene02'):
    vs = {'scene05': 0.05, 'scene02': 0.02}[case]
    x, im, pan, info, cams, clean = voxel_ref.overlapping_scene([(H, W)] * V, seed=4)
    xd = [{k: torch.from_numpy(v).to(dev) for k, v in d.items()} for d in x]
    cloud = panoptic_point_cloud(xd, [torch.from_numpy(i).to(dev) for i in im], None, [torch.from_numpy(p).to(dev) for p in pan], info,
                                 [torch.from_numpy(c) for c in cams], min_conf_thr=0.0, colors=default_colors(len(info) + 1))
    vox = cloud.voxelize(vs)
    del xd, cloud
elif case == 'solid':
    a = np.arange(128, dtype=np.int32)
    cells = np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3)
    n = len(cells)
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    rgb, one = t(np.full((n, 3), 0.25, dtype=np.float32)), t(np.ones(n, dtype=np.int32))
    vox = VoxelCloud(t(cells.astype(np.float32)), rgb, t(np.full(n, 2, dtype=np.int32)), rgb, one, one, t(np.arange(n, dtype=np.int64)),
                     t(np.arange(n, dtype=np.int32)), [], None, [0, n], 1.0, 0, opacity=0.5, cells=t(cells))
else:
    sys.exit('unknown case %r (scene05 | scene02 | solid)' % case)
Mv = len(vox)
out = {'workload': 'voxel components: %s, connectivity %d, min_voxels %d' % (case, CONN, MIN_VOXELS), 'voxels': Mv, 'setup_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    cells, pan, count = vox.cells.cpu().numpy(), vox.pan.cpu().numpy(), vox.count.cpu().numpy()
    for rep in range(2):
        t0 = time.perf_counter()
        ref = vcc_ref.components(cells, pan, count, CONN)
        out.setdefault('vcc_ref_components_s', []).append(round(time.perf_counter() - t0, 3))
        t0 = time.perf_counter()
        vcc_ref.clean_pan(cells, pan, count, MIN_VOXELS, CONN, comp=ref)
        out.setdefault('vcc_ref_clean_s', []).append(round(time.perf_counter() - t0, 3))
    out['components'] = len(ref['size'])
    print(json.dumps(out))
    sys.exit(0)

cells, pan, count = vox.cells.contiguous(), vox.pan.contiguous(), vox.count.contiguous()
rgb, ctab = vox.rgb.contiguous(), torch.as_tensor(default_colors(16), dtype=torch.float32).to(dev)
nwg = (Mv + hip.CLOUD_WG - 1) // hip.CLOUD_WG
i32 = dict(dtype=torch.int32, device=dev)
pairs = hip.vcc_pair_capacity(Mv, len(vox.segments) or 26)


def timed(fn, n, setup=None):
    """ms per call of fn, device events around each call (setup, untimed, restores the state fn consumes)"""
    tot = 0.0
    for _ in range(n):
        if setup:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        tot += a.elapsed_time(b)
    return round(tot / n, 4)


def kernels(merge):
    """every entry point alone, on the state its predecessors left: {name: ms}"""
    st = {}
    counts, base, component = torch.empty(nwg, **i32), torch.empty(nwg + 1, **i32), torch.empty(Mv, **i32)
    table = {'root': torch.empty(Mv, **i32), 'pan': torch.empty(Mv, **i32), 'size': torch.empty(Mv, **i32), 'points': torch.empty(Mv, dtype=torch.int64, device=dev),
             'cell_lo': torch.empty(Mv, 3, **i32), 'cell_hi': torch.empty(Mv, 3, **i32)}
    out_pan, out_colors = torch.empty(Mv, **i32), torch.empty(Mv, 3, dtype=torch.float32, device=dev)

    def fresh():
        st['ws'] = hip.vcc_workspace(Mv, dev, pairs)

    def built():
        fresh(); hip.vcc_build(cells, pan, st['ws'])

    def linked():
        built(); hip.vcc_link(cells, pan, CONN, st['ws'])

    def flat():
        linked(); hip.vcc_flatten(count, cells, st['ws'], merge)

    def voted():
        flat(); hip.vcc_votes(cells, pan, CONN, MIN_VOXELS, st['ws'])

    ms = {}
    ms['workspace'] = timed(fresh, N)
    ms['build'] = timed(lambda: hip.vcc_build(cells, pan, st['ws']), N, fresh)
    ms['link'] = timed(lambda: hip.vcc_link(cells, pan, CONN, st['ws']), N, built)
    ms['flatten'] = timed(lambda: hip.vcc_flatten(count, cells, st['ws'], merge), N, linked)
    flat()
    ms['count'] = timed(lambda: hip.vcc_count(st['ws'], counts), N)
    hip.cloud_scan(counts, base)
    ms['rank'] = timed(lambda: hip.vcc_rank(pan, st['ws'], base, component, table), N)
    ms['votes'] = timed(lambda: hip.vcc_votes(cells, pan, CONN, MIN_VOXELS, st['ws']), N, flat)
    ws = st['ws']
    vote = lambda: hip.voxel_vote({'cap': ws['pair_cap'], 'pair_keys': ws['pair_keys'], 'pair_cnt': ws['pair_cnt'], 'best': ws['best']})
    ms['vote'] = timed(vote, N)
    ms['apply'] = timed(lambda: hip.vcc_apply(pan, MIN_VOXELS, rgb, ctab, 0.5, 0.5, ws, out_pan, out_colors), N)
    return ms


for merge in (1, 0):                                                          # warm-up of both settings
    hip.VCC_MERGE = merge
    comps, cleaned = vox.components(CONN), vox.clean_labels(MIN_VOXELS, CONN)
out.update(components=len(comps), relabelled=cleaned.relabelled, floaters=cleaned.floaters, pair_capacity=pairs)
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for merge in (1, 0):                                                      # merge on / off next to each other
        tag = 'merge' if merge else 'plain'
        for k, v in kernels(merge).items():
            out.setdefault('ms_%s_%s' % (k, tag), []).append(v)
        hip.VCC_MERGE = merge
        for name, fn in (('components', lambda: vox.components(CONN)), ('clean_labels', lambda: vox.clean_labels(MIN_VOXELS, CONN))):
            t0 = time.perf_counter()
            for _ in range(N):
                fn()
            out.setdefault('ms_call_%s_%s' % (name, tag), []).append(round((time.perf_counter() - t0) * 1e3 / N, 3))
print(json.dumps(out))
