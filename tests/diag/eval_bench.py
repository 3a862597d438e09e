#!/usr/bin/env python
"""Time the GPU panoptic evaluation (panst3r_amd.engine.panoptic_quality) on the full-size case of tests/test_hip_eval.py: 50 views of 384x512 (9.8 M
pixels) in three variants - `coherent`: the noisy maps of voxel_ref.overlapping_scene against its clean ones; `incoherent`: eval_ref.random_segments
with coherent=False, independent labels per pixel (P = 200, G = 300); `one_pair`: every pixel the same (p, g) pair.

    eval_bench.py VARIANT        both scopes, hip.EVAL_MERGE 1 and 0 alternating: pst_pq_count alone, pst_pq_match alone and the whole panoptic_quality call
                                 with its host sync; device events around N calls after a warm-up (the whole call: wall clock), the series twice
    eval_bench.py VARIANT --ref  tests/eval_ref.py (numpy, np.bincount) on the same maps, both scopes: what the host would do

Each prints one JSON line.  Every mode is one process: on a shared GPU box run each under its own `timeout -k 10 SECONDS`, chained with `&&`."""
import sys, os, json, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import eval_ref
import voxel_ref
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_quality

V, H, W = 50, 384, 512
N = 10
variant = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith('-') else 'coherent'
t0 = time.perf_counter()
if variant == 'coherent':
    x, im, pred, info, cams, gt = voxel_ref.overlapping_scene([(H, W)] * V, seed=4)
    gseg = info
elif variant == 'incoherent':
    pred, info, gt, gseg = eval_ref.random_segments([(H, W)] * V, 200, 300, seed=4, coherent=False)
elif variant == 'one_pair':
    pred, gt = [np.full((H, W), 9, dtype=np.int32)] * V, [np.full((H, W), 2, dtype=np.int32)] * V
    info, gseg = [{'id': 4, 'category_id': 1}, {'id': 9, 'category_id': 3}], [{'id': 2, 'category_id': 3}]
else:
    sys.exit('unknown variant %r (coherent | incoherent | one_pair)' % variant)
out = {'workload': 'panoptic_quality: %d views of %dx%d, %s, P=%d G=%d' % (V, H, W, variant, len(info), len(gseg)), 'pixels': V * H * W,
       'scene_s': round(time.perf_counter() - t0, 1)}

if '--ref' in sys.argv:
    for scope in ('scene', 'view'):
        for rep in range(2):
            t0 = time.perf_counter()
            r = eval_ref.panoptic_quality(pred, info, gt, gseg, scope=scope)
            out.setdefault('eval_ref_%s_s' % scope, []).append(round(time.perf_counter() - t0, 3))
        out['pq_%s' % scope] = r['pq']
    print(json.dumps(out))
    sys.exit(0)

dev = 'cuda:0'
pd, gd = [torch.from_numpy(m).to(dev) for m in pred], [torch.from_numpy(m).to(dev) for m in gt]
flat_p, flat_g = torch.cat([m.reshape(-1) for m in pd]), torch.cat([m.reshape(-1) for m in gd])
P, G = len(info), len(gseg)
tab = lambda segs: eval_ref.id_table(segs)
(tp, cp), (tg, cg) = tab(info), tab(gseg)
tp, cp, tg, cg = (torch.from_numpy(a).to(dev) for a in (tp, cp, tg, cg))
i32 = dict(dtype=torch.int32, device=dev)


def kernels(scope, merge):
    """the operands of the two entry points, as panoptic_quality builds them"""
    S = 1 if scope == 'scene' else V
    off = torch.arange(0, S + 1, dtype=torch.int64, device=dev) * (V * H * W // S)
    counts = torch.zeros(S, P + 1, G + 1, **i32)
    rest = (torch.empty(S, P, **i32), torch.empty(S, G, **i32), torch.empty(S, G, **i32), torch.empty(S, G, dtype=torch.float64, device=dev), torch.empty(S, P, **i32))
    return (lambda: hip.pq_count(flat_p, flat_g, off, tp, tg, P, G, counts, merge=merge)), (lambda: hip.pq_match(counts, cp, cg, *rest))


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / n, 4)


settings = [(scope, merge) for scope in ('scene', 'view') for merge in (1, 0)]
for scope, merge in settings:                                                 # warm-up of every shape
    hip.EVAL_MERGE = merge
    r = panoptic_quality(pd, info, gd, gseg, scope=scope)
    out['pq_%s' % scope] = r['pq']
torch.cuda.synchronize()
for rep in range(2):                                                          # the whole series twice: the spread between the two is the noise
    for scope, merge in settings:                                             # merge on / off next to each other
        tag = '%s_%s' % (scope, 'merge' if merge else 'plain')
        count, match = kernels(scope, merge)
        count(); match()
        out.setdefault('ms_count_' + tag, []).append(timed(count, N))
        out.setdefault('ms_match_' + tag, []).append(timed(match, N))
        hip.EVAL_MERGE = merge
        t0 = time.perf_counter()
        for _ in range(N):
            panoptic_quality(pd, info, gd, gseg, scope=scope)
        out.setdefault('ms_call_' + tag, []).append(round((time.perf_counter() - t0) * 1e3 / N, 3))
print(json.dumps(out))
