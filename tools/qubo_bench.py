"""Time of the QUBO mask selection with the device solver (csrc/qubo_solve.hip) next to the host annealer.

    python tools/qubo_bench.py [--views 50] [--launches 20] [--no-host] [--out FILE.json]

1. kernel: HIP-event time of `qubo_anneal` (anneal + winner kernels) at N = 200, the default replicas, 10 000 moves on a fixture matrix of
   tests/golden/qubo_solver.npz, median and spread over --launches launches after warm-up, and the ns per move per replica it implies
   (launch time x CUs-worth of waves is NOT divided out: it is wall time / (moves x replicas)).  W is LDS-resident; no L2 variant is built.
2. whole call: wall time of `panoptic_inference_qubo` for a synthetic scene of --views views of 384 x 512 with 200 queries (mask logits at 96 x 128),
   solver='device' and solver='host', and of the host annealing step alone on the same weight matrix, in the same run.
3. what the device call consists of: weights (up-sampling + overlap sums + finalisation), annealing, and the rest (arg-max, bincounts, bookkeeping):
   medians of three repetitions each, the rest as the difference of the medians.
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

from panst3r_amd import hip                                                                                   # noqa: E402
from panst3r_amd.engine import postprocess as PP                                                              # noqa: E402

DEV = 'cuda:0'


def scene(V, Q=200, h=96, w=128, nobj=40, seed=0):
    """mask logits [1, Q, h, w] per view: nobj boxes, each claimed by several jittered queries; class logits [1, Q, 8]"""
    g = np.random.Generator(np.random.PCG64(seed))
    boxes = [(g.uniform(0, h), g.uniform(0, w), g.integers(8, 24), g.integers(8, 28)) for _ in range(nobj)]
    owner = np.concatenate([np.arange(nobj), g.integers(0, nobj, Q - nobj)])
    masks = []
    for v in range(V):
        m = np.full((Q, h, w), -8.0, dtype=np.float32)
        for q in range(Q):
            cy, cx, hh, ww = boxes[owner[q]]
            y0, x0 = int(cy - hh / 2 + g.normal(0, 2)), int(cx - ww / 2 + g.normal(0, 2))
            m[q, max(y0, 0):max(y0 + hh, 0), max(x0, 0):max(x0 + ww, 0)] = g.uniform(1.0, 5.0)
        masks.append(torch.from_numpy(m)[None].to(DEV))
    return torch.from_numpy(g.standard_normal((1, Q, 8)).astype(np.float32)), masks


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=50)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'device': torch.cuda.get_device_name(0), 'replicas': PP.QUBO_REPLICAS, 'num_iters': 10000, 'N': 200}

    W = np.load(os.path.join(ROOT, 'tests', 'golden', 'qubo_solver.npz'))['Wneg.0']
    Wd = torch.from_numpy(W).to(DEV)
    R = PP.QUBO_REPLICAS
    out = (torch.empty(R, 200, dtype=torch.uint8, device=DEV), torch.empty(R, device=DEV), torch.empty(200, dtype=torch.uint8, device=DEV), torch.empty(1, device=DEV))
    run = lambda: hip.qubo_anneal(Wd, R, 10000, 0.5, 1e-4, 1e-3, 0, *out)
    for _ in range(3):
        run()
    ms = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res['kernel_ms'] = {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'launches': a.launches, 'variant': 'LDS-resident W'}
    res['ns_per_move_per_replica'] = float(np.median(ms)) * 1e6 / (10000 * R)
    print('qubo_anneal N=200 replicas=%d moves=10000: %.3f ms (min %.3f, max %.3f) = %.4f ns per move per replica' %
          (R, res['kernel_ms']['median'], res['kernel_ms']['min'], res['kernel_ms']['max'], res['ns_per_move_per_replica']), flush=True)

    H, Wd_ = 384, 512
    logits, masks = scene(a.views)
    size = np.array([[H, Wd_]] * a.views)
    call = lambda **kw: PP.panoptic_inference_qubo(logits, masks, size, device=DEV, silent=True, multi_ar=True, **kw)
    call(solver='device')                                                                                     # warm
    t_dev = [wall(lambda: call(solver='device'))[0] for _ in range(3)]
    views = [m[0].contiguous() for m in masks]
    shapes = [(H, Wd_)] * a.views
    tw, ta = [], []
    for _ in range(3):                                                    # the same three repetitions as the whole call: medians throughout
        t, Wq = wall(lambda: PP.qubo_weights_device(views, shapes, torch.device(DEV)))
        tw.append(t)
        t, _ = wall(lambda: PP.solve_qubo_device(Wq, energy=False))
        ta.append(t)
    t_w, t_a = float(np.median(tw)), float(np.median(ta))
    sol = PP.solve_qubo_device(Wq)
    res['scene'] = {'views': a.views, 'shape': [H, Wd_], 'queries': 200, 'selected_device': int(sol[0].sum()), 'energy_device': sol[1]}
    res['device_call_s'] = {'runs': t_dev, 'median': float(np.median(t_dev)), 'weights': t_w, 'weights_runs': tw, 'anneal_incl_transfers': t_a, 'anneal_runs': ta,
                            'rest_argmax_bincount_bookkeeping': float(np.median(t_dev)) - t_w - t_a}
    print('solver=device: whole call %.3f s = weights %.3f + anneal %.4f + rest %.3f' % (np.median(t_dev), t_w, t_a, np.median(t_dev) - t_w - t_a), flush=True)
    if not a.no_host:
        Wh = Wq.cpu().numpy()
        np.random.seed(0)
        t0 = time.perf_counter()
        hs, he = PP.solve_qubo_simulated_annealing(Wh, silent=True)
        t_ha = time.perf_counter() - t0
        np.random.seed(0)
        t_host = wall(lambda: call(solver='host'))[0]
        res['host_s'] = {'anneal_alone': t_ha, 'whole_call': t_host, 'selected': int(np.sum(hs)), 'energy': float(he)}
        res['whole_device_call_over_host_anneal_alone'] = float(np.median(t_dev)) / t_ha
        print('solver=host: whole call %.2f s, annealing alone %.2f s (energy %.6f; device %.6f); device call / host annealing = %.4f' %
              (t_host, t_ha, he, sol[1], res['whole_device_call_over_host_anneal_alone']), flush=True)
        assert float(np.median(t_dev)) < t_ha, 'the whole device-solver call must take less wall time than the host annealing step alone'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
