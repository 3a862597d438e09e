"""Generates tests/golden/qubo_solver.npz: the yardstick of the device QUBO solver (csrc/qubo_solve.hip, restated in tests/qubo_ref.py).

Run:  python tests/golden/make_qubo_solver_golden.py          (needs the reference tree, as make_golden.py does; never runs on the GPU box)

Three 200 x 200 `Wneg` matrices from the reference's `weight_from_masks` on synthetic multi-view masks, and for each the reference annealer's
(solution, energy) at its defaults (redo=20) for np.random.seed(0..4), with the wall time of every run as recorded information.  The masks are the
regime QUBO exists for: ~40 objects (boxes that partly overlap their neighbours), each claimed by several queries that are jittered copies of it
with their own confidence, plus a few queries that claim nearly nothing.  Nothing here is computed by this project's code.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

Q, V, H, W = 200, 4, 48, 64
N_OBJ = 40


def synthetic_masks(seed):
    """[Q, V, H, W] float32 mask probabilities"""
    g = np.random.Generator(np.random.PCG64(seed))
    boxes = []                                                     # per object and view: y0, y1, x0, x1
    for _ in range(N_OBJ):
        hh, ww = int(g.integers(4, 12)), int(g.integers(4, 14))
        cy, cx = g.uniform(0, H), g.uniform(0, W)
        per_view = []
        for _v in range(V):
            y, x = cy + g.normal(0, 3), cx + g.normal(0, 3)        # the object moves a little between views
            per_view.append((y - hh / 2, y + hh / 2, x - ww / 2, x + ww / 2))
        boxes.append(per_view)
    owner = np.concatenate([np.arange(N_OBJ), g.integers(0, N_OBJ, Q - N_OBJ - 10), np.full(10, -1)])      # every object claimed at least once; 10 empty queries
    g.shuffle(owner)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64) + 0.5
    masks = np.empty((Q, V, H, W), dtype=np.float32)
    for q in range(Q):
        masks[q] = g.uniform(0.0, 0.001, (V, H, W))
        if owner[q] < 0:
            continue
        peak = g.uniform(0.55, 0.98)
        jit = g.normal(0, 1.5, (V, 4))
        for v in range(V):
            y0, y1, x0, x1 = np.asarray(boxes[owner[q]][v]) + jit[v]
            # soft box: a product of two smooth steps, one pixel wide edges
            sy = 1 / (1 + np.exp(-(yy - y0) * 2)) * 1 / (1 + np.exp((yy - y1) * 2))
            sx = 1 / (1 + np.exp(-(xx - x0) * 2)) * 1 / (1 + np.exp((xx - x1) * 2))
            masks[q, v] = np.maximum(masks[q, v], (peak * sy * sx).astype(np.float32))
    return torch.from_numpy(masks)


def main():
    from make_golden import import_reference
    PP = import_reference()['postprocess']
    out = {}
    for m, seed in enumerate((7101, 7102, 7103)):
        masks = synthetic_masks(seed)
        cls_probs = torch.full((Q, 3), 0.5)
        _, Wneg = PP.weight_from_masks(masks.clone(), cls_probs, silent=True)
        Wneg = np.ascontiguousarray(Wneg, dtype=np.float32)
        assert Wneg.shape == (Q, Q)
        sols, ens, secs = [], [], []
        for s in range(5):
            np.random.seed(s)
            t0 = time.perf_counter()
            sol, en = PP.solve_qubo_simulated_annealing(Wneg, silent=True)
            secs.append(time.perf_counter() - t0)
            sols.append(np.asarray(sol, dtype=np.uint8))
            ens.append(float(en))
            print('matrix %d seed %d: energy %.6f, %d selected, %.1f s' % (m, s, en, int(sol.sum()), secs[-1]), flush=True)
        out['Wneg.%d' % m] = Wneg
        out['solution.%d' % m] = np.stack(sols)
        out['energy.%d' % m] = np.asarray(ens, dtype=np.float64)
        out['seconds.%d' % m] = np.asarray(secs, dtype=np.float64)
    path = os.path.join(HERE, 'qubo_solver.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
