"""The device QUBO solver (csrc/qubo_solve.hip, engine.solve_qubo_device, panoptic_inference_qubo(solver='device')) on the GPU.

The kernel against the numpy restatement of tests/qubo_ref.py: every replica's state and energy, the winner's state and energy, BIT FOR BIT - the
contract is integer work and separately rounded fp32 operations, so there is no tolerance to choose.  Quality against brute force and against the
reference annealer's own recorded runs (tests/golden/qubo_solver.npz), with the bars of tests/test_qubo_solver_host.py.  End to end against the
reference-generated goldens under the comparisons tests/test_hip_postprocess.py applies to the host solver."""
import os

import numpy as np
import pytest
import torch

import qubo_ref as R
import tiny
from panst3r_amd import hip
from panst3r_amd import ops  # noqa: F401  (registers torch.ops.panst3r_hip.*)
from panst3r_amd.engine.postprocess import (QUBO_REPLICAS, panoptic_inference_qubo, qubo_weights, qubo_weights_device, solve_qubo_device)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def problem(N, seed=5):
    """a seeded N-variable problem of the product's kind; the first fixture matrix for N = 200, a committed golden for N = 12"""
    if N == 200:
        return np.load(os.path.join(GOLDEN, 'qubo_solver.npz'))['Wneg.0']
    if N == 12:
        return np.load(os.path.join(GOLDEN, 'postprocess_qubo.npz'))['Wneg']
    g = np.random.Generator(np.random.PCG64(seed + N))
    A = g.uniform(0, 0.05, (N, N)) * (g.uniform(0, 1, (N, N)) < 0.3)
    W = (A + A.T) / 2
    np.fill_diagonal(W, -g.uniform(0.01, 0.06, N))
    return W.astype(F)


def launch(W, replicas, num_iters, seed, fn=None, **kw):
    Wd = torch.from_numpy(W).to(DEV)
    N = W.shape[0]
    out = (torch.full((replicas, N), 7, dtype=torch.uint8, device=DEV), torch.full((replicas,), 7.0, device=DEV),
           torch.full((N,), 7, dtype=torch.uint8, device=DEV), torch.full((1,), 7.0, device=DEV))
    (fn or hip.qubo_anneal)(Wd, replicas, num_iters, kw.get('T0', 0.5), kw.get('T_end', 1e-4), kw.get('lambda_reg', 1e-3), seed, *out)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


# the whole cross product.  Waves per workgroup = ceil(replicas / 256) up to 16: 1, 5 and 64 replicas run one wave per workgroup, 999 and 1000 four
# (999 leaves the last workgroup with 3 of its 4 waves in use), 2990 twelve (the last workgroup holds 2 of 12), the default 4096 sixteen.  Only the
# full length samples replicas (8 of them), to keep the numpy side short; every other case compares every replica.
REPS = (1, 5, 64, 999, 1000, 2990, QUBO_REPLICAS)
ITERS = (0, 1, 257, 10000)
SEEDS = (0, 0x1234567887654321)


@pytest.mark.parametrize('N', [1, 2, 12, 63, 64, 65, 127, 200])
def test_kernel_equals_the_restatement_bit_for_bit(N):
    W = problem(N)
    for seed in SEEDS:
        for replicas in REPS:
            for iters in ITERS:
                sample = np.arange(replicas) if iters <= 257 or replicas <= 8 else np.unique(np.r_[0, replicas - 1, np.random.Generator(
                    np.random.PCG64(N)).integers(0, replicas, 6)])
                want_x, want_e = R.anneal(W, sample, num_iters=iters, seed=seed)
                for fn in (hip.qubo_anneal, torch.ops.panst3r_hip.qubo_anneal):
                    x_all, e_all, best_x, best_e = launch(W, replicas, iters, seed, fn)
                    what = (N, replicas, iters, seed)
                    assert np.array_equal(x_all[sample], want_x), what
                    assert np.array_equal(e_all[sample].view(np.uint32), want_e.view(np.uint32)), what
                    w = R.winner(x_all, e_all)                            # every replica took part: the winner rule on the kernel's own table
                    assert np.array_equal(best_x, x_all[w]) and best_e.view(np.uint32)[0] == e_all.view(np.uint32)[w], what
                    if len(sample) == replicas:
                        w2 = R.winner(want_x, want_e)
                        assert w == w2 and np.array_equal(best_x, want_x[w2]) and best_e.view(np.uint32)[0] == want_e.view(np.uint32)[w2], what
                    assert set(np.unique(x_all)) <= {0, 1}, what


def test_other_schedule_arguments_are_restated_too():
    W = problem(65)
    kw = dict(T0=0.25, T_end=1e-3, lambda_reg=0.02)
    x_all, e_all, _, _ = launch(W, 32, 500, 3, **kw)
    want_x, want_e = R.anneal(W, 32, num_iters=500, seed=3, **kw)
    assert np.array_equal(x_all, want_x) and np.array_equal(e_all.view(np.uint32), want_e.view(np.uint32))


def test_launches_repeat_seeds_differ_and_streams_work():
    W = problem(200)
    a = launch(W, 256, 2000, 0)
    b = launch(W, 256, 2000, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = launch(W, 256, 2000, 1)
    assert not np.array_equal(a[0], c[0])
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        d = launch(W, 256, 2000, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, d))


def test_a_refused_size_leaves_the_outputs_alone_and_names_the_host_solver():
    N = hip.qubo_anneal_max_n() + 1
    Wd = torch.zeros(N, N, device=DEV)
    out = (torch.full((4, N), 7, dtype=torch.uint8, device=DEV), torch.full((4,), 7.0, device=DEV), torch.full((N,), 7, dtype=torch.uint8, device=DEV),
           torch.full((1,), 7.0, device=DEV))
    with pytest.raises(RuntimeError, match="solver='host'"):
        hip.qubo_anneal(Wd, 4, 10, 0.5, 1e-4, 1e-3, 0, *out)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)
    with pytest.raises(RuntimeError, match="solver='host'"):
        solve_qubo_device(np.zeros((N, N), dtype=F), device=DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip.qubo_anneal(torch.zeros(4, 4), 1, 1, 0.5, 1e-4, 1e-3, 0, torch.zeros(1, 4, dtype=torch.uint8), torch.zeros(1), torch.zeros(4, dtype=torch.uint8),
                        torch.zeros(1))


@pytest.mark.parametrize('name', ['postprocess_qubo', 'postprocess_qubo_multiar'])
def test_device_solver_finds_the_global_optimum_of_the_tiny_goldens(name):
    W = np.load(os.path.join(GOLDEN, name + '.npz'))['Wneg']
    es, best = R.brute_force(W)
    x, e = solve_qubo_device(W, device=DEV)
    assert np.array_equal(x, best) and abs(e - es[0]) < 1e-12 and x.dtype.kind == 'i' and isinstance(e, float)
    x2, e2 = solve_qubo_device(torch.from_numpy(W).to(DEV), replicas=64)         # a device tensor; fewer replicas
    assert np.array_equal(x2, best) and e2 == e


def test_device_solver_finds_the_global_optimum_of_16_variable_problems():
    for seed in range(10):
        g = np.random.Generator(np.random.PCG64(1000 + seed))
        A = g.uniform(0, 0.05, (16, 16)) * (g.uniform(0, 1, (16, 16)) < 0.4)
        W = (A + A.T) / 2
        np.fill_diagonal(W, -g.uniform(0.01, 0.06, 16))
        W = W.astype(F)
        es, _ = R.brute_force(W)
        x, e = solve_qubo_device(W, replicas=64, device=DEV)
        assert e <= es[0] + 1e-9, (seed, e, es[0])


@pytest.mark.parametrize('m', range(3))
def test_device_solver_is_as_good_as_the_reference_on_200_variables(m):
    g = np.load(os.path.join(GOLDEN, 'qubo_solver.npz'))
    W, en = g['Wneg.%d' % m], g['energy.%d' % m]
    for seed, bar, what in ((0, en.min() + 1e-9, 'best'), (1, float(np.median(en)), 'median'), (2, float(np.median(en)), 'median')):
        x, e = solve_qubo_device(W, seed=seed, device=DEV)
        assert abs(e - R.energy64(x, W)) < 1e-12
        print('matrix %d seed %d: %.6f against the reference\'s %s %.6f' % (m, seed, e, what, bar))
        assert e <= bar, (m, seed, e, bar)


@pytest.mark.parametrize('tag', ['', '_multiar'])
def test_postprocess_qubo_device_solver_golden(golden, tag):
    """solver='device' selects the same queries as the reference's seeded run (the global optimum), so it reproduces the golden's maps and segments
    under the comparisons of test_hip_postprocess.py::test_postprocess_qubo_golden; the device-side weight matrix equals qubo_weights bit for bit;
    and solver='host' still returns what it returned before."""
    g = golden('postprocess_qubo' + tag)
    masks = [m.to(DEV) for m in g.lst('masks')]
    shapes = [tuple(int(v) for v in s) for s in g.z['size']]
    views = [m[0].contiguous() for m in masks]
    Wneg = qubo_weights(views, shapes, torch.device(DEV))
    Wdev = qubo_weights_device(views, shapes, torch.device(DEV))
    assert Wdev.dtype == torch.float32 and Wdev.is_cuda and np.array_equal(Wdev.cpu().numpy().view(np.uint32), Wneg.view(np.uint32))
    assert float(np.abs(Wneg - g.z['Wneg']).max()) < 1e-5 * float(np.abs(g.z['Wneg']).max())

    def check(res):
        assert [[d['id'], d['query_id'], int(d['category_id']), d['area']] for d in res['segments_info']] == g.z['info'].tolist()
        for d, (cp, mc) in zip(res['segments_info'], g.z['probs'].tolist()):
            assert abs(d['class_prob'] - cp) < 1e-6 and abs(d['mask_conf'] - mc) < 1e-5
        same = tot = 0
        for a, b, ca, cb in zip(res['pan'], g.lst('pan'), res['conf'], g.lst('conf')):
            eq = a.cpu() == b
            same += int(eq.sum()); tot += eq.numel()
            assert float((ca.cpu() - cb)[eq].abs().max()) < 1e-5
        assert same == tot, (same, tot)

    state = np.random.get_state()
    dev = panoptic_inference_qubo(g.t('logits'), masks, g.z['size'], device=DEV, num_redo=3, silent=True, multi_ar=True, solver='device')[0]
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(state, np.random.get_state()))      # np.random is not drawn from
    check(dev)
    np.random.seed(1234)
    host = panoptic_inference_qubo(g.t('logits'), masks, g.z['size'], device=DEV, num_redo=3, silent=True, multi_ar=True, solver='host')[0]
    check(host)
    np.random.seed(1234)
    plain = panoptic_inference_qubo(g.t('logits'), masks, g.z['size'], device=DEV, num_redo=3, silent=True, multi_ar=True)[0]       # the default is 'host'
    assert plain['segments_info'] == host['segments_info'] and all(torch.equal(a, b) for a, b in zip(plain['pan'], host['pan']))
    assert all(torch.equal(a, b) for a, b in zip(plain['conf'], host['conf']))
    few = panoptic_inference_qubo(g.t('logits'), masks, g.z['size'], device=DEV, multi_ar=True, solver='device', replicas=64, seed=5)[0]
    check(few)


def test_reconstruct_with_the_device_solver_equals_the_stages_called_by_hand():
    V, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    ppkw = dict(solver='device', replicas=256, seed=3, prob_threshold=0.0, device=DEV)
    cloud, cameras, pan_preds = h.reconstruct(imgs, ts, tiny.NAMES, postprocess='qubo', min_conf_thr=1.5, postprocess_kwargs=ppkw, num_keyframes=K, amp='fp16')
    pms, panout = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, amp='fp16')
    pp = panoptic_inference_qubo(panout['pred_logits'], panout['pred_masks'], ts, label_mode=h.panoptic_decoder.label_mode, multi_ar=True, **ppkw)
    strip = lambda info: [{k: (int(v) if k == 'category_id' else v) for k, v in d.items()} for d in info]
    assert strip(pan_preds[0]['segments_info']) == strip(pp[0]['segments_info']) and len(pp[0]['segments_info']) > 0
    assert all(torch.equal(a, b) for a, b in zip(pan_preds[0]['pan'], pp[0]['pan']))
    assert sorted(s['id'] for s in cloud.segments) == sorted(set(s['id'] for s in cloud.segments)) and len(cameras) == V
