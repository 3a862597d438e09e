"""Host side of the device QUBO solver (csrc/qubo_solve.hip): the C ABI, and the numpy restatement the GPU tests hold the kernel to
(tests/qubo_ref.py) - its generator, its exponential, the optima it must find, the reference's recorded runs it must match, and planted mistakes
it must not survive.  No GPU needed.

Yardsticks: brute-force enumeration in float64 (tiny problems) and tests/golden/qubo_solver.npz, the reference annealer's own five seeded runs at
its defaults on three 200 x 200 matrices (tests/golden/make_qubo_solver_golden.py).  Bars: seed 0 not above the reference's BEST recorded energy
(+1e-9 for the float64 re-evaluation), seeds 1 and 2 not above its median."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import abi_header
import qubo_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SYMBOLS = ['pst_qubo_anneal', 'pst_qubo_anneal_max_n']


def test_header_declares_and_library_exports_the_symbols():
    from panst3r_amd.build import build
    from panst3r_amd import hip
    declared = {p[0] for p in abi_header.prototypes()}
    lib = ctypes.CDLL(build(verbose=False))
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s) and s in hip.EXPORTS, s
    assert lib.pst_qubo_anneal_max_n() == R.NMAX == 200
    assert lib.pst_abi_version() == 20                                  # additive: the ABI version stays


def test_refused_arguments_name_the_host_solver_without_a_gpu():
    """argument checks come before any launch: N out of range is PST_EINVAL with a message that says what remains"""
    from panst3r_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.pst_last_error.restype = ctypes.c_char_p
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    args = lambda N, reps=4, it=10, T0=0.5: (one, N, reps, it, ctypes.c_float(T0), ctypes.c_float(1e-4), ctypes.c_float(1e-3), ctypes.c_uint64(0), one, one, one,
                                             one, None)
    for N in (0, -1, 201, 1000):
        assert lib.pst_qubo_anneal(*args(N)) == -1
        assert b"solver='host'" in lib.pst_last_error()
    assert lib.pst_qubo_anneal(*args(10, reps=0)) == -1 and lib.pst_qubo_anneal(*args(10, it=-1)) == -1 and lib.pst_qubo_anneal(*args(10, T0=0.0)) == -1


# ---------------------------------------------------------------------------------------------------- generator
# Philox4x32-10 known answers: (counter, key, output).  Rows 1 and 3 are the Random123 `kat_vectors` entries for philox4x32 10 (zeros; the digits of pi),
# recalled and reproduced by this implementation.  Row 2 (all ones) is "recalled, unverified": the third output word was recalled as a20bc7c9, the
# implementation that reproduces rows 1 and 3 gives a20bc7c6, and that is what is written.  No independent Philox4x32 callable from Python was found
# here (numpy's Philox is the 4x64 variant); the constants were compared with rocRAND's rocrand_philox4x32_10.h.
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('ctr,key,out', KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in R.philox4x32_10(*ctr, *key)) == out


def test_philox_is_elementwise_over_arrays():
    c0 = np.array([0, 0x243f6a88], dtype=np.uint32)
    w = R.philox4x32_10(c0, np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344]), 0, 0)
    assert tuple(int(v[0]) for v in w) == KAT[0][2]


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


# upper 0.1 % points of chi-square: 9 dof 27.877, 199 dof 267.54 (Wilson-Hilferty: 199 (1 - 2/(9*199) + 3.0902 sqrt(2/(9*199)))^3), 63 dof 103.44
@pytest.mark.parametrize('N,crit', [(10, 27.877), (200, 267.54)])
def test_move_index_is_uniform(N, crit):
    j, u = R.draws(0, np.arange(100)[None, :], np.arange(10000)[:, None], N)
    assert j.min() >= 0 and j.max() < N and u.dtype == F and u.min() >= 0 and u.max() < 1
    assert _chi2(np.bincount(j.ravel(), minlength=N), j.size / N) < crit
    assert _chi2(np.bincount((u.ravel() * 64).astype(np.int64), minlength=64), u.size / 64) < 103.44


def test_streams_of_replicas_seeds_and_moves_differ():
    mv = np.arange(2000)
    a, b, c = R.draws(0, 0, mv, 200), R.draws(0, 1, mv, 200), R.draws(1, 0, mv, 200)
    big = R.draws(1 << 40, 0, mv, 200)                                  # the high key word is used
    for other in (b, c, big):
        assert (a[0] != other[0]).mean() > 0.9 and (a[1] != other[1]).mean() > 0.9
    assert (a[1][0::2] != a[1][1::2]).mean() > 0.9                      # the two moves of one block use different words
    x = R.initial_x(0, np.arange(512), 200)
    assert x.shape == (512, 200) and 0.48 < x.mean() < 0.52 and len({r.tobytes() for r in x}) == 512
    assert not np.array_equal(x, R.initial_x(1, np.arange(512), 200))
    assert np.array_equal(R.initial_x(0, [7], 130)[0], x[7, :130])      # a prefix: the bit of variable k does not depend on N


# ---------------------------------------------------------------------------------------------------- exponential
def test_exp_neg_against_float64():
    a = -np.linspace(0.0, 87.0, 1000001).astype(F)
    e = R.exp_neg(a)
    ref = np.exp(a.astype(np.float64))
    rel = float(np.max(np.abs(e.astype(np.float64) - ref) / ref))
    print('exp_neg: max relative error on [-87, 0] = %.3e' % rel)
    assert e.dtype == F and rel < 1e-6
    assert np.all(np.diff(e) <= 0)                                      # monotone non-increasing on the dense sample
    tiny = -np.logspace(-45, 0, 100000).astype(F)
    assert float(np.max(np.abs(R.exp_neg(tiny) - np.exp(tiny.astype(np.float64))) / np.exp(tiny.astype(np.float64)))) < 1e-6
    edge = R.exp_neg(np.array([0.0, -0.0, -87.0, np.nextafter(F(-87.0), F(-100)), -88.0, -1e30, -np.inf, np.nan], dtype=F))
    assert edge[0] == 1.0 and edge[1] == 1.0 and edge[2] > 0 and np.isfinite(edge).all()
    assert edge[3:].tolist() == [0.0] * 5


# ---------------------------------------------------------------------------------------------------- optima
@pytest.mark.parametrize('name', ['postprocess_qubo', 'postprocess_qubo_multiar'])
def test_restatement_finds_the_global_optimum_of_the_tiny_goldens(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    W = g['Wneg']
    es, best = R.brute_force(W)
    assert es[1] - es[0] > 0.05                                         # a unique optimum with a clear gap ...
    assert np.array_equal(best, g['solution'].astype(np.uint8))         # ... which is what the reference's annealer stored
    x, e = R.anneal(W, 64)
    w = R.winner(x, e)
    assert np.array_equal(x[w], best) and abs(R.energy64(x[w], W) - es[0]) < 1e-12
    assert abs(float(e[w]) - es[0]) < 1e-6


def small_problem(seed, N=16):
    """a seeded N-variable problem of the product's kind: negative diagonal (areas), non-negative symmetric off-diagonal (overlaps)"""
    g = np.random.Generator(np.random.PCG64(seed))
    A = g.uniform(0, 0.05, (N, N)) * (g.uniform(0, 1, (N, N)) < 0.4)
    W = (A + A.T) / 2
    np.fill_diagonal(W, -g.uniform(0.01, 0.06, N))
    return W.astype(F)


@pytest.mark.parametrize('seed', range(10))
def test_restatement_finds_the_global_optimum_of_16_variable_problems(seed):
    W = small_problem(1000 + seed)
    es, best = R.brute_force(W)
    x, e, bE, E, xc = R.anneal(W, 64, return_tracked=True)
    w = R.winner(x, e)
    assert R.energy64(x[w], W) <= es[0] + 1e-9, (R.energy64(x[w], W), es[0])
    # the incrementally tracked energies agree with a recomputation: the final state's, and the best state's
    assert np.max(np.abs(E.astype(np.float64) - [R.energy64(v, W) for v in xc])) < 1e-5
    assert np.max(np.abs(bE - e)) < 1e-5


@pytest.mark.parametrize('variant', ['lambda_sign', 'no_diag', 'accept_gt'])
def test_planted_mistakes_fail(variant):
    """each mistake loses to the brute-force optimum or to the incremental-against-recomputed energy check on the 16-variable problems (8 replicas of
    2000 moves: a budget under which a walk that accepts the wrong moves does not stumble over all 65 536 states)."""
    lost = 0
    for seed in range(10):
        W = small_problem(1000 + seed)
        es, _ = R.brute_force(W)
        x, e, bE, E, xc = R.anneal(W, 8, num_iters=2000, variant=variant, return_tracked=True)
        w = R.winner(x, e)
        drift = np.max(np.abs(E.astype(np.float64) - [R.energy64(v, W) for v in xc]))
        lost += (R.energy64(x[w], W) > es[0] + 1e-9) or drift > 1e-5
    assert lost >= 1, variant
    good = 0                                                            # ... and the unplanted code passes the very same checks
    for seed in range(10):
        W = small_problem(1000 + seed)
        es, _ = R.brute_force(W)
        x, e, bE, E, xc = R.anneal(W, 8, num_iters=2000, return_tracked=True)
        w = R.winner(x, e)
        drift = np.max(np.abs(E.astype(np.float64) - [R.energy64(v, W) for v in xc]))
        good += (R.energy64(x[w], W) <= es[0] + 1e-9) and drift <= 1e-5
    assert good == 10


# ---------------------------------------------------------------------------------------------------- against the reference's recorded runs
def test_fixture_holds_the_reference_runs():
    g = np.load(os.path.join(GOLDEN, 'qubo_solver.npz'))
    for m in range(3):
        W, sol, en = g['Wneg.%d' % m], g['solution.%d' % m], g['energy.%d' % m]
        assert W.shape == (200, 200) and W.dtype == F and np.array_equal(W, W.T) and sol.shape == (5, 200) and en.shape == (5,)
        for s in range(5):                                              # the recorded energy is the reference formula on the recorded solution
            assert abs(R.energy64(sol[s], W) - en[s]) < 1e-6
        assert len(set(np.round(en, 9))) > 1                            # its own runs differ: "as good as its best run" is a real bar


@pytest.mark.parametrize('m', range(3))
def test_restatement_is_as_good_as_the_reference_on_200_variables(m):
    from panst3r_amd.engine.postprocess import QUBO_REPLICAS
    g = np.load(os.path.join(GOLDEN, 'qubo_solver.npz'))
    W, en = g['Wneg.%d' % m], g['energy.%d' % m]
    for seed, bar, what in ((0, en.min() + 1e-9, 'best'), (1, float(np.median(en)), 'median'), (2, float(np.median(en)), 'median')):
        x, e = R.anneal(W, QUBO_REPLICAS, seed=seed)
        got = R.energy64(x[R.winner(x, e)], W)
        print('matrix %d seed %d: %.6f against the reference\'s %s %.6f' % (m, seed, got, what, bar))
        assert got <= bar, (m, seed, got, bar)


# ---------------------------------------------------------------------------------------------------- public interface
def test_solver_argument():
    import torch
    from panst3r_amd import engine
    from panst3r_amd.engine.postprocess import panoptic_inference_qubo, solve_qubo_device, QUBO_REPLICAS
    sig = inspect.signature(panoptic_inference_qubo)
    assert sig.parameters['solver'].default == 'host' and sig.parameters['replicas'].default is None and sig.parameters['seed'].default == 0
    assert engine.solve_qubo_device is solve_qubo_device
    p = inspect.signature(solve_qubo_device).parameters
    assert (p['num_iters'].default, p['T0'].default, p['T_end'].default, p['lambda_reg'].default, p['seed'].default) == (10000, 0.5, 1e-4, 1e-3, 0)
    assert p['replicas'].default == QUBO_REPLICAS == 4096
    with pytest.raises(ValueError, match='solver'):
        panoptic_inference_qubo(torch.zeros(1, 4, 3), [torch.zeros(1, 4, 8, 8)], [[16, 16]], solver='nonsense')
