"""numpy restatement of the device QUBO solver (csrc/qubo_solve.hip), bit for bit: the yardstick of tests/test_hip_qubo_solver.py.

Own code.  The algorithm is the reference's annealer (engine/postprocess.py:266-336: single bit flips, Metropolis acceptance, geometric cooling, best
state kept) run as independent replicas; everything that makes the result a pure function of its arguments is fixed by the kernel's header comment
and restated here operation by operation: the counter-based generator (Philox4x32-10), the incremental local fields, an exponential made of
separately rounded float32 operations, the evaluation order.  float32 numpy rounds every product and every sum on its own, which is what the kernel
(compiled without contraction) promises, so the comparison has zero tolerance.  All replicas advance together, one numpy operation per step of a move.

`variant` plants a mistake for the tests: 'lambda_sign' (s * lambda / N with the wrong sign), 'no_diag' (forgets W_jj), 'accept_gt' (u > p).
"""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
NMAX = 200


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11; constants of Random123 philox.h).  Counter words: uint32 arrays (broadcast together), key: two ints.
    Returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=U64) for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ U64(k0), p1 & M32, (p0 >> U64(32)) ^ c3 ^ U64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0.astype(U32), c1.astype(U32), c2.astype(U32), c3.astype(U32)


def draws(seed, replica, move, N):
    """(j, u) of `replica` at `move` (arrays broadcast together): j in [0, N) by multiply-high, u in [0, 1) from the top 24 bits"""
    move = np.asarray(move, dtype=np.int64)
    w = philox4x32_10(move >> 1, replica, 0, 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    odd = (move & 1).astype(bool)
    wj, wu = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    j = ((wj.astype(U64) * U64(N)) >> U64(32)).astype(np.int64)
    u = (wu >> U32(8)).astype(F) * F(2.0 ** -24)
    return j, u


def initial_x(seed, replicas, N):
    """uint8 [len(replicas), N]: bit (k mod 32) of word ((k / 32) mod 4) of block (k / 128) of stream 1"""
    replicas = np.asarray(replicas, dtype=np.int64)
    words = []
    for b in range(2):
        words += list(philox4x32_10(b, replicas, 1, 0, int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    words = np.stack(words, axis=1)                                    # [R, 8]
    k = np.arange(N)
    return ((words[:, k // 32] >> (k % 32).astype(U32)) & U32(1)).astype(np.uint8)


def exp_neg(a):
    """the kernel's exponential for a <= 0, float32 array -> float32 array"""
    a = np.asarray(a, dtype=F)
    ok = a >= F(-87.0)
    a = np.where(ok, a, F(0.0))
    n = np.rint(a * F(1.44269502e+00))
    r = (a - n * F(6.93145752e-01)) - n * F(1.42860677e-06)
    p = np.full_like(a, F(1.98412698e-04))
    for c in (1.38888889e-03, 8.33333333e-03, 4.16666667e-02, 1.66666667e-01, 0.5, 1.0, 1.0):
        p = p * r + F(c)
    out = (p.view(np.int32) + (n.astype(np.int32) << np.int32(23))).view(F)
    return np.where(ok, out, F(0.0))


def evaluate(x, W, lamN):
    """x uint8 [R, N] -> (h float32 [R, N], e float32 [R]): fields and energy from scratch, ascending j, then ascending k"""
    R, N = x.shape
    h = np.zeros((R, N), dtype=F)
    for j in range(N):
        on = x[:, j].astype(bool)
        h[on] = h[on] + W[j][None, :]
    e = np.zeros(R, dtype=F)
    for k in range(N):
        on = x[:, k].astype(bool)
        e[on] = e[on] + h[on, k]
    return h, e + lamN * x.sum(axis=1).astype(F)


def schedule(num_iters, T0, T_end, lambda_reg, N):
    """(beta0, cinv, lamN) as the C entry point computes them"""
    T0, T_end = float(F(T0)), float(F(T_end))
    beta0 = F(1.0 / T0)
    cinv = F((T0 / T_end) ** (1.0 / num_iters)) if num_iters > 0 else F(1.0)
    return beta0, cinv, F(lambda_reg) / F(N)


def anneal(W, replicas, num_iters=10000, T0=0.5, T_end=1e-4, lambda_reg=1e-3, seed=0, variant=None, return_tracked=False, chunk=512):
    """W float32 [N, N]; `replicas`: a count (replicas 0 .. count-1) or an array of replica indices (replicas are independent, so any subset can be
    restated on its own).  Returns (x uint8 [R, N], e float32 [R]): every replica's best state and its re-evaluated energy; with return_tracked also
    the incrementally tracked best energy and the tracked current energy / state (for the drift checks)."""
    W = np.ascontiguousarray(W, dtype=F)
    N = W.shape[0]
    assert W.shape == (N, N) and 1 <= N <= NMAX
    rep = np.arange(replicas, dtype=np.int64) if np.isscalar(replicas) else np.asarray(replicas, dtype=np.int64)
    R = len(rep)
    beta, cinv, lamN = schedule(num_iters, T0, T_end, lambda_reg, N)
    diag = np.ascontiguousarray(np.diag(W))
    x = initial_x(seed, rep, N)
    h, E = evaluate(x, W, lamN)
    bx, bE = x.copy(), E.copy()
    ar = np.arange(R)
    lam_s = -lamN if variant == 'lambda_sign' else lamN
    for i0 in range(0, num_iters, chunk):
        n = min(chunk, num_iters - i0)
        J, U = draws(seed, rep[None, :], np.arange(i0, i0 + n)[:, None], N)        # [n, R]
        for t in range(n):
            j, u = J[t], U[t]
            s = F(1.0) - F(2.0) * x[ar, j].astype(F)
            d = (F(2.0) * s) * h[ar, j]
            if variant != 'no_diag':
                d = d + diag[j]
            d = d + s * lam_s
            p = exp_neg(np.where(d < 0, F(0.0), -(d * beta)))                       # (the kernel does not evaluate it for d < 0)
            acc = (d < 0) | ((u > p) if variant == 'accept_gt' else (u < p))
            a = np.flatnonzero(acc)
            if len(a):
                ja, sa = j[a], s[a]
                x[a, ja] ^= 1
                E[a] = E[a] + d[a]
                h[a] = h[a] + sa[:, None] * W[ja]
                b = a[E[a] < bE[a]]
                bE[b] = E[b]
                bx[b] = x[b]
            beta = beta * cinv
    _, e = evaluate(bx, W, lamN)
    if return_tracked:
        return bx, e, bE, E, x
    return bx, e


def winner(x, e):
    """the smallest (energy, replica index); replica 0 if no energy compares"""
    ok = ~np.isnan(e)
    if not ok.any():
        return 0
    m = e[ok].min()
    return int(np.flatnonzero(ok & (e == m))[0])


def energy64(x, W, lambda_reg=1e-3):
    """the reference's formula (engine/postprocess.py:262-264) in float64"""
    x = np.asarray(x, dtype=np.float64)
    return float(x.dot(np.asarray(W, dtype=np.float64)).dot(x) + lambda_reg * x.mean())


def brute_force(W, lambda_reg=1e-3):
    """all 2^N states (N <= 20) in float64 -> (energies sorted ascending, the best state)"""
    W = np.asarray(W, dtype=np.float64)
    N = W.shape[0]
    assert N <= 20
    states = ((np.arange(1 << N)[:, None] >> np.arange(N)) & 1).astype(np.float64)
    e = np.einsum('si,ij,sj->s', states, W, states) + lambda_reg * states.mean(axis=1)
    order = np.argsort(e, kind='stable')
    return e[order], states[order[0]].astype(np.uint8)
