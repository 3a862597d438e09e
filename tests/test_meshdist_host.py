"""The host side of the exact point-to-mesh distance (panst3r_amd/engine/meshdist.py) and the properties of its contract, on the numpy restatement of
tests/meshdist_ref.py alone (no GPU here): the fp64 closest point against exact rational arithmetic with the error bound of docs/experiments.md §6p,
the binning as a superset of what a query needs, the refusals that precede any launch, the ABI."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi_header
import meshdist_ref as MD
import nearest_ref as N
from panst3r_amd import hip
from panst3r_amd.engine import mesh_distance, score_reconstruction
from panst3r_amd.engine.meshdist import MeshIndex

F = np.float32
U = 2.0 ** -53                                                                  # the unit roundoff of fp64


# ---------------------------------------------------------------- exact rational distance
def _fr(p):
    return [Fraction(float(x)) for x in p]


def _sub(p, q):
    return [x - y for x, y in zip(p, q)]


def _dotf(p, q):
    return sum(x * y for x, y in zip(p, q))


def _crossf(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


def _segment(q, a, b):
    ab = _sub(b, a)
    t = min(max(_dotf(_sub(q, a), ab) / _dotf(ab, ab), 0), 1)
    e = _sub(q, [x + t * y for x, y in zip(a, ab)])
    return _dotf(e, e)


def exact_d2(a, b, c, q):
    """the exact squared distance from q to the triangle (a, b, c): the minimum of the three segment distances, and of the plane distance when the foot
    of the perpendicular lies inside; every number a Fraction"""
    a, b, c, q = _fr(a), _fr(b), _fr(c), _fr(q)
    best = min(_segment(q, a, b), _segment(q, b, c), _segment(q, c, a))
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(q, a)
    g00, g01, g11, r0, r1 = _dotf(ab, ab), _dotf(ab, ac), _dotf(ac, ac), _dotf(ab, ap), _dotf(ac, ap)
    det = g00 * g11 - g01 * g01                                                 # |ab x ac|^2 > 0: the cases are not degenerate
    v, w = (r0 * g11 - r1 * g01) / det, (r1 * g00 - r0 * g01) / det
    if v >= 0 and w >= 0 and v + w <= 1:
        n = _crossf(ab, ac)
        best = min(best, _dotf(n, ap) ** 2 / _dotf(n, n))
    return best


def sine2(a, b, c):
    """sin^2 of the angle at a, exactly"""
    ab, ac = _sub(_fr(b), _fr(a)), _sub(_fr(c), _fr(a))
    n = _crossf(ab, ac)
    return _dotf(n, n) / (_dotf(ab, ab) * _dotf(ac, ac))


@functools.lru_cache(maxsize=None)
def cases():
    """640 triangles with one query each, every number an fp32 value -> (a, b, c, q [K,3] float32, kind [K]).  'generic': a within 5 of the origin per
    axis, two edges of length 1e-4 .. 3 (log-uniform) in random directions, the query at a + v ab + w ac + h n with v, w in [-1, 2] and h 0 .. 2 edge
    lengths.  'sliver': the second edge within 1e-6 of parallel to the first (checked exactly below), edges 0.5 .. 3, a within 1 of the origin so that
    fp32 keeps the shape; queries the same way.  'vertex' / 'edge' / 'inside': coordinates on a grid of 1 / 64, the query on corner b, on the midpoint
    of ab, and at a + ab / 4 + ac / 4: d2 = 0 exactly."""
    rng = np.random.default_rng(12)
    A, B, C, Q, kind = [], [], [], [], []

    def unit():
        u = rng.normal(size=3)
        return u / np.linalg.norm(u)

    def query(a, b, c):
        ab, ac = b - a, c - a
        n = np.cross(ab, ac)
        n /= np.linalg.norm(n)
        v, w = rng.uniform(-1, 2, 2)
        return a + v * ab + w * ac + rng.uniform(0, 2) * rng.choice([-1, 1]) * max(np.linalg.norm(ab), np.linalg.norm(ac)) * n * rng.integers(0, 2)

    def put(a, b, c, q, k):
        A.append(a); B.append(b); C.append(c); Q.append(q); kind.append(k)
    while len(kind) < 480:
        a = rng.uniform(-5, 5, 3)
        b, c = a + unit() * 10 ** rng.uniform(-4, np.log10(3)), a + unit() * 10 ** rng.uniform(-4, np.log10(3))
        a, b, c = (x.astype(F).astype(np.float64) for x in (a, b, c))
        if sine2(a, b, c) < Fraction(1, 10 ** 6):                               # fp32 has flattened a small face far from the origin: not a generic one
            continue
        put(a, b, c, query(a, b, c), 'generic')
    while len(kind) < 600:
        a, u = rng.uniform(-1, 1, 3), unit()
        p = np.cross(u, unit())
        p /= np.linalg.norm(p)
        L1, L2 = rng.uniform(0.5, 3, 2)
        b, c = a + L1 * u, a + L2 * (u + rng.uniform(0.2, 0.8) * 1e-6 * p)
        a, b, c = (x.astype(F).astype(np.float64) for x in (a, b, c))
        if not 0 < sine2(a, b, c) <= Fraction(1, 10 ** 12):
            continue
        put(a, b, c, query(a, b, c), 'sliver')
    while len(kind) < 640:
        a, ab, ac = rng.integers(-320, 321, 3) / 64.0, rng.integers(-48, 49, 3) / 16.0, rng.integers(-48, 49, 3) / 16.0      # halves and quarters stay fp32 values
        if not (ab.any() and ac.any()) or sine2(a, a + ab, a + ac) < Fraction(1, 100):
            continue
        k = ('vertex', 'edge', 'inside')[len(kind) % 3]
        put(a, a + ab, a + ac, {'vertex': a + ab, 'edge': a + ab / 2, 'inside': a + ab / 4 + ac / 4}[k], k)
    out = [np.array(x).astype(F) for x in (A, B, C, Q)]
    for x in out:
        assert np.abs(x).max() <= 16
    return out[0], out[1], out[2], out[3], np.array(kind)


@functools.lru_cache(maxsize=None)
def measured():
    a, b, c, q, kind = cases()
    D2, x, region = MD.closest_point(a, b, c, q)
    exact = [exact_d2(*t) for t in zip(a, b, c, q)]
    err = np.array([abs(float(Fraction(float(d)) - e)) for d, e in zip(D2, exact)])
    return D2, x, region, exact, err


def bound(a, b, c, q, region):
    """the bound of docs/experiments.md §6p on |D2 - exact|, per case.  S = the largest coordinate difference among the four points, M = the largest
    coordinate, l = the shortest edge, n2 = |ab x ac|^2, u = 2^-53:
        u (15 S^2 + 12 S M)                     the roundings of the last step, q - x and its square, x a rounded point of the triangle
      + (30 u S^2 / l)^2                        the edge parameter is off by 30 u S^2 / l^2; along the edge the distance is stationary: second order
      + (200 u S^4)^2 / (n2 l^2)                a region decided the other way next to an in-plane boundary, by a sign that rounding moved
      + interior only: (2800 u S^4 / n2)^2 S^2  the two weights are off by 800 u S^4 / n2 each; in the plane the distance is stationary: second order"""
    P = np.stack([a, b, c, q], 1).astype(np.float64)
    S = (P.max(1) - P.min(1)).max(1)
    Mx = np.abs(P).max((1, 2))
    ab, ac, bc = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 2] - P[:, 1]
    l2 = np.minimum(np.minimum((ab ** 2).sum(1), (ac ** 2).sum(1)), (bc ** 2).sum(1))
    n2 = (np.cross(ab, ac) ** 2).sum(1)
    first = U * (15 * S * S + 12 * S * Mx)
    return first + (30 * U * S * S) ** 2 / l2 + (200 * U * S ** 4) ** 2 / (n2 * l2) + (region == 6) * (2800 * U * S ** 4 / n2) ** 2 * S * S, first, S


def test_the_case_set_covers_every_region_slivers_and_the_exact_zeros():
    a, b, c, q, kind = cases()
    D2, x, region, exact, err = measured()
    assert len(kind) >= 500 and not np.isnan(D2).any() and (D2 >= 0).all()
    counts = np.bincount(region, minlength=7)
    assert (counts >= 10).all(), dict(zip(MD.REGIONS, counts.tolist()))        # the comparison cannot pass on vertices alone
    assert (np.bincount(region[kind == 'generic'], minlength=7) >= 10).all()
    sl = kind == 'sliver'
    assert sl.sum() >= 100 and all(0 < sine2(*t) <= Fraction(1, 10 ** 12) for t in zip(a[sl], b[sl], c[sl]))      # within 1e-6 of parallel, not degenerate
    assert len(set(region[sl].tolist())) >= 3
    edges = np.sqrt(np.stack([((b - a).astype(np.float64) ** 2).sum(1), ((c - a).astype(np.float64) ** 2).sum(1)]))
    assert edges.min() < 3e-4 and edges.max() > 2.5 and np.abs(np.stack([a, b, c])).max() > 7
    for k, r in (('vertex', 1), ('edge', 2), ('inside', 6)):
        m = kind == k
        assert m.sum() >= 10 and (D2[m] == 0).all() and (region[m] == r).all() and all(e == 0 for e, mm in zip(exact, m) if mm), k
        assert (x[m] == q[m]).all()


def test_the_fp64_closest_point_is_within_its_error_bound_of_exact_rational_arithmetic():
    """Measured on these 640 cases (printed below): the largest |D2 - exact| is 0.099 of the bound, so the assertion's factor 4 holds with room.  Outside
    the interiors of slivers the error stays below 0.099 of the bound's first term u (15 S^2 + 12 S M) alone - at the most 1 860 x 2^-52 S^2, on small
    faces far from the origin, where M S and not S^2 is the scale.  In the 7 cases whose query lies over the INTERIOR of a sliver within 1e-6 of
    parallel the error reaches 5.0e-8 S^2 (2.3e8 x 2^-52 S^2): the cancellation in (va + vb) + vc, which the bound's last term allows for (it is
    about 1e6 times above what is measured there)."""
    a, b, c, q, kind = cases()
    D2, x, region, exact, err = measured()
    full, first, S = bound(a, b, c, q, region)
    thin = (kind == 'sliver') & (region == 6)                                   # the interior of a sliver: the one place where the last term is large
    unit = 2.0 ** -52 * S * S
    print('max err / bound %.3g; all but sliver interiors: max err / first term %.3g, max err / (2^-52 S^2) %.3g; the %d sliver interiors: max err / (2^-52 S^2) '
          '%.3g, max err / S^2 %.3g' % ((err / full).max(), (err / first)[~thin].max(), (err / unit)[~thin].max(), thin.sum(), (err / unit)[thin].max(),
                                       (err / (S * S))[thin].max()))
    assert thin.sum() >= 3
    assert (err <= full).all()
    assert (4 * err <= full).all()                                              # the bound sits at least 4 times above what is measured


# ---------------------------------------------------------------- the binning
RADIUS = 0.11


@functools.lru_cache(maxsize=None)
def bin_scene():
    """420 faces of edges 0.05 .. 0.6 in a box of 3^3 around the origin (cells of both signs), 4 000 queries in a slightly larger box"""
    rng = np.random.default_rng(5)
    c = rng.uniform(-1.5, 1.5, (420, 1, 3))
    V = (c + rng.normal(size=(420, 3, 3)) * rng.uniform(0.03, 0.3, (420, 1, 1))).reshape(-1, 3).astype(F)
    return V, np.arange(1260).reshape(420, 3), rng.uniform(-1.7, 1.7, (4000, 3)).astype(F)


def test_every_face_within_the_radius_of_a_query_is_listed_in_the_querys_cell():
    V, Fc, Q = bin_scene()
    b = MD.binning(V, Fc, RADIUS)
    assert b['kept'].all() and b['total'] == b['counts'].sum() and (b['counts'] == b['ext'].prod(1)).all() and (b['ext'] >= 3).all()
    cq, _, ok = N.cells(Q, RADIUS)
    assert ok.all() and (cq < 0).any() and (cq > 0).any()
    tri = V[Fc].astype(np.float64)
    D2, _, _ = MD.closest_point(tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], Q[:, None, :].astype(np.float64))
    r, _, r2 = N.radius_numbers(RADIUS)
    within = D2.astype(F) <= r2
    listed = ((cq[:, None, :] >= b['lo'][None]) & (cq[:, None, :] < (b['lo'] + b['ext'])[None])).all(2)
    print('%d pairs within the radius, %d of them not listed' % (within.sum(), (within & ~listed).sum()))
    assert within.sum() > 1000 and not (within & ~listed).any()
    assert (listed.sum(1) >= within.sum(1)).all() and listed.sum() > 2 * within.sum()       # a superset, and a generous one: no pruning
    # the contract's precondition: no accepted distance sits within 2^-20 relative of the radius (this scene constructs no dyadic ones)
    assert not (np.abs(np.sqrt(D2) / float(r) - 1) < 2.0 ** -20).any()
    # the brute-force search agrees with a search through the restated lists
    want = MD.mesh_distance(Q[:400], V, Fc, RADIUS)
    lists = MD.cell_lists(V, Fc, RADIUS)
    assert sum(len(v) for v in lists.values()) == b['total']
    for i in range(400):
        cand = lists.get(tuple(int(x) for x in cq[i]), [])
        d = {f: F(MD.closest_point(tri[f, 0], tri[f, 1], tri[f, 2], Q[i].astype(np.float64))[0]) for f in cand}
        best = min(((v, f) for f, v in d.items()), default=(F(np.inf), -1))
        assert (best[1] if best[0] <= r2 else -1) == want['face'][i], i


def test_the_binning_drops_what_the_contract_drops_and_saturates():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [2, 0, 0], [0.25 * 2 ** 20, 0, 0], [3e38, 0, 0], [-3e38, 1, 0], [0, 0, 3e38]], dtype=F)
    faces = np.array([[0, 1, 2], [0, 0, 1], [0, 1, 4], [0, 1, 3], [0, 1, 9], [0, -1, 2], [0, 2, 5], [6, 7, 8]])
    b = MD.binning(V, faces, 0.25)
    assert b['kept'].tolist() == [True] + [False] * 7 and b['dropped_faces'] == 7
    assert b['lo'][0].tolist() == [-1, -1, -1] and b['ext'][0].tolist() == [7, 7, 3] and b['counts'].tolist() == [147] + [0] * 7
    wide = MD.binning(np.array([[-1000, -1000, 0], [1000, -1000, 0], [0, 1000, 100]], dtype=F), [[0, 1, 2]], 0.25)      # 8003 x 8003 x 403 cells
    assert wide['kept'].all() and wide['counts'].tolist() == [MD.FACE_CAP] and wide['total'] == hip.MESHDIST_FACE_CAP
    edge = MD.binning(np.array([[0, 0, 0], [0.25 * (2 ** 20 - 2), 0, 0], [0, 1, 0]], dtype=F), [[0, 1, 2]], 0.25)       # cell 2^20 - 2, dilated: the last one
    assert edge['kept'].all() and edge['lo'][0, 0] + edge['ext'][0, 0] - 1 == 2 ** 20 - 1
    assert not MD.binning(np.array([[0, 0, 0], [0.25 * (2 ** 20 - 1), 0, 0], [0, 1, 0]], dtype=F), [[0, 1, 2]], 0.25)['kept'].any()


# ---------------------------------------------------------------- refusals that precede any launch
def test_bad_arguments_are_refused_before_any_launch(monkeypatch):
    for name in ('meshdist_count', 'meshdist_insert', 'meshdist_scatter', 'meshdist_query', 'meshdist_workspace', 'mesh_sample_count', 'nn_insert'):
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail('a launch'))
    p, v, f = torch.zeros(5, 3), torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for radius in (0, -1.0, float('nan'), float('inf'), 1e-30, 1e30, '1', True, None):
        with pytest.raises(ValueError):
            mesh_distance(p, v, f, radius)
        with pytest.raises(ValueError):
            MeshIndex(v, f, radius)
    for bad in (0, -1, 1.5, True, None, '4'):
        with pytest.raises(ValueError, match='max_cell_faces'):
            mesh_distance(p, v, f, 0.1, max_cell_faces=bad)
        with pytest.raises(ValueError, match='max_pairs'):
            mesh_distance(p, v, f, 0.1, max_pairs=bad)
        with pytest.raises(ValueError, match='max_pairs'):
            MeshIndex(v, f, 0.1, max_pairs=bad)
    with pytest.raises(ValueError, match='max_pairs'):
        mesh_distance(p, v, f, 0.1, max_pairs=2 ** 30 + 1)
    for args in ((torch.zeros(5, 2), v, f), (torch.zeros(5, 3, dtype=torch.int32), v, f), (p, torch.zeros(4, 4), f), (p, v, torch.zeros(2, 4, dtype=torch.int64)),
                 (p, v, torch.zeros(2, 3)), (p, v, torch.zeros(6, dtype=torch.int64)), (p, v.numpy(), f), (p.numpy(), v, f), (p, v, f.numpy())):
        with pytest.raises(ValueError):
            mesh_distance(*args, 0.1)
    with pytest.raises(RuntimeError, match='GPU only'):                          # CPU tensors: there is no CPU fallback
        mesh_distance(p, v, f, 0.1)
    with pytest.raises(RuntimeError, match='GPU only'):
        MeshIndex(v, f, 0.1)
    with pytest.raises(RuntimeError, match='GPU only'):                          # ... for empty ones either
        mesh_distance(torch.zeros(0, 3), v, f, 0.1)
    for metric in ('nonsense', None, 'Surface', 1):
        with pytest.raises(ValueError, match='metric'):
            score_reconstruction(p, v, f, thresholds=[0.1], spacing=0.05, metric=metric)
    for kw in (dict(max_pairs=0), dict(max_cell_faces=0), dict(max_pairs=1.5)):    # the guards of the surface metric, before anything else
        with pytest.raises(ValueError, match='max_'):
            score_reconstruction(p, v, f, thresholds=[0.1], spacing=0.05, metric='surface', **kw)
    with pytest.raises(ValueError, match='beyond the search radius'):            # the other checks are the same under both metrics
        score_reconstruction(p, v, f, thresholds=[0.1], spacing=0.05, max_dist=0.05, metric='surface')


def test_abi_is_unchanged_and_the_new_prototypes_are_declared_once():
    defines = abi_header.defines()
    assert hip.ABI_VERSION == 20 == defines['PST_ABI_VERSION']
    assert (hip.MESHDIST_FULL, hip.MESHDIST_LISTS, hip.MESHDIST_TOTAL) == (defines['PST_MESHDIST_FULL'], defines['PST_MESHDIST_LISTS'], defines['PST_MESHDIST_TOTAL'])
    assert hip.MESHDIST_FACE_CAP == defines['PST_MESHDIST_FACE_CAP'] == MD.FACE_CAP and hip.MESHDIST_MAX == 2 ** 30 and MD.LIM == N.LIM
    names = [p[0] for p in abi_header.prototypes()]
    new = {'pst_meshdist_count', 'pst_meshdist_insert', 'pst_meshdist_scatter', 'pst_meshdist_query'}
    assert {n for n in names if n.startswith('pst_meshdist_')} == new == {n for n in hip.SIGNATURES if n.startswith('pst_meshdist_')}
    assert all(names.count(n) == 1 and hip.EXPORTS.count(n) == 1 for n in new)
    code = {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'uint64_t': 'u', 'float': 'f', 'double': 'd'}
    for name, ret, params in abi_header.prototypes():
        if name in new:
            assert hip.SIGNATURES[name] == code[ret] + ':' + ''.join('p' if t.endswith('*') else code[t] for t in params), name
