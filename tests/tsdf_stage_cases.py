"""Shared by tests/test_hip_tsdf_stages.py (GPU) and tests/test_tsdf_stage_checks.py (CPU): the cases that hold the seven kernels of csrc/tsdf.hip to
their contract STAGE BY STAGE, fed by hand, at the values, sign patterns and launch edges that a rendered scene never makes; the references composed of
the restatement (tests/tsdf_ref.py: NodeTable, integrate_planes, extract); and the planted mistakes.  Nothing here imports the code under test.

Every number is chosen to be exact in fp32: vs = 2^-6, f = 64, identity rotations.  A node (n, m, k) sits at (n, m, k) / 64; the camera of view A
(origin, pp = (4, 2), near = 0.5, a 4 x 8 image) sees it at zc = k / 64, u = 64 n / k + 4, v = 64 m / k + 2: at k = 128, u = n / 2 + 4, so n = -9
lands on pixel 0 (u + 0.5 == 0), n = -10 outside, n = 6 on pixel 7, n = 7 outside (u + 0.5 == W); k = 32 is exactly `near`, k = 31 nearer.

  node cases     `node_cases(band)`: cells -> NodeTable; `range_case(band)`: one step beyond the last legal cells; `wrap_cells(band)`: a table at its
                 smallest capacity with two node keys whose home is the last slot; `counted(N)`: exactly N nodes at band 1
  integrate      `integrate_case(band, Nn)`: seven views (3 x 5, 4 x 8, H W == npix + 1, H == 0, negative dims, and two whose only measured pixel
                 holds s one float below -tau and one above +tau), nodes written by hand; `many_views()`: 67 views of one pixel
  extraction     `extract_case(name)`: sdf, weight, count, pan, colours written by hand on a node table; `extract_ref(name)`
  mistakes       `v_nodes`, `v_integrate`, `v_extract`: the restatement again, with one decision changed by name; with no name they ARE the
                 restatement, which tests/test_tsdf_stage_checks.py asserts on every case before it asserts which case catches which mistake"""
import functools

import numpy as np

import geom_stage_cases as G
import tsdf_ref as T

F = np.float32
LIM = 1 << 20
WG, PT, LANES = 1024, 4, 256                     # nodes per workgroup, per lane, lanes (TS_WG, TS_PT, TS_T)
BANDS = (1, 2, 3, 4)
VS = F(2.0 ** -6)


def capacity(pairs):
    """slots of the node table: the next power of two >= twice the pairs"""
    return 1 << max(1, (2 * int(pairs) - 1).bit_length())


def offsets(band, z_fastest=False, shift=1):
    side = 2 * band
    o = np.arange(side ** 3)
    c = [o % side, (o // side) % side, o // (side * side)]
    return np.stack(c[::-1] if z_fastest else c, axis=1) - band + shift


def pairs_of(cells, band):
    """int64 [Mv (2 band)^3, 3]: the node of every (row, offset) pair, in pair order"""
    return (np.asarray(cells, dtype=np.int64).reshape(-1, 1, 3) + offsets(band)[None]).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------- node cases
def strip(n, origin=(0, 0, 0)):
    return np.stack([np.arange(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], axis=1) + np.asarray(origin, dtype=np.int64)


def block(nx, ny=None, nz=None, origin=(0, 0, 0)):
    """nx ny nz cells, x fastest"""
    ny, nz = nx if ny is None else ny, nx if nz is None else nz
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.int64) + np.asarray(origin, dtype=np.int64)


def counted(N, origin=(0, 0, 0), isolated=False):
    """cells with exactly N nodes at band 1: a strip along x (4 (n + 1) nodes) plus, as N asks, a cell touching its end in one corner (+ 7), one
    sharing an edge with its start (+ 6), or (`isolated`) one on its own (+ 8).  N = 0: no cell"""
    if N == 0:
        return np.zeros((0, 3), dtype=np.int64)
    extra = {0: (), 3: ('corner',), 2: ('edge',), 1: ('corner', 'edge')}[N % 4] + (('isolated',) if isolated else ())
    n = (N - sum({'corner': 7, 'edge': 6, 'isolated': 8}[e] for e in extra)) // 4 - 1
    assert n >= (2 if len(extra) > 1 else 1), N                # the extra cells share no node with each other
    at = {'corner': (n, 1, 1), 'edge': (0, 1, 1), 'isolated': (0, 4, 4)}
    return np.concatenate([strip(n)] + [np.array([at[e]], dtype=np.int64) for e in extra]) + np.asarray(origin, dtype=np.int64)


NODE_COUNTS = {8: {}, 1020: {}, 1023: {}, 1024: {'isolated': True}, 1025: {}, 1027: {}, 2049: {}}       # strip 1, 254, 253 + 7, 253 + 8, 252 + 13, 254 + 7, 508 + 13
BIG = 16                                                                                                 # 16^3 cells: 17^3 = 4913 nodes at band 1


def last_legal(band):
    hi, lo = LIM - 1 - band, -LIM + band
    return np.array([(hi, 0, 0), (0, hi, 0), (0, 0, hi), (lo, 0, 0), (0, lo, 0), (0, 0, lo), (hi, hi, hi), (lo, lo, lo), (hi, lo, hi)], dtype=np.int64)


def node_cases(band):
    """name -> cells int64 [Mv, 3] (unique rows)"""
    g = np.random.default_rng(band)
    c = {'one': np.zeros((1, 3), dtype=np.int64),
         'shuffled': block(3, 2, 2)[g.permutation(12)],
         'around_zero': block(2, origin=(-1, -1, -1))[g.permutation(8)],
         'last_legal': last_legal(band)}
    if band in WRAP_MV:
        c['wrap'] = wrap_cells(band)
    if band == 1:
        for N, kw in NODE_COUNTS.items():
            c['count_%d' % N] = counted(N, **kw)
        c['big'] = block(BIG)
    return c


def range_case(band):
    """(cells, out bool [P]): a legal cell, the last legal cells, and one step beyond them on three axes; `out`: the pairs whose node is outside"""
    hi, lo = LIM - 1 - band, -LIM + band
    cells = np.array([(0, 0, 0), (hi + 1, 0, 0), (hi, 1, 1), (0, lo - 1, 0), (3, 3, lo), (5, 5, hi + 1), (lo - 1, lo - 1, lo - 1)], dtype=np.int64)
    return cells, (np.abs(pairs_of(cells, band)) >= LIM).any(axis=1)


WRAP_MV = {1: 32, 2: 4, 4: 1}              # cells whose pairs are a power of two: the capacity is exactly twice the pairs (216 per cell never are)


@functools.lru_cache(maxsize=None)
def wrap_cells(band):
    """a strip of WRAP_MV[band] cells, moved until at least two of its node keys have the LAST slot of the table as home: whichever arrives second
    probes on to slot 0"""
    Mv = WRAP_MV[band]
    cap = capacity(Mv * (2 * band) ** 3)
    assert cap == 2 * Mv * (2 * band) ** 3
    for s in range(100000):
        cells = strip(Mv, (17 * s, -5 * s, 3 * s))
        nodes = np.unique(pairs_of(cells, band), axis=0)
        if (G.home_slot(G.vx_key(nodes), cap) == cap - 1).sum() >= 2:
            return cells
    raise AssertionError('no strip found')


@functools.lru_cache(maxsize=None)
def node_table(band, name):
    return T.NodeTable(node_cases(band)[name], band)


# ------------------------------------------------------------------------------------------------------------------------------------ integrate cases
def cam_row(t=(0.0, 0.0, 0.0), f=64.0, pp=(4.0, 2.0), near=0.5):
    """float32 [16] of a camera with identity rotation at t (render_ref.camera_table's layout)"""
    return np.array([1, 0, 0, -t[0], 0, 1, 0, -t[1], 0, 0, 1, -t[2], f, pp[0], pp[1], near], dtype=F)


K0 = 128                                         # the node layer at z = 2, where every view but B and C measures
KC, ZC = 64, 2.0 ** -12                          # view C stands 2^-12 in front of the layer k = 64
VIEWS = ('F', 'A', 'D', 'E', 'G', 'B', 'C')     # offsets 0, 15, 47, 79, 111, 143, 175: all but the first no multiple of 4 floats


def _specials(b):
    """name -> node (n, m, k) of the integrate case at band b; the most telling first (the small cases hold a prefix)"""
    return {'at_minus_tau': (0, 0, K0 + b), 'at_plus_tau': (0, 0, K0 - b), 'at_near': (0, 0, 32), 'left_in': (-9, 0, K0), 'd_neg_zero': (-2, 0, K0),
            'below_minus_tau_A': (2, 0, K0 + b), 'above_plus_tau_A': (0, -2, K0 - b), 'd_pos_zero': (4, 0, K0), 'nearer': (0, 0, 31), 'left_out': (-10, 0, K0),
            'right_in': (6, 0, K0), 'right_out': (7, 0, K0), 'top_in': (0, -5, K0), 'top_out': (0, -6, K0), 'bottom_in': (0, 2, K0), 'bottom_out': (0, 3, K0),
            'behind': (0, 0, -5), 'below_minus_tau_B': (0, 0, b + 1), 'above_plus_tau_C': (0, 0, KC), 'u_beyond_limit': (256, 0, KC), 'u_within_limit': (255, 0, KC),
            'u_overflows_int': (1 << 19, 0, KC), 'on_surface': (0, 0, K0), 'corner_in': (-9, -5, K0), 'corner_out': (7, 3, K0)}


INTEGRATE_NN = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def integrate_case(band, Nn):
    """dict(nodes int32 [Nn, 3], cams float32 [7, 16], depths [7 float32 planes], dims int32 [7, 2], npix [7], vs, band, special: name -> indices)"""
    b = band
    tau = F(F(b) * VS)
    ulp = np.spacing(tau)
    g = np.random.default_rng(100 * b + Nn % 97)
    sp = _specials(b)
    nodes = np.stack([g.integers(-12, 10, Nn), g.integers(-8, 6, Nn), g.integers(K0 - 8, K0 + 9, Nn)], axis=1)
    names, rows = list(sp), np.array(list(sp.values()), dtype=np.int64)
    special = {n: [] for n in names}
    starts = [0] + ([250] if Nn >= 300 else []) + ([1012] if Nn >= 1100 else []) + ([Nn - len(rows)] if Nn >= 2 * len(rows) else [])
    for s in starts:                              # at the start, across 255 | 256 (the lane's second node), across 1023 | 1024 (the workgroup), at the end
        n = min(len(rows), Nn - s)
        nodes[s:s + n] = rows[:n]
        for i in range(n):
            special[names[i]].append(s + i)
    # the planes
    A = np.full((4, 8), 2.0, dtype=F)
    A[2, 5] = np.nextafter(F(2), F(0))            # s = -(tau + 2^-23) at the node (2, 0, K0 + b): occluded
    A[1, 4] = np.nextafter(F(2), F(4))            # s = tau + 2^-22 at the node (0, -2, K0 - b): clamped
    A[2, 6], A[2, 3] = F(0.0), F(-0.0)            # measured nothing, of either sign
    B = np.zeros((4, 8), dtype=F)
    B[2, 4] = F(F(2.0 ** -6) - ulp)               # at the node (0, 0, b + 1), zc = (b + 1) 2^-6: s = -(tau + ulp(tau)), the float32 below -tau
    C = np.zeros((4, 8), dtype=F)
    C[2, 4] = F(F(ZC) + F(tau + ulp))             # at the node (0, 0, KC), zc = 2^-12: s = tau + ulp(tau), the float32 above tau
    assert float(B[2, 4]) == 2.0 ** -6 - float(ulp) and float(C[2, 4]) == ZC + float(tau) + float(ulp)
    two = lambda n: np.full(n, 2.0, dtype=F)
    planes = {'F': (two(15), (3, 5), cam_row(pp=(2.0, 1.0))), 'A': (A.reshape(-1), (4, 8), cam_row()), 'D': (two(32), (3, 11), cam_row()),
              'E': (two(32), (0, 8), cam_row()), 'G': (two(32), (-4, -8), cam_row()), 'B': (B.reshape(-1), (4, 8), cam_row(near=2.0 ** -10)),
              'C': (C.reshape(-1), (4, 8), cam_row(t=(0.0, 0.0, KC / 64.0 - ZC), near=2.0 ** -13))}
    return {'nodes': nodes.astype(np.int32), 'cams': np.stack([planes[v][2] for v in VIEWS]), 'depths': [planes[v][0] for v in VIEWS],
            'dims': np.array([planes[v][1] for v in VIEWS], dtype=np.int32), 'npix': [len(planes[v][0]) for v in VIEWS], 'vs': VS, 'band': b,
            'special': special}


def one_view(case, v):
    """the case with the view named v alone"""
    j = VIEWS.index(v)
    return dict(case, cams=case['cams'][j:j + 1], depths=case['depths'][j:j + 1], dims=case['dims'][j:j + 1], npix=case['npix'][j:j + 1])


MANY_V = 67


@functools.lru_cache(maxsize=None)
def many_views():
    """67 views of ONE pixel at one pose (origin, pp = (0, 0), near = 2^-10), each a seeded depth in [2^-6, 2^-3); the eight nodes (0, 0, k), k = 1 .. 8,
    on the one ray, at band 4: s = d - k / 64 spreads over many binades, so the fp32 sum of up to 67 terms rounds and its order shows, and most
    weights are no power of two, so the quotient differs from the product with the reciprocal"""
    g = np.random.default_rng(7)
    depths = [np.array([g.uniform(2.0 ** -6, 2.0 ** -3)], dtype=F) for _ in range(MANY_V)]
    nodes = np.array([(0, 0, k) for k in range(1, 9)], dtype=np.int32)
    return {'nodes': nodes, 'cams': np.stack([cam_row(pp=(0.0, 0.0), near=2.0 ** -10)] * MANY_V), 'depths': depths,
            'dims': np.array([(1, 1)] * MANY_V, dtype=np.int32), 'npix': [1] * MANY_V, 'vs': VS, 'band': 4, 'special': {}}


def integrate_ref(case):
    return T.integrate_planes(case['nodes'], case['cams'], case['depths'], case['dims'], case['npix'], case['vs'], case['band'])


# ----------------------------------------------------------------------------------------------------------------------------------- extraction cases
def voxel_attributes(Mv, seed=0):
    """(count, pan, colors): counts 1 .. 5, ids 0 .. 3 (0 among them), seeded colours"""
    g = np.random.default_rng(1000 + seed)
    return (1 + (np.arange(Mv) * 7) % 5).astype(np.int32), g.integers(0, 4, Mv).astype(np.int32), g.random((Mv, 3)).astype(F)


def checker(nodes):
    return np.where(np.asarray(nodes).sum(axis=1) & 1, F(-1), F(1)).astype(F)


def _case(cells, band=1, sdf=None, weight=None, min_weight=1, attributes=None, seed=0, **extra):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    tab = T.NodeTable(cells, band)
    count, pan, colors = voxel_attributes(len(cells), seed) if attributes is None else attributes
    sdf = sdf(tab) if callable(sdf) else sdf
    weight = np.full(len(tab), min_weight, dtype=np.int32) if weight is None else (weight(tab) if callable(weight) else weight)
    return dict(cells=cells, band=band, tab=tab, sdf=np.asarray(sdf, dtype=F), weight=np.asarray(weight, dtype=np.int32), min_weight=min_weight,
                count=np.asarray(count, dtype=np.int32), pan=np.asarray(pan, dtype=np.int32), colors=np.asarray(colors, dtype=F).reshape(-1, 3), vs=VS, **extra)


def _set(tab, values, default):
    """a field that is `default` but for {node: value}"""
    a = np.full(len(tab), default, dtype=F)
    for n, v in values.items():
        r = int(tab.rank(np.array(n)))
        assert r >= 0, n
        a[r] = v
    return a


def _plane(zero):
    # nodes z = 0 .. 3: the layer z = 0 inside, z = 1 holds `zero`, above it outside; the crossing sits exactly on the layer z = 1
    return _case(block(6, 6, 3), sdf=lambda t: np.where(t.nodes[:, 2] == 1, F(zero), (t.nodes[:, 2] - 1).astype(F) * F(0.25)),
                 gradient=lambda p: np.array([0.0, 0.0, 1.0]))


TINY = F(2.0 ** -149)


def _subnormal(lone, rest):
    return _case(block(3), sdf=lambda t: _set(t, {(1, 1, 1): lone, (2, 2, 2): lone}, rest))


def _lone(inside):
    s = F(-1) if inside else F(1)
    return _case(block(4), sdf=lambda t: _set(t, {(2, 2, 2): s}, -s), gradient=lambda p: (p - 2.0) * (1.0 if inside else -1.0))


def _weight_edge(min_weight):
    # the plane of _plane, one node of its inside layer and one of its zero layer one weight short
    def weight(t):
        w = _set(t, {(2, 2, 0): min_weight - 1, (4, 3, 1): min_weight - 1}, min_weight)
        return w.astype(np.int32)
    return _case(block(6, 6, 3), sdf=lambda t: (t.nodes[:, 2] - 1).astype(F) * F(0.25) + F(0.125), weight=weight, min_weight=min_weight)


def _labels(cells, counts, band=2):
    """every complete cell a surface cell (the checkerboard); ids and colours tell the rows apart"""
    Mv = len(cells)
    att = (np.asarray(counts, dtype=np.int32), 11 + np.arange(Mv, dtype=np.int32), (np.arange(3 * Mv).reshape(Mv, 3) + 1).astype(F) / F(64))
    return _case(cells, band=band, sdf=lambda t: checker(t.nodes), attributes=att)


def _sum_order():
    """one cell whose z component sums (1 + 1) + A + e in the edge order x, y, z and (A + e) + 1 + 1 in the order y, z, x; A = 2^-23 makes the mean
    without e a tie between two float32, e = 1.25 2^-52 is kept by the first order and lost by the second"""
    A, e = F(2.0 ** -23), F(1.25 * 2.0 ** -52)
    D = {(0, 0, 0): 1, (1, 0, 0): A, (0, 1, 0): 1, (1, 1, 0): e, (0, 0, 1): 1, (1, 0, 1): F(A - F(1)), (0, 1, 1): 1, (1, 1, 1): -1}
    return _case(block(1), sdf=lambda t: _set(t, D, 1))


def _big(seed, min_weight):
    g = np.random.default_rng(seed)

    def sdf(t):
        return (np.where(g.random(len(t)) < 0.5, -1, 1) * np.exp2(g.integers(-20, 1, len(t))) * (1 + g.random(len(t)))).astype(F)
    return _case(block(BIG), sdf=sdf, weight=lambda t: np.where(g.random(len(t)) < 0.03, min_weight - 1, min_weight + g.integers(0, 3, len(t))).astype(np.int32), min_weight=min_weight, seed=seed)


def _ball():
    c = np.array([8.25, 7.75, 8.5])
    return _case(block(BIG), sdf=lambda t: (np.sqrt(((t.nodes - c) ** 2).sum(axis=1)) - 5.3).astype(F), gradient=lambda p: p - c)


def _wg_gap():
    def weight(t):
        w = np.ones(len(t), dtype=np.int32)
        w[WG:2 * WG] = 0                           # no node of the second workgroup is valid: it emits nothing, its neighbours do
        return w
    return _case(block(BIG), sdf=lambda t: checker(t.nodes), weight=weight)


# gadgets of band-1 cells whose face-bearing nodes get chosen ranks: a node's rank is the order of its first appearance, so the order of the cells
# decides it.  `_filler(N)` puts exactly N flat nodes (no surface) in front.
def _one_edge(p, axis, corner):
    """four cells around the lattice edge from p along `axis`; the first listed holds p as its corner `corner` (x + 2 y + 4 z, the bit of `axis`
    clear), so that p is the (corner + 1)-th node to appear.  With inside = (coordinate `axis` <= p's), p is the ONLY face-bearing node."""
    assert not (corner >> axis) & 1
    b, c = (axis + 1) % 3, (axis + 2) % 3
    first = np.array([-(corner & 1), -((corner >> 1) & 1), -(corner >> 2)])
    cells = []
    for ob, oc in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
        o = np.zeros(3, dtype=np.int64)
        o[b], o[c] = ob, oc
        cells.append(o)
    cells.sort(key=lambda o: not np.array_equal(o, first))
    return np.array(cells) + np.asarray(p)


def _full8(p):
    """27 cells, the middle one first: its eight nodes are the first to appear and each has its eight cells, so under the checkerboard all have mask 7"""
    cells = block(3, origin=(-1, -1, -1))
    order = np.argsort([not (c == 0).all() for c in cells], kind='stable')
    return cells[order] + np.asarray(p)


def _last7(p):
    """64 cells around q = p + (1, 1, 1): the cells without q first, then q's eight with (0, 0, 0) in front, whose last corner q is - q is the last
    node to appear, and has its eight cells"""
    cells = block(4, origin=(-1, -1, -1))
    has_q = ((cells == 0) | (cells == 1)).all(axis=1)
    key = np.where(has_q, np.where((cells == 0).all(axis=1), 1, 2), 0)
    return cells[np.argsort(key, kind='stable')] + np.asarray(p)


def _compose(parts):
    """parts = [(kind, argument)]: 'flat' N nodes without a surface, or a gadget; each in a region of its own, 12 cells further along y.
    -> (cells, [(kind, argument, origin)])"""
    cells, regions = [], []
    for i, (kind, arg) in enumerate(parts):
        origin = np.array([0, 12 * i, 0])
        if kind == 'flat':
            c = counted(arg, origin)
        elif kind == 'edge':
            c = _one_edge(origin, *arg)
        elif kind == 'full8':
            c = _full8(origin)
        else:
            c = _last7(origin)
        cells.append(c)
        regions.append((kind, arg, origin))
    return np.concatenate(cells), regions


def _gadgets(parts):
    cells, regions = _compose(parts)

    def sdf(t):
        s = np.ones(len(t), dtype=F)
        y = t.nodes[:, 1]
        for i, (kind, arg, origin) in enumerate(regions):
            mine = (y >= 12 * i - 6) & (y < 12 * i + 6)
            if kind == 'edge':
                s[mine] = np.where(t.nodes[mine, arg[0]] <= origin[arg[0]], F(-0.5), F(0.25))
            elif kind in ('full8', 'last7'):
                s[mine] = checker(t.nodes[mine])
        return s
    return _case(cells, sdf=sdf)


EXTRACT = {
    'checker': lambda: _case(block(11), sdf=lambda t: checker(t.nodes)),
    'plane_pos_zero': lambda: _plane(0.0),
    'plane_neg_zero': lambda: _plane(-0.0),
    'subnormal_neg': lambda: _subnormal(-TINY, TINY),            # the only sign change of its cells is -2^-149 against +2^-149
    'subnormal_pos': lambda: _subnormal(TINY, -TINY),
    'tiny_inside': lambda: _case(block(3), sdf=lambda t: np.where(t.nodes[:, 0] <= 1, F(-2.0 ** -20), F(1))),      # t near 0
    'tiny_outside': lambda: _case(block(3), sdf=lambda t: np.where(t.nodes[:, 1] <= 1, F(-1), F(2.0 ** -20))),     # t near 1
    'lone_inside': lambda: _lone(True),
    'lone_outside': lambda: _lone(False),
    'weight_edge_1': lambda: _weight_edge(1),
    'weight_edge_3': lambda: _weight_edge(3),
    # the cell at the node (0, 0, 0) has no voxel; its neighbours (-1, 0, 0) and (1, 0, 0) are met at d = 12 and d = 14 of the scan
    'label_tie_later_smaller': lambda: _labels([(1, 0, 0), (-1, 0, 0)], [3, 3]),           # row 1 met first, row 0 later: the tie goes to row 0
    'label_tie_later_larger': lambda: _labels([(-1, 0, 0), (1, 0, 0)], [3, 3]),            # row 0 met first and kept
    'label_fuller_larger_row': lambda: _labels([(-1, 0, 0), (1, 0, 0)], [2, 5]),           # row 1 is fuller
    'label_none': lambda: _labels([(0, 0, 0)], [4], band=3),                               # cells two steps from the only voxel: id 0, colour 0
    'sum_order': _sum_order,
    'random_big': lambda: _big(11, 1),
    'random_big_min3': lambda: _big(12, 3),
    'ball': _ball,
    'wg_gap': _wg_gap,
    # one face-bearing node at a chosen rank (the filler in front has rank - corner nodes): 3 | 4, 255 | 256, 1023 | 1024, and in the last, partial lane
    'single_a': lambda: _gadgets([('edge', (2, 3)), ('flat', 255 - 18), ('edge', (0, 0)), ('flat', 1023 - 273 - 1), ('edge', (1, 1)), ('flat', 15)]),
    'single_b': lambda: _gadgets([('edge', (0, 4)), ('flat', 256 - 18), ('edge', (0, 0)), ('flat', 1024 - 274), ('edge', (0, 0)), ('flat', 15)]),
    'single_lane0': lambda: _gadgets([('flat', 1024), ('edge', (0, 0)), ('flat', 8)]),     # the only face-bearing node is the first of the second workgroup
    'single_lane255': lambda: _gadgets([('flat', 1020), ('edge', (2, 3)), ('flat', 16)]),  # ... the last of the first, the second has none
    # lanes whose four nodes all have mask 7: ranks 0 .. 7, 252 .. 259, 1020 .. 1027, and the last node, alone in its lane
    'full_lanes': lambda: _gadgets([('full8', None), ('flat', 252 - 64), ('full8', None), ('flat', 1020 - 316), ('full8', None), ('flat', 8), ('last7', None)]),
}
for _N in NODE_COUNTS:                                                                     # the counted tables: vertices, no faces
    EXTRACT['count_%d' % _N] = (lambda N: lambda: _case(counted(N, **NODE_COUNTS[N]), sdf=lambda t: checker(t.nodes)))(_N)
CLOSED = ('plane_pos_zero', 'plane_neg_zero', 'lone_inside', 'lone_outside', 'ball')       # fields with one sheet: sane topology, outward winding


@functools.lru_cache(maxsize=None)
def extract_case(name):
    return EXTRACT[name]()


@functools.lru_cache(maxsize=None)
def extract_ref(name):
    c = extract_case(name)
    return T.extract(c['tab'], c['sdf'], c['weight'], c['min_weight'], c['count'], c['pan'], c['colors'], c['vs'])


def winding(case, ref_or_got):
    """per face: its normal dotted with the gradient of the case's field at its centroid (> 0: the normal points from inside to outside)"""
    v = np.asarray(ref_or_got['vertices'], dtype=np.float64)
    f = np.asarray(ref_or_got['faces'], dtype=np.int64)
    centroid = v[f].mean(axis=1) / float(case['vs'])                                      # in node units
    return (T.face_normals(v, f) * case['gradient'](centroid)).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------- planted mistakes
NODE_MISTAKES = ('offset_minus_band', 'offset_z_fastest')
INTEGRATE_MISTAKES = ('occluded_le', 'no_clamp', 'floor_u', 'px_le_W', 'zc_gt_near', 'sum_descending', 'reciprocal')
EXTRACT_MISTAKES = ('inside_le', 'valid_gt', 't_upper', 'edge_order_yzx', 'fp32_crossings', 'tie_larger_row', 'scan_ge', 'q1_q3', 'no_flip', 'face_id_corner0',
                    'axis_major')


def v_nodes(cells, band, m=None):
    """-> (nodes int64 [Nn, 3], voxel_row int64 [Nn])"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    o = offsets(band, z_fastest=m == 'offset_z_fastest', shift=0 if m == 'offset_minus_band' else 1)
    pairs = (cells[:, None, :] + o[None]).reshape(-1, 3)
    k = T.keys_of(pairs)
    sk, first = np.unique(k, return_index=True)
    nodes = pairs[np.sort(first)]
    rank = {int(key): i for i, key in enumerate(T.keys_of(nodes))}
    voxel_row = np.full(len(nodes), -1, dtype=np.int64)
    for row, key in enumerate(T.keys_of(cells)):
        voxel_row[rank[int(key)]] = row
    return nodes, voxel_row


def v_integrate(case, m=None):
    """-> (sdf float32 [Nn], weight int32 [Nn])"""
    vs, band = F(case['vs']), case['band']
    tau = F(F(band) * vs)
    p = (case['nodes'].astype(F) * vs).astype(F)
    S, W = np.zeros(len(p), dtype=F), np.zeros(len(p), dtype=np.int32)
    order = range(len(case['dims']))
    for j in (reversed(order) if m == 'sum_descending' else order):
        H, Wd = (int(x) for x in case['dims'][j])
        if H < 1 or Wd < 1 or H * Wd > case['npix'][j]:
            continue
        cam, depth = case['cams'][j], case['depths'][j]
        with np.errstate(all='ignore'):
            xc, yc, zc = (((cam[4 * a] * p[:, 0] + cam[4 * a + 1] * p[:, 1]) + cam[4 * a + 2] * p[:, 2]) + cam[4 * a + 3] for a in range(3))
            ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & ((zc > cam[15]) if m == 'zc_gt_near' else (zc >= cam[15]))
            zs = np.where(ok, zc, F(1))
            u = ((cam[12] * xc).astype(np.float64) / zs.astype(np.float64)).astype(F) + cam[13]
            v = ((cam[12] * yc).astype(np.float64) / zs.astype(np.float64)).astype(F) + cam[14]
            ok &= (np.abs(u) <= F(LIM)) & (np.abs(v) <= F(LIM))
            half = F(0) if m == 'floor_u' else F(0.5)
            px = np.floor(np.where(ok, u, F(0)) + half).astype(np.int64)
            py = np.floor(np.where(ok, v, F(0)) + F(0.5)).astype(np.int64)
            ok &= (px >= 0) & ((px <= Wd) if m == 'px_le_W' else (px < Wd)) & (py >= 0) & (py < H)
            d = np.where(ok, depth[np.minimum(np.where(ok, py * Wd + px, 0), len(depth) - 1)], F(0)).astype(F)
            s = (d - zc).astype(F)
            use = ok & (d != 0) & ~((s <= -tau) if m == 'occluded_le' else (s < -tau))
            S = np.where(use, (S + (s if m == 'no_clamp' else np.minimum(s, tau))).astype(F), S)
        W += use
    with np.errstate(all='ignore'):
        q = (S * (F(1) / W.astype(F))).astype(F) if m == 'reciprocal' else (S / W.astype(F)).astype(F)
    return np.where(W > 0, q, F(0)).astype(F), W


def v_extract(case, m=None):
    """-> dict(vertices, vertex_ids, colors, faces, face_ids, edge, cell_vertex)"""
    tab, sdf, weight, mw = case['tab'], case['sdf'], case['weight'], case['min_weight']
    Nn = len(tab)
    inside = (sdf <= 0) if m == 'inside_le' else (sdf < 0)
    valid = (weight > mw) if m == 'valid_gt' else (weight >= mw)
    q = np.stack([tab.rank(tab.nodes + c) for c in T.CORNERS], axis=1)
    qq = np.maximum(q, 0)
    n_in = inside[qq].sum(axis=1)
    is_cell = (q >= 0).all(axis=1) & valid[qq].all(axis=1) & (n_in > 0) & (n_in < 8)
    rows = np.nonzero(is_cell)[0]
    cell_vertex = np.full(Nn, -1, dtype=np.int64)
    cell_vertex[rows] = np.arange(len(rows))
    # vertices
    D, I = sdf[q[rows]].reshape(-1, 8), inside[q[rows]].reshape(-1, 8)
    wide = F if m == 'fp32_crossings' else np.float64
    total, num = np.zeros((len(rows), 3), dtype=wide), np.zeros(len(rows), dtype=np.int64)
    for a in ((1, 2, 0) if m == 'edge_order_yzx' else (0, 1, 2)):
        b, c = (a + 1) % 3, (a + 2) % 3
        for e in range(4):
            ob, oc = e & 1, e >> 1
            lo = (ob << b) | (oc << c)
            hi = lo | (1 << a)
            Da, Db = D[:, lo].astype(wide), D[:, hi].astype(wide)
            cross = I[:, lo] != I[:, hi]
            with np.errstate(all='ignore'):
                t = Db / (Db - Da) if m == 't_upper' else Da / (Da - Db)
            pos = np.zeros((len(rows), 3), dtype=wide)
            pos[:, a], pos[:, b], pos[:, c] = t, ob, oc
            total = np.where(cross[:, None], total + pos, total)
            num += cross
    mean = total / np.maximum(num, 1).astype(wide)[:, None]
    vertices = ((tab.nodes[rows].astype(wide) + mean) * wide(F(case['vs']))).astype(F)
    # labels
    own = tab.voxel_row[rows]
    best, best_n = np.full(len(rows), -1, dtype=np.int64), np.zeros(len(rows), dtype=np.int64)
    for d in range(27):
        if d == 13:
            continue
        g = tab.rank(tab.nodes[rows] + np.array([d % 3 - 1, (d // 3) % 3 - 1, d // 9 - 1]))
        w = np.where(g >= 0, tab.voxel_row[np.maximum(g, 0)], -1)
        n = np.where(w >= 0, case['count'].astype(np.int64)[np.maximum(w, 0)], 0)
        if m == 'scan_ge':
            better = n >= best_n
        else:
            better = (n > best_n) | ((n == best_n) & ((w > best) if m == 'tie_larger_row' else (w < best)))
        take = (w >= 0) & ((best < 0) | better)
        best, best_n = np.where(take, w, best), np.where(take, n, best_n)
    w = np.where(own >= 0, own, best)
    vertex_ids = np.where(w >= 0, case['pan'][np.maximum(w, 0)], 0).astype(np.int32)
    colors = np.where((w >= 0)[:, None], case['colors'][np.maximum(w, 0)], F(0)).astype(F).reshape(-1, 3)
    # faces
    edge_cells = [(0, 0), (0, -1), (-1, -1), (-1, 0)] if m == 'q1_q3' else T.EDGE_CELLS
    keys, tris = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = np.zeros(3, dtype=np.int64)
        e[a] = 1
        g = tab.rank(tab.nodes + e)
        gg = np.maximum(g, 0)
        emit = valid & (g >= 0) & valid[gg] & (inside != inside[gg])
        v = []
        for ob, oc in edge_cells:
            o = np.zeros(3, dtype=np.int64)
            o[b], o[c] = ob, oc
            h = tab.rank(tab.nodes + o)
            cv = np.where(h >= 0, cell_vertex[np.maximum(h, 0)], -1)
            emit &= cv >= 0
            v.append(cv)
        r = np.nonzero(emit)[0]
        v = [x[r] for x in v]
        ins = np.ones(len(r), dtype=bool) if m == 'no_flip' else inside[r]
        first = np.stack([v[0], np.where(ins, v[1], v[2]), np.where(ins, v[2], v[1])], axis=1)
        second = np.stack([v[0], np.where(ins, v[2], v[3]), np.where(ins, v[3], v[2])], axis=1)
        keys.append(np.repeat(3 * r + a, 2))
        tris.append(np.stack([first, second], axis=1).reshape(-1, 3))
    edge, faces = np.concatenate(keys).astype(np.int64), np.concatenate(tris).astype(np.int32).reshape(-1, 3)
    order = np.argsort((edge % 3) * (3 * Nn) + edge // 3 if m == 'axis_major' else edge, kind='stable')
    edge, faces = edge[order], faces[order]
    if m == 'face_id_corner0':
        face_ids = vertex_ids[faces[:, 0]].astype(np.int32)
    else:
        face_ids = T.face_id(vertex_ids[faces[:, 0]], vertex_ids[faces[:, 1]], vertex_ids[faces[:, 2]]) if len(faces) else np.zeros(0, dtype=np.int32)
    return {'vertices': vertices, 'vertex_ids': vertex_ids, 'colors': colors, 'faces': faces, 'face_ids': face_ids, 'edge': edge, 'cell_vertex': cell_vertex}


EXTRACT_FIELDS = (('vertices', F), ('vertex_ids', np.int32), ('colors', F), ('faces', np.int32), ('face_ids', np.int32), ('edge', np.int64), ('cell_vertex', np.int64))


def same_extract(a, b):
    """the names of the fields in which two extraction results differ (bit for bit)"""
    return [k for k, dt in EXTRACT_FIELDS if not G.same_bits(np.asarray(a[k]).astype(dt, copy=False), np.asarray(b[k]).astype(dt, copy=False))]
