"""Shared by tests/test_hip_geom_stages.py (GPU) and tests/test_geom_stage_checks.py (CPU): the cases and the numpy references that hold the kernels of
csrc/cloud.hip (count, scan, compact, segment median) and csrc/voxel.hip (with the table of csrc/voxel_table.h) to their contract stage by stage, at the
value classes and alignments where such kernels go wrong, and the two other users of the workgroup rank of csrc/wave_ops.h - the component ranks of
csrc/components.hip (four rows per lane) and the face compaction of csrc/surface.hip (one face per lane) - at the wave and workgroup edges of that rank.
Nothing here imports the code under test.

The references are the restatements the end-to-end tests already use (cloud_ref.cloud, cloud_ref.median_two_stat, voxel_ref.voxelize) plus `scan_ref`.
Every comparison is bit for bit; where the reference is NaN the result must be NaN (sign and payload of a NaN are not part of the contract).

`radix_select` emulates the four byte passes of pst_cloud_segment_median, with four planted mistakes as variants: the CPU module asserts which median
case catches which mistake, so the value classes are known to bite before a GPU sees them.  `vx_hash` / `vx_key` restate the table's hash, so that
cells and (rank, id) pairs with a chosen home slot can be planted: a probe chain that wraps from the last slot to slot 0, at load factor 1 / 2."""
import numpy as np

import cloud_ref
import voxel_ref

F = np.float32
LIM = 1 << 20
WG = 1024                                   # points per workgroup of the count / compact / rank passes (CL_WG, VX_WG)


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint32)).view(F)


def same_bits(got, ref):
    """bit for bit, except that a NaN of the reference only asks for a NaN"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return False
    if ref.dtype.kind != 'f':
        return bool(np.array_equal(got, ref))
    n = np.isnan(ref)
    if not np.array_equal(np.isnan(got), n):
        return False
    u = {4: np.uint32, 8: np.uint64}[ref.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(got).view(u)[~n], np.ascontiguousarray(ref).view(u)[~n]))


def first_difference(got, ref):
    """for an assertion message: where two arrays that are not `same_bits` part"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return 'shape %s != %s' % (got.shape, ref.shape)
    with np.errstate(invalid='ignore'):
        bad = ~((got == ref) | (np.isnan(got.astype(np.float64)) & np.isnan(ref.astype(np.float64))))
    if ref.dtype.kind == 'f':
        bad |= (np.signbit(got) != np.signbit(ref)) & ~np.isnan(ref)
    i = np.argwhere(bad)
    if len(i) == 0:
        return 'no difference'
    j = tuple(i[0])
    return '%d elements differ, first at %s: got %r, want %r' % (len(i), j, got[j], ref[j])


# ---------------------------------------------------------------------------------------------------------------------------------------------- scan
SCAN_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000]      # the 64-lane wave and the 1024-count round, each exact, - 1 and + 1
SCAN_ZEROS = (0, 1023, 1024)                                                # ... and n - 1: counts forced to 0 at a round's last and first index


def scan_counts(n, seed=0):
    g = np.random.Generator(np.random.PCG64(1000 + seed + n))
    c = g.integers(0, 1025, n).astype(np.int32)
    for i in SCAN_ZEROS + (n - 1,):
        if 0 <= i < n:
            c[i] = 0
    return c


def scan_big():
    """2047 counts of 2^20: the total, 2^31 - 2^20, is the largest such that stays below 2^31"""
    return np.full(2047, 1 << 20, dtype=np.int32)


def scan_ref(counts):
    """int32 [n + 1]: the exclusive prefix sums, the total appended"""
    s = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    assert s[-1] < 2 ** 31
    return s.astype(np.int32)


# -------------------------------------------------------------------------------------------------------------------------------------------- median
def median_cases():
    """name -> float32 array: one segment's values on one axis"""
    g = np.random.Generator(np.random.PCG64(77))
    one = 0x3f800000
    sh = lambda a: a[g.permutation(len(a))]
    nan, inf = np.nan, np.inf
    c = {
        'ties_all_equal': [1.5] * 10,
        'ties_half': [1, 2, 1, 2, 2, 1, 1, 2, 2, 1],
        'straddle_zero_even': [5, -1e-3, -3, 2e-3],
        'neg_only': -(np.abs(g.standard_normal(1000)) * 3 + 1e-3),
        'neg_zero_pos_zero': [-0.0, 0.0],
        'zeros_mixed': [0.0, -1, -0.0, 1, -0.0, 0.0],
        'denormals': [1e-45, -1e-45, 3e-45, 1e-40, -1e-40, 0.0, -0.0, 1e-38],
        'denormal_pair': from_bits([3, 5]),                               # (a + b) * 0.5f = bits 4: a flushed sum gives 0
        'denormal_odd': from_bits([7, 0x80000002, 9, 1, 0x00400000]),
        'low_byte_only': sh(from_bits(one + np.arange(300))),            # the two middle ones share three leading key bytes
        'mid_bytes': sh(from_bits(one + 256 * np.arange(300))),          # ... two
        'share_one_byte': sh(from_bits(one + 65536 * np.arange(100))),   # ... one
        'two_bins': [1e10, 1, 2, 1.9999999],                              # ... none: 0x3fffffff | 0x40000000
        'inf': [inf, 1, inf, -inf, 2, inf],
        'inf_pm': [-inf, inf],
        'fmax': [3.4e38, 3.3e38, 3.40282e38, 3.39e38],
        'single': [2.5],
        'pair': [0.7, 0.1],
        'with_nan': [1, 2, nan, 3, 4],
        'with_neg_nan': from_bits([0x3f800000, 0xffc00001, 0x40000000]),  # a NaN with the sign bit set: its key sorts below every number
        'random_even': g.standard_normal(4096) * 3,
        'random_odd': g.standard_normal(4097) * 3,
    }
    return {k: np.asarray(v, dtype=F) for k, v in c.items()}


RANDOM_CASES = ('random_even', 'random_odd', 'neg_only')
VARIANTS = ('sign_flip_only', 'one_prefix', 'upper_only', 'ge_walk')


def median_ref(x):
    with np.errstate(over='ignore', invalid='ignore'):
        return F(cloud_ref.median_two_stat(x))


def radix_select(x, variant=None):
    """the four passes of pst_cloud_segment_median on one (segment, axis): a 256-bin histogram of byte 3 - pass of the keys whose higher bytes equal
    the rank's prefix, a walk to the first bin whose inclusive count exceeds the rank, two ranks ((n - 1) / 2 and n / 2) with a prefix each.
    variants: 'sign_flip_only' key = bits ^ 0x80000000 (negative floats in reverse order); 'one_prefix' both ranks' histograms filtered by rank 0's
    prefix; 'upper_only' rank n / 2 for both; 'ge_walk' the first bin whose inclusive count is >= the rank."""
    assert variant is None or variant in VARIANTS
    u = f32_bits(x).reshape(-1)
    n = len(u)
    top = np.uint32(0x80000000)
    if variant == 'sign_flip_only':
        key = u ^ top
        unkey = lambda k: np.uint32(k) ^ top
    else:
        key = np.where(u & top, ~u, u | top).astype(np.uint32)
        unkey = lambda k: (np.uint32(k) & np.uint32(0x7fffffff)) if (np.uint32(k) & top) else ~np.uint32(k)
    has_nan = bool(((u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)).any())
    rank = [n // 2 if variant == 'upper_only' else (n - 1) // 2 if n else 0, n // 2]
    prefix = [0, 0]
    for p in range(4):
        shift = 24 - 8 * p
        new = list(prefix)
        for j in range(2):
            if p == 0:
                sel = np.ones(n, dtype=bool)
            else:
                sel = (key >> np.uint32(shift + 8)) == np.uint32(prefix[0 if variant == 'one_prefix' else j] >> (shift + 8))
            hist = np.bincount(((key[sel] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
            cum = np.cumsum(hist)
            hit = (cum >= rank[j]) if variant == 'ge_walk' else (cum > rank[j])
            if hit.any():
                b = int(np.argmax(hit))
                new[j], rank[j] = prefix[j] | (b << shift), int(rank[j] - (cum[b] - hist[b]))
            else:
                rank[j] = 0                                                  # an empty histogram: bin 0, as the kernel's max(bin, 0)
        prefix = new
    if n == 0 or has_nan:
        return F(np.nan)
    a, b = from_bits([unkey(prefix[0])])[0], from_bits([unkey(prefix[1])])[0]
    with np.errstate(over='ignore', invalid='ignore'):
        return a if n % 2 else F(F(a + b) * F(0.5))


def median_segments(S, M, seed=0):
    """S segments in one call: segment s holds case (3 s + a) mod N on axis a (cut or repeated to the length of its axis-0 case), its rows spread over
    the M rows of the cloud by a seeded permutation.  The segments' ids go through an id2row that permutes the rows and holds a -1 entry; the other
    rows carry ids that take part in nothing (0, -5, ntab and the id whose row is -1) and large values.
    -> points [M, 3], pan [M], id2row [ntab], want_count [S], want_median [S, 3]"""
    cases = list(median_cases().values())
    N = len(cases)
    g = np.random.Generator(np.random.PCG64(500 + 31 * S + seed))
    ntab = S + 2
    ids = g.permutation(S + 1) + 1                                           # ids 1 .. S + 1: the last of the draw is the id without a row
    id2row = np.full(ntab, -1, dtype=np.int32)
    id2row[ids[:S]] = np.arange(S, dtype=np.int32)
    dead = (0, -5, ntab, int(ids[S]))
    pts, pan, count, med = [], [], np.zeros(S, np.int32), np.zeros((S, 3), F)
    for s in range(S):
        cols = [cases[(3 * s + a) % N] for a in range(3)]
        n = len(cols[0])
        seg = np.stack([cols[0]] + [np.resize(c, n) for c in cols[1:]], axis=1).astype(F)
        pts.append(seg)
        pan.append(np.full(n, ids[s], dtype=np.int32))
        count[s] = n
        med[s] = [median_ref(seg[:, a]) for a in range(3)]
    live = sum(len(p) for p in pan)
    assert live <= M
    pts.append((g.standard_normal((M - live, 3)) * 1e6).astype(F))
    pan.append(np.asarray(dead, dtype=np.int32)[g.integers(0, len(dead), M - live)])
    order = g.permutation(M)
    return np.concatenate(pts)[order], np.concatenate(pan)[order], id2row, count, med


# ---------------------------------------------------------------------------------------------------------------------------- the table's hash and key
def vx_hash(keys):
    k = np.array(keys, dtype=np.uint64).reshape(-1)
    with np.errstate(over='ignore'):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def vx_key(cells):
    c = (np.asarray(cells, dtype=np.int64).reshape(-1, 3) + LIM).astype(np.uint64)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


def home_slot(keys, cap):
    return (vx_hash(keys) & np.uint64(0xffffffff) & np.uint64(cap - 1)).astype(np.int64)


def lattice():
    """the 64^3 cells with every coordinate in [-32, 32), x fastest"""
    r = np.arange(-32, 32)
    z, y, x = np.meshgrid(r, r, r, indexing='ij')
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def colliding_cells(cap, home, n=None):
    """the first n cells of the lattice (all of them for n = None) whose home slot in a table of `cap` slots is `home`"""
    cells = lattice()
    hit = cells[home_slot(vx_key(cells), cap) == home]
    assert n is None or len(hit) >= n
    return hit if n is None else hit[:n]


def pair_key(rank, pid):
    return (np.asarray(rank, dtype=np.uint64) << np.uint64(32)) | np.asarray(pid, dtype=np.uint64)


def colliding_pairs(cap, home, ranks, max_id):
    """[(rank, id)]: for every rank that has one, the smallest id in [1, max_id) whose pair key (rank << 32) | id has home slot `home`"""
    ids = np.arange(1, max_id, dtype=np.uint64)
    out = []
    for r in ranks:
        hit = np.nonzero(home_slot(pair_key(np.full(len(ids), r), ids), cap) == home)[0]
        if len(hit):
            out.append((int(r), int(ids[hit[0]])))
    return out


# --------------------------------------------------------------------------------------------------------------------------------------------- voxel
def offsets_q(points, voxel_size):
    """(c int64 [M, 3], q int64 [M, 3], keep [M]) of steps 1 and 2 of the voxel contract"""
    t, c, keep = voxel_ref.cells(points, voxel_size)
    with np.errstate(invalid='ignore'):
        q = np.floor(((t - c).astype(F) * F(65536)).astype(F))
    q = np.where(keep[:, None], q, 0).astype(np.int64)
    return np.where(keep[:, None], c, 0).astype(np.int64), q, keep


def _table(g, n):
    c = g.uniform(0, 1, (n, 3)).astype(F)
    c[0] = 0
    return c


def _case(g, points, pan, segment_ids, voxel_size, ncolors, rgb=None, opacity=0.3, **extra):
    M = len(points)
    rgb = g.uniform(0, 1, (M, 3)).astype(F) if rgb is None else np.asarray(rgb, dtype=F)
    d = dict(points=np.asarray(points, dtype=F), rgb=rgb, pan=np.asarray(pan, dtype=np.int32), index=(np.arange(M, dtype=np.int64) * 3 + 7)[::-1].copy(),
             segment_ids=[int(i) for i in segment_ids], voxel_size=voxel_size, colors=_table(g, ncolors), opacity=opacity)
    d.update(extra)
    return d


def _exact_points(g, cells, denom=1024):
    """(cell + k / denom) * 0.25 for a seeded k in [0, denom): exact in float32, so the cell of every point is the planted one"""
    cells = np.asarray(cells, dtype=np.int64)
    k = g.integers(0, denom, cells.shape)
    return ((cells + k / denom) * 0.25).astype(F)


def cell_edge_values(vs):
    """the 1-D coordinates of `cell_edges`: (small, kept_extremes, dropped_extremes)"""
    k = np.arange(-50, 51)
    on = (k * vs).astype(F)
    small = np.concatenate([on, np.nextafter(on, F(-np.inf)), np.nextafter(on, F(np.inf)), np.asarray([1e-12, -1e-12, 0.0, -0.0], dtype=F)])
    kept = np.asarray([(LIM - 0.5) * vs, -(LIM - 1.5) * vs], dtype=F)        # cells 2^20 - 1 and -(2^20 - 1): the last ones inside
    dropped = np.asarray([(LIM + 0.5) * vs, -(LIM - 0.5) * vs], dtype=F)     # cells 2^20 and -2^20: the first ones outside
    return small, kept, dropped


def _cell_edges(vs):
    g = np.random.Generator(np.random.PCG64(int(vs * 1000)))
    small, kept, dropped = cell_edge_values(vs)
    n = len(small)
    pts = np.stack([small, small[(np.arange(n) * 7 + 3) % n], small[(np.arange(n) * 11 + 5) % n]], axis=1)
    for a in range(3):
        pts[a::3] = np.roll(pts[a::3], a, axis=1)                            # the walk through the values runs along every axis in turn
    ext = []
    for v in np.concatenate([kept, dropped, np.asarray([np.nan, np.inf, -np.inf, 3.4e38], dtype=F)]):
        for a in range(3):
            p = small[[5, 160, 290]].copy()
            p[a] = v
            ext.append(p)
    pts = np.concatenate([pts, np.asarray(ext, dtype=F)])
    pts = pts[g.permutation(len(pts))]
    return _case(g, pts, g.integers(0, 6, len(pts)), range(1, 6), vs, 6, dropped=3 * (len(dropped) + 4), kept_extremes=kept, dropped_extremes=dropped)


def _load_half():
    g = np.random.Generator(np.random.PCG64(11))
    cap, home, M = 1024, 1023, 512
    hit = colliding_cells(cap, home, 200)
    lat = lattice()
    rest = lat[home_slot(vx_key(lat), cap) != home]
    cells = np.concatenate([hit, rest[g.choice(len(rest), M - len(hit), replace=False)]])[g.permutation(M)]
    # every cell is its own voxel and the voxels come in row order: the rank of row r is r
    pan = g.integers(1, 4096, M)
    planted = colliding_pairs(cap, home, range(M), 4096)[:24]
    for r, i in planted:
        pan[r] = i
    return _case(g, _exact_points(g, cells), pan, sorted(set(int(p) for p in pan)), 0.25, 4096, dropped=0, cap=cap, home=home, cells=cells, planted_pairs=planted)


RUNS = {'wave': (60, 71), 'workgroup': (250, 261), 'rank_group': (1020, 1031)}      # rows [a, b) of one cell: 63 | 64, 255 | 256, 1023 | 1024
RUN_INTERLEAVE, RUN_WAVE, RUN_FAR = (128, 160), (320, 384), (500, 3500)


def _runs():
    g = np.random.Generator(np.random.PCG64(12))
    M = 4200
    cells = np.stack([np.arange(M) - 2100, np.full(M, 5), np.full(M, -3)], axis=1)       # every row its own cell ...
    for n, (a, b) in enumerate(RUNS.values()):
        cells[a:b] = (n, 100, 0)                                                         # ... but the runs
    a, b = RUN_INTERLEAVE
    cells[a:b:2], cells[a + 1:b:2] = (0, 101, 0), (1, 101, 0)
    a, b = RUN_WAVE
    cells[a:b] = (0, 102, -1)
    cells[list(RUN_FAR)] = (0, 103, 0)
    pan = g.integers(0, 7, M)
    pan[a:b] = np.resize([1, 1, 2, 2, 1, 0, 1], b - a)                                   # the voxel run is the wave, the pair runs are not
    return _case(g, _exact_points(g, cells), pan, range(1, 7), 0.25, 7, dropped=0, cells=cells)


VOTE_VOXELS = {                     # name -> (ids of its points in row order, winner, votes); segment table {1, 2, 3, 5, 9}, 6 colours, ntab = 10
    'tie_3_3': ([3, 2, 3, 2, 2, 3], 2, 3),
    'tie_2_2_1': ([5, 1, 3, 5, 1], 1, 2),
    'void_only': ([0, -4, 10, 4], 0, 4),            # void, negative, ntab, and 4: in range but without a row
    'beyond_colours': ([9, 1, 9], 9, 2),
    'void_majority': ([0, 0, 4, 2, 0], 2, 1),       # void only wins alone
}
VOTE_IDS, VOTE_NCOLORS = [1, 2, 3, 5, 9], 6


def _votes():
    g = np.random.Generator(np.random.PCG64(13))
    cells, pan = [], []
    for n, (ids, _, _) in enumerate(VOTE_VOXELS.values()):
        cells += [(n - 2, 3 * n - 5, 0)] * len(ids)
        pan += ids
    return _case(g, _exact_points(g, cells), pan, VOTE_IDS, 0.25, VOTE_NCOLORS, dropped=0)


BIG_N = 70000


def _big_voxel():
    g = np.random.Generator(np.random.PCG64(14))
    k = g.integers(1, 9, (BIG_N, 3))                                         # offsets 65536 - k: the sums pass 2^32 (70 000 x 65 528 = 4.59e9)
    pts = ((np.asarray([3, -2, 7]) + (65536 - k) / 65536) * 0.25).astype(F)
    pts = np.concatenate([pts[:40000], _exact_points(g, [(-9, 0, 1)]), pts[40000:]])
    return _case(g, pts, g.integers(1, 4, len(pts)), range(1, 4), 0.25, 4, dropped=0)


def colour_values():
    s = [np.nan, -0.0, -1.0, 2.0, np.inf, -np.inf, 0.0, 1.0]
    for k in (0, 1, 127, 128, 253, 254):
        v = F((k + 0.5) / 255)
        s += [v, np.nextafter(v, F(-1)), np.nextafter(v, F(2))]
    return np.asarray(s, dtype=F)


def _colours():
    g = np.random.Generator(np.random.PCG64(15))
    s = colour_values()
    n = len(s)
    i = np.arange(3 * n)
    rgb = np.stack([s[i % n], s[(i + 5) % n], s[(2 * i + 11) % n]], axis=1)
    cells = np.stack([i // 3 - 10, i // 3 % 2, np.zeros_like(i)], axis=1)   # three points per voxel: the means mix the classes
    return _case(g, _exact_points(g, cells), g.integers(0, 4, len(i)), range(1, 4), 0.25, 4, rgb=rgb, dropped=0)


CELL_EDGE_SIZES = (0.05, 0.07, 0.25)
_VOXEL = {}


def voxel_cases():
    """name -> dict(points, rgb, pan, index, segment_ids, voxel_size, colors, opacity, dropped = the planted number of points left out, ...)"""
    if not _VOXEL:
        for vs in CELL_EDGE_SIZES:
            _VOXEL['cell_edges_%g' % vs] = _cell_edges(vs)
        _VOXEL.update(load_half=_load_half(), runs=_runs(), votes=_votes(), big_voxel=_big_voxel(), colours=_colours())
    return _VOXEL


_VOXEL_REF = {}


def voxel_reference(name):
    """voxel_ref.voxelize of a case, computed once"""
    if name not in _VOXEL_REF:
        c = voxel_cases()[name]
        _VOXEL_REF[name] = voxel_ref.voxelize(c['points'], c['rgb'], c['pan'], c['index'], c['segment_ids'], c['voxel_size'], c['colors'], c['opacity'])
    return _VOXEL_REF[name]


VOXEL_FIELDS = ('points', 'rgb', 'pan', 'colors', 'count', 'votes', 'first_index', 'point_voxel')


def assert_voxel_case(name):
    """the case holds what it was built for, on voxel_ref alone"""
    c, r = voxel_cases()[name], voxel_reference(name)
    pv, M = r['point_voxel'], len(c['pan'])
    assert r['dropped'] == c['dropped'] == int((pv < 0).sum()), (name, r['dropped'])
    assert int(r['count'].sum()) == M - r['dropped']
    if name.startswith('cell_edges'):
        cell, q, keep = offsets_q(c['points'], c['voxel_size'])
        assert (q[keep] >= 0).all() and (q[keep] <= 65536).all()
        assert ((q == 65536) & keep[:, None]).any(), 'no point with an offset of exactly one cell'
        assert ((cell == -1) & (q == 65536)).any() and (cell[keep] < 0).any() and (cell[keep] >= 0).any() and ((cell == 0) & (q == 0) & keep[:, None]).any()
        assert (cell[keep].max() == LIM - 1) and (cell[keep].min() == -(LIM - 1)), 'the last kept cells are missing'
        inv = F(1.0 / c['voxel_size'])
        assert list(np.floor(c['dropped_extremes'] * inv)) == [LIM, -LIM] and list(np.floor(c['kept_extremes'] * inv)) == [LIM - 1, -(LIM - 1)]
        small = cell_edge_values(c['voxel_size'])[0]
        t, k = np.floor(small * inv), np.arange(-50, 51)
        assert (t[:101] == k).any() and (t[101:202] == k - 1).any() and (t[202:303] == k).any(), 'the walk does not sit on the cell faces'
    elif name == 'load_half':
        cap, home = c['cap'], c['home']
        assert M * 2 == cap and len(r['pan']) == M and (r['count'] == 1).all() and np.array_equal(pv, np.arange(M))
        cell = offsets_q(c['points'], 0.25)[0]
        assert np.array_equal(cell, c['cells'])
        assert int((home_slot(vx_key(cell), cap) == home).sum()) >= 200
        pairs = pair_key(pv, c['pan'])
        assert len(np.unique(pairs)) == M and int((home_slot(pairs, cap) == home).sum()) >= 20
        assert np.array_equal(r['pan'], c['pan']) and (r['votes'] == 1).all()
    elif name == 'runs':
        for a, b in RUNS.values():
            assert (pv[a:b] == pv[a]).all() and pv[a - 1] != pv[a] and pv[b] != pv[a] and r['count'][pv[a]] == b - a
        assert RUNS['wave'][0] <= 63 < 64 < RUNS['wave'][1] and RUNS['workgroup'][0] <= 255 < 256 < RUNS['workgroup'][1]
        assert RUNS['rank_group'][0] <= 1023 < 1024 < RUNS['rank_group'][1]
        a, b = RUN_INTERLEAVE
        assert (pv[a:b:2] == pv[a]).all() and (pv[a + 1:b:2] == pv[a + 1]).all() and pv[a] != pv[a + 1]
        a, b = RUN_WAVE
        assert a % 64 == 0 and b - a == 64 and (pv[a:b] == pv[a]).all() and len(np.unique(c['pan'][a:b])) == 3 and (np.diff(c['pan'][a:b]) != 0).sum() > 20
        assert r['pan'][pv[a]] == 1
        a, b = RUN_FAR
        assert pv[a] == pv[b] and a // WG != b // WG and r['count'][pv[a]] == 2
    elif name == 'votes':
        row = 0
        assert len(r['pan']) == len(VOTE_VOXELS)
        for v, (ids, winner, votes) in enumerate(VOTE_VOXELS.values()):
            assert (pv[row:row + len(ids)] == v).all() and r['pan'][v] == winner and r['votes'][v] == votes and r['count'][v] == len(ids), (v, ids)
            row += len(ids)
        v = list(VOTE_VOXELS).index('tie_3_3')
        ids = VOTE_VOXELS['tie_3_3'][0]
        assert ids.count(2) == ids.count(3) == 3 and r['pan'][v] == 2
        v = list(VOTE_VOXELS).index('void_only')
        assert r['pan'][v] == 0 and r['votes'][v] == r['count'][v]
        v = list(VOTE_VOXELS).index('beyond_colours')
        assert r['pan'][v] == 9 >= VOTE_NCOLORS and same_bits(r['colors'][v], cloud_ref.blend(r['rgb'][v], np.zeros(3, F), c['opacity']))
    elif name == 'big_voxel':
        cell, q, keep = offsets_q(c['points'], 0.25)
        assert keep.all() and len(r['pan']) == 2 and list(r['count']) == [BIG_N, 1]
        assert (q[pv == 0].sum(axis=0) > 2 ** 32).all()
    elif name == 'colours':
        g = c['rgb']
        assert np.isnan(g).any() and np.isinf(g).any() and (g < 0).any() and (g > 1).any() and (np.signbit(g) & (g == 0)).any()
        with np.errstate(invalid='ignore'):
            u = np.floor(np.clip(np.where(np.isnan(g), F(0), g), F(0), F(1)) * F(255) + F(0.5))
        for k in (0, 1, 127, 128, 253, 254):                                 # the ulp below (k + 0.5) / 255 and the ulp above fall on two sides
            assert (u == k).any() and (u == k + 1).any()
        assert (r['count'] == 3).all()


# --------------------------------------------------------------------------------------------------------------------------------------------- cloud
CLOUD_NPIX = [1, 3, 4, 5, 1023, 1024, 1025, 2049]       # one-point view, the scalar path alone, one vector load, + 1, the workgroup exact and +- 1, three workgroups
CLOUD_THRESHOLDS = {'present': 3.0, 'inf': np.inf, 'zero': 0.0}
CLOUD_NCOLORS = (1, 7, 4096)
FULL_VIEW = CLOUD_NPIX.index(2049)                      # its workgroups keep 1024, 0 and 1 points


def cloud_offsets(shift):
    """first element of every view's conf in one flat float32 allocation: view v starts 4 ((v + shift) mod 4) bytes past a 16-byte boundary"""
    out, at = [], 0
    for v, n in enumerate(CLOUD_NPIX):
        at = (at + 3) // 4 * 4 + (v + shift) % 4
        out.append(at)
        at += n
    return out, at


def cloud_case(thr_name, ncolors, seed=0):
    """-> dict(x_out, imgs, pan, cams, colors, thr, opacity): numpy arrays in the layout of cloud_ref.cloud (views of 1 x npix pixels)"""
    g = np.random.Generator(np.random.PCG64(900 + seed))
    thr = F(CLOUD_THRESHOLDS[thr_name])
    nan, inf = F(np.nan), F(np.inf)
    keep, drop = {'present': ([thr, np.nextafter(thr, inf), F(50)], [np.nextafter(thr, -inf), F(-1), nan, F(-0.0)]),
                  'inf': ([inf], [F(3.4e38), F(5), nan, -inf]),
                  'zero': ([F(-0.0), F(0.0), F(1e-45), F(5)], [F(-1e-45), F(-1), nan, -inf])}[thr_name]
    keep, drop = np.asarray(keep, dtype=F), np.asarray(drop, dtype=F)
    ids = np.asarray([0, -1, ncolors - 1, ncolors, 2 ** 31 - 1, 1, ncolors // 2, -2 ** 31], dtype=np.int64).astype(np.int32)
    x_out, imgs, pan, cams = [], [], [], []
    for v, n in enumerate(CLOUD_NPIX):
        conf = np.where(g.uniform(0, 1, n) < 0.6, keep[g.integers(0, len(keep), n)], drop[g.integers(0, len(drop), n)]).astype(F)
        if v == FULL_VIEW:
            conf[:WG] = keep[np.arange(WG) % len(keep)]
            conf[WG:2 * WG] = drop[np.arange(WG) % len(drop)]
            conf[2 * WG:] = keep[0]
        pts, loc = (g.standard_normal((n, 3)) * 2).astype(F), (g.standard_normal((n, 3)) * 2).astype(F)
        if n >= 1023:                                                        # a kept row of denormal coordinates and one of infinities, in both maps
            conf[[7, 9]] = keep[0]
            for m in (pts, loc):
                m[7] = from_bits([1, 0x80000003, 0x007fffff])
                m[9] = [inf, -inf, 1.0]
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        c = np.eye(4, dtype=F)
        c[:3, :3], c[:3, 3] = q.astype(F), g.standard_normal(3).astype(F)
        x_out.append({'conf': conf.reshape(1, n), 'pts3d': pts.reshape(1, n, 3), 'pts3d_local': loc.reshape(1, n, 3)})
        imgs.append(g.uniform(-1, 1, (3, 1, n)).astype(F))
        pan.append(ids[g.integers(0, len(ids), n)].reshape(1, n))
        cams.append(c)
    return dict(x_out=x_out, imgs=imgs, pan=pan, cams=cams, colors=_table(g, ncolors), thr=float(thr), opacity=0.3)


CLOUD_FIELDS = ('points', 'points_local', 'rgb', 'pan', 'colors', 'index')


def cloud_reference(case):
    with np.errstate(over='ignore', invalid='ignore'):
        return cloud_ref.cloud(case['x_out'], case['imgs'], case['pan'], [], case['cams'], min_conf_thr=case['thr'], opacity=case['opacity'], colors=case['colors'])


def cloud_wg_counts(case):
    """kept points of every workgroup, in the order of the kernels' workgroups"""
    out = []
    for x in case['x_out']:
        c = x['conf'].reshape(-1)
        with np.errstate(invalid='ignore'):
            m = c >= F(case['thr'])
        out += [int(m[i:i + WG].sum()) for i in range(0, len(c), WG)]
    return np.asarray(out, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------- the workgroup rank: components and surface keep
RANK_PATTERNS = ('none', 'all', 'wave_last', 'wg_first', 'alternating', 'random', 'wg_blocks')
VCC_MV = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]            # rows; a workgroup ranks 1024 rows, four per lane
VCC_PT = 4
KEEP_F = [1, 63, 64, 65, 255, 256, 257, 513]                                # faces; a workgroup ranks 256 faces, one per lane
KEEP_WG, KEEP_PT = 256, 1
KEEP_MIN_FACES = 3
RANK_EDGES = ('empty_wave', 'full_wave', 'lane0_only', 'lane63_only', 'full_wg_next_to_empty', 'last_wg_one_row')


def rank_pattern(name, n, wg, pt):
    """bool [n]: which rows hold an item.  A lane owns pt consecutive rows, a wave 64 pt, a workgroup wg.
    none / all; wave_last: the last row of every wave (lane 63 alone); wg_first: the first row of every workgroup (lane 0 alone, three waves without an
    item); alternating; random: seeded, half of the rows; wg_blocks: every row of the even workgroups, none of the odd ones"""
    i = np.arange(n)
    if name == 'random':
        return np.random.Generator(np.random.PCG64(7000 + n)).uniform(size=n) < 0.5
    return {'none': i < 0, 'all': i >= 0, 'wave_last': i % (64 * pt) == 64 * pt - 1, 'wg_first': i % wg == 0, 'alternating': i % 2 == 0,
            'wg_blocks': (i // wg) % 2 == 0}[name]


def rank_edges(mask, wg, pt):
    """the names of RANK_EDGES that a pattern over len(mask) rows holds"""
    n, W = len(mask), 64 * pt
    m = np.zeros((n + wg - 1) // wg * wg, dtype=bool)
    m[:n] = mask
    exists = np.arange(len(m)) < n
    waves, lanes = m.reshape(-1, W), m.reshape(-1, 64, pt).any(axis=2)
    whole = exists.reshape(-1, W).all(axis=1)
    per_wg = m.reshape(-1, wg).sum(axis=1)
    out = set()
    if (~waves.any(axis=1) & whole).any():
        out.add('empty_wave')
    if waves.all(axis=1).any():
        out.add('full_wave')
    one = waves.sum(axis=1) == 1
    if (one & lanes[:, 0]).any():
        out.add('lane0_only')
    if (one & lanes[:, 63]).any():
        out.add('lane63_only')
    if ((per_wg[:-1] == wg) & (per_wg[1:] == 0) & exists.reshape(-1, wg)[1:].any(axis=1)).any():
        out.add('full_wg_next_to_empty')
    if n % wg == 1 and n > wg and mask[-1]:
        out.add('last_wg_one_row')
    return out


def wg_counts(mask, wg):
    return np.asarray([int(mask[i:i + wg].sum()) for i in range(0, len(mask), wg)], dtype=np.int32)


def vcc_rank_case(Mv, pattern):
    """the inputs of vcc_count / vcc_rank written by hand and what they must give.  root[v] = v for a root, else the nearest lower root, -1 where there is
    none; size, points (beyond 32 bits), lo, hi and pan identify their row.
    -> dict(root, pan, size, points, lo, hi; want: counts, base, C, roots, component, table{root, pan, size, points, cell_lo, cell_hi})"""
    is_root = rank_pattern(pattern, Mv, WG, VCC_PT)
    v = np.arange(Mv, dtype=np.int64)
    root = np.maximum.accumulate(np.where(is_root, v, -1)).astype(np.int32)
    pan = (v % 97 + 1).astype(np.int32)
    size = (3 * v + 1).astype(np.int32)
    points = (v << 33) + 5
    lo = np.stack([-v, v + 1, 2 * v], axis=1).astype(np.int32)
    hi = np.stack([v + 7, -3 * v, 5 * v], axis=1).astype(np.int32)
    roots = np.nonzero(is_root)[0]
    rank_of = np.full(Mv, -1, dtype=np.int32)
    rank_of[roots] = np.arange(len(roots), dtype=np.int32)
    counts = wg_counts(is_root, WG)
    want = dict(counts=counts, base=scan_ref(counts), C=len(roots), roots=roots, rank_of=rank_of,
                component=np.where(root >= 0, rank_of[np.maximum(root, 0)], -1).astype(np.int32),
                table={'root': roots.astype(np.int32), 'pan': pan[roots], 'size': size[roots], 'points': points[roots], 'cell_lo': lo[roots], 'cell_hi': hi[roots]})
    return dict(is_root=is_root, root=root, pan=pan, size=size, points=points, lo=lo, hi=hi, want=want)


def keep_case(F_, pattern):
    """the inputs of surface_keep_count / surface_keep_emit written by hand.  M = the vertex rows of the workspace, a multiple of 4; size[r] cycles through
    0, min_faces - 1, min_faces and 50 faces.  A face that survives points to a row of exactly min_faces or of 50 faces, one that does not to a row of
    min_faces - 1 or of no faces, or carries component -1.  faces, face_ids and quad identify their face.
    -> dict(M, component, size, faces, face_ids, quad, min_faces; want: survives, counts, base, kept, faces, face_ids, quad)"""
    survives = rank_pattern(pattern, F_, KEEP_WG, KEEP_PT)
    f = np.arange(F_, dtype=np.int64)
    M = 4 * ((F_ + 3) // 4)
    size = np.asarray([0, KEEP_MIN_FACES - 1, KEEP_MIN_FACES, 50], dtype=np.int32)[np.arange(M) % 4]
    klass = np.where(survives, 2 + f % 2, f % 3 - 1)                       # of a face that goes: -1 = no component, 0 = a row of none, 1 = of min_faces - 1
    component = np.where(klass < 0, -1, 4 * ((7 * f) % (M // 4)) + klass).astype(np.int32)
    faces = np.stack([3 * f, 3 * f + 1, 3 * f + 2], axis=1).astype(np.int32)
    face_ids = (f % 11).astype(np.int32)
    quad = (f << 33) + 9
    keep = (component >= 0) & (size[np.maximum(component, 0)] >= KEEP_MIN_FACES)
    counts = wg_counts(keep, KEEP_WG)
    want = dict(survives=keep, counts=counts, base=scan_ref(counts), kept=int(keep.sum()), faces=faces[keep], face_ids=face_ids[keep], quad=quad[keep])
    return dict(M=M, component=component, size=size, faces=faces, face_ids=face_ids, quad=quad, min_faces=KEEP_MIN_FACES, pattern=survives, want=want)
