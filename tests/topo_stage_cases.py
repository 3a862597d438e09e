"""Shared by tests/test_hip_topo_stages.py (GPU) and tests/test_topo_stage_checks.py (CPU): the cases that hold the kernels of csrc/surface.hip
(rows, count, emit, link, components), csrc/simplify.hip (used, mask, remap, count, emit) and csrc/components.hip (cells, build, link, flatten, votes,
apply; with the wait-free union-find of csrc/union_find.h and the table of csrc/voxel_table.h) to their contract STAGE BY STAGE, fed by hand, at the
float decisions, status bits, wrapped probe chains and face orders that a rendered scene never makes; the per-stage restatements composed of
surface_ref (mesh, row_table, face_component), simplify_ref (simplify, face_id), vcc_ref (components, clean_pan, pairs) and geom_stage_cases (vx_hash,
vx_key, home_slot, colliding_cells, colliding_pairs, scan_ref); and the planted mistakes.  Nothing here imports the code under test.

  quads     `quad_case(absent)`: eleven views in one table (1 x 7 first, 17 x 17 = 256 quads, 7 x 1 between, 2 x 258 = 257 quads, 13 x 24 whose quad
            rows straddle the workgroups, the GADGET view, 1 x 1 between, the rank strip, a full workgroup next to an empty one, 2 x 2, 1 x 4 last); the
            z of an absent pixel is NaN or +inf.  A gadget is one hand-written quad: presence, depths, ids.  `v_surface(case, k, m)`.
  islands   `island_cases()`: faces written by hand (strips in three orders, a star, two interleaved components, duplicates, equal corners, unused
            rows, M = 1, corners outside the rows).  `v_islands(faces, M, m)`.
  simplify  `simplify_case(name)`: faces, cluster and the new vertex ids written by hand; `v_simplify(case, dedupe, m)`.
  vcc       `vcc_case(name)`: cells, ids and counts written by hand; `v_vcc(case, connectivity, min_voxels, ncolors, m)`.
Every `v_*` takes m = the name of one planted mistake; with no name it IS the restatement, which tests/test_topo_stage_checks.py asserts against the
reused references before it asserts which named case catches which mistake."""
import functools
import itertools

import numpy as np

import cloud_ref
import geom_stage_cases as G
import simplify_ref
import surface_ref as S
import vcc_ref

F = np.float32
LIM = 1 << 20
SURFACE_WG = 256                               # quads, faces or vertices per workgroup of csrc/surface.hip and csrc/simplify.hip (PST_SURFACE_WG)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = np.uint64(2 ** 64 - 1)
FULL, DUPLICATE, RANGE, LOOP = 1, 2, 4, 8      # PST_VCC_* (and PST_SIMPLIFY_FULL / _RANGE): the bits of status[0]


def capacity(n):
    """slots of an open-addressing table of n items: the next power of two >= 2 n"""
    return 1 << max(1, (2 * int(n) - 1).bit_length())


def wgs(n, wg=SURFACE_WG):
    return (int(n) + wg - 1) // wg


def probe(keys, key):
    """the restated probe of a finished table: from the key's home slot onwards, -1 at the first empty slot (or after every slot)"""
    keys = np.asarray(keys).view(np.uint64)
    cap = len(keys)
    h = int(G.home_slot(np.array([key], dtype=np.uint64), cap)[0])
    for _ in range(cap):
        if keys[h] == np.uint64(key):
            return h
        if keys[h] == EMPTY:
            return -1
        h = (h + 1) & (cap - 1)
    return -1


# ============================================================================================================================================ quads
K = {'cut': F(1.1), 'none': F(np.inf), 'one': F(1.0)}             # the three bounds every quad case runs under
RATIO = {'cut': 0.1, 'none': None, 'one': 0.0}                    # what surface_ref.depth_bound makes them of
TINY, FMAX = F(2.0 ** -149), np.finfo(F).max
B2 = F(F(2) * K['cut'])                                           # rn(zmin k) for zmin = 2: exact, a double product gives the same


def _rounding_up_zmin():
    """the smallest whole zmin >= 3 whose float32 product with float32(1.1) rounds UP: zmax == rn(zmin k) passes in fp32 and fails against the double product"""
    for z in range(3, 100):
        if float(F(F(z) * K['cut'])) > float(z) * float(K['cut']):
            return F(z)
    raise AssertionError


ZR = _rounding_up_zmin()
up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
NAN, INF = F(np.nan), F(np.inf)
D = F(2.125)

# name -> (present a b c d, z a b c d, ids of the face's corners (v0, v1, v2) or None); a missing d makes the face (a, c, b)
GADGETS = {'p%d' % p: (tuple((p >> j) & 1 for j in range(4)), (2, 2, 2, 2), None) for p in range(16)}
GADGETS.update({
    'cut_eq': ((1, 1, 1, 0), (2, B2, 2, 0), None),                # zmax == rn(zmin k): kept
    'cut_above': ((1, 1, 1, 0), (2, up(B2), 2, 0), None),
    'cut_below': ((1, 1, 1, 0), (2, down(B2), 2, 0), None),
    'round_eq': ((1, 1, 1, 0), (ZR, F(ZR * K['cut']), ZR, 0), None),
    'zmin_pos_zero': ((1, 1, 1, 0), (0.0, 1, 1, 0), None),
    'zmin_neg_zero': ((1, 1, 1, 0), (-0.0, 1, 1, 0), None),
    'subnormal_eq': ((1, 1, 1, 0), (TINY, TINY, TINY, 0), None),  # rn(1.1 2^-149) = 2^-149: kept unless subnormals are flushed
    'subnormal_next': ((1, 1, 1, 0), (TINY, 2 * TINY, TINY, 0), None),
    'negative': ((1, 1, 1, 0), (-1, 1, 1, 0), None),
    'nan_corner': ((1, 1, 1, 0), (NAN, 1, 1, 0), None),
    'inf_all': ((1, 1, 1, 0), (INF, INF, INF, 0), None),         # inf <= inf: kept
    'inf_one': ((1, 1, 1, 0), (1, INF, 1, 0), None),
    'overflow': ((1, 1, 1, 0), (3.2e38, FMAX, 3.2e38, 0), None),  # the product overflows to +inf: kept
    'none_subnormal': ((1, 1, 1, 0), (TINY, 1, 1e30, 0), None),   # kept only without a cut (k = +inf)
    'one_equal': ((1, 1, 1, 0), (2, 2, 2, 0), None),              # k = 1: three equal depths stay
    'one_ulp': ((1, 1, 1, 0), (2, up(2), 2, 0), None),            # ... one ulp apart go
    'diag_tie': ((1, 1, 1, 1), (2, D, 2, D), None),               # |b - c| == |a - d|: a-d
    'diag_below': ((1, 1, 1, 1), (2, down(D), 2, D), None),       # one ulp less: b-c
    'diag_above': ((1, 1, 1, 1), (2, up(D), 2, D), None),
    'diag_nan_b': ((1, 1, 1, 1), (2, NAN, 2, 2), None),           # NaN on the b-c side: a-d, T1 = (a, d, b) cut by it
    'diag_nan_a': ((1, 1, 1, 1), (NAN, 2, 2, 2), None),           # NaN on the a-d side: a-d, both cut
    't1_only': ((1, 1, 1, 1), (2, 2, 4, 2), None),
    't0_only': ((1, 1, 1, 1), (2, 4, 2, 2), None),
    'ids_aaa': ((1, 1, 1, 0), (2, 2, 2, 0), (5, 5, 5)),
    'ids_aab': ((1, 1, 1, 0), (2, 2, 2, 0), (5, 5, 7)),
    'ids_aba': ((1, 1, 1, 0), (2, 2, 2, 0), (5, 7, 5)),
    'ids_baa': ((1, 1, 1, 0), (2, 2, 2, 0), (7, 5, 5)),
    'ids_abc': ((1, 1, 1, 0), (2, 2, 2, 0), (5, 6, 7)),
    'ids_00b': ((1, 1, 1, 0), (2, 2, 2, 0), (0, 0, 7)),
    'ids_b00': ((1, 1, 1, 0), (2, 2, 2, 0), (7, 0, 0)),
    'ids_0bb': ((1, 1, 1, 0), (2, 2, 2, 0), (0, 7, 7)),
    'ids_0bc': ((1, 1, 1, 0), (2, 2, 2, 0), (0, 5, 7)),
})
GADGET_NAMES = list(GADGETS)
STRIP_W, STRIP_DEEP = 515, (64, 127, 193, 256, 511)              # the rank strip: a deep bottom pixel at column x makes quad x - 1 T0-only and quad x T1-only
VIEW_NAMES = ('row_first', 'sq17', 'column_between', 'strip258', 'straddle', 'gadgets', 'pixel_between', 'rank_strip', 'full_empty', 'two_by_two', 'row_last')


def _views(absent):
    """[(name, z float32 [H, W], present bool [H, W], ids int32 [H, W])]"""
    g = np.random.default_rng(5)
    out = []

    def view(name, H, W, z=None, present=None, ids=None):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        z = np.full((H, W), 2.0, dtype=F) if z is None else np.asarray(z, dtype=F)
        present = np.ones((H, W), dtype=bool) if present is None else present
        ids = ((3 * yy + 5 * xx) % 7).astype(np.int32) if ids is None else ids
        out.append((name, np.where(present, z, F(absent)).astype(F), present, ids))

    def noisy(H, W, drop):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        return (2.0 + 0.05 * np.sin(xx / 3.0) * np.cos(yy / 2.0) + 0.08 * g.standard_normal((H, W))).astype(F), g.random((H, W)) >= drop

    view('row_first', 1, 7)
    view('sq17', 17, 17, *noisy(17, 17, 0.1))
    view('column_between', 7, 1)
    view('strip258', 2, 258, *noisy(2, 258, 0.0))
    view('straddle', 13, 24, *noisy(13, 24, 0.15))
    n = len(GADGETS)
    z, present, ids = np.zeros((2, 3 * n), dtype=F), np.zeros((2, 3 * n), dtype=bool), np.ones((2, 3 * n), dtype=np.int32)
    for j, (p, zz, fid) in enumerate(GADGETS.values()):
        at = [(0, 3 * j), (0, 3 * j + 1), (1, 3 * j), (1, 3 * j + 1)]                 # a b c d
        for c in range(4):
            present[at[c]], z[at[c]] = bool(p[c]), F(zz[c])
        if fid is not None:                                                            # the face is (a, c, b)
            ids[at[0]], ids[at[2]], ids[at[1]] = fid
    view('gadgets', 2, 3 * n, z, present, ids)
    view('pixel_between', 1, 1)
    z = np.full((2, STRIP_W), 2.0, dtype=F)
    z[1, list(STRIP_DEEP)] = 4.0
    view('rank_strip', 2, STRIP_W, z)
    present = np.ones((2, 513), dtype=bool)
    present[:, 257:] = False                                                           # quads 0 .. 255 hold two faces each, quads 256 .. 511 none
    view('full_empty', 2, 513, None, present)
    view('two_by_two', 2, 2, [[2, 2.1], [2.05, 2.15]])
    view('row_last', 1, 4)
    assert tuple(v[0] for v in out) == VIEW_NAMES
    return out


def surface_dims(shapes):
    """int32 [V, 4] = (H, W, first_wg, 0) and the number of quad workgroups, as the header defines the table"""
    rows, wg = [], 0
    for H, W in shapes:
        rows.append((H, W, wg, 0))
        wg += wgs(max(H - 1, 0) * max(W - 1, 0))
    return np.array(rows, dtype=np.int32).reshape(-1, 4), wg


@functools.lru_cache(maxsize=None)
def quad_case(absent='nan', views=None):
    """dict(shapes, depths [float32 [H, W]], present, N, index int64 [M], vertex_ids int32 [M], offsets, quad_offsets, names); `views` = a tuple of
    view names keeps only those (the tables without an empty view)"""
    vs = [v for v in _views({'nan': np.nan, 'inf': np.inf}[absent]) if views is None or v[0] in views]
    shapes = [v[1].shape for v in vs]
    present = np.concatenate([v[2].reshape(-1) for v in vs])
    ids = np.concatenate([v[3].reshape(-1) for v in vs])
    index = np.nonzero(present)[0].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).astype(np.int64)
    quads = np.concatenate([[0], np.cumsum([max(h - 1, 0) * max(w - 1, 0) for h, w in shapes])]).astype(np.int64)
    return {'shapes': shapes, 'depths': [v[1] for v in vs], 'present': present, 'N': int(offsets[-1]), 'index': index, 'vertex_ids': ids[present].astype(np.int32),
            'offsets': offsets, 'quad_offsets': quads, 'names': [v[0] for v in vs]}


def quad_of(case, view, i):
    """the row of quad i of the named view in the per-quad detail of surface_ref.mesh"""
    return int(case['quad_offsets'][case['names'].index(view)]) + i


def gadget_quad(case, name):
    return quad_of(case, 'gadgets', 3 * GADGET_NAMES.index(name))


def surface_ref_of(case, k):
    return S.mesh(case['index'], case['vertex_ids'], case['shapes'], case['depths'], RATIO[k])


SURFACE_MISTAKES = ('bound_double', 'cut_lt', 'tie_bc', 'three_corner_winding', 'view_first_of_equal')
ABC = 4                                                            # a fifth code for the mistake: (a, b, c) where the contract says (a, c, b)
_TRI = np.concatenate([S.TRI, [[0, 1, 2]]])


def v_surface(case, k, m=None):
    """steps 1 - 5 as csrc/surface.hip divides them: per workgroup of 256 quads of the view that owns it.
    -> dict(row int32 [N], counts int32 [nwg], base int32 [nwg + 1], faces int32 [F, 3], face_ids int32 [F], quad int64 [F])
    mistakes: bound_double zmin k in double; cut_lt zmax < bound; tie_bc |b - c| <= |a - d| takes b-c; three_corner_winding a missing d gives (a, b, c);
    view_first_of_equal of the views that share the largest first_wg <= wg the FIRST one (an empty view) owns the workgroup"""
    k = F(K[k])
    row = S.row_table(case['index'], case['N'])
    vid = case['vertex_ids']
    zflat = np.concatenate([d.reshape(-1) for d in case['depths']]) if case['depths'] else np.zeros(0, dtype=F)
    dims, nwg = surface_dims(case['shapes'])
    first = dims[:, 2]
    counts, faces, fids, quads = np.zeros(nwg, dtype=np.int32), [], [], []
    for wg in range(nwg):
        top = first[first <= wg].max()
        owners = np.nonzero(first == top)[0]
        v = owners[0] if m == 'view_first_of_equal' else owners[-1]
        H, W = case['shapes'][v]
        if H < 2 or W < 2:
            continue
        i = np.arange((wg - first[v]) * SURFACE_WG, min((H - 1) * (W - 1), (wg - first[v] + 1) * SURFACE_WG))
        if len(i) == 0:
            continue
        y, x = np.divmod(i, W - 1)
        pa = y * W + x
        px = case['offsets'][v] + np.stack([pa, pa + 1, pa + W, pa + W + 1], axis=1)
        R = row[px]
        Z = np.where(R >= 0, zflat[px], F(0)).astype(F)
        n = (R >= 0).sum(axis=1)
        with np.errstate(all='ignore'):
            dbc, dad = np.abs((Z[:, 1] - Z[:, 2]).astype(F)), np.abs((Z[:, 0] - Z[:, 3]).astype(F))
            bc = (dbc <= dad) if m == 'tie_bc' else (dbc < dad)
        three = np.where(R[:, 3] < 0, ABC if m == 'three_corner_winding' else S.ACB, np.where(R[:, 0] < 0, S.BCD, np.where(R[:, 1] < 0, S.ACD, S.ADB)))
        code = np.stack([np.where(n == 4, np.where(bc, S.ACB, S.ACD), three), np.where(bc, S.BCD, S.ADB)], axis=1)
        has = np.stack([n >= 3, n == 4], axis=1)
        tr = np.take_along_axis(R[:, None, :], _TRI[code], axis=2)
        tz = np.take_along_axis(Z[:, None, :], _TRI[code], axis=2)
        with np.errstate(all='ignore'):
            pos = (tz > 0).all(axis=2)
            zmin, zmax = np.fmin.reduce(tz, axis=2), np.fmax.reduce(tz, axis=2)
            if m == 'bound_double':
                inside = zmax.astype(np.float64) <= zmin.astype(np.float64) * np.float64(k)
            else:
                bound = (zmin * k).astype(F)
                inside = (zmax < bound) if m == 'cut_lt' else (zmax <= bound)
        keep = has & pos & inside
        ids = vid[np.where(tr >= 0, tr, 0)]
        counts[wg] = keep.sum()
        faces.append(tr[keep])
        fids.append(simplify_ref.face_id(ids[keep].reshape(-1, 3)))
        quads.append(np.broadcast_to((case['offsets'][v] + pa)[:, None], keep.shape)[keep])
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt).reshape(shape) if parts else np.zeros(shape, dtype=dt).reshape(shape)
    return {'row': row, 'counts': counts, 'base': G.scan_ref(counts), 'faces': cat(faces, (-1, 3), np.int32), 'face_ids': cat(fids, (-1,), np.int32),
            'quad': cat(quads, (-1,), np.int64)}


SURFACE_FIELDS = (('faces', np.int32), ('face_ids', np.int32), ('quad', np.int64))


def same_surface(a, b):
    """the names of the fields in which two meshes differ"""
    return [n for n, dt in SURFACE_FIELDS if not np.array_equal(np.asarray(a[n]).astype(dt), np.asarray(b[n]).astype(dt))]


# ========================================================================================================================================== islands
STRIP_F = (1, 63, 64, 65, 255, 256, 257, 1025, 4097)
DEEP_F = 4097                                                      # only as the shuffle: the deep tree of cc_find


def strip(Fn, order='ascending'):
    """face i joins the vertex rows i, i + 1, i + 2 -> (faces int32 [F, 3], M = F + 2)"""
    i = np.arange(Fn)
    faces = np.stack([i, i + 1, i + 2], axis=1)
    if order == 'descending':
        faces = faces[::-1]
    elif order == 'shuffle':
        faces = faces[np.random.default_rng(Fn).permutation(Fn)]
    return np.ascontiguousarray(faces, dtype=np.int32), Fn + 2


def _star(Fn=300):
    i = np.arange(Fn)
    M = 2 * Fn + 1
    return np.stack([2 * i, 2 * i + 1, np.full(Fn, M - 1)], axis=1)[::-1].astype(np.int32).copy(), M          # the face that holds row 0 comes last


def _interleaved(n=150):
    j = np.arange(n)
    even, odd = np.stack([2 * j, 2 * j + 2, 2 * j + 4], axis=1), np.stack([2 * j + 1, 2 * j + 3, 2 * j + 5], axis=1)
    return np.stack([even, odd], axis=1).reshape(-1, 3).astype(np.int32), 2 * n + 5                          # the last row is named by no face


def _duplicates():
    f, M = strip(70)
    rot = np.roll(f, 1, axis=1)
    return np.concatenate([f, f, rot[::-1], f[:, ::-1]]).astype(np.int32), M


def _equal_corners():
    faces = [(0, 0, 1), (2, 2, 2), (3, 4, 3), (5, 6, 6), (1, 1, 3), (7, 7, 7), (6, 6, 8), (9, 9, 9)]
    return np.array(faces, dtype=np.int32), 11                                                                # {0 1 3 4}, {2}, {5 6 8}, {7}, {9}; row 10 unused


def _unused_rows():
    f, M = strip(40)
    return (f * 3 + 2).astype(np.int32), 3 * M + 4                                                            # two rows in three, the first two and the last four: no face


RANGE_BAD = (4, 9, 12)                                            # the faces of `range_case` with a corner outside the rows


def range_case():
    """two strips of six faces on the rows 0 .. 7 and 8 .. 15 (two components) and, as faces 4, 9 and 12, three faces with one corner outside the
    rows - a second corner equal to M, a first corner -1, a third corner equal to M - whose two other corners lie one in each strip: a kernel that
    unites what it can of such a face joins the two components"""
    M = 16
    f = np.concatenate([strip(6)[0], strip(6)[0] + 8]).tolist()
    for at, bad in zip(RANGE_BAD, ((3, M, 9), (-1, 10, 2), (12, 4, M))):
        f.insert(at, bad)
    return np.array(f, dtype=np.int32), M


@functools.lru_cache(maxsize=None)
def island_cases():
    """name -> (faces int32 [F, 3], M): every corner inside [0, M)"""
    c = {}
    for Fn in STRIP_F:
        for order in ('ascending', 'descending', 'shuffle'):
            if Fn < DEEP_F or order == 'shuffle':
                c['strip_%d_%s' % (Fn, order)] = strip(Fn, order)
    c.update(star=_star(), interleaved=_interleaved(), duplicates=_duplicates(), equal_corners=_equal_corners(), unused_rows=_unused_rows(),
             one_row=(np.zeros((3, 3), dtype=np.int32), 1))
    return c


ISLAND_MISTAKES = ('root_largest', 'drop_leftover')


def vertex_roots(faces, M, m=None):
    """int64 [M]: the smallest vertex row of every row's component (its own for a row no face names), by rounds of hooking every edge's larger
    label under the smaller at once and pointer jumping.  mistakes: drop_leftover an edge that loses the hook of its round (another edge brought a
    smaller label to the same row) is dropped where the contract unites what is left over; root_largest the component's largest row"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [0, 2]]])
    v, n = e[:, 0], e[:, 1]
    label = np.arange(M, dtype=np.int64)
    while len(v):
        lv, ln = label[v], label[n]
        open_ = lv != ln
        if not open_.any():
            break
        hi, lo = np.maximum(lv, ln), np.minimum(lv, ln)
        np.minimum.at(label, hi[open_], lo[open_])
        if m == 'drop_leftover':
            open_ &= label[hi] == lo                                # the winners stay (and agree from now on); the losers are gone
        while True:
            j = label[label]
            if np.array_equal(j, label):
                break
            label = j
        v, n = v[open_], n[open_]
    if m == 'root_largest':
        top = np.zeros(M, dtype=np.int64)
        np.maximum.at(top, label, np.arange(M))
        label = top[label]
    return label


def v_islands(faces, M, m=None):
    """-> dict(root int64 [M], component int32 [F], size int32 [M], status).  A face with a corner outside [0, M) joins nothing, has component -1,
    is counted nowhere and sets the RANGE bit."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < M)).all(axis=1)
    root = vertex_roots(faces[ok], M, m)
    component = np.where(ok, root[np.where(ok, faces[:, 0], 0)], -1).astype(np.int32)
    size = np.bincount(component[ok], minlength=M).astype(np.int32)
    return {'root': root, 'component': component, 'size': size, 'status': 0 if ok.all() else RANGE}


def chase(parent, v, limit):
    """the end of the parent chain from v (at most `limit` steps), or None"""
    for _ in range(limit + 1):
        p = int(parent[v])
        if p == v:
            return v
        v = p
    return None


# ========================================================================================================================================= simplify
SIMPLIFY_F, SIMPLIFY_M = (1, 255, 256, 257, 513), (64, 256)
CELL = 0.25
SIMPLIFY_MISTAKES = ('winner_last', 'key_unsorted')


def face_key(n, m=None):
    """uint64 [F]: the sorted new corners + 1 in 3 x 21 bits, smallest lowest (m = 'key_unsorted': as they come)"""
    s = np.asarray(n, dtype=np.int64).reshape(-1, 3)
    s = (s if m == 'key_unsorted' else np.sort(s, axis=1)).astype(np.uint64) + np.uint64(1)
    return s[:, 0] | (s[:, 1] << np.uint64(21)) | (s[:, 2] << np.uint64(42))


def colliding_triples(cap, home, Mv, n):
    """the first n corner triples a < b < c < Mv whose face key has the home slot `home` in a table of `cap` slots"""
    t = np.array(list(itertools.combinations(range(Mv), 3)), dtype=np.int64)
    hit = t[G.home_slot(face_key(t), cap) == home]
    assert len(hit) >= n, (cap, home, Mv, len(hit))
    return hit[:n]


def first_ranks(group, used):
    """cluster int32 [M] of hand-written groups: the used vertices with group >= 0, numbered by the first row of their group; -1 for the others"""
    cluster = np.full(len(group), -1, dtype=np.int32)
    seen = {}
    for v in np.nonzero(used & (group >= 0))[0]:
        cluster[v] = seen.setdefault(int(group[v]), len(seen))
    return cluster, len(seen)


def _simplify(faces, M, group, vertices=None, **extra):
    """a case from hand-written groups: cluster by `first_ranks`, the vertex of group g in the cell (g, 0, 0) of edge CELL so that simplify_ref finds the
    same clusters; a vertex with group -1 gets a NaN coordinate (left out by the voxel stage).  The new ids are written by hand: 0 among them, runs"""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    group = np.asarray(group, dtype=np.int64)
    used = np.zeros(M, dtype=bool)
    used[faces[((faces >= 0) & (faces < M)).all(axis=1)].reshape(-1)] = True              # a face with a corner outside the rows marks none
    cluster, Mv = first_ranks(group, used)
    if vertices is None:
        vertices = np.stack([(group + 0.5) * CELL, np.full(M, 0.125), np.full(M, 0.125)], axis=1).astype(F)
        vertices[group < 0, 0] = np.nan
    ids = ((np.arange(max(Mv, 1)) // 2) % 5).astype(np.int32)                              # 0 0 1 1 2 2 ...: pairs share an id, 0 among them
    case = dict(faces=faces, M=M, cluster=cluster, Mv=max(Mv, 1), ids=ids, vertices=np.asarray(vertices, dtype=F), quad=(np.arange(len(faces), dtype=np.int64) << 33) + 11,
                group=group, by_ref=True)
    case.update(extra)
    return case


def _sized(Fn, M):
    g = np.random.default_rng(31 * Fn + M)
    named = M - 3                                                                          # the last three rows: no face names them
    faces = g.integers(0, named, (Fn, 3))
    group = g.integers(0, max(2, M // 3), M)
    group[g.random(M) < 0.05] = -1
    group[[M - 5, M - 6]], group[M - 7] = -1, 1
    if Fn >= 255:
        faces[7], faces[8] = (M - 5, M - 6, M - 7), (M - 7, 0, 1)                          # the three special rows are used
    v = np.stack([(group + 0.5) * CELL, np.full(M, 0.125), np.full(M, 0.125)], axis=1).astype(F)
    v[group < 0, 0] = np.nan
    v[M - 5] = (0.125, 0.125, np.inf)                                                      # used vertices with a non-finite coordinate: left out, the bits copied
    v[M - 6] = (np.nan, 0.125, -0.0)
    v[M - 7, 1] = -0.0                                                                     # the cell of -0.0 is the cell of +0.0; its sign must arrive
    return _simplify(faces, M, group, vertices=v)


def _dups():
    """Mv = M = 40, every vertex its own cluster.  T = (3, 9, 20): reversed first (face 0), rotated (5), plain (500): far apart; runs of one key across
    the wave edge (faces 60 .. 70) and the workgroup edge (250 .. 260); a triple copy whose first stands in lane 63 (faces 191, 192, 193)"""
    M = 40
    g = np.random.default_rng(8)
    faces = np.stack([np.sort(g.choice(M, 3, replace=False)) for _ in range(513)])
    faces[0], faces[5], faces[500] = (20, 9, 3), (9, 20, 3), (3, 9, 20)
    faces[60:71] = (1, 2, 30)
    faces[62], faces[66] = (30, 1, 2), (2, 1, 30)
    faces[250:261] = (4, 5, 31)
    faces[191:194] = (6, 7, 32)
    faces[400] = (1, 2, 30)                                                               # a late copy of the wave-edge run: the merge path and the probe path meet in one slot
    return _simplify(faces, M, np.arange(M))


def _degenerate():
    M = 12
    group = np.array([0, 0, 1, 2, 3, 3, 3, 4, 5, 6, 7, 8])
    faces = [(0, 2, 3), (0, 1, 2), (4, 5, 6), (7, 7, 8), (9, 9, 9), (7, 8, 9), (1, 3, 2), (10, 11, 7), (4, 7, 5)]
    # a candidate, two equal new corners, three equal, degenerate in the input (twice), a candidate, a duplicate of face 0 through the merged rows, ...
    return _simplify(faces, M, group)


def _collide(Fn=32, Mv=32):
    """a table at exactly the next power of two >= 2 F in which eight keys share the LAST slot as home: the chain wraps to slot 0.  The first eleven
    faces name every vertex, so every vertex is its own cluster and the new rows are the old ones"""
    cap = capacity(Fn)
    assert cap == 2 * Fn
    hit = colliding_triples(cap, cap - 1, Mv, 8)
    g = np.random.default_rng(9)
    cover = [(3 * j % Mv, (3 * j + 1) % Mv, (3 * j + 2) % Mv) for j in range(11)]
    rest = np.stack([np.sort(g.choice(Mv, 3, replace=False)) for _ in range(Fn - 19)])
    faces = np.concatenate([cover, hit[:4], rest[:6], hit[4:], rest[6:]])
    faces[-1] = hit[0][::-1]                                                              # a duplicate inside the wrapped chain
    return _simplify(faces, Mv, np.arange(Mv), cap=cap, chain=hit)


def _bad_cluster():
    """cluster written by hand, Mv = 6: values Mv and -2 (outside [-1, Mv): RANGE, the face left out), -1 (left out quietly), Mv - 1 (the last legal one)"""
    M, Mv = 10, 6
    cluster = np.array([0, 1, 2, 3, 4, 5, Mv, -2, -1, 5], dtype=np.int32)
    faces = np.array([(0, 1, 2), (3, 4, 5), (0, 6, 1), (7, 2, 3), (8, 0, 1), (9, 4, 3), (5, 9, 0), (2, 1, 0)], dtype=np.int32)
    return dict(faces=faces, M=M, cluster=cluster, Mv=Mv, ids=np.array([4, 0, 4, 2, 2, 9], dtype=np.int32), vertices=np.ones((M, 3), dtype=F),
                quad=(np.arange(len(faces), dtype=np.int64) << 33) + 11, by_ref=False)


def _bad_corner():
    """a face with a corner equal to M and one with -1: simplify_used and simplify_remap both report RANGE and leave the face alone"""
    c = _simplify([(0, 1, 2), (3, 8, 4), (-1, 5, 6), (5, 6, 7), (2, 1, 0)], 8, np.arange(8))
    c['by_ref'] = False                                                                    # (simplify_ref raises on such a mesh)
    return c


SIMPLIFY_CASES = {'sized_%d_%d' % (Fn, M): (lambda Fn, M: lambda: _sized(Fn, M))(Fn, M) for Fn in SIMPLIFY_F for M in SIMPLIFY_M}
SIMPLIFY_CASES.update(dups=_dups, degenerate=_degenerate, collide=_collide, bad_cluster=_bad_cluster, bad_corner=_bad_corner,
                      identity=lambda: _simplify(strip(62)[0], 64, np.arange(64)),                                  # Mv = M
                      one=lambda: _simplify(strip(62)[0], 64, np.zeros(64, dtype=np.int64)))                          # Mv = 1: every face collapses


@functools.lru_cache(maxsize=None)
def simplify_case(name):
    return SIMPLIFY_CASES[name]()


def v_simplify(case, dedupe=True, m=None):
    """the five kernels of csrc/simplify.hip on a hand-written cluster -> dict(used int32 [M], masked float32 [M, 3], status int32 [5] (bits, used,
    left out, degenerate, candidates), klass int32 [F] (-1 left out, -2 degenerate, 0 a candidate), key uint64 [F] (0: no candidate), winner {key: face},
    counts, base, faces, face_ids, quad, src_face).  mistakes: winner_last the LAST face of every key survives; key_unsorted"""
    faces, M, cluster, Mv = case['faces'].astype(np.int64), case['M'], case['cluster'].astype(np.int64), case['Mv']
    inside = ((faces >= 0) & (faces < M)).all(axis=1)
    used = np.zeros(M, dtype=np.int32)
    used[faces[inside].reshape(-1)] = 1
    masked = np.where(used[:, None] != 0, case['vertices'], F(np.nan)).astype(F)
    corner_ok = (faces >= 0) & (faces < M)
    n = np.where(corner_ok, cluster[np.where(corner_ok, faces, 0)], -1)
    bad = ~corner_ok | (corner_ok & ((n < -1) | (n >= Mv)))
    n = np.where(bad, -1, n)
    left = (n == -1).any(axis=1)
    deg = ~left & ((n[:, 0] == n[:, 1]) | (n[:, 0] == n[:, 2]) | (n[:, 1] == n[:, 2]))
    cand = ~left & ~deg
    klass = np.where(left, -1, np.where(deg, -2, 0)).astype(np.int32)
    key = np.where(cand, face_key(np.where(cand[:, None], n, 0), m), np.uint64(0))
    winner = {}
    for f in np.nonzero(cand)[0]:
        k = int(key[f])
        winner[k] = int(f) if (m == 'winner_last' or k not in winner) else winner[k]
    survives = cand & (np.array([winner.get(int(k), -1) for k in key]) == np.arange(len(faces))) if dedupe else cand
    keep = np.nonzero(survives)[0]
    counts = np.array([survives[i:i + SURFACE_WG].sum() for i in range(0, len(faces), SURFACE_WG)], dtype=np.int32)
    nf = n[keep].astype(np.int32).reshape(-1, 3)
    status = np.array([RANGE if bad.any() else 0, used.sum(), left.sum(), deg.sum(), cand.sum()], dtype=np.int32)
    return {'used': used, 'masked': masked, 'status': status, 'klass': klass, 'key': key, 'winner': winner, 'counts': counts, 'base': G.scan_ref(counts),
            'new': n, 'faces': nf, 'face_ids': simplify_ref.face_id(case['ids'][nf]) if len(nf) else np.zeros(0, dtype=np.int32),
            'quad': case['quad'][keep], 'src_face': keep.astype(np.int32)}


SIMPLIFY_FIELDS = ('faces', 'face_ids', 'quad', 'src_face')


def simplify_by_ref(case, dedupe=True):
    """simplify_ref.simplify(detail=True) of the case's vertices: the clusters it finds must be the hand-written ones"""
    old_ids = np.zeros(case['M'], dtype=np.int32)
    return simplify_ref.simplify(case['vertices'], np.zeros((case['M'], 3), dtype=F), old_ids, case['faces'], case['quad'], (), CELL, dedupe, detail=True)


# ============================================================================================================================================== vcc
VCC_MV = (1, 63, 64, 65, 256, 257, 1024, 1025, 2049)
NCOLORS = (1, 7, 4096)
OPACITY = 0.3
VCC_MISTAKES = ('votes_per_neighbour', 'tie_larger', 'known_le', 'link_27')
OFFSETS26 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def _vcc(cells, pan, count=None, seed=0, **extra):
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 3)
    Mv = len(cells)
    g = np.random.default_rng(4000 + seed)
    count = (1 + (np.arange(Mv) * 7) % 5) if count is None else count
    table = g.random((4096, 3)).astype(F)
    table[0] = 0
    case = dict(cells=cells, pan=np.asarray(pan, dtype=np.int32).reshape(-1), count=np.asarray(count, dtype=np.int32), rgb=g.random((Mv, 3)).astype(F), colors=table)
    case.update(extra)
    return case


def _blob(Mv):
    """Mv cells of a box around zero at density 0.4, seeded order; ids 1 .. 3, void 0 and a negative among them"""
    g = np.random.default_rng(Mv)
    side = max(2, int(np.ceil((Mv / 0.4) ** (1 / 3))))
    r = np.arange(side) - side // 2
    z, y, x = np.meshgrid(r, r, r, indexing='ij')
    box = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    cells = box[g.permutation(len(box))[:Mv]]
    return _vcc(cells, np.array([0, -3, 1, 1, 2, 2, 3])[g.integers(0, 7, Mv)], seed=Mv)


def _last_legal():
    L = LIM - 1
    cells = [(L, 0, 0), (L - 1, 0, 0), (-L, 5, 5), (-L + 1, 5, 5), (L, L, L), (L - 1, L - 1, L - 1), (0, -L, 0), (0, -L + 1, 1), (3, 3, -L), (3, 3, -L + 1)]
    return _vcc(cells, np.ones(len(cells)))


def _offsets():
    """52 voxels: pair j = a voxel at (5 j, 0, 0) and one at the j-th of the 26 offsets from it, one id per pair (so no pair joins another through a
    diagonal): the pair is one component iff the connectivity includes its offset"""
    cells, pan = [], []
    for j, d in enumerate(OFFSETS26):
        cells += [(5 * j, 0, 0), (5 * j + d[0], d[1], d[2])]
        pan += [1 + j % 3] * 2
    return _vcc(cells, pan)


def _ids():
    """void rows of id 0 and negative ids between solid ones; equal ids that touch only through a void cell"""
    cells = [(x, 0, 0) for x in range(12)]
    pan = [1, 0, 1, 1, -2, 1, 2, 2, 0, 0, 2, -1]
    return _vcc(cells, pan)


def _line(Mv=2049, shuffle=True):
    x = np.arange(Mv) - Mv // 2
    if shuffle:
        x = x[np.random.default_rng(77).permutation(Mv)]
    return _vcc(np.stack([x, np.zeros(Mv, dtype=np.int64), np.zeros(Mv, dtype=np.int64)], axis=1), np.ones(Mv))


def _runs():
    """a line in row order whose ids change at rows 60, 71, 250 and 261: runs of one root across the lane 63 | 64 and the workgroup 255 | 256 edges; the
    counts of the run 60 .. 70 are 2^31 - 1, so its `points` pass 2^32"""
    Mv = 600
    row = np.arange(Mv)
    pan = 1 + np.searchsorted([60, 71, 250, 261], row, side='right')
    count = np.where((row >= 60) & (row < 71), INT_MAX, 1 + row % 5)
    return _vcc(np.stack([row - 300, np.zeros(Mv, dtype=np.int64), np.zeros(Mv, dtype=np.int64)], axis=1), pan, count)


def _wrap(Mv=64):
    """a table at capacity exactly 2 Mv in which twelve cells share the LAST slot as home"""
    cap = capacity(Mv)
    assert cap == 2 * Mv
    hit = G.colliding_cells(cap, cap - 1, 12)
    lat = G.lattice()
    rest = lat[G.home_slot(G.vx_key(lat), cap) != cap - 1]
    g = np.random.default_rng(3)
    cells = np.concatenate([hit, rest[g.choice(len(rest), Mv - 12, replace=False)]])[g.permutation(Mv)]
    return _vcc(cells, 1 + g.integers(0, 2, Mv), cap=cap)


MIN_VOXELS = 3
SPECKLE_MARKS = {}


def _speckle():
    """hand-written despeckling, connectivity 26, min_voxels 3 (marks: name -> rows):
    block       4 x 4 x 4 voxels of id 1 at (0 .. 3)^3 and `single`, one voxel of id 2 on its face: nine votes for id 1
    floater     two voxels of id 3 far from everything, a void voxel beside them: no vote, void
    tie         A = three voxels of id 5, S of id 2, B = three voxels of id 4 in one line, each touching S with one voxel: 1 : 1, the smaller id 4 wins
    pairs       s1, s2 of id 7 (one component of two); P1, P2 of id 1 touch BOTH (four pairs, two neighbours), Q1, Q2, Q3 of id 6 touch one each (three
                pairs, three neighbours): per pair id 1 wins, per neighbour id 6 would
    last        a voxel of id 2 beside a line of id 6 = ncolors - 1 at seven colours, and one beside a line of id 7 = ncolors"""
    cells, pan, marks = [], [], {}

    def add(name, cs, ids):
        marks[name] = list(range(len(cells), len(cells) + len(cs)))
        cells.extend(cs)
        pan.extend([ids] * len(cs) if np.isscalar(ids) else ids)
    add('block', [(x, y, z) for z in range(4) for y in range(4) for x in range(4)], 1)
    add('single', [(4, 1, 1)], 2)
    add('floater', [(40, 0, 0), (41, 0, 0)], 3)
    add('floater_void', [(42, 0, 0)], 0)
    add('tie_A', [(20, 10, 0), (21, 10, 0), (22, 10, 0)], 5)
    add('tie_S', [(23, 10, 0)], 2)
    add('tie_B', [(24, 10, 0), (25, 10, 0), (26, 10, 0)], 4)
    o = np.array([0, 30, 0])
    add('pairs_s', [tuple(o + c) for c in ((0, 0, 0), (1, 0, 0))], 7)
    add('pairs_P', [tuple(o + c) for c in ((0, 1, 0), (0, 2, 0), (0, 3, 0), (0, -1, 0), (0, -2, 0), (0, -3, 0))], 1)
    add('pairs_Q', [tuple(o + c) for c in ((-1, 0, 0), (-2, 0, 0), (-3, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (-1, 0, 1))], 6)
    add('last_6', [(0, 50, 0), (1, 50, 0), (2, 50, 0)], 6)
    add('last_6_S', [(3, 50, 0)], 2)
    add('last_7', [(0, 60, 0), (1, 60, 0), (2, 60, 0)], 7)
    add('last_7_S', [(3, 60, 0)], 2)
    SPECKLE_MARKS.update(marks)
    return _vcc(cells, pan, marks=marks)


PAIR_GADGETS = 8


def _pair_wrap():
    """eight gadgets of four rows: a voxel S (row 4 j, its own root) beside a line of three of an id chosen so that the pair key (4 j << 32) | id has
    the LAST slot of a 16-slot pair table as home: eight distinct pairs, one chain that wraps"""
    cap = capacity(PAIR_GADGETS)
    planted = G.colliding_pairs(cap, cap - 1, [4 * j for j in range(PAIR_GADGETS)], 4095)
    assert len(planted) == PAIR_GADGETS
    cells, pan = [], []
    for j, (r, pid) in enumerate(planted):
        cells += [(0, 5 * j, 0), (1, 5 * j, 0), (2, 5 * j, 0), (3, 5 * j, 0)]
        pan += [4095, pid, pid, pid]
    return _vcc(cells, pan, pair_cap=cap, planted=planted)


VCC_CASES = {'blob_%d' % Mv: (lambda Mv: lambda: _blob(Mv))(Mv) for Mv in VCC_MV}
VCC_CASES.update(last_legal=_last_legal, offsets=_offsets, ids=_ids, line=_line, runs=_runs, wrap=_wrap, speckle=_speckle, pair_wrap=_pair_wrap)


@functools.lru_cache(maxsize=None)
def vcc_case(name):
    return VCC_CASES[name]()


def beyond_case():
    """`ids` plus, as its LAST row, a solid voxel one step beyond the range: the RANGE bit, that voxel in no table (its own root), the rest as `ids`"""
    c = vcc_case('ids')
    return _vcc(np.concatenate([c['cells'], [[LIM, 0, 0]]]), np.concatenate([c['pan'], [1]]))


def duplicate_case():
    c = vcc_case('ids')
    return _vcc(np.concatenate([c['cells'], c['cells'][3:4]]), np.concatenate([c['pan'], [1]]))


def vote_pairs(comp, pan, small_c, m=None):
    """{(root << 32) | id: votes} from vcc_ref's pairs: one vote per (voxel of a small component, adjacent solid voxel of a component that is not
    small).  m = 'votes_per_neighbour': a neighbour counts once per small COMPONENT it touches, however many of its voxels"""
    cv, root = comp['component'], comp['root'].astype(np.int64)
    small = (cv >= 0) & small_c[np.maximum(cv, 0)]
    large = (cv >= 0) & ~small
    v, n = comp['pairs']
    vote = small[v] & large[n]
    v, n = v[vote], n[vote]
    if m == 'votes_per_neighbour' and len(v):
        rn = np.unique(np.stack([root[v], n], axis=1), axis=0)
        r, n = rn[:, 0], rn[:, 1]
    else:
        r = root[v]
    keys, votes = np.unique((r << 32) | pan[n].astype(np.int64), return_counts=True)
    return {int(k): int(c) for k, c in zip(keys, votes)}


def best_of(pairs, Mv, m=None):
    """uint64 [Mv] as pst_voxel_vote encodes the winner of every root: (votes << 32) | (0xFFFFFFFF - id), the largest such word - most votes, then the
    smallest id; 0 without a vote.  m = 'tie_larger': the largest id of the most voted"""
    best = np.zeros(Mv, dtype=np.uint64)
    chosen = {}
    for k, votes in pairs.items():
        r, pid = k >> 32, k & 0xFFFFFFFF
        rank = (votes, pid) if m == 'tie_larger' else (votes, -pid)
        if r not in chosen or rank > chosen[r][0]:
            chosen[r] = (rank, votes, pid)
    for r, (_, votes, pid) in chosen.items():
        best[r] = (votes << 32) | (0xFFFFFFFF - pid)
    return best


def v_vcc(case, connectivity=26, min_voxels=MIN_VOXELS, ncolors=7, m=None):
    """build .. apply on hand-written voxels -> dict(root int32 [Mv], size int32 [Mv], points int64 [Mv], lo, hi int32 [Mv, 3] (the workspace arrays:
    their initial values away from the roots), component, table, C, pairs, best uint64 [Mv], out_pan, out_colors, moved, gone).
    mistakes: votes_per_neighbour, tie_larger; known_le the colour of an id == ncolors is read (here: from one row beyond the table); link_27 the
    components of connectivity 26 whatever was asked (the votes still look at the asked neighbourhood)"""
    cells, pan, count = case['cells'], case['pan'], case['count']
    Mv = len(pan)
    comp = vcc_ref.components(cells, pan, count, 26 if m == 'link_27' else connectivity)
    if m == 'link_27':
        comp['pairs'] = vcc_ref.pairs(cells, connectivity)
    roots = comp['roots'].astype(np.int64)
    size, points = np.zeros(Mv, dtype=np.int32), np.zeros(Mv, dtype=np.int64)
    lo, hi = np.full((Mv, 3), INT_MAX, dtype=np.int32), np.full((Mv, 3), INT_MIN, dtype=np.int32)
    size[roots], points[roots], lo[roots], hi[roots] = comp['size'], comp['points'], comp['cell_lo'], comp['cell_hi']
    small_c = comp['size'] < min_voxels
    pairs = vote_pairs(comp, pan, small_c, m)
    best = best_of(pairs, Mv, m)
    cv = comp['component']
    small = (cv >= 0) & small_c[np.maximum(cv, 0)]
    b = best[np.maximum(comp['root'], 0)]
    won = np.where(b != 0, np.uint64(0xFFFFFFFF) - (b & np.uint64(0xFFFFFFFF)), np.uint64(0)).astype(np.int64)
    out_pan = np.where(small, won, pan).astype(np.int32)
    table = np.concatenate([case['colors'][:ncolors], np.full((1, 3), 0.5, dtype=F)])
    known = (out_pan > 0) & ((out_pan <= ncolors) if m == 'known_le' else (out_pan < ncolors))
    vis = np.where(known[:, None], table[np.where(known, out_pan, 0)], F(0)).astype(F)
    return {'root': comp['root'], 'size': size, 'points': points, 'lo': lo, 'hi': hi, 'component': comp['component'], 'C': len(roots),
            'table': {'root': comp['roots'], 'pan': comp['pan'], 'size': comp['size'], 'points': comp['points'], 'cell_lo': comp['cell_lo'], 'cell_hi': comp['cell_hi']},
            'pairs': pairs, 'best': best, 'out_pan': out_pan, 'out_colors': cloud_ref.blend(case['rgb'], vis, OPACITY),
            'moved': int((small & (out_pan > 0)).sum()), 'gone': int((small & (out_pan == 0)).sum()), 'small': small}


def loop_case():
    """(faces, M, (r, w)): two interleaved components on 205 rows; after the link parent[r] and parent[w] are overwritten to name each other - r the
    root of the second component, w another of its rows: every chain of that component ends in the two-cycle, none of the first does"""
    faces, M = _interleaved(100)
    return faces, M, (1, 3)


def vcc_loop_case():
    """(case, (r, w)): `blob_257` and the root and the last row of its first component of two voxels or more"""
    c = vcc_case('blob_257')
    v = v_vcc(c)
    r = int(v['table']['root'][np.argmax(v['table']['size'] >= 2)])
    return c, (r, int(np.nonzero(v['root'] == r)[0][-1]))
