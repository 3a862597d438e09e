"""Shared by tests/test_hip_score_stages.py (GPU) and tests/test_score_stage_checks.py (CPU): the cases that hold the kernels of csrc/depth_eval.hip
(sum, reduce, histogram, narrow) and csrc/evaluate.hip (count, areas, match, state) to their contract STAGE BY STAGE, fed by hand, at the bit patterns,
row counts, equalities and launch edges that a random depth map or a scene-shaped panoptic map hardly ever makes; and the plain restatements.  Numpy
only; nothing here imports the code under test (depth_eval_ref reads the three constants of the summation order from panst3r_amd.hip).

  median    `median_cases()`: name -> a list of slabs, each a list of views (pred, gt) fp32, written as uint32 bit patterns.  `median_ref(case)` sorts
            the bits of the valid values and takes the elements (n - 1) // 2 and n // 2.  `radix_median(bits, m)` walks the four byte passes with two
            ranks and two histograms as the kernels do (m = a planted mistake).
  reducer   `reducer_case(R)`: one slab of R one-pixel views (one block, one row of partials each) and a one-view slab after it; `moments_ref`,
            `errors_ref` are depth_eval_ref's fixed-order sums.
  match     `match_cases()`: name -> hand-made counts int32 [S, P+1, G+1] with cat_p, cat_g and what every probed pair was built for.  `v_match(counts,
            cat_p, cat_g, m)` restates areas, match, iou and state over a given table (m = a planted mistake); with no mistake it is
            eval_ref.tables_of_counts.
            "The first p wins" cannot be reached through a table: pst_pq_match sums the areas from the same table, union = ga + (pa - inter - void)
            >= ga >= inter + inter', so 2 inter > union and 2 inter' > union for two rows of one column contradict each other.  No case claims it.
  count     `count_cases()`: name -> pred, gt, slab_off, both id tables.  `count_ref(case)` is np.add.at over (slab, row, column); `v_count(case, m)`
            adds the pixels as pq_count_kernel<true> does - a lane of four pixels, runs of uniform lanes, heads by ballot - (m = a planted mistake).
            Equal slab offsets are allowed by include/panst3r_hip.h (step 2: such a slab is empty and its table stays cleared), so the cases hold them.
Every `v_*` / `radix_median` with no mistake IS the restatement, which tests/test_score_stage_checks.py asserts before it asserts which case catches
which planted mistake."""
import numpy as np

import depth_eval_ref as D
import eval_ref as E

F32, U32, I32, I64 = np.float32, np.uint32, np.int32, np.int64
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NAN_BITS = 0x7fc00000
CHUNK, LANES = D.ICP_CHUNK, D.ICP_LANES
FLT_MAX_BITS, ONE_DENORMAL = 0x7f7fffff, 0x00000001


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def f32(bits):
    """fp32 values of uint32 bit patterns"""
    return np.asarray(bits, dtype=np.uint64).astype(U32).view(F32)


def bits_of(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


# ============================================================================================================================================ median
def valid(p, g, min_depth=0.0, max_depth=np.inf):
    """step 1 of the contract without a confidence plane, in fp32"""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(g) & (g > F32(min_depth)) & (g <= F32(max_depth)) & np.isfinite(p) & (p > F32(0))


def median_of_bits(b):
    """the middle pair of sorted uint32 bit patterns of positive finite floats -> (a, b, the fp32 median as bits)"""
    b = np.sort(np.asarray(b, dtype=U32))
    n = len(b)
    if n == 0:
        return None, None, NAN_BITS
    lo, hi = b[(n - 1) // 2], b[n // 2]
    if n & 1:
        return int(lo), int(hi), int(lo)
    with np.errstate(over='ignore'):
        m = F32(F32(f32([lo])[0] + f32([hi])[0]) * F32(0.5))
    return int(lo), int(hi), int(bits_of([m])[0])


def median_ref(case, min_depth=0.0, max_depth=np.inf):
    """count int32 [S], median fp32 [S, 2] (of pred, of gt) of a case"""
    count, med = np.zeros(len(case), dtype=I32), np.zeros((len(case), 2), dtype=U32)
    for s, views in enumerate(case):
        p, g = np.concatenate([v[0] for v in views]), np.concatenate([v[1] for v in views])
        ok = valid(p, g, min_depth, max_depth)
        count[s] = ok.sum()
        med[s] = median_of_bits(bits_of(p)[ok])[2], median_of_bits(bits_of(g)[ok])[2]
    return count, med.view(F32)


def radix_median(b, m=None):
    """the radix select of depth_hist_kernel / select_narrow_kernel over the bits of the valid values of one (slab, quantity) -> the median's bits.
    m = 'rank0_hist': rank 1 walks rank 0's histogram from pass 1 on; 'below_own_lane': `below` is not taken from the lane that holds the bin"""
    b = np.asarray(b, dtype=np.uint64)
    n = len(b)
    prefix, rank = [0, 0], [(n - 1) // 2, n // 2]
    for q in range(4):
        shift = 24 - 8 * q
        hists = []
        for r in range(2):
            sel = b if q == 0 else b[(b >> (shift + 8)) == (prefix[r] >> (shift + 8))]
            hists.append(np.bincount(((sel >> shift) & 255).astype(np.int64), minlength=256))
        for r in range(2):
            h = hists[0 if (m == 'rank0_hist' and q > 0) else r]
            c, k = np.cumsum(h), rank[r]
            if c[-1] == 0 or k >= c[-1]:
                binr, below = 0, k
            else:
                binr = int(np.searchsorted(c, k, side='right'))
                below = int(c[binr] - h[binr])
                if m == 'below_own_lane':                          # the exclusive count of lane 0's first bin, as if the shuffle were left out
                    below = 0
            prefix[r] |= binr << shift
            rank[r] = k - below
    if n == 0:
        return NAN_BITS
    if n & 1:
        return prefix[0]
    with np.errstate(over='ignore'):
        return int(bits_of([F32(F32(f32([prefix[0]])[0] + f32([prefix[1]])[0]) * F32(0.5))])[0])


def _view(pb, gb, seed):
    """one view of the given bit patterns in a seeded order (pred and gt shuffled on their own: every pixel stays valid)"""
    r = rng(seed)
    return f32(r.permutation(np.asarray(pb, dtype=np.uint64))), f32(r.permutation(np.asarray(gb, dtype=np.uint64)))


def divergent_bits(k, prefix, c, m=6):
    """2 m + 2 bit patterns whose two middle values share the bytes above k (`prefix`, zero below) and differ first in byte k (c and c + 1): a has
    every lower byte 0xff, b every lower byte 0x00.  The m values below a share its byte k with other lower bytes, the m above b likewise, so that
    in every later pass the two ranks sit in different bins of DIFFERENT histograms: rank 0 is the last of its group, rank 1 the first of its own."""
    low = (1 << (8 * k)) - 1
    a, b = prefix | (c << (8 * k)) | low, prefix | ((c + 1) << (8 * k))
    if k == 0:
        below, above = [prefix | (c - 1 - i) for i in range(m)], [prefix | (c + 2 + i) for i in range(m)]
    else:
        step = max(low // (m + 2), 1)
        below = [prefix | (c << (8 * k)) | (low - (i + 1) * step) for i in range(m)]
        above = [prefix | ((c + 1) << (8 * k)) | ((i + 1) * step + 0x010101 % (low + 1)) for i in range(m)]
    out = below + [a, b] + above
    assert len(set(out)) == 2 * m + 2 and sorted(out)[m] == a and sorted(out)[m + 1] == b
    return out


# level -> (prefix of the bytes above it, the byte c of the lower middle value): k = 3 is 0x3fffffff next to 0x40000000
DIVERGE = {3: (0, 0x3f), 2: (0x41000000, 0x7f), 1: (0x3e990000, 0x10), 0: (0x42f6e900, 0x80)}


def first_different_byte(a, b):
    """the most significant byte (3 .. 0) at which two bit patterns differ, -1 if they are equal"""
    x = int(a) ^ int(b)
    return -1 if x == 0 else (x.bit_length() - 1) // 8


def bin_bits(B, c=3):
    """2 c + 1 bit patterns whose median lies in top-byte bin B, with c values below and c above it spread over the bins of OTHER lanes (B - 4, B - 9;
    B + 4, B + 9), the neighbouring bins of the same lane, and - where the positive floats end - the bin itself"""
    med = 0x00000003 if B == 0 else (B << 24) | 0x345678                             # (bin 0: denormals; bin 0x7f: FLT_MAX, three times, lies above)
    lo = [((B - d) << 24) | 0x7fffff for d in (1, 4, 9) if B - d >= 0]
    hi = [((B + d) << 24) | 0x000001 for d in (1, 4, 9) if B + d <= 0x7f]
    lo += [ONE_DENORMAL, 0x00000002, ONE_DENORMAL][:c - len(lo)] if B == 0 else [(B << 24) | 0x000010 + i for i in range(c - len(lo))]
    hi += [FLT_MAX_BITS] * (c - len(hi)) if B == 0x7f else [(B << 24) | 0x7ffff0 + i for i in range(c - len(hi))]
    out = lo[:c] + [med] + hi[:c]
    assert sorted(out)[c] == med and all(0 < x <= FLT_MAX_BITS for x in out)
    return out


BIN_SLABS = [4 * lane + q for lane in (0, 31) for q in range(4)]                     # slab i: pred's median in this bin, gt's in BIN_SLABS[7 - i]
TIES = (0x3f000000, 0x3f800001, 0x40490fdb)                                          # three distinct values: 0.5, 1 + ulp, pi
# pixels that are NOT valid, with bits that would move a median if they reached a histogram: (pred, gt)
INVALID = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (-np.inf, 1.0), (1.0, 0.0), (3e38, 0.0), (0.0, 1.0), (-0.0, 1.0), (-2.5, 1.0),
           (1.0, -1.0), (1e-45, -0.0), (-1e-45, 3e38)]


def with_invalid(view, seed):
    """the view with every INVALID pixel mixed in at seeded positions"""
    p, g = view
    r = rng(seed)
    at = np.sort(r.choice(len(p) + 1, len(INVALID)))
    bad = np.array(INVALID, dtype=F32)
    return np.insert(p, at, bad[:, 0]), np.insert(g, at, bad[:, 1])


def median_cases():
    cases = {}
    # n = 1 .. 4 distinct values, then all values equal for n = 5 and n = 4097
    small = []
    vals = [0x3f800000, 0x40400000, 0x3dcccccd, 0x41200000]
    for n in (1, 2, 3, 4):
        small.append([_view(vals[:n], [v + 0x00010203 for v in vals[:n]], n)])
    small.append([_view([0x3fc00000] * 5, [0x40a00001] * 5, 5)])
    small.append([_view([0x3fc00000] * (CHUNK + 1), [0x40a00001] * (CHUNK + 1), 6)])
    cases['small'] = small
    # the ranks part at byte k of pred and at byte 3 - k of gt, all four slabs in one launch
    cases['diverge'] = [[_view(divergent_bits(k, *DIVERGE[k]), divergent_bits(3 - k, *DIVERGE[3 - k]), 10 + k)] for k in (3, 2, 1, 0)]
    cases['bins'] = [[_view(bin_bits(B), bin_bits(BIN_SLABS[7 - i]), 20 + i)] for i, B in enumerate(BIN_SLABS)]
    # an even count at the top of the range: FLT_MAX + FLT_MAX rounds to +inf, and so does the median
    cases['overflow'] = [[_view([FLT_MAX_BITS, FLT_MAX_BITS], [0x7f000000, FLT_MAX_BITS], 25)]]
    # 4097 pixels of three values; the rank 2048 is the FIRST of its tie group for pred and the LAST of its group for gt
    n = CHUNK + 1
    first = [TIES[0]] * (n // 2) + [TIES[1]] * (n // 4 + 1) + [TIES[2]] * (n // 4)
    last = [TIES[0]] * (n // 4) + [TIES[1]] * (n // 4 + 1) + [TIES[2]] * (n // 2)
    assert len(first) == len(last) == n and first[n // 2 - 1] != first[n // 2] and last[n // 2] != last[n // 2 + 1]
    cases['ties'] = [[_view(first, last, 30)]]
    # valid counts 1, 0, 4097, 2; the slab with no valid pixel (every gt 0) between two that have some; slab 2 = three views of 5, 4097 + |INVALID|
    # and 3 pixels, the second of which straddles a chunk
    r = rng(31)
    body = r.integers(0x3e000000, 0x42000000, size=(2, CHUNK + 1 - 3), dtype=np.int64)
    zero = (f32(body[0][:9]), np.zeros(9, dtype=F32))
    cases['slabs'] = [[_view([0x3f8ccccd], [0x40133333], 32)],
                      [zero],
                      [_view(body[0][:5], body[1][:5], 33), with_invalid(_view(body[0][5:], body[1][5:], 34), 35), _view([0x42480000] * 3, [0x3c23d70a] * 3, 36)],
                      [_view([0x3f000000, 0x3f800000], [0x40000000, 0x40800000], 37)]]
    # invalid pixels around an even count whose ranks part at byte 1 (pred) and at byte 2 (gt)
    cases['invalid'] = [[with_invalid(_view(divergent_bits(1, *DIVERGE[1]), divergent_bits(2, *DIVERGE[2]), 40), 41)]]
    return cases


# ============================================================================================================================================ reducer
ALIGN = ((1.25, -0.125), (0.75, 0.5))                                                # (s, b) of the two slabs
THRESHOLDS = (1.03, 1.25)


def reducer_case(R):
    """one slab of R one-pixel views and a slab of one five-pixel view: R + 1 rows of partials, the first slab's rows [0, R).  Magnitudes over six
    decades, so that a sum in another order rounds differently; every 37th view has no valid pixel (its row of partials is +0.0)"""
    r = rng(100 + R)
    g = (10.0 ** r.uniform(-3, 3, R + 5)).astype(F32)
    p = (g * r.uniform(0.5, 1.5, R + 5).astype(F32)).astype(F32)
    g[36:R:37] = 0
    return [[(p[i:i + 1], g[i:i + 1]) for i in range(R)], [(p[R:], g[R:])]]


def _sums(case, terms):
    """partials float64 [nblocks, 16] and out float64 [S, 16] of a case under terms(slab, p, g, ok) -> float64 [live, npix]"""
    rows, out = [], np.zeros((len(case), D.DEPTH_MOMENTS))
    for s, views in enumerate(case):
        first = len(rows)
        for p, g in views:
            t = terms(s, p, g, valid(p, g))
            part = np.zeros(((len(p) + CHUNK - 1) // CHUNK, D.DEPTH_MOMENTS))
            for k in range(len(t)):
                part[:, k] = D.view_partials(t[k])
            rows.extend(part)
        slab = np.array(rows[first:])
        for k in range(slab.shape[1]):
            out[s, k] = D.reduce_rows(slab[:, k])
    return np.array(rows), out


def moments_ref(case):
    return _sums(case, lambda s, p, g, ok: D.align_terms(p, g, ok))


def errors_ref(case, align=ALIGN, thresholds=THRESHOLDS):
    return _sums(case, lambda s, p, g, ok: D.error_terms(p, g, ok, align[s][0], align[s][1], thresholds))


# ============================================================================================================================================ match / state
def v_match(counts, cat_p, cat_g, m=None):
    """steps 4 - 6 of the contract over a given table -> dict(pred_area, gt_area, match, iou, pred_state).  m = 'ge': 2 inter >= union matches;
    'uni_int32': the union is computed in wrapping int32; 'ignore_ge': 2 void >= area is ignored; 'no_void': the void column stays in the union"""
    c = np.asarray(counts).astype(I64)
    S, P, G = c.shape[0], c.shape[1] - 1, c.shape[2] - 1
    pa, ga = c[:, :P, :].sum(axis=2), c[:, :, :G].sum(axis=1)
    match, iou, state = np.full((S, G), -1, dtype=I32), np.zeros((S, G)), np.zeros((S, P), dtype=I32)
    for s in range(S):
        for g in range(G):
            if ga[s, g] == 0:
                continue
            for p in range(P):
                if pa[s, p] == 0 or cat_p[p] != cat_g[g]:
                    continue
                inter = int(c[s, p, g])
                union = int(pa[s, p]) + int(ga[s, g]) - inter - (0 if m == 'no_void' else int(c[s, p, G]))
                if m == 'uni_int32':
                    union = (union + 2 ** 31) % 2 ** 32 - 2 ** 31
                if (2 * inter >= union if m == 'ge' else 2 * inter > union) and match[s, g] < 0:
                    match[s, g] = p
                    with np.errstate(divide='ignore', invalid='ignore'):
                        iou[s, g] = np.float64(inter) / np.float64(union)
        for p in range(P):
            if pa[s, p] > 0:
                v, a = 2 * int(c[s, p, G]), int(pa[s, p])
                state[s, p] = E.MATCHED if (match[s] == p).any() else (E.IGNORED if (v >= a if m == 'ignore_ge' else v > a) else E.FP)
    return {'pred_area': pa.astype(I32), 'gt_area': ga.astype(I32), 'match': match, 'iou': iou, 'pred_state': state}


def pair_margin(counts, s, p, g):
    """2 inter - union of a pair, in Python integers"""
    c = np.asarray(counts).astype(I64)
    inter, pa, ga = int(c[s, p, g]), int(c[s, p, :].sum()), int(c[s, :, g].sum())
    return 2 * inter - (pa + ga - inter - int(c[s, p, -1]))


def _table(S, P, G):
    return np.zeros((S, P + 1, G + 1), dtype=I32)


def random_table(S, P, G, seed):
    """a seeded table with a heavy diagonal p == g (matches), light clutter (misses), void row and column, absent rows and columns, categories
    that cycle through three; the LAST column (void, or the only one) and column 64 hold non-zero counts"""
    r = rng(seed)
    c = r.integers(0, 3, (S, P + 1, G + 1)) * (r.random((S, P + 1, G + 1)) < 0.05)
    for s in range(S):
        for g in range(G):
            if g < P and g % 7 != 5:
                c[s, g, g] += r.integers(20, 40)
    c[:, :, G] += 1
    if G >= 64:
        c[:, :, 64] += 2
    if P > 3:
        c[:, 2, :] = 0                                                               # an absent row ...
        c[S - 1, 3, :G] = 0
        c[S - 1, 3, G] = 9                                                           # ... and one that lies on void alone
    if G > 3:
        c[:, :, 1] = 0                                                               # an absent column
    return c.astype(I32), (np.arange(P) % 3).astype(I32), (np.arange(G) % 3).astype(I32)


# (S, P, G): G + 1 in {1, 63, 64, 65, 129}; S P in {1, 3, 4, 5}; S G and S P in {255, 256, 257}; an empty side
EDGE_SHAPES = [(1, 1, 0), (1, 3, 62), (2, 2, 63), (1, 5, 64), (1, 2, 128), (3, 85, 85), (4, 64, 64), (1, 257, 257), (1, 256, 255), (2, 0, 5), (2, 5, 0), (1, 0, 0)]


def match_cases():
    """name -> dict(counts, cat_p, cat_g, margins = {(s, p, g): 2 inter - union the pair was built for}, states = {(s, p): state})"""
    cases = {}
    # rule: rows 0 and 1 have inter 5, pa 8, ga 7 against columns 0 and 1; row 1 has ONE of its pixels on void.  Column 2 (another category) takes
    # the rest of the rows, the void row the rest of the columns.
    c = _table(1, 2, 3)
    c[0, 0, 0], c[0, 0, 2], c[0, 2, 0] = 5, 3, 2
    c[0, 1, 1], c[0, 1, 2], c[0, 1, 3], c[0, 2, 1] = 5, 2, 1, 2
    cases['rule'] = dict(counts=c, cat_p=[0, 0], cat_g=[0, 0, 1], margins={(0, 0, 0): 0, (0, 1, 1): 1}, states={(0, 0): E.FP, (0, 1): E.MATCHED})
    # exclusions: (0, 0) IoU 1 in different categories; column 1 and row 1 absent, next to (2, 2) with IoU 1
    c = _table(1, 3, 3)
    c[0, 0, 0], c[0, 2, 2] = 11, 7
    cases['exclusions'] = dict(counts=c, cat_p=[0, 1, 1], cat_g=[1, 1, 1], margins={(0, 0, 0): 11, (0, 2, 2): 7}, states={(0, 0): E.FP, (0, 1): E.ABSENT, (0, 2): E.MATCHED})
    # int64: pa = ga = 1.5e9.  Three cells, N = 1.6e9 <= 2^31 - 1: a match with iou 14 / 15
    c = _table(1, 1, 1)
    c[0, 0, 0], c[0, 0, 1], c[0, 1, 0] = 1_400_000_000, 100_000_000, 100_000_000
    cases['int64_match'] = dict(counts=c, cat_p=[2], cat_g=[2], margins={(0, 0, 0): 2_800_000_000 - 1_500_000_000}, states={(0, 0): E.MATCHED})
    # int64: inter = 5e8 of the same areas, the rest of the row in a column of another category: union = 2.5e9 > 2^31, no match
    c = _table(1, 1, 2)
    c[0, 0, 0], c[0, 0, 1], c[0, 1, 0] = 500_000_000, 1_000_000_000, 1_000_000_000
    cases['int64_none'] = dict(counts=c, cat_p=[2], cat_g=[2, 1], margins={(0, 0, 0): 1_000_000_000 - 2_500_000_000}, states={(0, 0): E.FP})
    # state, two slabs: row 0 has 3 of 6 pixels on void (FP) and row 1 has 4 of 7 (ignored), both on a column of another category; row 2 matches;
    # row 3 is absent; row 4 matches column 3 in slab 0 and lies on void, with one pixel on column 3, in slab 1
    c = _table(2, 5, 4)
    for s in (0, 1):
        c[s, 0, 0], c[s, 0, 4] = 3, 3
        c[s, 1, 0], c[s, 1, 4] = 3, 4
        c[s, 2, 2] = 9
    c[0, 4, 3], c[1, 4, 4], c[1, 4, 3], c[1, 5, 3] = 6, 5, 1, 4
    st = {(s, p): v for s in (0, 1) for p, v in ((0, E.FP), (1, E.IGNORED), (2, E.MATCHED), (3, E.ABSENT))}
    st.update({(0, 4): E.MATCHED, (1, 4): E.IGNORED})
    cases['state'] = dict(counts=c, cat_p=[0, 0, 1, 1, 2], cat_g=[1, 0, 1, 2], margins={(0, 4, 3): 6, (1, 4, 3): -3}, states=st)
    for i, (S, P, G) in enumerate(EDGE_SHAPES):
        c, cp, cg = random_table(S, P, G, 200 + i)
        cases['edge_%d_%d_%d' % (S, P, G)] = dict(counts=c, cat_p=cp, cat_g=cg, margins={}, states={})
    return cases


# ============================================================================================================================================ count
PT, WAVE, WG = 4, 64, 1024                                                            # pixels per lane, lanes per wave, pixels per workgroup
NONE = 0xffffffff


def rows_of(ids, tab, n):
    """step 1: 0 < i < ntab and tab[i] in [0, n) -> tab[i], else the void row n"""
    ids, tab = np.asarray(ids).astype(I64), np.asarray(tab).astype(I64)
    ok = (ids > 0) & (ids < len(tab))
    r = np.full(len(ids), n, dtype=I64)
    r[ok] = tab[ids[ok]]
    r[(r < 0) | (r >= n)] = n
    return r


def pixel_keys(case):
    """(slab * (P + 1) + row) * (G + 1) + column of every pixel"""
    off, P, G = np.asarray(case['slab_off']), case['P'], case['G']
    i = np.arange(len(case['pred']))
    slab = np.searchsorted(off[1:], i, side='right')                                  # the slab whose [off[s], off[s + 1]) holds i: empty slabs hold none
    return (slab * (P + 1) + rows_of(case['pred'], case['tab_p'], P)) * (G + 1) + rows_of(case['gt'], case['tab_g'], G)


def count_ref(case):
    S, P, G = len(case['slab_off']) - 1, case['P'], case['G']
    c = np.zeros(S * (P + 1) * (G + 1), dtype=I64)
    np.add.at(c, pixel_keys(case), 1)
    return c.reshape(S, P + 1, G + 1).astype(I32)


def lane_keys(case):
    """uint32 [waves, 64, 4]: the key of every pixel slot of every lane, NONE beyond N"""
    k = pixel_keys(case)
    waves = (len(k) + WG - 1) // WG * (WG // (WAVE * PT))
    out = np.full(waves * WAVE * PT, NONE, dtype=np.int64)
    out[:len(k)] = k
    return out.reshape(waves, WAVE, PT)


def lane_runs(case):
    """wave -> [(a, b, key)]: the maximal intervals [a, b) of adjacent UNIFORM lanes (four equal keys) that hold one key, NONE included"""
    runs = {}
    for w, lanes in enumerate(lane_keys(case)):
        out, a = [], None
        for l in range(WAVE + 1):
            uni = l < WAVE and (lanes[l] == lanes[l, 0]).all()
            if a is not None and (not uni or lanes[l, 0] != lanes[a, 0]):
                out.append((a, l, int(lanes[a, 0])))
                a = None
            if uni and a is None:
                a = l
        runs[w] = out
    return runs


def v_count(case, m=None):
    """the adds of pq_count_kernel<true>.  m = 'no_prev_uniform': a uniform lane after a NON-uniform one that starts with its key is no head;
    'none_adds': the run of lanes beyond N is added like any other (to the last cell, where key NONE would wrap to in a table of that size)"""
    S, P, G = len(case['slab_off']) - 1, case['P'], case['G']
    c = np.zeros(S * (P + 1) * (G + 1), dtype=I64)
    for lanes in lane_keys(case):
        uni = (lanes == lanes[:, :1]).all(axis=1)
        head = np.array([l == 0 or not uni[l] or (m != 'no_prev_uniform' and not uni[l - 1]) or lanes[l - 1, 0] != lanes[l, 0] for l in range(WAVE)])
        for l in range(WAVE):
            if uni[l]:
                if head[l]:
                    nxt = [j for j in range(l + 1, WAVE) if head[j]]
                    n = (nxt[0] if nxt else WAVE) - l
                    if lanes[l, 0] != NONE:
                        c[lanes[l, 0]] += PT * n
                    elif m == 'none_adds':
                        c[-1] += PT * n
            else:
                for k in lanes[l][lanes[l] != NONE]:
                    c[k] += 1
    return c.reshape(S, P + 1, G + 1).astype(I32)


TAB_P = np.array([0, 0, 1, -1, 3, 2], dtype=I32)                                      # P = 3: id 1 -> 0, 2 -> 1, 3 -> entry -1, 4 -> entry P, 5 = ntab - 1 -> 2
TAB_G = np.array([1, -1, 0, 1, 7, INT_MIN, 2, 3], dtype=I32)                          # G = 4: id 1 -> entry -1, 2 -> 0, 3 -> 1, 4 -> 7 (> G), 5 -> INT_MIN, 6 -> 2, 7 -> 3
EDGE_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, INT_MIN, INT_MAX]                           # 0, ntab - 1 and ntab of either table, the negative and the huge ones


def _stream(N, seed, slab_off=None):
    r = rng(seed)
    return dict(pred=r.choice(EDGE_IDS, N).astype(I32), gt=r.choice(EDGE_IDS, N).astype(I32), slab_off=np.array([0, N] if slab_off is None else slab_off, dtype=I64),
                tab_p=TAB_P, tab_g=TAB_G, P=3, G=4)


def _paint(N, spans, slab_off=None):
    """a stream of N pixels, (1, 2) everywhere but the given spans (first pixel, end pixel, pred id, gt id)"""
    case = _stream(N, 0, slab_off)
    case['pred'][:], case['gt'][:] = 1, 2
    for a, b, p, g in spans:
        case['pred'][a:b], case['gt'][a:b] = p, g
    return case


def lane(w, l):
    """the first pixel of lane l of wave w"""
    return (w * WAVE + l) * PT


# the run case: wave -> the runs [a, b) it is built to hold (keys aside); tests/test_score_stage_checks.py compares them with lane_runs
RUNS = {0: [(0, 64)], 1: [(0, 1), (1, 63), (63, 64)], 2: [(10, 64)], 3: [(0, 20), (20, 32), (32, 64)], 4: [(0, 17), (18, 64)], 5: [(0, 30), (30, 64)],
        6: [(0, 40), (41, 64)], 7: [(0, 64)]}
RUN_N = lane(6, 40) + 2


def run_case():
    """eight waves in two workgroups; the stream ends two pixels into lane 40 of wave 6, wave 7 lies beyond N"""
    spans = [(lane(1, 0), lane(1, 1), 2, 3), (lane(1, 63), lane(2, 0), 5, 6)]                     # [0, 1) and [63, 64) of wave 1 around [1, 63)
    spans += [(lane(2, l) + 1, lane(2, l) + 2, 2, 7) for l in range(10)]                          # ten non-uniform lanes, each starting with the key (1, 2)
    spans += [(lane(2, 10), lane(3, 20), 2, 6)]                                                   # [10, 64) continued to lane 20 of wave 3
    spans += [(lane(3, 20), lane(3, 32), 5, 3), (lane(3, 32), lane(4, 0), 1, 7)]                  # two runs meet at lane 32
    spans += [(lane(4, 17) + 2, lane(4, 17) + 3, 5, 2)]                                           # one lane (1, 2) (1, 2) (5, 2) (1, 2) inside a run of (1, 2)
    return _paint(RUN_N, spans, [0, lane(5, 30), RUN_N])                                          # a slab boundary between lanes 29 and 30 of wave 5


def count_cases():
    cases = {'n_%d' % N: _stream(N, 300 + N) for N in (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)}
    cases['n_1027_two_slabs'] = _stream(1027, 299, [0, 513, 1027])
    # lengths 0, 1, 2, 3, 0, 0, 5, ...: a lane crosses up to three boundaries; boundaries at every residue mod 4, at a wave edge (256) and a workgroup
    # edge (1024); empty slabs first, in the middle and last
    cases['slabs'] = _stream(1030, 310, [0, 0, 1, 3, 6, 6, 6, 11, 256, 257, 1024, 1026, 1030, 1030])
    cases['slabs_uniform'] = _paint(1030, [], [0, 0, 1, 3, 6, 6, 6, 11, 256, 257, 1024, 1026, 1030, 1030])
    cases['runs'] = run_case()
    whole, n = run_case(), lane(6, 40)                                                # the stream ends between two lanes: a run of (1, 2) next to the run beyond N
    cases['runs_whole_lanes'] = dict(whole, pred=whole['pred'][:n].copy(), gt=whole['gt'][:n].copy(), slab_off=np.array([0, lane(5, 30), n], dtype=I64))
    one = _stream(77, 320)
    cases['ntab_1'] = dict(one, tab_p=np.array([0], dtype=I32), tab_g=np.array([-1], dtype=I32))
    return cases
