"""The cases of tests/score_stage_cases.py hold what they were built for, the restatements agree with the references that exist, and the planted
mistakes are caught (CPU only, no GPU), as tests/test_topo_stage_checks.py shows for the surface, simplify and component stages.

Median: for every divergence case the first byte at which the two order statistics differ is computed from the bits; for the bin cases the top byte
of the median; the sort-based reference equals np.median (odd counts) and depth_eval_ref.median32, and the byte-wise walk `radix_median` equals both.
Match: 2 inter - union of every probed pair is the number the case names, the areas of the int64 cases add to more than 2^31, `v_match` equals
eval_ref.tables_of_counts and, on tables that come from maps, eval_ref.tables.  Count: the lane intervals of equal keys are the ones the run case
names, and `v_count`, which adds as the merging kernel does, equals the plain np.add.at.  CAUGHT records which case differs from the restatement under
which planted mistake, BLIND which case must not."""
import numpy as np
import pytest

import depth_eval_ref as D
import eval_ref as E
import score_stage_cases as C

MEDIAN, MATCH, COUNT = C.median_cases(), C.match_cases(), C.count_cases()


def slab_bits(views):
    """the bits of the valid (pred, gt) of a slab"""
    p, g = np.concatenate([v[0] for v in views]), np.concatenate([v[1] for v in views])
    ok = C.valid(p, g)
    return C.bits_of(p)[ok], C.bits_of(g)[ok]


# ============================================================================================================================================ median
def test_the_ranks_part_at_the_byte_each_case_names():
    for slab, k in zip(MEDIAN['diverge'], (3, 2, 1, 0)):
        pb, gb = slab_bits(slab)
        assert len(pb) % 2 == 0
        a, b, _ = C.median_of_bits(pb)
        assert C.first_different_byte(a, b) == k and (k != 3 or (a, b) == (0x3fffffff, 0x40000000))
        a, b, _ = C.median_of_bits(gb)
        assert C.first_different_byte(a, b) == 3 - k
    pb, gb = slab_bits(MEDIAN['invalid'][0])
    assert C.first_different_byte(*C.median_of_bits(pb)[:2]) == 1 and C.first_different_byte(*C.median_of_bits(gb)[:2]) == 2
    assert float(C.f32([0x3fffffff])[0]) < 2.0 == float(C.f32([0x40000000])[0])


def test_every_pass0_bin_position_and_the_ends_of_the_range():
    assert C.BIN_SLABS == [0, 1, 2, 3, 124, 125, 126, 127]
    seen = set()
    for i, slab in enumerate(MEDIAN['bins']):
        pb, gb = slab_bits(slab)
        mp, mg = C.median_of_bits(pb)[2], C.median_of_bits(gb)[2]
        assert mp >> 24 == C.BIN_SLABS[i] and mg >> 24 == C.BIN_SLABS[7 - i]
        seen |= {mp, mg}
        for b, B in ((pb, C.BIN_SLABS[i]), (gb, C.BIN_SLABS[7 - i])):             # counts below and above the bin; where the range allows, in other lanes
            top = (b >> 24).astype(int)
            assert (b < C.median_of_bits(b)[2]).sum() == 3 == (np.sort(b)[4:] >= C.median_of_bits(b)[2]).sum()
            assert B < 4 or (top // 4 < B // 4).any()
            assert B > 123 or (top // 4 > B // 4).any()
    assert 0x7f345678 in seen and 0x00000003 in seen and C.FLT_MAX_BITS in slab_bits(MEDIAN['bins'][7])[0]
    assert C.ONE_DENORMAL in slab_bits(MEDIAN['bins'][0])[0] and float(C.f32([C.ONE_DENORMAL])[0]) > 0
    assert C.median_ref(MEDIAN['overflow'])[1].view(np.uint32).tolist() == [[0x7f800000, 0x7f800000]]


def test_small_counts_ties_and_slabs():
    assert C.median_ref(MEDIAN['small'])[0].tolist() == [1, 2, 3, 4, 5, C.CHUNK + 1]
    for slab in MEDIAN['small'][4:]:
        assert all(len(set(b.tolist())) == 1 for b in slab_bits(slab))
    pb, gb = (np.sort(b) for b in slab_bits(MEDIAN['ties'][0]))
    n = C.CHUNK + 1
    assert len(pb) == n and set(pb.tolist()) == set(gb.tolist()) == set(C.TIES)
    assert pb[n // 2 - 1] != pb[n // 2] == pb[n // 2 + 1] and gb[n // 2 - 1] == gb[n // 2] != gb[n // 2 + 1]      # first and last of a tie group
    count, med = C.median_ref(MEDIAN['slabs'])
    assert count.tolist() == [1, 0, C.CHUNK + 1, 2] and med.view(np.uint32)[1].tolist() == [C.NAN_BITS] * 2
    assert [len(v[0]) for v in MEDIAN['slabs'][2]] == [5, C.CHUNK + 1 - 8 + len(C.INVALID), 3]
    assert len(MEDIAN['slabs'][2][1][0]) > C.CHUNK and (MEDIAN['slabs'][1][0][1] == 0).all()


def test_no_invalid_pixel_is_valid_and_each_would_move_a_median():
    bad = np.array(C.INVALID, dtype=np.float32)
    assert not C.valid(bad[:, 0], bad[:, 1]).any()
    p, g = MEDIAN['invalid'][0][0]
    assert len(p) == 14 + len(C.INVALID) and C.valid(p, g).sum() == 14
    every = np.ones(len(p), dtype=bool)
    assert C.median_of_bits(C.bits_of(p))[2] != C.median_of_bits(C.bits_of(p)[C.valid(p, g)])[2] and every.sum() > 14


def test_the_median_restatement_is_the_reference():
    r = C.rng(1)
    for name, case in MEDIAN.items():
        count, med = C.median_ref(case)
        for s, slab in enumerate(case):
            p, g = np.concatenate([v[0] for v in slab]), np.concatenate([v[1] for v in slab])
            ok = D.valid(p, g, None, None, 0.0, np.inf)
            assert np.array_equal(ok, C.valid(p, g)) and count[s] == ok.sum()
            for q, x in enumerate((p[ok], g[ok])):
                want = D.median32(x)
                assert np.array_equal(med[s, q:q + 1].view(np.uint32), np.array([want], dtype=np.float32).view(np.uint32)), (name, s, q)
                assert C.radix_median(C.bits_of(x)) == int(med[s, q:q + 1].view(np.uint32)[0]), (name, s, q)
                if len(x) & 1:
                    with np.errstate(over='ignore'):
                        assert np.float32(np.median(x.astype(np.float64))) == med[s, q]
    for n in (1, 2, 7, 100, 101):                                                # and on random bits, where a walk and a sort have nothing in common
        b = r.integers(1, C.FLT_MAX_BITS + 1, n, dtype=np.int64)
        assert C.radix_median(b) == C.median_of_bits(b)[2] == int(C.bits_of([D.median32(C.f32(b))])[0])


# mistake -> median cases in which some (slab, quantity) must differ from the restatement under it
CAUGHT_MEDIAN = {'rank0_hist': {'diverge', 'invalid'}, 'below_own_lane': {'bins', 'diverge', 'slabs'}}
BLIND_MEDIAN = {'rank0_hist': {'bins', 'ties'}}                                 # odd counts: one rank


@pytest.mark.parametrize('m', sorted(CAUGHT_MEDIAN))
def test_planted_median_mistakes(m):
    def differs(name):
        return any(C.radix_median(b, m) != C.radix_median(b) for slab in MEDIAN[name] for b in slab_bits(slab))
    assert all(differs(n) for n in CAUGHT_MEDIAN[m]) and not any(differs(n) for n in BLIND_MEDIAN.get(m, ()))
    if m == 'rank0_hist':                                                        # every level with a later pass catches it, for pred or for gt
        for slab, k in zip(MEDIAN['diverge'], (3, 2, 1, 0)):
            pb, gb = slab_bits(slab)
            assert (C.radix_median(pb, m) != C.radix_median(pb)) == (k > 0) and (C.radix_median(gb, m) != C.radix_median(gb)) == (3 - k > 0)


# ============================================================================================================================================ reducer
@pytest.mark.parametrize('R', (255, 256, 257, 513))
def test_reducer_cases(R):
    case = C.reducer_case(R)
    assert [len(s) for s in case] == [R, 1] and all(len(v[0]) == 1 for v in case[0]) and len(case[1][0][0]) == 5
    partials, out = C.moments_ref(case)
    assert partials.shape == (R + 1, D.DEPTH_MOMENTS) and out.shape == (2, D.DEPTH_MOMENTS)
    n = sum(int(C.valid(*v).sum()) for v in case[0])
    assert out[0, 0] == n and R - R // 37 - 1 <= n < R and out[1, 0] == 5 and (out[:, 5:] == 0).all()
    # the reference is depth_eval_ref's own slab sum; and the order is felt: a plain left-to-right sum of the rows differs in some moment
    terms = [D.align_terms(p, g, C.valid(p, g)) for p, g in case[0]]
    assert all(out[0, k] == D.slab_sum([t[k] for t in terms]) for k in range(5))
    assert any(out[0, k] != np.cumsum(partials[:R, k])[-1] for k in range(1, 5))
    ep, eo = C.errors_ref(case)
    assert eo[0, 0] == n and (eo[:, 5:7] <= eo[:, :1]).all() and (eo[:, 7:] == 0).all() and 0 < eo[0, 5] < eo[0, 6] < n


# ============================================================================================================================================ match / state
def test_every_probed_pair_has_the_margin_it_names():
    for name, case in MATCH.items():
        for (s, p, g), want in case['margins'].items():
            assert C.pair_margin(case['counts'], s, p, g) == want, (name, s, p, g)
    rule = MATCH['rule']
    c = rule['counts'].astype(np.int64)
    assert sorted(rule['margins'].values()) == [0, 1]
    assert c[0, 0, 0] == c[0, 1, 1] and c[0, 0].sum() == c[0, 1].sum() and c[0, :, 0].sum() == c[0, :, 1].sum() and (c[0, 0, -1], c[0, 1, -1]) == (0, 1)
    for name in ('int64_match', 'int64_none'):
        c = MATCH[name]['counts'].astype(np.int64)
        assert c[0, 0].sum() == c[0, :, 0].sum() == 1_500_000_000 and c[0, 0].sum() + c[0, :, 0].sum() > 2 ** 31 and c.max() < 2 ** 31
    assert MATCH['int64_match']['counts'].astype(np.int64).sum() <= C.INT_MAX and np.count_nonzero(MATCH['int64_match']['counts']) == 3
    st = MATCH['state']['counts'].astype(np.int64)
    assert 2 * st[0, 0, -1] == st[0, 0].sum() and 2 * st[0, 1, -1] == st[0, 1].sum() + 1


def test_the_table_restatement_is_the_reference():
    for name, case in MATCH.items():
        got, want = C.v_match(case['counts'], case['cat_p'], case['cat_g']), E.tables_of_counts(case['counts'], case['cat_p'], case['cat_g'])
        assert all(got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() for k in want), name
        for (s, p), v in case['states'].items():
            assert want['pred_state'][s, p] == v, (name, s, p)
        for (s, p, g), margin in case['margins'].items():
            assert (want['match'][s, g] == p) == (margin > 0 and case['cat_p'][p] == case['cat_g'][g]), (name, s, p, g)
    assert MATCH['rule']['margins'] and E.tables_of_counts(**{k: MATCH['rule'][k] for k in ('counts', 'cat_p', 'cat_g')})['iou'][0, 1] == 5.0 / 9.0
    assert E.tables_of_counts(**{k: MATCH['int64_match'][k] for k in ('counts', 'cat_p', 'cat_g')})['iou'][0, 0] == 1.4e9 / 1.5e9
    # and on tables that come from maps: two of the random cases of tests/test_hip_eval.py, both scopes
    for shapes in ([(24, 32), (24, 32)], [(24, 32), (32, 24), (23, 31)]):
        pred, info, gt, gseg = E.random_segments(shapes, 6, 5, seed=1)
        for scope in ('scene', 'view'):
            want = E.tables(pred, info, gt, gseg, scope)
            cat_p, cat_g = E.id_table(info)[1], E.id_table(gseg)[1]
            for got in (C.v_match(want['counts'], cat_p, cat_g), E.tables_of_counts(want['counts'], cat_p, cat_g)):
                assert all(got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() for k in got)
            assert (want['match'] >= 0).any() and (want['pred_state'] == E.IGNORED).any()


def test_the_launch_edges_are_the_ones_named():
    shapes, states = C.EDGE_SHAPES, set()
    assert {G + 1 for _, _, G in shapes} >= {1, 63, 64, 65, 129} and {S * P for S, P, _ in shapes} >= {1, 3, 4, 5, 255, 256, 257}
    assert {S * G for S, _, G in shapes} >= {255, 256, 257} and any(P == 0 and G > 0 for _, P, G in shapes) and any(P > 0 and G == 0 for _, P, G in shapes)
    for S, P, G in shapes:
        case = MATCH['edge_%d_%d_%d' % (S, P, G)]
        c = case['counts']
        assert c.shape == (S, P + 1, G + 1) and c.dtype == np.int32 and c[:, :, G].any() and (G < 64 or c[:, :, 64].any())
        if P > 3 and G > 3:
            ref = E.tables_of_counts(c, case['cat_p'], case['cat_g'])
            states |= set(ref['pred_state'].reshape(-1).tolist())
            assert (ref['match'] >= 0).any() and (ref['gt_area'] == 0).any() and (ref['pred_area'] == 0).any()
    assert states == {0, 1, 2, 3}


# mistake -> match cases that must differ from the restatement under it.  int64_match is blind to a wrapping int32 union: its areas add to 3e9, but
# the union itself, 1.5e9, fits, and a sum that wraps twice comes back to it; int64_none, whose union is 2.5e9, catches it.
CAUGHT_MATCH = {'ge': {'rule'}, 'uni_int32': {'int64_none'}, 'ignore_ge': {'state'}, 'no_void': {'rule', 'int64_match'}}
BLIND_MATCH = {'ge': {'exclusions', 'int64_match', 'int64_none'}, 'uni_int32': {'rule', 'state', 'int64_match'}, 'ignore_ge': {'rule'}}


@pytest.mark.parametrize('m', sorted(CAUGHT_MATCH))
def test_planted_match_mistakes(m):
    def differs(name):
        case = MATCH[name]
        got, want = C.v_match(case['counts'], case['cat_p'], case['cat_g'], m), C.v_match(case['counts'], case['cat_p'], case['cat_g'])
        return any(got[k].tobytes() != want[k].tobytes() for k in want)
    assert all(differs(n) for n in CAUGHT_MATCH[m]) and not any(differs(n) for n in BLIND_MATCH.get(m, ()))


# ============================================================================================================================================ count
def test_the_runs_are_the_lane_intervals_named():
    runs = C.lane_runs(COUNT['runs'])
    assert {w: [(a, b) for a, b, _ in r] for w, r in runs.items()} == C.RUNS
    key = {w: [k for _, _, k in r] for w, r in runs.items()}
    assert key[2][0] == key[3][0] and key[3][1] != key[3][2]                     # [10, 64) goes on into the next wave; two keys meet at lane 32
    assert key[4][0] == key[4][1] and C.lane_keys(COUNT['runs'])[4, 17].tolist().count(key[4][0]) == 3 and C.lane_keys(COUNT['runs'])[4, 17, 0] == key[4][0]
    assert key[5][0] != key[5][1] and COUNT['runs']['slab_off'][1] == C.lane(5, 30)                    # the same ids on either side of a slab boundary
    assert (COUNT['runs']['pred'][C.lane(5, 0):C.lane(6, 0)] == 1).all()
    assert key[6][1] == key[7][0] == C.NONE and C.lane_keys(COUNT['runs'])[6, 40].tolist().count(C.NONE) == 2
    assert [(a, b) for a, b, _ in C.lane_runs(COUNT['runs_whole_lanes'])[6]] == [(0, 40), (40, 64)]


def test_the_streams_hold_the_sizes_slabs_and_ids_named():
    assert {len(COUNT['n_%d' % n]['pred']) for n in (1, 2, 3, 4, 5, 1023, 1024, 1025, 1027)} == {1, 2, 3, 4, 5, 1023, 1024, 1025, 1027}
    off = COUNT['slabs']['slab_off']
    assert np.diff(off).tolist()[:7] == [0, 1, 2, 3, 0, 0, 5] and off[0] == 0 and off[-1] == off[-2] == 1030 == len(COUNT['slabs']['pred'])
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and {256, 1024} <= set(off.tolist()) and (np.diff(off) >= 0).all()
    assert max(np.bincount(off[1:-1] // 4)) >= 3                                 # three boundaries inside one lane's four pixels
    ref = C.count_ref(COUNT['slabs'])
    assert ref.sum(axis=(1, 2)).tolist() == np.diff(off).tolist()
    ids = set(C.EDGE_IDS)
    assert {0, -1, C.INT_MIN, C.INT_MAX, len(C.TAB_P) - 1, len(C.TAB_P), len(C.TAB_G) - 1, len(C.TAB_G)} <= ids
    assert C.rows_of(C.EDGE_IDS, C.TAB_P, 3).tolist() == [3, 0, 1, 3, 3, 2, 3, 3, 3, 3, 3, 3]          # entry -1, entry P and id 0 (whose entry is a row) are void
    assert C.rows_of(C.EDGE_IDS, C.TAB_G, 4).tolist() == [4, 4, 0, 1, 4, 4, 2, 3, 4, 4, 4, 4]
    for name in ('n_1027', 'slabs'):
        assert ids <= set(COUNT[name]['pred'].tolist()) and ids <= set(COUNT[name]['gt'].tolist())
    one = C.count_ref(COUNT['ntab_1'])
    assert one[0, 3, 4] == 77 == one.sum()


def test_the_count_restatements_agree():
    for name, case in COUNT.items():
        ref = C.count_ref(case)
        assert ref.sum() == len(case['pred']) and np.array_equal(C.v_count(case), ref), name
    # against eval_ref.rows_of / tables on maps whose tables have no entry beyond the rows
    pred, info, gt, gseg = E.random_segments([(24, 32), (23, 31)], 6, 5, seed=1)
    tp, tg = E.id_table(info)[0], E.id_table(gseg)[0]
    case = dict(pred=np.concatenate([m.reshape(-1) for m in pred]), gt=np.concatenate([m.reshape(-1) for m in gt]), slab_off=np.array([0, 768, 768 + 713]),
                tab_p=tp, tab_g=tg, P=6, G=5)
    assert np.array_equal(C.count_ref(case), E.tables(pred, info, gt, gseg, 'view')['counts']) and np.array_equal(C.v_count(case), C.count_ref(case))


CAUGHT_COUNT = {'no_prev_uniform': {'runs', 'runs_whole_lanes'}, 'none_adds': {'runs', 'runs_whole_lanes', 'n_1', 'n_1025', 'slabs_uniform'}}
BLIND_COUNT = {'no_prev_uniform': {'n_1', 'n_4'}, 'none_adds': {'n_1024'}}


@pytest.mark.parametrize('m', sorted(CAUGHT_COUNT))
def test_planted_count_mistakes(m):
    def differs(name):
        return not np.array_equal(C.v_count(COUNT[name], m), C.count_ref(COUNT[name]))
    assert all(differs(n) for n in CAUGHT_COUNT[m]) and not any(differs(n) for n in BLIND_COUNT.get(m, ()))
