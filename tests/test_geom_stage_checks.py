"""The cases of tests/geom_stage_cases.py hold what they were built for (CPU only, no GPU), as tests/test_pp_stage_checks.py shows for the
post-processing stages.

Median: the numpy emulation of the four radix passes equals cloud_ref.median_two_stat on every case (bits, or both NaN), and each of four planted
mistakes - a key that only flips the sign bit, one prefix shared by both ranks, the upper rank for both, >= for > in the bin walk - differs on the
cases listed in CAUGHT and on no other: the value classes tell the mistakes apart before a GPU sees them.  Hash: the restatement finds cells and
(rank, id) pairs with a chosen home slot.  Voxel: every case's built-for property, asserted on voxel_ref.voxelize alone.  Scan and cloud: the sizes,
counts, thresholds and conf offsets of the GPU module really contain the edges they name.  Rank: the sizes and patterns of the component-rank and
surface-keep cases hold every edge of the workgroup rank (a wave without an item, a full wave, an item in lane 0 or lane 63 alone, a full workgroup next
to an empty one, a last workgroup of one row), and the hand-written inputs are what the cases say they are."""
import numpy as np
import pytest

import cloud_ref
import geom_stage_cases as G

F = np.float32

# variant -> the non-random cases on which it differs from the reference
CAUGHT = {
    'sign_flip_only': {'straddle_zero_even', 'zeros_mixed'},
    'one_prefix': {'ties_half', 'straddle_zero_even', 'neg_zero_pos_zero', 'zeros_mixed', 'two_bins', 'inf', 'inf_pm', 'pair'},
    'upper_only': {'ties_half', 'straddle_zero_even', 'denormals', 'denormal_pair', 'mid_bytes', 'share_one_byte', 'inf_pm', 'pair'},
    'ge_walk': {'ties_half', 'straddle_zero_even', 'neg_zero_pos_zero', 'zeros_mixed', 'denormal_pair', 'denormal_odd', 'low_byte_only', 'mid_bytes',
                'share_one_byte', 'two_bins', 'inf', 'single', 'pair'},
}


def _same(a, b):
    return G.same_bits(np.asarray(a, dtype=F), np.asarray(b, dtype=F))


# -------------------------------------------------------------------------------------------------------------------------------------------- median
def test_median_cases_are_the_listed_ones():
    c = G.median_cases()
    for name in ('ties_all_equal', 'ties_half', 'straddle_zero_even', 'neg_only', 'neg_zero_pos_zero', 'zeros_mixed', 'denormals', 'low_byte_only', 'mid_bytes',
                 'two_bins', 'inf', 'inf_pm', 'fmax', 'single', 'pair', 'with_nan', 'random_even', 'random_odd'):
        assert name in c and c[name].dtype == F
    assert len(c['neg_only']) == 1000 and (c['neg_only'] < 0).all() and len(c['random_even']) == 4096 and len(c['random_odd']) == 4097
    assert np.isnan(G.median_ref(c['inf_pm'])) and np.isnan(G.median_ref(c['with_nan'])) and np.isnan(G.median_ref(c['with_neg_nan']))
    with np.errstate(over='ignore'):
        assert np.isinf(c['fmax'].sum()) and np.isfinite(c['fmax']).all() and np.isinf(G.median_ref(c['fmax']))
    # how many leading key bytes the two middle statistics share
    # (positive values: the key is the bit pattern with the top bit set)
    for name, shared in (('low_byte_only', 3), ('mid_bytes', 2), ('share_one_byte', 1), ('two_bins', 0)):
        s = np.sort(c[name])
        assert (s > 0).all() and len(s) % 2 == 0
        a, b = (int(x) for x in G.f32_bits(s[[len(s) // 2 - 1, len(s) // 2]]))
        assert a != b and [a >> 24 == b >> 24, a >> 16 == b >> 16, a >> 8 == b >> 8].count(True) == shared, (name, hex(a), hex(b))
    s = np.sort(c['straddle_zero_even'])
    assert s[1] < 0 < s[2]                                                    # ... and the two sides of zero: the other half of the key
    d = c['denormals']
    assert ((np.abs(d) < F(1.1754944e-38)) & (d != 0)).sum() >= 5
    assert G.f32_bits(G.median_ref(c['denormal_pair'])) == 4                  # a subnormal sum, halved exactly
    assert G.f32_bits(G.median_ref(c['neg_zero_pos_zero'])) == 0              # -0 + +0 = +0
    assert G.f32_bits(G.median_ref(c['zeros_mixed'])) == 0                    # -0 sorts below +0: the middle two are (-0, +0), not (-0, -0)
    assert G.f32_bits(cloud_ref.median_two_stat([0.0, -0.0, -0.0])) == 0x80000000


@pytest.mark.parametrize('name', list(G.median_cases()))
def test_radix_select_equals_the_contract(name):
    x = G.median_cases()[name]
    assert _same(G.radix_select(x), G.median_ref(x)), (name, G.radix_select(x), G.median_ref(x))


def test_radix_select_of_nothing():
    assert np.isnan(G.radix_select(np.zeros(0, F))) and np.isnan(G.median_ref(np.zeros(0, F)))


def test_median_contract_is_np_median_where_that_is_defined():
    """np.median agrees wherever it rounds the same way: no overflowing sum, and the sign of a zero is left open by np.sort"""
    for name, x in G.median_cases().items():
        if name == 'fmax':
            continue
        with np.errstate(invalid='ignore'):
            m, r = np.median(x), G.median_ref(x)
        assert (np.isnan(m) and np.isnan(r)) or m == r, (name, m, r)


@pytest.mark.parametrize('variant', G.VARIANTS)
def test_planted_median_mistake_is_caught(variant):
    cases = G.median_cases()
    differs = {name for name, x in cases.items() if not _same(G.radix_select(x, variant), G.median_ref(x))}
    assert differs - set(G.RANDOM_CASES) == CAUGHT[variant], sorted(differs)
    assert len(CAUGHT[variant]) >= 2


def test_every_value_class_but_the_quiet_ones_catches_a_mistake():
    quiet = {'ties_all_equal', 'fmax', 'with_nan', 'with_neg_nan'}           # one value / an overflow / a NaN: right under every planted mistake
    assert set().union(*CAUGHT.values()) == set(G.median_cases()) - quiet - set(G.RANDOM_CASES)


@pytest.mark.parametrize('S', [1, 8, 9, 17])
def test_median_segments(S):
    for M in (32768, 32769):
        pts, pan, id2row, count, med = G.median_segments(S, M)
        assert pts.shape == (M, 3) and pan.shape == (M,) and len(id2row) == S + 2
        assert sorted(id2row[id2row >= 0]) == list(range(S)) and (id2row[1:] == -1).sum() == 1 and id2row[0] == -1
        assert {0, -5, S + 2} <= set(pan.tolist()) and int(np.nonzero(id2row[1:] < 0)[0][0]) + 1 in set(pan.tolist())
        live = (pan > 0) & (pan < S + 2)
        row = np.where(live, id2row[np.clip(pan, 0, S + 1)], -1)
        for s in range(S):
            assert (row == s).sum() == count[s]
            for a in range(3):
                assert _same(G.median_ref(pts[row == s, a]), med[s, a])
            at = np.nonzero(row == s)[0]
            assert count[s] < 4 or at[-1] - at[0] > 4 * count[s]              # spread over the cloud row by row, not a block of its own
        if M == 32769:
            assert row[:32768].max() >= 0


# ---------------------------------------------------------------------------------------------------------------------------------------------- hash
def test_colliding_cells():
    cells = G.colliding_cells(1024, 1023, 200)
    assert cells.shape == (200, 3) and len(np.unique(cells, axis=0)) == 200 and np.abs(cells).max() <= 32
    assert (G.home_slot(G.vx_key(cells), 1024) == 1023).all()
    assert len(G.colliding_cells(1024, 1023)) == 251
    k = G.vx_key([[0, 0, 0], [-G.LIM + 1, 0, 0], [0, 0, G.LIM - 1]])
    assert list(k) == [(1 << 20) | (1 << 41) | (1 << 62), 1 | (1 << 41) | (1 << 62), (1 << 20) | (1 << 41) | ((2 ** 21 - 1) << 42)]
    assert int(G.vx_hash([0])[0]) == 0 and int(G.vx_hash([1])[0]) == 0xb456bcfc34c2cb2c      # the 64-bit finaliser of MurmurHash3


def test_colliding_pairs():
    pairs = G.colliding_pairs(1024, 1023, range(512), 4096)
    assert len(pairs) >= 24 and len(set(pairs)) == len(pairs)
    for r, i in pairs:
        assert 0 <= r < 512 and 0 < i < 4096 and G.home_slot([(r << 32) | i], 1024)[0] == 1023


# --------------------------------------------------------------------------------------------------------------------------------------------- voxel
@pytest.mark.parametrize('name', list(G.voxel_cases()))
def test_voxel_case_holds_what_it_was_built_for(name):
    G.assert_voxel_case(name)


def test_voxel_cases_are_the_listed_ones():
    c = G.voxel_cases()
    assert {'cell_edges_0.05', 'cell_edges_0.07', 'cell_edges_0.25', 'load_half', 'runs', 'votes', 'big_voxel', 'colours'} == set(c)
    assert max(len(v['pan']) for v in c.values()) == G.BIG_N + 1
    assert c['cell_edges_0.05']['dropped'] == 18 and all(v['dropped'] == 0 for k, v in c.items() if not k.startswith('cell_edges'))


# ------------------------------------------------------------------------------------------------------------------------------------- scan and cloud
def test_scan_cases_hold_their_edges():
    assert {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 5000} <= set(G.SCAN_N)
    for n in G.SCAN_N:
        c = G.scan_counts(n)
        assert c.dtype == np.int32 and len(c) == n and c.min() >= 0 and c.max() <= 1024 and c[0] == 0 and c[n - 1] == 0
        if n > 1024:
            assert c[1023] == 0 and c[1024] == 0                              # the last count of a round and the first of the next
        if n > 4:
            assert (c > 0).sum() > n // 2
        r = G.scan_ref(c)
        assert len(r) == n + 1 and r[0] == 0 and r[n] == c.sum() and (np.diff(r) == c).all()
    big = G.scan_ref(G.scan_big())
    assert int(big[-1]) == 2 ** 31 - 2 ** 20 and int(big[-1]) + 2 ** 20 == 2 ** 31


@pytest.mark.parametrize('thr', list(G.CLOUD_THRESHOLDS))
def test_cloud_cases_hold_their_edges(thr):
    for ncolors in G.CLOUD_NCOLORS:
        case = G.cloud_case(thr, ncolors)
        w = G.cloud_wg_counts(case)
        first = sum((n + G.WG - 1) // G.WG for n in G.CLOUD_NPIX[:G.FULL_VIEW])
        assert list(w[first:first + 3]) == [1024, 0, 1] and len(w) == first + 3          # staging buffer full | the early return | one point
        conf = np.concatenate([x['conf'].reshape(-1) for x in case['x_out']])
        t = F(case['thr'])
        assert np.isnan(conf).any() and (conf == t).any() and (conf[~np.isnan(conf)] < t).any()
        if thr == 'inf':
            assert np.isposinf(conf).any()
        if thr == 'zero':
            assert ((conf == 0) & np.signbit(conf)).any() and (G.f32_bits(conf) == 0x80000001).any()
        pan = np.concatenate([p.reshape(-1) for p in case['pan']])
        assert {0, -1, ncolors - 1, ncolors, 2 ** 31 - 1} <= set(pan.tolist())
        r = G.cloud_reference(case)
        assert len(r['pan']) == w.sum() and {0, -1, ncolors - 1, ncolors, 2 ** 31 - 1} <= set(r['pan'].tolist())
        sub = (np.abs(r['points']) < F(1.1754944e-38)) & (r['points'] != 0)
        assert sub.any() and np.isinf(r['points']).any() and np.isnan(r['points_local']).any()
        for c in case['cams']:
            assert np.abs(c[:3, :3] - np.eye(3)).max() > 0.1                  # a rotation that is not trivial
    assert G.CLOUD_NPIX == [1, 3, 4, 5, 1023, 1024, 1025, 2049]


def test_cloud_conf_offsets_cover_every_alignment():
    seen = {}
    for shift in range(4):
        off, total = G.cloud_offsets(shift)
        assert all(a + n <= b for a, n, b in zip(off, G.CLOUD_NPIX, off[1:] + [total]))
        for n, o in zip(G.CLOUD_NPIX, off):
            seen.setdefault(n, set()).add(o * 4 % 16)
    assert all(s == {0, 4, 8, 12} for s in seen.values()), seen


# ------------------------------------------------------------------------------------------------------- the workgroup rank: components and surface keep
RANK_FAMILIES = {'vcc': (G.VCC_MV, G.WG, G.VCC_PT), 'keep': (G.KEEP_F, G.KEEP_WG, G.KEEP_PT)}


@pytest.mark.parametrize('family', list(RANK_FAMILIES))
def test_rank_patterns_hold_every_edge_of_the_workgroup_rank(family):
    sizes, wg, pt = RANK_FAMILIES[family]
    W = 64 * pt
    assert {1, W - 1, W, W + 1, wg - 1, wg, wg + 1, 2 * wg + 1} <= set(sizes) and wg == 4 * W
    assert set(G.RANK_PATTERNS) >= {'none', 'all', 'wave_last', 'wg_first', 'alternating', 'random'}
    big = max(sizes)
    edges = {p: G.rank_edges(G.rank_pattern(p, big, wg, pt), wg, pt) for p in G.RANK_PATTERNS}
    assert 'empty_wave' in edges['none'] and 'empty_wave' in edges['wg_first']
    assert 'full_wave' in edges['all'] and 'last_wg_one_row' in edges['all']
    assert 'lane0_only' in edges['wg_first'] and 'lane63_only' in edges['wave_last']
    assert 'full_wg_next_to_empty' in edges['wg_blocks'] and 'last_wg_one_row' in edges['wg_blocks']
    assert set().union(*edges.values()) == set(G.RANK_EDGES)
    assert G.rank_edges(G.rank_pattern('all', wg + 1, wg, pt), wg, pt) >= {'full_wave', 'last_wg_one_row'}
    for n in sizes:
        m = {p: G.rank_pattern(p, n, wg, pt) for p in G.RANK_PATTERNS}
        assert all(v.dtype == bool and v.shape == (n,) for v in m.values())
        assert not m['none'].any() and m['all'].all() and m['alternating'].sum() == (n + 1) // 2
        assert m['wave_last'].sum() == n // W and m['wg_first'].sum() == (n + wg - 1) // wg
        if n >= 63:
            assert 0 < m['random'].sum() < n
    lane = (np.nonzero(G.rank_pattern('wave_last', big, wg, pt))[0] // pt) % 64
    assert (lane == 63).all() and len(lane) >= 2


@pytest.mark.parametrize('Mv', G.VCC_MV)
def test_vcc_rank_cases_are_what_they_say(Mv):
    for p in G.RANK_PATTERNS:
        c = G.vcc_rank_case(Mv, p)
        w, root, v = c['want'], c['root'], np.arange(Mv)
        assert np.array_equal(root == v, c['is_root']) and (root <= v).all() and (root >= -1).all()
        for i in range(Mv):                                                   # the nearest lower root, by hand
            below = np.nonzero(c['is_root'][:i + 1])[0]
            assert root[i] == (below[-1] if len(below) else -1)
        assert w['C'] == c['is_root'].sum() == w['counts'].sum() == w['base'][-1] and len(w['counts']) == (Mv + G.WG - 1) // G.WG
        assert np.array_equal(w['table']['root'], np.nonzero(c['is_root'])[0]) and (np.diff(w['table']['root']) > 0).all()
        assert ((w['component'] == -1) == (root < 0)).all() and (w['component'][root >= 0] == w['rank_of'][root[root >= 0]]).all()
        # every value identifies its row: a table row taken from a neighbouring voxel shows
        assert len(set(c['size'].tolist())) == Mv and len(set(c['points'].tolist())) == Mv and (c['points'] >= 5).all() and (Mv < 2 or c['points'].max() > 2 ** 32)
        assert len(np.unique(c['lo'], axis=0)) == Mv and len(np.unique(c['hi'], axis=0)) == Mv
        assert c['root'].dtype == c['pan'].dtype == c['size'].dtype == c['lo'].dtype == np.int32 and c['points'].dtype == np.int64


@pytest.mark.parametrize('F_', G.KEEP_F)
def test_keep_cases_are_what_they_say(F_):
    seen = set()
    for p in G.RANK_PATTERNS:
        c = G.keep_case(F_, p)
        w, comp, size = c['want'], c['component'], c['size']
        assert np.array_equal(w['survives'], c['pattern']), p               # the hand-written inputs realise the pattern
        assert c['M'] >= F_ and c['M'] % 4 == 0 and len(size) == c['M'] and comp.min() >= -1 and comp.max() < c['M']
        assert w['kept'] == c['pattern'].sum() == w['base'][-1] and len(w['counts']) == (F_ + G.KEEP_WG - 1) // G.KEEP_WG
        of = np.where(comp >= 0, size[np.maximum(comp, 0)], -1)
        seen |= set(of.tolist())
        assert set(of[c['pattern']].tolist()) <= {c['min_faces'], 50} and set(of[~c['pattern']].tolist()) <= {-1, 0, c['min_faces'] - 1}
        assert np.array_equal(w['faces'][:, 0] // 3, np.nonzero(c['pattern'])[0]) and np.array_equal(w['quad'] >> 33, np.nonzero(c['pattern'])[0])
    if F_ >= 63:
        assert seen == {-1, 0, c['min_faces'] - 1, c['min_faces'], 50}        # no component, sizes 0, min_faces - 1, min_faces and beyond
