"""The cases of tests/tsdf_stage_cases.py hold what they were built for, the planted mistakes are caught, and the split of tests/tsdf_ref.py is neutral
(CPU only, no GPU), as tests/test_geom_stage_checks.py shows for the cloud and voxel stages.

Everything is asserted on the restatement alone.  Nodes: the ranks follow the smallest pair, the last legal cells are legal and one step beyond is
not, the wrap tables really have two keys at home in the last slot, the counted tables have the counts they name.  Integrate: the hand-written planes
give the exact equalities s == -tau, s == tau, zc == near, u + 0.5 == 0 and == W, and the views that must take no part take none.  Extraction: the
checkerboard's counts, the zero and subnormal fields, the label ties, the face-id patterns, the launch edges of the gadget tables.  CAUGHT records which
named case differs from the restatement under which planted mistake; the variants without a mistake equal the restatement on every case."""
import numpy as np
import pytest

import consistency_ref
import geom_stage_cases as G
import tsdf_ref as T
import tsdf_stage_cases as C

F = np.float32


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


# mistake -> named cases that must differ from the restatement under it (node cases as name@band, integrate cases by the special nodes that differ)
CAUGHT = {
    'offset_minus_band': {'one@1', 'one@4', 'shuffled@2', 'around_zero@3', 'last_legal@1', 'wrap@1', 'count_1025@1', 'big@1'},
    'offset_z_fastest': {'one@1', 'one@4', 'shuffled@2', 'around_zero@3', 'last_legal@1', 'wrap@1', 'count_1025@1', 'big@1'},
    'occluded_le': {'at_minus_tau'},
    'no_clamp': {'above_plus_tau_A', 'above_plus_tau_C', 'at_near', 'many_views'},
    'floor_u': {'left_in', 'right_out', 'corner_in'},
    'px_le_W': {'right_out'},
    'zc_gt_near': {'at_near'},
    'sum_descending': {'many_views'},
    'reciprocal': {'many_views'},
    'inside_le': {'plane_pos_zero', 'plane_neg_zero'},
    'valid_gt': {'weight_edge_1', 'weight_edge_3', 'checker'},
    't_upper': {'tiny_inside', 'tiny_outside', 'plane_pos_zero', 'random_big', 'ball'},
    'edge_order_yzx': {'sum_order'},
    'fp32_crossings': {'subnormal_neg', 'subnormal_pos', 'lone_inside', 'sum_order', 'random_big', 'ball'},
    'tie_larger_row': {'label_tie_later_smaller', 'label_tie_later_larger'},
    'scan_ge': {'label_tie_later_larger'},
    'q1_q3': {'checker', 'lone_inside', 'lone_outside', 'single_lane0', 'single_lane255', 'full_lanes', 'ball'},
    'no_flip': {'checker', 'lone_outside', 'subnormal_pos', 'full_lanes', 'ball'},
    'face_id_corner0': {'checker', 'label_fuller_larger_row', 'random_big'},
    'axis_major': {'checker', 'lone_inside', 'single_a', 'full_lanes', 'random_big'},
}


def test_every_planted_mistake_is_listed():
    assert set(CAUGHT) == set(C.NODE_MISTAKES) | set(C.INTEGRATE_MISTAKES) | set(C.EXTRACT_MISTAKES) and all(CAUGHT.values())


# -------------------------------------------------------------------------------------------------------------------------------------------- nodes
@pytest.mark.parametrize('band', C.BANDS)
def test_node_cases_hold_what_they_name(band):
    cases = C.node_cases(band)
    side = 2 * band
    for name, cells in cases.items():
        assert len(np.unique(cells, axis=0)) == len(cells), name
        tab = C.node_table(band, name)
        nodes, voxel_row = C.v_nodes(cells, band)                                          # the variant without a mistake is the restatement
        assert np.array_equal(nodes, tab.nodes) and np.array_equal(voxel_row, tab.voxel_row), name
        assert (np.sort(tab.voxel_row[tab.voxel_row >= 0]) == np.arange(len(cells))).all() and np.array_equal(tab.nodes[tab.rank(cells)], cells), name
        assert C.capacity(len(cells) * side ** 3) >= 2 * len(cells) * side ** 3
    assert len(C.node_table(band, 'one')) == side ** 3
    # shuffled rows whose bands overlap: some node's smallest pair is not the pair of its smallest row among the rows listed before ... i.e. the
    # order of the nodes is the order of the pairs, not of the cells: sorting the cells changes the ranks
    cells = cases['shuffled']
    pairs = C.pairs_of(cells, band)
    keys, first, cnt = np.unique(T.keys_of(pairs), return_index=True, return_counts=True)
    assert (cnt > 1).any() and len(keys) < len(pairs)
    tab = C.node_table(band, 'shuffled')
    assert np.array_equal(tab.nodes, pairs[np.sort(first)])
    assert not np.array_equal(T.NodeTable(cells[np.lexsort(cells.T)], band).nodes, tab.nodes)
    shared = np.nonzero(cnt > 1)[0]
    owner = first[shared] // side ** 3                                                    # the row of the smallest pair of a shared node ...
    last = np.array([np.nonzero(T.keys_of(pairs) == keys[i])[0].max() // side ** 3 for i in shared])
    assert (owner < last).all() and (cells[owner] > cells[last]).any(axis=1).any()        # ... is listed earlier, whichever cell is the smaller
    z = C.node_table(band, 'around_zero').nodes
    assert all((z[:, a] < 0).any() and (z[:, a] > 0).any() and (z[:, a] == 0).any() for a in range(3))
    n = C.node_table(band, 'last_legal').nodes
    assert n.max() == C.LIM - 1 and n.min() == -C.LIM + 1
    cells, out = C.range_case(band)
    assert 0 < out.sum() < len(out) and not out[:side ** 3].any()
    per_row = out.reshape(len(cells), -1).sum(axis=1)
    assert per_row.tolist() == [0, side ** 2, 0, side ** 2, 0, side ** 2, side ** 3 - (side - 1) ** 3]
    with pytest.raises(RuntimeError, match='outside'):
        T.NodeTable(cells, band)


@pytest.mark.parametrize('band', sorted(C.WRAP_MV))
def test_wrap_tables_have_two_keys_at_home_in_the_last_slot(band):
    cells = C.wrap_cells(band)
    pairs = len(cells) * (2 * band) ** 3
    cap = C.capacity(pairs)
    assert cap == 2 * pairs and pairs & (pairs - 1) == 0                                  # the smallest capacity a launcher takes
    home = G.home_slot(G.vx_key(C.node_table(band, 'wrap').nodes), cap)
    assert (home == cap - 1).sum() >= 2


def test_counted_tables_have_their_counts():
    for N in C.NODE_COUNTS:
        assert len(C.node_table(1, 'count_%d' % N)) == N
    assert {N % 4 for N in C.NODE_COUNTS} == {0, 1, 3} and len(C.node_table(1, 'big')) == 17 ** 3 > 4096
    for N in (8, 12, 15, 237, 238, 749, 750):
        assert len(T.NodeTable(C.counted(N), 1)) == N


# ---------------------------------------------------------------------------------------------------------------------------------------- integrate
def per_view(case, v):
    return C.integrate_ref(C.one_view(case, v))


@pytest.mark.parametrize('band', C.BANDS)
def test_integrate_case_holds_its_exact_equalities(band):
    case = C.integrate_case(band, 2049)
    sp = {k: v[0] for k, v in case['special'].items()}
    assert all(len(v) == 4 for v in case['special'].values())                             # at the start, across 255 | 256, across 1023 | 1024, at the end
    starts = sorted(case['special']['at_minus_tau'])
    assert starts[0] == 0 and starts[1] < 255 < starts[1] + 25 and starts[2] < 1023 < starts[2] + 25 and starts[3] == 2049 - 25
    tau = F(F(band) * C.VS)
    off = np.concatenate([[0], np.cumsum(case['npix'])])
    assert off.tolist() == [0, 15, 47, 79, 111, 143, 175, 207] and all(o % 4 for o in off[1:-1])
    sA, wA = per_view(case, 'A')
    # s == -tau is kept and counts -tau; one float of [1, 2) less at the pixel next to it is occluded
    assert wA[sp['at_minus_tau']] == 1 and sA[sp['at_minus_tau']] == -tau and wA[sp['below_minus_tau_A']] == 0
    # s == tau, and above it: both give tau
    assert wA[sp['at_plus_tau']] == 1 and sA[sp['at_plus_tau']] == tau and wA[sp['above_plus_tau_A']] == 1 and sA[sp['above_plus_tau_A']] == tau
    assert float(case['depths'][1][1 * 8 + 4]) - (128 - band) / 64 > float(tau)
    # d = +0.0 and -0.0: nothing measured
    assert u32(case['depths'][1][2 * 8 + 6]) == 0 and u32(case['depths'][1][2 * 8 + 3]) == 0x80000000 and wA[sp['d_pos_zero']] == 0 and wA[sp['d_neg_zero']] == 0
    # zc == near is in front, one node nearer is not; behind the camera
    assert wA[sp['at_near']] == 1 and sA[sp['at_near']] == tau and wA[sp['nearer']] == 0 and wA[sp['behind']] == 0
    # the four borders: u + 0.5 == 0 is pixel 0, u + 0.5 == W is outside
    for name, inside in (('left_in', 1), ('left_out', 0), ('right_in', 1), ('right_out', 0), ('top_in', 1), ('top_out', 0), ('bottom_in', 1), ('bottom_out', 0),
                         ('corner_in', 1), ('corner_out', 0), ('on_surface', 1)):
        assert wA[sp[name]] == inside and sA[sp[name]] == 0, name
    p = case['nodes'][[sp['left_in'], sp['right_out'], sp['top_in'], sp['bottom_out']]].astype(np.float64) / 64
    assert (64 * p[0, 0] / p[0, 2] + 4 + 0.5, 64 * p[1, 0] / p[1, 2] + 4 + 0.5, 64 * p[2, 1] / p[2, 2] + 2 + 0.5, 64 * p[3, 1] / p[3, 2] + 2 + 0.5) == (0, 8, 0, 4)
    # the float32 below -tau (view B) and above tau (view C), exactly
    sB, wB = per_view(case, 'B')
    assert wB.sum() == 0                                                                  # its one measured pixel occludes the one node that sees it nearly
    zc, d = F((band + 1) / 64), case['depths'][5][2 * 8 + 4]
    assert F(d - zc) == np.nextafter(-tau, F(-1)) and float(d) - float(zc) == float(np.nextafter(-tau, F(-1)))
    sC, wC = per_view(case, 'C')
    d = case['depths'][6][2 * 8 + 4]
    assert wC[sp['above_plus_tau_C']] == 1 and sC[sp['above_plus_tau_C']] == tau and F(d - F(C.ZC)) == np.nextafter(tau, F(1))
    assert wC[sp['u_beyond_limit']] == 0 and wC[sp['u_within_limit']] == 0 and 64 * (256 / 64) / C.ZC + 4 > 2 ** 20 > 64 * (255 / 64) / C.ZC + 4
    # H W == npix + 1, H == 0 and negative dims whose product fits: no part, though their planes would measure
    for v, j in (('D', 2), ('E', 3), ('G', 4)):
        H, W = case['dims'][j]
        assert per_view(case, v)[1].sum() == 0 and (H * W == case['npix'][j] + 1 or H < 1) and (case['depths'][j] == 2).all()
    assert tuple(case['dims'][2]) == (3, 11) and tuple(case['dims'][4]) == (-4, -8)
    fair = dict(C.one_view(case, 'D'), dims=np.array([[4, 8]], dtype=np.int32))
    assert C.integrate_ref(fair)[1].sum() > 100                                           # (with honest dims it would take part)
    sdf, w = C.integrate_ref(case)
    assert w.max() == w[sp['above_plus_tau_C']] == 3 and (w == 0).any() and (w == 1).any() and (w == 2).any()      # views F, A and C measure: sums of up to three


def test_integrate_sizes_and_many_views():
    assert C.INTEGRATE_NN == (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
    for band in C.BANDS:
        for Nn in C.INTEGRATE_NN:
            case = C.integrate_case(band, Nn)
            assert case['nodes'].shape == (Nn, 3) and case['nodes'].dtype == np.int32
            got, ref = C.v_integrate(case), C.integrate_ref(case)
            assert np.array_equal(u32(got[0]), u32(ref[0])) and np.array_equal(got[1], ref[1])
    case = C.many_views()
    sdf, w = C.integrate_ref(case)
    got = C.v_integrate(case)
    assert np.array_equal(u32(got[0]), u32(sdf)) and np.array_equal(got[1], w)
    assert len(case['depths']) == C.MANY_V >= 64 and w.max() == C.MANY_V and len(set(w.tolist())) > 2 and all(x & (x - 1) for x in w.tolist())
    d = np.concatenate(case['depths'])
    assert (d >= case['cams'][0][15]).all() and np.isfinite(d).all()
    # non-dyadic: the exact sum of the terms of a node needs more than 24 bits
    s = d.astype(np.float64) - 1 / 64
    assert float(F(s.sum())) != float(s.sum())


def integrate_differences(mistake):
    """the names of the special nodes (band-1 .. band-4 cases of 2049 nodes) and 'many_views' where the mistake changes sdf or weight"""
    hit = set()
    for band in C.BANDS:
        case = C.integrate_case(band, 2049)
        ref, got = C.integrate_ref(case), C.v_integrate(case, mistake)
        bad = set(np.nonzero((u32(ref[0]) != u32(got[0])) | (ref[1] != got[1]))[0].tolist())
        here = {n for n, ix in case['special'].items() if bad & set(ix)}
        hit = here if band == C.BANDS[0] else hit & here                                   # at every band
    case = C.many_views()
    ref, got = C.integrate_ref(case), C.v_integrate(case, mistake)
    if ((u32(ref[0]) != u32(got[0])) | (ref[1] != got[1])).any():
        hit.add('many_views')
    return hit


@pytest.mark.parametrize('mistake', C.INTEGRATE_MISTAKES)
def test_integrate_mistakes_are_caught(mistake):
    hit = integrate_differences(mistake)
    assert CAUGHT[mistake] <= hit, (mistake, sorted(hit))


@pytest.mark.parametrize('mistake', C.NODE_MISTAKES)
def test_node_mistakes_are_caught(mistake):
    for entry in CAUGHT[mistake]:
        name, band = entry.split('@')
        tab = C.node_table(int(band), name)
        nodes, voxel_row = C.v_nodes(C.node_cases(int(band))[name], int(band), mistake)
        assert not (np.array_equal(nodes, tab.nodes) and np.array_equal(voxel_row, tab.voxel_row)), entry


# --------------------------------------------------------------------------------------------------------------------------------------- extraction
@pytest.mark.parametrize('name', list(C.EXTRACT))
def test_variant_without_a_mistake_is_the_restatement(name):
    case, ref = C.extract_case(name), C.extract_ref(name)
    assert C.same_extract(ref, C.v_extract(case)) == []
    Nv, Nf = len(ref['vertices']), len(ref['faces'])
    assert Nf <= 6 * Nv and ref['cell_counts'].sum() == Nv and ref['face_counts'].sum() == Nf and ref['is_cell'].sum() == Nv
    assert np.array_equal(ref['is_cell'], ref['cell_vertex'] >= 0)
    assert 2 * sum(bin(int(x)).count('1') for x in ref['face_mask']) == Nf and (ref['face_mask'] >> 3 == 0).all()
    assert np.isfinite(ref['vertices']).all()


@pytest.mark.parametrize('mistake', C.EXTRACT_MISTAKES)
def test_extraction_mistakes_are_caught(mistake):
    for name in CAUGHT[mistake]:
        assert C.same_extract(C.extract_ref(name), C.v_extract(C.extract_case(name), mistake)) != [], (mistake, name)


def lane_masks(face_mask):
    """per lane of four consecutive nodes: its 12-bit mask (the last lane padded with zeros)"""
    m = np.concatenate([face_mask, np.zeros(-len(face_mask) % C.PT, dtype=face_mask.dtype)]).reshape(-1, C.PT)
    return m[:, 0] | (m[:, 1] << 3) | (m[:, 2] << 6) | (m[:, 3] << 9)


def test_checkerboard():
    case, ref = C.extract_case('checker'), C.extract_ref('checker')
    Nv, Nf = len(ref['vertices']), len(ref['faces'])
    assert (len(case['tab']), Nv, Nf) == (1728, 1331, 6600) and 4.5 * Nv < Nf <= 6 * Nv
    assert (ref['face_mask'] == 7).sum() == 1000 and (lane_masks(ref['face_mask']) == 0xfff).sum() == 81       # lanes with all twelve bits; how many depends on the order the cells are listed in (here x fastest)
    assert len(ref['face_counts']) == 2 and (ref['face_counts'] > 2048).all()
    # every face-id pattern on chosen triangles, 0 among the ids
    ids = ref['vertex_ids'][ref['faces']]
    a, b, c = ids[:, 0], ids[:, 1], ids[:, 2]
    for what, sel, want in (('aaa', (a == b) & (b == c), a), ('aab', (a == b) & (b != c), a), ('aba', (a == c) & (a != b), a), ('baa', (b == c) & (a != b), b),
                            ('abc', (a != b) & (b != c) & (a != c), np.zeros_like(a))):
        assert sel.sum() > 10 and np.array_equal(ref['face_ids'][sel], want[sel]), what
        assert (want[sel] == 0).any() and (ids[sel] == 0).any(), what
    assert ((a != b) & (b != c) & (a != c) & (ids != 0).all(axis=1)).any()


def test_zero_and_subnormal_fields():
    pos, neg = C.extract_ref('plane_pos_zero'), C.extract_ref('plane_neg_zero')
    assert C.same_extract(pos, neg) == [] and len(pos['faces']) == 50 and (pos['vertices'][:, 2] == F(1 / 64)).all()
    for name, zero in (('plane_pos_zero', 0), ('plane_neg_zero', 0x80000000)):
        case = C.extract_case(name)
        layer = case['tab'].nodes[:, 2] == 1
        assert (u32(case['sdf'][layer]) == zero).all() and (case['sdf'][~layer] != 0).all()
    for name, lone in (('subnormal_neg', 0x80000001), ('subnormal_pos', 0x00000001)):
        case, ref = C.extract_case(name), C.extract_ref(name)
        assert set(u32(case['sdf']).tolist()) == {0x80000001, 0x00000001} and (u32(case['sdf']) == lone).sum() == 2
        assert len(ref['vertices']) == 15 and len(ref['faces']) == 24
        flushed = dict(case, sdf=np.where(np.abs(case['sdf']) < F(2.0 ** -126), F(0), case['sdf']))
        assert len(C.v_extract(flushed)['vertices']) == 0                                  # a compare that flushes subnormals sees no surface at all
    for name, axis, near in (('tiny_inside', 0, 1 + 2.0 ** -20 / (1 + 2.0 ** -20)), ('tiny_outside', 1, 1 + 1 / (1 + 2.0 ** -20))):
        v = C.extract_ref(name)['vertices'].astype(np.float64) * 64
        assert len(v) == 9 and np.allclose(v[:, axis], near, rtol=0, atol=1e-6) and (v[:, axis] != np.round(v[:, axis])).all()


def test_lone_nodes_weights_and_closed_fields():
    for name in ('lone_inside', 'lone_outside'):
        case, ref = C.extract_case(name), C.extract_ref(name)
        assert ((case['sdf'] < 0).sum() == 1) == (name == 'lone_inside') and ((case['sdf'] >= 0).sum() == 1) == (name == 'lone_outside')
        assert len(ref['vertices']) == 8 and len(ref['faces']) == 12 and sorted(ref['face_mask'][ref['face_mask'] > 0].tolist()) == [1, 2, 4, 7]
    for mw in (1, 3):
        case, ref = C.extract_case('weight_edge_%d' % mw), C.extract_ref('weight_edge_%d' % mw)
        full = C.v_extract(dict(case, weight=np.full_like(case['weight'], mw)))
        assert case['min_weight'] == mw and sorted(set(case['weight'].tolist())) == [mw - 1, mw] and (case['weight'] == mw - 1).sum() == 2
        assert len(full['vertices']) == 36 and len(ref['vertices']) == 28 and len(full['faces']) == 50 and len(ref['faces']) == 18
        # surface cells next to cells that are none: a crossing edge between valid nodes with one to three surface cells around it emits nothing
        tab, valid = case['tab'], case['weight'] >= mw
        rows = np.nonzero(tab.nodes[:, 2] == 0)[0]
        up = tab.rank(tab.nodes[rows] + np.array([0, 0, 1]))
        around = sum(np.where(tab.rank(tab.nodes[rows] + np.array(o)) >= 0, ref['is_cell'][np.maximum(tab.rank(tab.nodes[rows] + np.array(o)), 0)], False).astype(int)
                     for o in ((0, 0, 0), (-1, 0, 0), (-1, -1, 0), (0, -1, 0)))
        partial = valid[rows] & valid[up] & (around > 0) & (around < 4)
        interior = (tab.nodes[rows, :2] > 0).all(axis=1) & (tab.nodes[rows, :2] < 6).all(axis=1)
        assert (partial & interior).sum() >= 4 and (ref['face_mask'][rows][partial] == 0).all() and (ref['face_mask'][rows][around == 4] == 4).all()
    for name in C.CLOSED:
        case, ref = C.extract_case(name), C.extract_ref(name)
        sane, directed, undirected = T.topology(ref['faces'], len(ref['vertices']))
        assert sane and directed == 1 and undirected == 2 and len(ref['faces']) > 0, name
        assert (C.winding(case, ref) > 0).all(), name


def test_label_cases():
    def at_origin(name):
        case, ref = C.extract_case(name), C.extract_ref(name)
        r = int(case['tab'].rank(np.zeros(3, dtype=np.int64)))
        assert case['tab'].voxel_row[r] == -1 and ref['is_cell'][r]
        v = ref['cell_vertex'][r]
        return case, ref['vertex_ids'][v], ref['colors'][v]
    scan = [(d % 3 - 1, (d // 3) % 3 - 1, d // 9 - 1) for d in range(27)]
    assert scan.index((-1, 0, 0)) == 12 < scan.index((1, 0, 0)) == 14
    case, vid, col = at_origin('label_tie_later_smaller')                                 # row 0 at (1, 0, 0) is met later and wins the tie
    assert case['cells'].tolist() == [[1, 0, 0], [-1, 0, 0]] and case['count'].tolist() == [3, 3] and vid == case['pan'][0] and np.array_equal(col, case['colors'][0])
    case, vid, col = at_origin('label_tie_later_larger')                                  # row 0 at (-1, 0, 0) is met first and stays
    assert case['cells'].tolist() == [[-1, 0, 0], [1, 0, 0]] and vid == case['pan'][0] and np.array_equal(col, case['colors'][0])
    case, vid, col = at_origin('label_fuller_larger_row')
    assert case['count'].tolist() == [2, 5] and vid == case['pan'][1] and np.array_equal(col, case['colors'][1])
    case, ref = C.extract_case('label_none'), C.extract_ref('label_none')
    far = (np.abs(case['tab'].nodes[ref['is_cell']]).max(axis=1) == 2)                    # cells two steps from the only voxel
    assert far.sum() == 125 - 27 and (ref['vertex_ids'][far] == 0).all() and (ref['colors'][far] == 0).all()
    assert (ref['vertex_ids'][~far] == case['pan'][0]).all() and case['pan'][0] != 0 and (case['colors'] != 0).all()
    assert (ref['face_ids'] == 0).any() and (ref['face_ids'] == case['pan'][0]).any()


def test_sum_order_case_sits_on_a_tie():
    ref = C.extract_ref('sum_order')
    assert len(ref['vertices']) == 1 and float(ref['vertices'][0, 2]) * 64 == 0.5 + 2.0 ** -24
    assert float(C.v_extract(C.extract_case('sum_order'), 'edge_order_yzx')['vertices'][0, 2]) * 64 == 0.5


def test_launch_edges_of_the_gadget_tables():
    face_nodes = lambda name: np.nonzero(C.extract_ref(name)['face_mask'])[0].tolist()
    assert face_nodes('single_a') == [3, 255, 1023] and face_nodes('single_b') == [4, 256, 1024]
    assert face_nodes('single_lane0') == [1024] and C.extract_ref('single_lane0')['face_counts'].tolist() == [0, 2]
    assert face_nodes('single_lane255') == [1023] and C.extract_ref('single_lane255')['face_counts'].tolist() == [2, 0]
    assert all(len(C.extract_case(n)['tab']) % 4 for n in ('single_a', 'single_b', 'single_lane0', 'single_lane255', 'full_lanes'))
    ref = C.extract_ref('full_lanes')
    Nn = len(ref['face_mask'])
    full = np.nonzero(lane_masks(ref['face_mask']) == 0xfff)[0].tolist()
    assert {0, 1, 63, 64, 255, 256} <= set(full)                                          # across 3 | 4, 255 | 256 and 1023 | 1024
    assert Nn % 4 == 1 and ref['face_mask'][Nn - 1] == 7 and lane_masks(ref['face_mask'])[-1] == 7       # the last node, alone in the last lane
    gap = C.extract_ref('wg_gap')
    assert len(gap['face_counts']) == 5 and gap['face_counts'][1] == 0 and (gap['cell_counts'][[0, 2]] > 256).all() and (gap['face_counts'][[0, 2, 3, 4]] > 2048).all()
    for name in ('random_big', 'random_big_min3', 'ball', 'wg_gap'):
        ref = C.extract_ref(name)
        assert len(C.extract_case(name)['tab']) == 4913 and len(ref['vertices']) > 256 and len(ref['faces']) > 1000, name
    assert C.extract_case('random_big_min3')['min_weight'] == 3 and (C.extract_case('random_big_min3')['weight'] == 2).any()
    for N in C.NODE_COUNTS:                                                               # the counted tables: vertices, no faces
        ref = C.extract_ref('count_%d' % N)
        assert len(ref['face_mask']) == N and len(ref['vertices']) >= 1 and len(ref['faces']) == 0


# ------------------------------------------------------------------------------------------------------------------------------- the split is neutral
COLORS = (np.arange(15).reshape(5, 3) / F(16)).astype(F)
INFO = [{'id': i, 'query_id': i - 1, 'category_id': i} for i in (1, 2, 3)]


def by_hand(sc, fused, vox, cells, vs, thr, band, min_weight=1):
    x_out, cams, focals = sc[0], sc[4], sc[5]
    shapes = [tuple(x['conf'].shape) for x in x_out]
    cam = consistency_ref.camera_tables(cams, focals, shapes, None, 1e-3)
    world = consistency_ref.world_points(x_out, cams, False)
    depths = [consistency_ref.own_depth(world[j], x_out[j]['conf'], cam[j], thr) for j in range(len(shapes))]
    tab = T.NodeTable(cells, band)
    sdf, weight = T.integrate_planes(tab.nodes, cam, depths, shapes, [H * W for H, W in shapes], vs, band)
    return T.extract(tab, sdf, weight, min_weight, vox['count'], vox['pan'], vox['colors'], vs)


@pytest.mark.parametrize('scene', ['plane', 'rotated'])
def test_fuse_is_integrate_planes_and_extract(scene):
    if scene == 'plane':
        sc, vs, thr, band = T.plane_scene(), 0.25, 3.0, 2
    else:
        shapes = [(5, 7), (6, 4), (9, 3)]
        x, cams, focals, pan = consistency_ref.rotated_scene(shapes, seed=3, spread=0.1)
        sc, vs, thr, band = (x, [np.zeros((3,) + s, dtype=F) for s in shapes], pan, INFO, cams, focals), 0.2, 1.2, 1
    fused, vox, cells = T.fuse_scene(*sc[:6], vs, COLORS, min_conf_thr=thr, band=band)
    hand = by_hand(sc, fused, vox, cells, vs, thr, band)
    assert len(fused['faces']) > 20 and set(fused) == set(hand)
    for k in fused:
        if k == 'stats':
            assert fused[k] == hand[k]
        else:
            assert fused[k].dtype == hand[k].dtype and G.same_bits(fused[k], hand[k]), k
