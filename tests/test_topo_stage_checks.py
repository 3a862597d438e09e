"""The cases of tests/topo_stage_cases.py hold what they were built for and the planted mistakes are caught (CPU only, no GPU), as
tests/test_tsdf_stage_checks.py shows for the TSDF stages.

Everything is asserted on the restatements alone.  Quads: the per-quad detail of surface_ref.mesh shows every presence pattern, every exact equality
(zmax == rn(zmin k), |b - c| == |a - d|) and its two neighbours one ulp away, the zero, subnormal, negative, NaN, infinite and overflowing depths, every
face-id pattern and the T0-only / T1-only quads at the lane, wave and workgroup edges; `v_surface`, which divides the work as the kernels do, equals it.
Islands: `v_islands` equals surface_ref.face_component.  Simplify: the hand-written clusters are the ones simplify_ref.simplify finds and the emitted
faces are its faces.  Vcc: `v_vcc` equals vcc_ref.components / clean_pan.  CAUGHT records which named case differs from the restatement under which
planted mistake, BLIND which named case must not.  The last test reads tests/test_hip_topo_stages.py: every surface, simplify and vcc wrapper of
panst3r_amd/hip.py is called there by hand."""
import os
import re

import numpy as np
import pytest

import geom_stage_cases as G
import surface_ref as S
import topo_stage_cases as C
import vcc_ref

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))

# mistake -> named cases that must differ from the restatement under it.  Quads: gadget@bound, or `table` = the whole eleven-view table; vcc:
# case@connectivity@colours
CAUGHT = {
    'bound_double': {'round_eq@cut'},
    'cut_lt': {'cut_eq@cut', 'round_eq@cut', 'one_equal@one', 'subnormal_eq@cut', 'inf_all@cut', 'p7@one'},
    'tie_bc': {'diag_tie@cut', 'diag_tie@none', 'p15@cut'},
    'three_corner_winding': {'p7@cut', 'cut_eq@cut', 'ids_aab@none'},
    'view_first_of_equal': {'table@cut', 'table@none'},
    'root_largest': {'strip_1_ascending', 'strip_4097_shuffle', 'star', 'interleaved', 'equal_corners'},
    'drop_leftover': {'star'},
    'winner_last': {'dups', 'degenerate', 'collide'},
    'key_unsorted': {'dups', 'degenerate', 'collide'},
    'votes_per_neighbour': {'speckle@26@7'},
    'tie_larger': {'speckle@6@7', 'speckle@26@7'},
    'known_le': {'speckle@26@7', 'speckle@26@1'},
    'link_27': {'offsets@6@7', 'offsets@18@7', 'last_legal@6@7'},
}
BLIND = {
    'bound_double': {'cut_eq@cut', 'cut_above@cut', 'cut_below@cut'},
    'cut_lt': {'cut_above@cut', 'cut_below@cut', 'one_ulp@one'},
    'tie_bc': {'diag_below@cut', 'diag_above@cut', 'diag_nan_a@none', 'diag_nan_b@none', 'p7@cut'},
    'three_corner_winding': {'p15@cut', 'p14@cut', 'p13@cut', 'p11@cut', 'diag_tie@cut'},
    'view_first_of_equal': {'dense@cut'},
    'root_largest': {'one_row'},
    'drop_leftover': {'strip_1_ascending', 'strip_257_shuffle', 'one_row'},
    'winner_last': {'identity', 'one', 'sized_1_64'},
    'key_unsorted': {'identity', 'one', 'sized_1_64'},
    'votes_per_neighbour': {'speckle@6@7', 'pair_wrap@26@7', 'ids@26@7'},
    'tie_larger': {'pair_wrap@26@7', 'offsets@26@7'},
    'known_le': {'speckle@26@4096'},
    'link_27': {'offsets@26@7', 'line@6@7'},
}
DENSE = ('sq17', 'strip258', 'gadgets')                            # a table without an empty view


def test_every_planted_mistake_is_listed():
    every = set(C.SURFACE_MISTAKES) | set(C.ISLAND_MISTAKES) | set(C.SIMPLIFY_MISTAKES) | set(C.VCC_MISTAKES)
    assert set(CAUGHT) == every == set(BLIND) and all(CAUGHT.values()) and all(BLIND.values()) and len(every) == 13


# ============================================================================================================================================ quads
def rows_of(out, pixel):
    sel = np.asarray(out['quad']) == pixel
    return np.asarray(out['faces'])[sel].tolist(), np.asarray(out['face_ids'])[sel].tolist()


def gadget_pixel(case, name):
    return int(case['offsets'][case['names'].index('gadgets')]) + 3 * C.GADGET_NAMES.index(name)


@pytest.mark.parametrize('absent', ['nan', 'inf'])
@pytest.mark.parametrize('k', list(C.K))
def test_variant_without_a_mistake_is_the_restatement(k, absent):
    case = C.quad_case(absent)
    ref, got = C.surface_ref_of(case, k), C.v_surface(case, k)
    assert C.same_surface(ref, got) == [] and len(ref['faces']) > 1000
    assert np.array_equal(got['row'], S.row_table(case['index'], case['N'])) and got['counts'].sum() == len(ref['faces']) == got['base'][-1]
    assert S.depth_bound(C.RATIO[k]) == C.K[k] or (np.isinf(C.K[k]) and np.isinf(S.depth_bound(C.RATIO[k])))
    other = C.surface_ref_of(C.quad_case('inf' if absent == 'nan' else 'nan'), k)       # the z of an absent pixel is never looked at
    assert C.same_surface(ref, other) == []


def test_table_shapes():
    case = C.quad_case('nan')
    shapes = dict(zip(case['names'], case['shapes']))
    dims, nwg = C.surface_dims(case['shapes'])
    quads = {n: max(h - 1, 0) * max(w - 1, 0) for n, (h, w) in shapes.items()}
    assert quads['sq17'] == 256 and quads['strip258'] == 257 and quads['two_by_two'] == 1 and 256 % (shapes['straddle'][1] - 1) != 0 and quads['straddle'] > 256
    assert shapes['row_first'] == (1, 7) and shapes['column_between'] == (7, 1) and shapes['pixel_between'] == (1, 1) and shapes['row_last'] == (1, 4)
    assert case['names'][0] == 'row_first' and case['names'][-1] == 'row_last' and 0 < case['names'].index('column_between') < len(shapes) - 1
    first = dict(zip(case['names'], dims[:, 2].tolist()))
    assert first['row_first'] == first['sq17'] == 0 and first['column_between'] == first['strip258'] == 1 and first['pixel_between'] == first['rank_strip']
    assert first['row_last'] == nwg == sum(C.wgs(q) for q in quads.values()) == 12
    assert case['index'][-1] == case['N'] - 1 and (np.diff(case['index']) > 0).all() and len(case['index']) < case['N'] <= 2049 * 2
    assert max(len(d.reshape(-1)) for d in case['depths']) <= 2049
    for absent, test in (('nan', np.isnan), ('inf', np.isposinf)):
        c = C.quad_case(absent)
        z = np.concatenate([d.reshape(-1) for d in c['depths']])
        assert test(z[~c['present']]).all() and (~c['present']).sum() > 300


def test_presence_and_depth_cut_cases():
    case = C.quad_case('nan')
    cut, none, one = (C.surface_ref_of(case, k) for k in ('cut', 'none', 'one'))
    q = lambda name: C.gadget_quad(case, name)
    for p in range(16):                                                                    # every pattern of present corners
        i = q('p%d' % p)
        want = [(p >> j) & 1 == 1 for j in range(4)]
        assert cut['present'][i].tolist() == want and cut['corners'][i] == sum(want)
        assert cut['keep'][i].tolist() == [sum(want) >= 3, sum(want) == 4]
    assert {int(cut['corners'][q('p%d' % p)]) for p in range(16)} == {0, 1, 2, 3, 4}
    three = {p: rows_of(cut, gadget_pixel(case, 'p%d' % p))[0] for p in (7, 14, 13, 11)}   # missing d, a, b, c: each code once
    R = lambda name: S.row_table(case['index'], case['N'])[gadget_pixel(case, name) + np.array([0, 1, 3 * len(C.GADGETS), 3 * len(C.GADGETS) + 1])]
    for p, corners in ((7, (0, 2, 1)), (14, (1, 2, 3)), (13, (0, 2, 3)), (11, (0, 3, 1))):
        assert three[p] == [R('p%d' % p)[list(corners)].tolist()], p
    # the cut at equality and one float on either side, exactly
    i = q('cut_eq')
    assert cut['zmin'][i, 0] == 2 and cut['zmax'][i, 0] == cut['bound'][i, 0] == C.B2 and cut['keep'][i, 0]
    assert cut['zmax'][q('cut_above'), 0] == np.nextafter(C.B2, F(3)) and not cut['keep'][q('cut_above'), 0]
    assert cut['zmax'][q('cut_below'), 0] == np.nextafter(C.B2, F(0)) and cut['keep'][q('cut_below'), 0]
    assert float(C.B2) == 2.0 * float(C.K['cut'])                                          # exact: this one cannot tell a double product
    i = q('round_eq')
    assert cut['zmax'][i, 0] == cut['bound'][i, 0] and cut['keep'][i, 0] and float(cut['bound'][i, 0]) > float(C.ZR) * float(C.K['cut'])
    for name, kept in (('zmin_pos_zero', False), ('zmin_neg_zero', False), ('negative', False), ('nan_corner', False), ('inf_one', False), ('subnormal_next', False),
                       ('subnormal_eq', True), ('inf_all', True), ('overflow', True)):
        assert bool(cut['keep'][q(name), 0]) == kept and cut['has'][q(name), 0], name
    u32 = lambda x: np.asarray(x, dtype=F).view(np.uint32)
    z = case['depths'][case['names'].index('gadgets')]
    col = lambda name: 3 * C.GADGET_NAMES.index(name)
    assert u32(z[0, col('zmin_pos_zero')]) == 0 and u32(z[0, col('zmin_neg_zero')]) == 0x80000000 and u32(z[0, col('subnormal_eq')]) == 1
    assert cut['bound'][q('subnormal_eq'), 0] == C.TINY == cut['zmax'][q('subnormal_eq'), 0]  # a product that flushes subnormals gives 0 and cuts
    assert np.isposinf(cut['bound'][q('overflow'), 0]) and np.isfinite(cut['zmax'][q('overflow'), 0])
    assert np.isposinf(cut['zmin'][q('inf_all'), 0]) and np.isnan(cut['zmin'][q('nan_corner'), 0])
    # k = +inf: no cut, zmin > 0 still applies; k = 1: three equal depths stay, one ulp apart go
    assert not cut['keep'][q('none_subnormal'), 0] and none['keep'][q('none_subnormal'), 0] and np.isposinf(none['bound'][q('none_subnormal'), 0])
    assert not none['keep'][q('zmin_pos_zero'), 0] and not none['keep'][q('negative'), 0] and not none['keep'][q('nan_corner'), 0] and none['keep'][q('inf_one'), 0]
    assert one['keep'][q('one_equal'), 0] and one['zmax'][q('one_equal'), 0] == one['bound'][q('one_equal'), 0]
    assert not one['keep'][q('one_ulp'), 0] and one['zmax'][q('one_ulp'), 0] == np.nextafter(F(2), F(3)) and cut['keep'][q('one_ulp'), 0]


def test_diagonal_face_id_and_rank_cases():
    case = C.quad_case('nan')
    cut, none = C.surface_ref_of(case, 'cut'), C.surface_ref_of(case, 'none')
    q = lambda name: C.gadget_quad(case, name)
    assert cut['tie'][q('diag_tie')] and not cut['bc'][q('diag_tie')] and cut['keep'][q('diag_tie')].all()
    assert cut['bc'][q('diag_below')] and not cut['tie'][q('diag_below')] and not cut['bc'][q('diag_above')] and not cut['tie'][q('diag_above')]
    z = case['depths'][case['names'].index('gadgets')]
    x = 3 * C.GADGET_NAMES.index('diag_below')
    assert float(z[1, x + 1]) - float(z[0, x]) - (float(z[0, x + 1]) - float(z[1, x])) == 2.0 ** -22       # one ulp of 2.125 between the two differences
    for name, keep in (('diag_nan_b', [True, False]), ('diag_nan_a', [False, False])):
        assert not none['bc'][q(name)] and not none['tie'][q(name)] and none['corners'][q(name)] == 4 and none['keep'][q(name)].tolist() == keep, name
    assert cut['keep'][q('t1_only')].tolist() == [False, True] and cut['keep'][q('t0_only')].tolist() == [True, False]
    for name, want in (('ids_aaa', 5), ('ids_aab', 5), ('ids_aba', 5), ('ids_baa', 5), ('ids_abc', 0), ('ids_00b', 0), ('ids_b00', 0), ('ids_0bb', 7), ('ids_0bc', 0)):
        faces, fid = rows_of(cut, gadget_pixel(case, name))
        assert fid == [want] and case['vertex_ids'][faces[0]].tolist() == list(C.GADGETS[name][2]), name
    # the rank strip: quad x - 1 keeps T0 alone and quad x keeps T1 alone for every deep column x
    strip = lambda i: C.quad_of(case, 'rank_strip', i)
    for x in C.STRIP_DEEP:
        assert cut['keep'][strip(x - 1)].tolist() == [True, False] and cut['keep'][strip(x)].tolist() == [False, True], x
    lanes = {(x - 1) % 256: 'T0' for x in C.STRIP_DEEP}
    lanes.update({x % 256 + 1000: 'T1' for x in C.STRIP_DEEP})
    assert lanes[63] == 'T0' and lanes[1064] == 'T1' and lanes[1127] == 'T1' and lanes[192] == 'T0' and lanes[255] == 'T0' and lanes[1255] == 'T1'
    # T0-only in lane 63 | T1-only in lane 0 of the next wave; T1-only in lane 63; T0-only in lane 0; both in the last thread of a workgroup
    assert (127 % 64, 192 % 64, 255 % 256, 511 % 256) == (63, 0, 255, 255)
    counts = C.v_surface(case, 'cut')['counts']
    dims, nwg = C.surface_dims(case['shapes'])
    wg = dims[case['names'].index('full_empty'), 2]
    assert counts[wg] == 512 and counts[wg + 1] == 0 and dims[case['names'].index('two_by_two'), 2] == wg + 2    # a full workgroup next to an empty one


def surface_hits(mistake):
    hit = set()
    for k in C.K:
        case = C.quad_case('nan')
        ref, got = C.v_surface(case, k), C.v_surface(case, k, mistake)
        for name in C.GADGETS:
            if rows_of(ref, gadget_pixel(case, name)) != rows_of(got, gadget_pixel(case, name)):
                hit.add('%s@%s' % (name, k))
        if C.same_surface(ref, got):
            hit.add('table@%s' % k)
        dense = C.quad_case('nan', DENSE)
        if C.same_surface(C.v_surface(dense, k), C.v_surface(dense, k, mistake)):
            hit.add('dense@%s' % k)
    return hit


@pytest.mark.parametrize('mistake', C.SURFACE_MISTAKES)
def test_surface_mistakes_are_caught(mistake):
    hit = surface_hits(mistake)
    assert CAUGHT[mistake] <= hit and not (BLIND[mistake] & hit), (mistake, sorted(hit))


def test_dense_table_is_the_same_views():
    dense = C.quad_case('nan', DENSE)
    assert dense['names'] == list(DENSE) and len(np.unique(C.surface_dims(dense['shapes'])[0][:, 2])) == len(DENSE)
    assert C.same_surface(C.surface_ref_of(dense, 'cut'), C.v_surface(dense, 'cut')) == []


# ========================================================================================================================================== islands
def test_island_cases_hold_what_they_name():
    cases = C.island_cases()
    for name, (faces, M) in cases.items():
        assert faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < M and (len(faces) <= 2049 or name == 'strip_4097_shuffle'), name
        v = C.v_islands(faces, M)
        assert np.array_equal(v['component'], S.face_component(faces, M)) and v['status'] == 0 and v['size'].sum() == len(faces), name
        named = np.zeros(M, dtype=bool)
        named[faces.reshape(-1)] = True
        assert (v['root'][~named] == np.nonzero(~named)[0]).all() and (v['size'][~named] == 0).all() and (v['root'] <= np.arange(M)).all(), name
    assert {len(cases['strip_%d_shuffle' % n][0]) for n in C.STRIP_F} == {1, 63, 64, 65, 255, 256, 257, 1025, 4097}
    for Fn in C.STRIP_F:
        f, M = cases['strip_%d_shuffle' % Fn]
        assert (C.v_islands(f, M)['component'] == 0).all() and M == Fn + 2
        if Fn > 1:
            assert not np.array_equal(f, C.strip(Fn)[0]) and np.array_equal(f[np.argsort(f[:, 0])], C.strip(Fn)[0])
            assert np.array_equal(cases['strip_%d_descending' % Fn][0], C.strip(Fn)[0][::-1]) if Fn < C.DEEP_F else True
    f, M = cases['star']
    assert (f[:, 2] == M - 1).all() and (C.v_islands(f, M)['component'] == 0).all() and f[-1, 0] == 0 and len(f) > 256
    f, M = cases['interleaved']
    comp = C.v_islands(f, M)
    assert comp['component'].tolist() == [0, 1] * (len(f) // 2) and comp['size'][:2].tolist() == [len(f) // 2] * 2 and comp['root'][M - 1] == M - 1
    f, M = cases['duplicates']
    assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f) // 4 and len(f) > 256
    f, M = cases['equal_corners']
    eq = (f[:, 0] == f[:, 1]).astype(int) + (f[:, 1] == f[:, 2]) + (f[:, 0] == f[:, 2])
    assert (eq == 1).sum() >= 4 and (eq == 3).sum() >= 3 and sorted(set(C.v_islands(f, M)['component'].tolist())) == [0, 2, 5, 7, 9]
    f, M = cases['unused_rows']
    assert len(np.unique(f)) * 3 < M + 6 and f.min() == 2 and f.max() == M - 5
    assert cases['one_row'][1] == 1
    f, M = C.range_case()
    v = C.v_islands(f, M)
    assert v['status'] == C.RANGE and np.array_equal(np.nonzero(v['component'] < 0)[0], C.RANGE_BAD) and v['size'].sum() == len(f) - 3
    bad = f[list(C.RANGE_BAD)]
    assert sorted(bad[(bad < 0) | (bad >= M)].tolist()) == [-1, M, M] and [int(np.argmax((b < 0) | (b >= M))) for b in bad] == [1, 0, 2]
    assert len(set(v['component'][v['component'] >= 0].tolist())) >= 2


@pytest.mark.parametrize('mistake', C.ISLAND_MISTAKES)
def test_island_mistakes_are_caught(mistake):
    cases = C.island_cases()
    differs = lambda name: not np.array_equal(C.v_islands(*cases[name], mistake)['component'], C.v_islands(*cases[name])['component'])
    assert all(differs(n) for n in CAUGHT[mistake]) and not any(differs(n) for n in BLIND[mistake])


# ========================================================================================================================================= simplify
@pytest.mark.parametrize('name', list(C.SIMPLIFY_CASES))
def test_simplify_cases_are_the_reference(name):
    c = C.simplify_case(name)
    Fn = len(c['faces'])
    assert Fn <= 2049 and c['M'] <= 2049 and 1 <= c['Mv'] <= c['M'] and len(c['ids']) >= c['Mv'] and len(c['cluster']) == c['M']
    for dedupe in (True, False):
        v = C.v_simplify(c, dedupe)
        assert v['status'][2] + v['status'][3] + v['status'][4] == Fn and v['counts'].sum() == len(v['faces']) <= v['status'][4]
        assert np.isnan(v['masked'][v['used'] == 0]).all() and G.same_bits(v['masked'][v['used'] != 0], c['vertices'][v['used'] != 0])
        if not c['by_ref']:
            continue
        r = C.simplify_by_ref(c, dedupe)
        st = r['stats']
        assert (st['vertices_used'], st['faces_left_out'], st['faces_degenerate']) == tuple(v['status'][1:4]) and st['faces_out'] == len(v['faces'])
        if 'used' in r:                                                                    # (a mesh whose every face goes has no detail)
            assert np.array_equal(r['cluster'], c['cluster']) and st['vertices_out'] == c['Mv'] and np.array_equal(r['used'], v['used'] != 0)
            assert np.array_equal(r['new'], v['new']) and np.array_equal(r['left'], v['klass'] == -1) and np.array_equal(r['degenerate'], v['klass'] == -2)
            for k in ('faces', 'quad', 'src_face'):
                assert np.array_equal(r[k], v[k]), k
            assert np.array_equal(v['face_ids'], C.simplify_ref.face_id(c['ids'][r['faces']]))


def test_simplify_cases_hold_what_they_name():
    sizes = {(len(C.simplify_case(n)['faces']), C.simplify_case(n)['M']) for n in C.SIMPLIFY_CASES if n.startswith('sized')}
    assert sizes == {(f, m) for f in (1, 255, 256, 257, 513) for m in (64, 256)}
    c = C.simplify_case('sized_513_256')
    v, M = C.v_simplify(c), c['M']
    assert (v['used'][M - 3:] == 0).all() and v['used'][[M - 5, M - 6, M - 7]].all() and v['status'][1] == v['used'].sum() < M
    assert np.isposinf(c['vertices'][M - 5, 2]) and np.isnan(c['vertices'][M - 6, 0]) and np.signbit(c['vertices'][M - 7, 1]) and c['vertices'][M - 7, 1] == 0
    assert c['cluster'][M - 5] == c['cluster'][M - 6] == -1 and c['cluster'][M - 7] >= 0 and (c['cluster'] == -1).sum() > 5
    assert c['cluster'].max() == c['Mv'] - 1 and v['status'][2] > 0 and v['status'][3] > 0 and (c['ids'][:c['Mv']] == 0).any()
    ids = c['ids'][v['faces']]
    same = (ids[:, 0] == ids[:, 1]).astype(int) + (ids[:, 1] == ids[:, 2]) + (ids[:, 0] == ids[:, 2])
    assert {0, 1, 3} <= set(same.tolist())
    assert C.simplify_case('identity')['Mv'] == C.simplify_case('identity')['M'] and C.simplify_case('one')['Mv'] == 1
    assert C.v_simplify(C.simplify_case('one'))['status'][3] == 62
    # degenerate: two equal, three equal, already degenerate in the input
    c = C.simplify_case('degenerate')
    v = C.v_simplify(c)
    n = v['new']
    eq = (n[:, 0] == n[:, 1]).astype(int) + (n[:, 1] == n[:, 2]) + (n[:, 0] == n[:, 2])
    raw = (c['faces'][:, 0] == c['faces'][:, 1]) | (c['faces'][:, 1] == c['faces'][:, 2])
    assert (eq == 1).any() and (eq == 3).any() and raw.sum() == 2 and (v['klass'][raw] == -2).all() and ((v['klass'] == -2) & ~raw).sum() >= 2
    # duplicates
    c = C.simplify_case('dups')
    v, f = C.v_simplify(c), c['faces']
    assert c['Mv'] == c['M'] == 40 and np.array_equal(c['cluster'], np.arange(40))
    assert f[0].tolist() == [20, 9, 3] and f[5].tolist() == [9, 20, 3] and f[500].tolist() == [3, 9, 20] and len({int(v['key'][i]) for i in (0, 5, 500)}) == 1
    assert 0 in v['src_face'] and 5 not in v['src_face'] and 500 not in v['src_face'] and v['faces'][0].tolist() == [20, 9, 3]       # the reversed copy came first: its winding stays
    assert len(set(v['key'][60:71].tolist())) == 1 and len(set(v['key'][250:261].tolist())) == 1 and v['key'][400] == v['key'][60]
    assert 60 in v['src_face'] and not np.isin(np.r_[61:71, 400], v['src_face']).any() and 250 in v['src_face'] and not np.isin(np.arange(251, 261), v['src_face']).any()
    assert 191 % 64 == 63 and len(set(v['key'][191:194].tolist())) == 1 and 191 in v['src_face'] and 192 not in v['src_face']
    assert len(v['faces']) < v['status'][4] == 513 and len(C.v_simplify(c, dedupe=False)['faces']) == 513
    # the wrapped chain
    c = C.simplify_case('collide')
    v = C.v_simplify(c)
    cap = c['cap']
    assert cap == C.capacity(len(c['faces'])) == 2 * len(c['faces']) and np.array_equal(c['cluster'], np.arange(c['M']))
    assert (G.home_slot(np.array(sorted(v['winner']), dtype=np.uint64), cap) == cap - 1).sum() == 8 and len(v['winner']) < len(c['faces']) and int(v['key'][-1]) == int(v['key'][11])
    # cluster values outside [-1, Mv), and corners outside [0, M)
    c = C.simplify_case('bad_cluster')
    v = C.v_simplify(c)
    assert sorted(set(c['cluster'].tolist())) == [-2, -1, 0, 1, 2, 3, 4, 5, 6] and c['Mv'] == 6 and v['status'][0] == C.RANGE
    assert v['klass'].tolist() == [0, 0, -1, -1, -1, 0, -2, 0] and v['src_face'].tolist() == [0, 1] and (v['new'] == c['Mv'] - 1).any()
    c = C.simplify_case('bad_corner')
    v = C.v_simplify(c)
    assert v['status'].tolist() == [C.RANGE, 6, 2, 0, 3] and v['used'].tolist() == [1, 1, 1, 0, 0, 1, 1, 1] and v['src_face'].tolist() == [0, 3]
    assert c['faces'][1, 1] == c['M'] and c['faces'][2, 0] == -1
    # the face key: 3 x 21 bits of the sorted corners + 1; the largest field value is 2^21 - 2 + 1
    assert int(C.face_key([[5, 0, 2 ** 21 - 3]])[0]) == 1 | (6 << 21) | ((2 ** 21 - 2) << 42) and int(C.face_key([[2, 1, 0]], 'key_unsorted')[0]) == 3 | (2 << 21) | (1 << 42)
    assert len(C.colliding_triples(64, 63, 32, 8)) == 8


@pytest.mark.parametrize('mistake', C.SIMPLIFY_MISTAKES)
def test_simplify_mistakes_are_caught(mistake):
    def differs(name):
        a, b = C.v_simplify(C.simplify_case(name), True, mistake), C.v_simplify(C.simplify_case(name))
        return any(not np.array_equal(a[k], b[k]) for k in C.SIMPLIFY_FIELDS)
    assert all(differs(n) for n in CAUGHT[mistake]) and not any(differs(n) for n in BLIND[mistake])


# ============================================================================================================================================== vcc
@pytest.mark.parametrize('name', list(C.VCC_CASES))
def test_vcc_cases_are_the_reference(name):
    c = C.vcc_case(name)
    Mv = len(c['pan'])
    assert Mv <= 2049 and len(np.unique(c['cells'], axis=0)) == Mv and np.abs(c['cells']).max() < C.LIM
    for conn in (6, 18, 26):
        for mv in (1, C.MIN_VOXELS, C.MIN_VOXELS + 1):
            v = C.v_vcc(c, conn, mv)
            ref = vcc_ref.components(c['cells'], c['pan'], c['count'], conn)
            for k in ('root', 'component'):
                assert np.array_equal(v[k], ref[k]), k
            out, moved, gone = vcc_ref.clean_pan(c['cells'], c['pan'], c['count'], mv, conn)
            assert np.array_equal(v['out_pan'], out) and (v['moved'], v['gone']) == (moved, gone)
            assert np.array_equal(v['root'] == -1, c['pan'] <= 0) and (v['size'] > 0).sum() == v['C'] and v['size'].sum() == (c['pan'] > 0).sum()
            assert sum(v['pairs'].values()) >= len(v['pairs']) and (mv > 1 or not v['pairs'])
            for key, votes in v['pairs'].items():                                          # best: most votes, then the smallest id
                r, pid = key >> 32, key & 0xFFFFFFFF
                b = int(v['best'][r])
                assert (b >> 32, -(0xFFFFFFFF - (b & 0xFFFFFFFF))) >= (votes, -pid)


def test_vcc_cases_hold_what_they_name():
    assert [len(C.vcc_case('blob_%d' % n)['pan']) for n in C.VCC_MV] == [1, 63, 64, 65, 256, 257, 1024, 1025, 2049]
    c = C.vcc_case('blob_2049')
    assert (c['cells'] < 0).any() and (c['cells'] > 0).any() and {0, -3, 1, 2, 3} == set(c['pan'].tolist())
    v = C.v_vcc(c)
    assert v['C'] > 100 and v['moved'] > 50 and v['gone'] > 10 and len(v['pairs']) > 100
    c = C.vcc_case('last_legal')
    assert c['cells'].max() == C.LIM - 1 and c['cells'].min() == -(C.LIM - 1) and C.v_vcc(c)['C'] == 5       # every pair joined: their neighbours out of range are never formed
    assert C.beyond_case()['cells'][-1].tolist() == [C.LIM, 0, 0] and len(C.duplicate_case()['pan']) == 13
    d = C.duplicate_case()
    assert (d['cells'][-1] == d['cells'][3]).all()
    # each of the 26 offsets is the only link once: the pair is one component exactly from the connectivity that includes it
    c = C.vcc_case('offsets')
    for conn, axes in ((6, 1), (18, 2), (26, 3)):
        root = C.v_vcc(c, conn)['root']
        for j, d in enumerate(C.OFFSETS26):
            assert (root[2 * j] == root[2 * j + 1]) == (sum(x != 0 for x in d) <= axes), (conn, d)
    assert len(set(C.OFFSETS26)) == 26 and [sum(sum(x != 0 for x in d) == a for d in C.OFFSETS26) for a in (1, 2, 3)] == [6, 12, 8]
    # ids: equal ids that touch only through a void cell stay apart
    c = C.vcc_case('ids')
    root = C.v_vcc(c, 26)['root']
    assert c['pan'].tolist()[:4] == [1, 0, 1, 1] and root[0] == 0 and root[1] == -1 and root[2] == root[3] == 2 and root[4] == -1 and root[5] == 5
    assert root[6] == root[7] == 6 and root[10] == 10 and root[11] == -1
    c = C.vcc_case('line')
    assert len(c['pan']) == 2049 and C.v_vcc(c, 6)['C'] == 1 and not np.array_equal(np.sort(c['cells'][:, 0]), c['cells'][:, 0]) and (np.diff(np.sort(c['cells'][:, 0])) == 1).all()
    c = C.vcc_case('runs')
    v = C.v_vcc(c, 6)
    assert v['table']['root'].tolist() == [0, 60, 71, 250, 261] and v['table']['size'].tolist() == [60, 11, 179, 11, 339]
    assert v['table']['points'][1] == 11 * (2 ** 31 - 1) > 2 ** 32
    c = C.vcc_case('wrap')
    cap = c['cap']
    assert cap == 2 * len(c['pan']) and (G.home_slot(G.vx_key(c['cells']), cap) == cap - 1).sum() == 12


def test_speckle_and_pair_cases():
    c = C.vcc_case('speckle')
    mk = c['marks']
    v = C.v_vcc(c, 26, 3, 7)
    root, pan = v['root'], c['pan']
    s = mk['single'][0]
    assert v['pairs'] [(int(root[s]) << 32) | 1] == 9 and v['out_pan'][s] == 1                                 # nine voxels of the block touch it
    fl = mk['floater']
    assert v['small'][fl].all() and (v['out_pan'][fl] == 0).all() and not any(k >> 32 == root[fl[0]] for k in v['pairs']) and v['best'][root[fl[0]]] == 0
    t = mk['tie_S'][0]
    assert v['pairs'][(int(root[t]) << 32) | 5] == v['pairs'][(int(root[t]) << 32) | 4] == 1 and v['out_pan'][t] == 4
    assert int(v['best'][root[t]]) == (1 << 32) | (0xFFFFFFFF - 4)
    s1, s2 = mk['pairs_s']
    assert root[s1] == root[s2] == s1 and v['pairs'][(s1 << 32) | 1] == 4 and v['pairs'][(s1 << 32) | 6] == 3 and (v['out_pan'][[s1, s2]] == 1).all()
    per_neighbour = C.v_vcc(c, 26, 3, 7, 'votes_per_neighbour')
    assert per_neighbour['pairs'][(s1 << 32) | 1] == 2 and per_neighbour['pairs'][(s1 << 32) | 6] == 3 and (per_neighbour['out_pan'][[s1, s2]] == 6).all()
    # min_voxels at size, size + 1 and 1
    A = mk['tie_A']
    assert v['size'][root[A[0]]] == 3 and not v['small'][A].any() and C.v_vcc(c, 26, 4, 7)['small'][A].all() and not C.v_vcc(c, 26, 1, 7)['small'].any()
    assert C.v_vcc(c, 26, 1, 7)['moved'] == C.v_vcc(c, 26, 1, 7)['gone'] == 0 and np.array_equal(C.v_vcc(c, 26, 1, 7)['out_pan'], pan)
    # the winner equal to ncolors - 1 (read) and to ncolors (not read: 0 is blended)
    s6, s7 = mk['last_6_S'][0], mk['last_7_S'][0]
    assert v['out_pan'][s6] == 6 and v['out_pan'][s7] == 7
    blend = lambda row, colour: C.cloud_ref.blend(c['rgb'][row], colour, C.OPACITY)
    assert G.same_bits(v['out_colors'][s6], blend(s6, c['colors'][6])) and G.same_bits(v['out_colors'][s7], blend(s7, np.zeros(3, dtype=F)))
    assert (c['colors'][6] != 0).all() and (c['colors'][7] != 0).all()
    one = C.v_vcc(c, 26, 3, 1)
    assert G.same_bits(one['out_colors'], C.cloud_ref.blend(c['rgb'], np.zeros_like(c['rgb']), C.OPACITY))
    # the two products and the sum each round
    w1, w2 = F(1.0 - C.OPACITY), F(C.OPACITY)
    x, t6 = c['rgb'][s6].astype(np.float64), c['colors'][6].astype(np.float64)
    assert (float(w1) * x != (w1 * c['rgb'][s6]).astype(np.float64)).any() and (float(w2) * t6 != (w2 * c['colors'][6]).astype(np.float64)).any()
    p1, p2 = (w1 * c['rgb'][s6]).astype(np.float64), (w2 * c['colors'][6]).astype(np.float64)
    assert (p1 + p2 != v['out_colors'][s6].astype(np.float64)).any()
    # the pair table at its smallest power of two: eight distinct pairs at home in the last of 16 slots
    c = C.vcc_case('pair_wrap')
    v = C.v_vcc(c, 6, 3, 4096)
    keys = np.array(sorted(v['pairs']), dtype=np.uint64)
    assert c['pair_cap'] == 16 == C.capacity(len(keys)) and len(keys) == 8 and (G.home_slot(keys, 16) == 15).all() and set(v['pairs'].values()) == {1}
    assert [(k >> 32, k & 0xFFFFFFFF) for k in sorted(v['pairs'])] == sorted(c['planted']) and v['moved'] == 8 and max(p for _, p in c['planted']) < 4095


@pytest.mark.parametrize('mistake', C.VCC_MISTAKES)
def test_vcc_mistakes_are_caught(mistake):
    def differs(entry):
        name, conn, nc = entry.split('@')
        a, b = (C.v_vcc(C.vcc_case(name), int(conn), C.MIN_VOXELS, int(nc), m) for m in (mistake, None))
        return not (np.array_equal(a['out_pan'], b['out_pan']) and np.array_equal(a['root'], b['root']) and G.same_bits(a['out_colors'], b['out_colors']) and
                    a['pairs'] == b['pairs'] and np.array_equal(a['best'], b['best']))
    assert all(differs(n) for n in CAUGHT[mistake]) and not any(differs(n) for n in BLIND[mistake])


def test_probe_restatement():
    keys = np.full(8, C.EMPTY, dtype=np.uint64)
    k = G.vx_key(G.colliding_cells(8, 7, 3))
    keys[7], keys[0], keys[1] = k[0], k[1], k[2]
    assert [C.probe(keys, int(x)) for x in k] == [7, 0, 1] and C.probe(keys, int(G.vx_key([[100, 100, 100]])[0])) == -1
    assert C.probe(np.full(8, 5, dtype=np.uint64), 6) == -1 and C.capacity(1) == 2 and C.capacity(4) == 8 and C.capacity(5) == 16


# ===================================================================================================================== every wrapper is called by hand
def test_gpu_file_calls_every_wrapper_by_hand():
    with open(os.path.join(HERE, '..', 'panst3r_amd', 'hip.py')) as fh:
        wrappers = set(re.findall(r'^def ((?:surface|simplify|vcc)_\w+)\(', fh.read(), flags=re.M))
    assert {'surface_rows', 'surface_count', 'surface_emit', 'surface_link', 'surface_components', 'simplify_used', 'simplify_mask', 'simplify_remap', 'simplify_count',
            'simplify_emit', 'vcc_cells', 'vcc_build', 'vcc_link', 'vcc_flatten', 'vcc_votes', 'vcc_apply', 'vcc_count', 'vcc_rank'} <= wrappers
    with open(os.path.join(HERE, 'test_hip_topo_stages.py')) as fh:
        text = fh.read()
    missing = sorted(w for w in wrappers if not re.search(r'\bhip\.%s\(' % w, text))
    assert not missing, missing
