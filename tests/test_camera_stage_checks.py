"""The cases of tests/camera_stage_cases.py hold what they were built for (CPU only, no GPU), as tests/test_geom_stage_checks.py shows for the cloud and
voxel stages.

Each case's built-for property is asserted on the yardsticks (render_ref, mesh_ref) alone: this u IS an integer, this cell has two candidates with equal
depth bits, more than 8 192 entries have a box above 64 pixels and each wins a row that is all its own.  The restated steps with a `variant=` equal the
yardsticks on every case without one, and every planted mistake changes the output of the cases that CAUGHT names for it - so a kernel that made that
mistake would fail tests/test_hip_camera_stages.py on a case known by name.  `gap_table()` keeps on record which of the mistakes the scenes of the
end-to-end GPU tests let through before these cases existed (docs/experiments.md §18)."""
import numpy as np
import pytest

import camera_stage_cases as C
import mesh_ref as M
import render_ref as R

F = np.float32
SPLAT, MESH = C.splat_cases(), C.mesh_cases()
SPLAT_NAMES = [g + '/' + n for g, d in SPLAT.items() for n in d]
MESH_NAMES = [g + '/' + n for g, d in MESH.items() for n in d]


def _case(table, name):
    g, n = name.split('/')
    return table[g][n]


def _uv(case, cam=0):
    """float32 u, v, zc of every point of a splat case in one camera, as step 3 computes them"""
    cam = case['cams'][cam]
    with np.errstate(all='ignore'):
        xc, yc, zc = R.camera_coords(case['points'], cam)
        return (R.quotient(cam[12] * xc, zc) + cam[13]).astype(F), (R.quotient(cam[12] * yc, zc) + cam[14]).astype(F), zc


def _hit(z):
    return z != C.EMPTY


# ------------------------------------------------------------------------------------------------------------------------ the restated steps
@pytest.mark.parametrize('name', SPLAT_NAMES)
def test_splat_v_without_a_variant_is_the_yardstick(name):
    case = _case(SPLAT, name)
    want = C.splat_zbuf(case)
    got = np.stack([C.splat_v(case['points'], cam, case['H'], case['W'], case['half'], case['radius'], case['max_radius']) for cam in case['cams']])
    assert np.array_equal(got, want)
    assert _hit(want).any()                                                    # every splat case draws something


@pytest.mark.parametrize('name', MESH_NAMES)
def test_setup_v_and_raster_v_without_a_variant_are_the_yardstick(name):
    case = _case(MESH, name)
    for cam, s in zip(case['cams'], C.mesh_setups(case)):
        sv = C.setup_v(case['vertices'], case['faces'], cam, case['H'], case['W'], case['near'])
        assert set(sv) == set(s) and all(np.array_equal(sv[k], s[k], equal_nan=(k == 'q')) for k in s)
        assert np.array_equal(C.raster_v(sv, case['H'], case['W'], case['near'], case['far']), M.raster(s, case['H'], case['W'], case['near'], case['far'])[0])


@pytest.mark.parametrize('key', sorted(C.CAUGHT), ids=lambda k: k[0] + '-' + k[1])
def test_every_planted_mistake_changes_its_named_cases(key):
    stage, variant = key
    assert C.CAUGHT[key]
    for name in C.CAUGHT[key]:
        if stage == 'splat':
            case = _case(SPLAT, name)
            changed = (C.splat_zbuf(case, variant) != C.splat_zbuf(case)).any()
        elif stage == 'mesh':
            case = _case(MESH, name)
            changed = (C.mesh_zbuf(case, variant) != C.mesh_zbuf(case)).any()
        elif stage == 'mesh_resolve':
            case = _case(MESH, name)
            z = C.mesh_zbuf(case)
            changed = (C.mesh_resolved(case, z, 'vertex', variant)[2] != C.mesh_resolved(case, z, 'vertex')[2]).any()
        else:
            pan = C.area_cases()[name]
            changed = (C.area_ref(pan, C.AREA_ID2ROW, C.AREA_S, C.AREA_MIN, variant)[0] != C.area_ref(pan, C.AREA_ID2ROW, C.AREA_S, C.AREA_MIN)[0]).any()
        assert changed, (key, name)


def test_the_gap_that_was_closed_is_on_record():
    """the issue's two lists as data: eight mistakes the end-to-end scenes caught (some by accident), eleven they let through; all of them, and the five
    added here, now change a named case"""
    table = C.gap_table()
    before = {(s, n): seen for s, n, seen, cases in table}
    assert sum(v is True for v in before.values()) == 8 and sum(v is False for v in before.values()) == 11 and sum(v is None for v in before.values()) == 5
    assert {k for k, v in before.items() if v is None} == {('mesh', 'snap_half_away'), ('mesh', 'box_in'), ('splat', 'tie_larger_row'), ('mesh', 'tie_larger_face'),
                                                           ('area', 'drop_cross_camera_run')}
    assert all(cases for s, n, seen, cases in table)
    for s, n, seen, cases in table:
        print('%-13s %-22s scenes before: %-5s now: %s' % (s, n, {True: 'some', False: 'none', None: '-'}[seen], ', '.join(cases)))


# ------------------------------------------------------------------------------------------------------------------------------------ splatter
def test_pixel_rule_cases():
    for axis, name in ((0, 'pixel/u_r0'), (1, 'pixel/v_r0')):
        case = _case(SPLAT, name)
        t = _uv(case)[axis]
        n = (case['W'], case['H'])[axis]
        assert n == 8 and C.f32_bits(t).tolist() == C.f32_bits(np.asarray([3, C.below(3), -0.0, -0.5, 8, C.below(8)], dtype=F)).tolist()      # exact, -0.0 included
        z = C.splat_zbuf(case)[0].reshape(case['H'], case['W'])
        line = lambda k: z[1 + 3 * k, :] if axis == 0 else z[:, 1 + 3 * k]
        assert [np.nonzero(_hit(line(k)))[0].tolist() for k in range(6)] == [[3], [2], [0], [], [], [7]]
        z1 = C.splat_zbuf(_case(SPLAT, name.replace('r0', 'r1')))[0].reshape(case['H'], case['W'])
        line = lambda k: z1[1 + 3 * k, :] if axis == 0 else z1[:, 1 + 3 * k]
        assert [np.nonzero(_hit(line(k)))[0].tolist() for k in range(6)] == [[2, 3, 4], [1, 2, 3], [0, 1], [0], [7], [6, 7]]     # (-1, 0) and W reach in at radius 1


def test_cull_cases():
    case = _case(SPLAT, 'cull/planes_and_non_finite')
    u, v, zc = _uv(case)
    assert zc[0] == case['cams'][0, 15] == C.NEAR_S and C.f32_bits(zc[1]) == C.f32_bits(C.NEAR_S) - 1
    z = C.splat_zbuf(case)
    assert np.nonzero(_hit(z[0]))[0].tolist() == [2 * 8 + 2, 3 * 8 + 5] and (z[0][[18, 29]] & C.LOW).tolist() == [0, 11]      # near itself, and the plain point
    assert np.isinf(zc[2:4]).all() and np.isnan(zc[4]) and zc[5] < 0 and zc[12] == 0
    with np.errstate(all='ignore'):
        ident, rot = R.camera_coords(case['points'], case['cams'][0]), R.camera_coords(case['points'], case['cams'][1])
    assert np.isfinite([c[10] for c in ident]).all() and np.isinf(rot[0][10]) and np.isfinite(rot[2][10]) and rot[2][10] >= C.NEAR_S      # xc overflows inside affine34 under the
    # rotated pose only, with zc good: the one way to a non-finite xc beside a usable zc - a NaN or an infinity in the point itself reaches zc as 0 x inf = NaN
    assert all(not np.isfinite(ident[a][r]) and np.isnan(ident[2][r]) for a, r in ((0, 6), (1, 7), (0, 8), (1, 9)))
    r = _case(SPLAT, 'cull/rotated')
    assert 0 < R.splat(r['points'], r['cams'][0], r['H'], r['W'], r['half'], r['radius'], r['max_radius'])[2] < 150      # its near plane cuts through the soup


def test_limit_cases():
    for axis, name in ((0, 'limit/u'), (1, 'limit/v')):
        case = _case(SPLAT, name)
        t = _uv(case)[axis]
        assert t[0] == 2.0 ** 20 and t[1] == 2.0 ** 20 + 0.125 and np.floor(t[1]) == 2 ** 20 < max(case['H'], case['W']) - 1 and t[3] == -2.0 ** 20
        assert np.nonzero(_hit(C.splat_zbuf(case)[0]))[0].tolist() == [7, 2 ** 20]


def test_footprint_cases():
    side = lambda name: int(np.sqrt(_hit(C.splat_zbuf(_case(SPLAT, 'footprint/' + name))).sum()))
    assert [side(n) for n in ('quotient_integer', 'quotient_below_integer', 'radius_below_size', 'radius_above_size', 'max_below_radius', 'quotient_inf', 'half_zero')] == \
        [9, 7, 9, 13, 7, 33, 3]
    case = _case(SPLAT, 'footprint/quotient_integer')
    assert R.quotient(F(case['cams'][0, 12] * case['half']), case['points'][0, 2]) == 4
    case = _case(SPLAT, 'footprint/quotient_below_integer')
    assert C.f32_bits(R.quotient(F(case['cams'][0, 12] * case['half']), case['points'][0, 2])) == C.f32_bits(F(4)) - 1
    case = _case(SPLAT, 'footprint/quotient_inf')
    with np.errstate(over='ignore'):
        assert np.isposinf(R.quotient(F(case['cams'][0, 12] * case['half']), case['points'][0, 2])) and case['points'][0, 2] == case['cams'][0, 15] == F(2.0 ** -126)
    case = _case(SPLAT, 'footprint/clipped_on_four_sides')
    assert (case['H'], case['W'], case['max_radius']) == (5, 7, 16) and _hit(C.splat_zbuf(case)).all()
    case = _case(SPLAT, 'footprint/product_fp32_not_fp64')
    f, h, zc = case['cams'][0, 12], case['half'], case['points'][0, 2]
    assert F(f * h) > np.float64(f) * np.float64(h) and zc * F(2) == F(f * h)
    assert np.floor(R.quotient(F(f * h), zc)) == 2 and np.floor(F(np.float64(f) * np.float64(h) / np.float64(zc))) == 1 and _hit(C.splat_zbuf(case)).sum() == 25


def test_depth_and_launch_cases():
    case = _case(SPLAT, 'depth/rows_3_and_300')
    z, cand, _ = R.splat(case['points'], case['cams'][0], 8, 8, case['half'], 0, 16)
    assert len(case['points']) == 301 and cand[2 * 8 + 2] == 2 and z[2 * 8 + 2] == C.key(1, 3) and C.f32_bits(case['points'][3]).tolist() == C.f32_bits(case['points'][300]).tolist()
    u, v, zc = _uv(case)
    assert (u[5], v[5]) == (u[6], v[6]) == (5.5, 2.5) and C.f32_bits(zc[5]) == C.f32_bits(zc[6]) + 1 and cand[2 * 8 + 5] == 2 and z[2 * 8 + 5] == C.key(1, 6)
    case = _case(SPLAT, 'depth/rows_1_3_4')
    z, cand, _ = R.splat(case['points'], case['cams'][0], 8, 8, case['half'], 1, 16)
    assert cand[3 * 8 + 4] == 3 and ((z[_hit(z)] & C.LOW) == 1).all() and _hit(z).sum() == 9
    for m in (1, 255, 256, 257):
        case = _case(SPLAT, 'launch/M_%d' % m)
        z = C.splat_zbuf(case)[0]
        assert len(case['points']) == m and np.nonzero(_hit(z))[0].tolist() == [1 * 8 + 2] and z[10] == C.key(1, m - 1)
    case = _case(SPLAT, 'launch/three_cameras')
    z = C.splat_zbuf(case)
    assert len({tuple(c[12:]) for c in case['cams']}) == 3 and all(_hit(zb).sum() > 50 for zb in z)
    for a in range(3):                                                         # a kernel that gave every grid.y row camera a would differ in the other two
        other = np.stack([R.splat(case['points'], case['cams'][a], 12, 16, case['half'], 1, 16)[0]] * 3)
        assert sum(np.array_equal(other[b], z[b]) for b in range(3)) == 1


def test_many_cameras_rule_is_the_yardstick():
    case, want = C.many_cameras()
    assert len(case['cams']) == 65535 and want.shape == (65535, 1)
    sample = list(range(0, 40)) + list(range(997, 65535, 997)) + [65534]
    for b in sample:
        assert R.splat(case['points'], case['cams'][b], 1, 1, case['half'], 0, 16)[0][0] == want[b, 0], b
    assert (want[:15, 0] == C.EMPTY).sum() > 0 and len(set(want[:15, 0].tolist())) == 4       # three different winners, and cameras whose near plane hides theirs


def test_render_resolve_cells_and_the_rule_for_rows_out_of_range():
    rgb, colors, pan = C.cloud_fields(C.RESOLVE_M)
    for npix in (255, 256, 257):
        z = C.render_resolve_case(npix)
        index, depth, opan, orgb, ocol = R.resolve(z, rgb, colors, pan)
        assert index[:4].tolist() == [-1, C.RESOLVE_M - 1, -1, -1] and (depth[[0, 2, 3]] == 0).all() and (opan[[0, 2, 3]] == 0).all() and (orgb[[0, 2, 3]] == 0).all()
        assert z[2] != C.EMPTY and z[3] != C.EMPTY and int(z[3] & C.LOW) == 2 ** 32 - 1
        assert index[4] == 4 and C.bits1(depth[4]) == 0x7FC00001 and np.isnan(depth[5]) and C.bits1(depth[6]) == 0x80000000
        assert (orgb[index >= 0] == rgb[index[index >= 0]]).all() and (opan[index >= 0] == index[index >= 0] + 1).all() and (index >= 0).sum() > npix - 10


# ---------------------------------------------------------------------------------------------------------------------------------- rasteriser
def test_top_left_cases_are_those_of_the_host_test():
    H, W = C.QUAD_SHAPE
    for qi, quad in enumerate(C.QUADS):
        where = C.inside_quad(quad, H, W)
        for rev in ('fwd', 'rev'):
            for d in (0, 1):
                case = _case(MESH, 'topleft/quad%d_%s_d%d' % (qi, rev, d))
                n = M.raster(C.mesh_setups(case)[0], H, W, case['near'], case['far'])[1].reshape(H, W)
                assert (n[where == 1] == 1).all() and (n[where == -1] == 0).all() and (n[where == 0] <= 1).all()
    case = _case(MESH, 'topleft/strip')
    n = M.raster(C.mesh_setups(case)[0], H, W, case['near'], case['far'])[1].reshape(H, W)
    want = np.zeros((H, W), dtype=int)
    want[1:9, 1:13] = 1
    assert np.array_equal(n, want)


def test_snap_cases():
    for name, (ua, (b, d)) in C.SNAP.items():
        case = _case(MESH, 'snap/' + name)
        k2 = abs(ua) - 1                                                       # u = +-(2 k + 1) / 512
        assert k2 % 2 == 0 and ((k2 // 2) % 2 == 0) == name.endswith('even') and (ua > 0) == name.startswith('positive')
        with np.errstate(all='ignore'):
            u = R.camera_coords(case['vertices'], case['cams'][0])[0][0]
        assert u * F(256) == ua / 2 and (ua / 2) % 1 == 0.5                    # exactly half-way between two snapped positions
        x = {v: C.setup_v(case['vertices'], case['faces'], case['cams'][0], 4, 4, case['near'], v)['X'][0] for v in (None, 'snap_half_up', 'snap_half_away')}
        moved = {v: (x[v] != x[None]).any() for v in ('snap_half_up', 'snap_half_away')}
        assert moved == {'positive_even': dict(snap_half_up=True, snap_half_away=True), 'negative_odd': dict(snap_half_up=True, snap_half_away=False),
                         'negative_even': dict(snap_half_up=False, snap_half_away=True)}[name]


def test_plane_and_limit_cases():
    drawn = lambda name: C.mesh_zbuf(_case(MESH, name))[0]
    depth = lambda z: (z[_hit(z)] >> np.uint64(32)).astype(np.uint32).view(F)
    assert (depth(drawn('planes/at_near')) == 0.5).all() and (depth(drawn('planes/at_far')) == 8).all() and _hit(drawn('planes/at_near')).sum() == 23
    for name in ('planes/beyond_near', 'planes/beyond_far', 'planes/corner_below_near', 'limit/beyond', 'limit/beyond_v'):
        assert not _hit(drawn(name)).any(), name
    assert C.mesh_setups(_case(MESH, 'planes/beyond_far'))[0]['ok'][0] and not C.mesh_setups(_case(MESH, 'planes/beyond_near'))[0]['usable'][0]      # the depth test, the vertex test
    for name, d in (('planes/corner_at_near', 0.5), ('planes/corner_at_far', 8.0)):
        z = drawn(name)
        assert z[2 * 16 + 2] == C.key(d, 0) and (depth(z) == d).sum() == 1 and _hit(z).sum() == 23      # the corner's pixel alone lies on the plane
    for name, axis in (('limit/at', 0), ('limit/at_v', 1)):
        case = _case(MESH, name)
        assert case['vertices'][0, axis] == 2.0 ** 14 and _hit(drawn(name)).sum() == 7 and (case['H'], case['W'])[1 - axis] == 2 ** 14 + 2
        assert _case(MESH, name.replace('at', 'beyond'))['vertices'][0, axis] == C.above(2.0 ** 14)


def test_bad_corner_depth_and_duplicate_cases():
    case = _case(MESH, 'bad/every_kind')
    s = C.mesh_setups(case)[0]
    assert s['ok'].tolist() == [False] * 7 + [True] and s['usable'].tolist() == [False] * 4 + [True, True, False, True]      # a repeated corner and A == 0 after snapping are usable, not drawn
    v = case['vertices'][[6, 7, 8]].astype(np.float64)
    a, b = v[1, :2] - v[0, :2], v[2, :2] - v[0, :2]
    assert a[0] * b[1] - a[1] * b[0] != 0             # ... not collinear before the snap
    for k in range(4):
        case = _case(MESH, 'corner/tie_listing%d' % k)
        z = C.mesh_zbuf(case)
        face, depth, pan, ties = M.resolve(z[0], C.mesh_setups(case)[0], case['faces'], 12, 16, case['vertex_ids'])
        assert ties.reshape(12, 16)[2, 5] and pan.reshape(12, 16)[2, 5] == (10, 20, 20, 10)[k] and set(np.unique(pan)) == {0, 10, 20, 30}
    case = _case(MESH, 'corner/clockwise_no_tie')
    s = C.mesh_setups(case)[0]
    face, depth, pan, ties = M.resolve(C.mesh_zbuf(case)[0], s, case['faces'], 12, 16, case['vertex_ids'])
    assert s['swapped'][0] and not ties.any() and set(np.unique(pan)) == {0, 10, 20, 30}
    for name in ('depth/assoc_listed', 'depth/assoc_swapped'):
        case = _case(MESH, name)
        s = C.mesh_setups(case)[0]
        i, j = C.ASSOC_PIXEL
        E = [int(e) for e in M.edges(s, 0, i, j)]
        assert s['swapped'][0] == (name == 'depth/assoc_swapped') and E[0] == 2 ** 20 and int(s['A'][0]) == sum(E) == 17631603 and len(set(s['q'][0])) == 3
        e = [E[k] * s['q'][0][k] for k in range(3)]
        assert (e[0] + e[1]) + e[2] == e[0] < e[0] + (e[1] + e[2])
        a, b = C.mesh_zbuf(case)[0], C.mesh_zbuf(case, 'assoc_other')[0]
        assert np.nonzero(a != b)[0].tolist() == [i * 32 + j] and (a[i * 32 + j] >> np.uint64(32)) == (b[i * 32 + j] >> np.uint64(32)) + np.uint64(1)
    case = _case(MESH, 'duplicate/faces_2_and_300')
    z, cand = M.raster(C.mesh_setups(case)[0], 12, 16, case['near'], case['far'])
    assert len(case['faces']) == 301 and (cand[_hit(z)] == 2).all() and ((z[_hit(z)] & C.LOW) == 2).all() and C.mesh_setups(case)[0]['ok'].sum() == 2


def test_path_and_launch_cases():
    case = _case(MESH, 'paths/boxes')
    box = C.mesh_setups(case)[0]['box'].tolist()
    assert box == [C.PATH_PIXELS[k] for k in C.PATH_BOXES] + [72 * 72] and sorted(C.PATH_PIXELS.values())[:2] == [64, 65]
    s = C.mesh_setups(case)[0]
    assert [(int(s['j1'][k] - s['j0'][k] + 1), int(s['i1'][k] - s['i0'][k] + 1)) for k in range(6)] == [(8, 8), (13, 5), (5, 13), (7, 10), (65, 1), (1, 65)]
    assert case['capacities'][:4] == (6, 5, 0, 1) and (s['j0'][6], s['j1'][6], s['i0'][6], s['i1'][6]) == (0, 71, 0, 71) and _hit(C.mesh_zbuf(case)).all()
    assert any((s['box'] > 64).any() for s in C.mesh_setups(_case(MESH, 'paths/rotated')))
    for nf in (1, 255, 256, 257):
        case = _case(MESH, 'launch/Nf_%d' % nf)
        z = C.mesh_zbuf(case)[0]
        assert len(case['faces']) == nf and _hit(z).sum() == 23 and ((z[_hit(z)] & C.LOW) == nf - 1).all()
    case = _case(MESH, 'launch/three_cameras')
    assert all(c[12] != c[13] for c in case['cams']) and len({tuple(c[12:]) for c in case['cams']}) == 3 and all(_hit(z).sum() > 30 for z in C.mesh_zbuf(case))


def test_the_stride_case_lists_more_entries_than_the_wave_path_has_waves():
    case = C.stride_case()
    setups = C.mesh_setups(case)
    assert len(setups) == 5 and all((s['box'] == 65).all() and (s['j1'] - s['j0'] == 64).all() and (s['i0'] == s['i1']).all() for s in setups)
    assert sum(len(s['box']) for s in setups) == 10245 > C.BIG_WAVES and case['capacities'] == (10245, 8192)
    z = C.mesh_zbuf(case, setups=setups).reshape(5, C.STRIDE_H, C.STRIDE_W)
    assert _hit(z).all() and ((z & C.LOW) == np.arange(C.STRIDE_H, dtype=np.uint64)[None, :, None]).all()      # entry (b, f) wins the 65 pixels of row f of camera b, and no other does


def test_mesh_resolve_cells_and_the_rules_for_faces_out_of_range_and_unseen():
    case, z = C.mesh_resolve_case()
    setups = C.mesh_setups(case)
    assert case['H'] * case['W'] == 35 and [s['ok'].tolist() for s in setups] == [[True, False, True]] * 2 and all(s['swapped'][2] for s in setups)
    face, depth, pan = C.mesh_resolved(case, z, 'vertex', setups=setups)
    assert face[0, [1, 2]].tolist() == [-1, -1] and (depth[0, [1, 2]] == 0).all() and (pan[0, [1, 2]] == 0).all()          # face >= Nf: an empty cell
    assert face[:, 3].tolist() == [1, 1] and (depth[:, 3] == 0.75).all() and (pan[:, 3] == 0).all()                        # not rasterised here: id 0, face and depth kept
    assert face[0, 34] == face[1, 0] == 0 and pan[0, 34] != pan[1, 0] and pan[0, 0] != pan[1, 34]                          # one key, two cameras: each its own nearest corner
    assert np.isnan(depth[1, 17]) and face[1, 17] == 2 and pan[1, 17] in (17, 18, 19)
    fid = C.mesh_resolved(case, z, 'face', setups=setups)[2]
    assert fid[:, 3].tolist() == [102, 102] and fid[0, 1] == 0 and (C.mesh_resolved(case, z, 'none', setups=setups)[2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------- area
def test_area_cases():
    c = C.area_cases()
    assert all(p.shape[1] == C.AREA_HW == 100 and (p.size % 256 != 0 or name == 'ids') for name, p in c.items()) and c['ids'].size % 256 != 0
    flat = c['runs'].reshape(-1)
    runs = {int(flat[i]): int((flat == flat[i]).sum()) for i in np.nonzero(flat)[0]}
    assert runs == {1: 63, 2: 64, 3: 65, 4: 257, 10: 40, 11: 39}
    counts, out = C.area_ref(c['runs'], C.AREA_ID2ROW, C.AREA_S, C.AREA_MIN)
    assert counts.sum() == 63 + 64 + 65 + 257 + 40 + 39 and (counts.sum(axis=0) == [63, 64, 65 + 39, 257 + 40]).all()
    assert np.array_equal(counts, np.stack([np.bincount(C.AREA_ID2ROW[p[p > 0]], minlength=C.AREA_S) for p in c['runs']]))      # the few lines of numpy, once more
    cross = c['across_a_camera']
    assert cross.reshape(-1)[64:128].tolist() == [0] * 6 + [3] * 50 + [0] * 8 and C.AREA_ID2ROW[1] == C.AREA_ID2ROW[7] == 0      # one run in one wave, two cameras
    counts, out = C.area_ref(cross, C.AREA_ID2ROW, C.AREA_S, C.AREA_MIN)
    assert counts[:, 2].tolist() == [30, 20, 0] and counts[:, 0].tolist() == [0, 40, 28] and (out[0] == 0).all() and (out[1] == np.where(cross[1] == 1, 1, 0)).all()
    ids = set(c['ids'].reshape(-1).tolist())
    assert {0, -1, -2 ** 31, C.AREA_NTAB - 1, C.AREA_NTAB, 2 ** 31 - 1, 5, 6, 8} <= ids and C.AREA_ID2ROW[[5, 6, 8]].tolist() == [-1, C.AREA_S, -5]
    assert C.AREA_S - 1 in C.AREA_ID2ROW.tolist()
    counts, out = C.area_ref(c['ids'], C.AREA_ID2ROW, C.AREA_S, 0)
    assert set(np.unique(out).tolist()) == {0, 1, 2, 9, C.AREA_NTAB - 1}       # min_area = 0 removes the ids that are not listed, and only them
    counts, out = C.area_ref(c['exactly_min_area'], C.AREA_ID2ROW, C.AREA_S, C.AREA_MIN)
    assert counts[:, 3].tolist() == [C.AREA_MIN, C.AREA_MIN - 1] and (out[0] == c['exactly_min_area'][0]).all() and (out[1] == 0).all() and counts[0, 0] == C.AREA_MIN
