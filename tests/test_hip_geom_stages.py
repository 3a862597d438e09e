"""Stage-level parity of csrc/cloud.hip and csrc/voxel.hip (with the table of csrc/voxel_table.h), and of the two other users of the workgroup rank of
csrc/wave_ops.h (the component ranks of csrc/components.hip, the face compaction of csrc/surface.hip): every wrapper of panst3r_amd.hip called by hand
and compared BIT FOR BIT with the numpy restatement of the same stage (tests/geom_stage_cases.py: scan_ref, cloud_ref.median_two_stat, cloud_ref.cloud,
voxel_ref.voxelize), at the value classes and alignments the end-to-end scenes of test_hip_cloud.py / test_hip_voxel.py never reach.  No tolerance and no
cap; where the reference is NaN the result must be NaN.  tests/test_geom_stage_checks.py asserts without a GPU that every case holds what it was built
for and that the median cases catch four planted mistakes.

  scan     the 64-lane and 1024-count edges, zeros at a round's last and first index, a total just below 2^31, exactly n + 1 words written, n <= 0 refused
  median   ties, negatives only, -0.0 / +0.0, subnormals, infinities, an overflowing sum, NaNs of both signs, middle statistics that share 3, 2, 1 or
           no leading key bytes; on every axis; S around the 8-segment block; one and two point slices; ids that take part in nothing; M below the
           buffer length; M = 0; two calls, identical bytes
  cloud    views of 1 .. 2049 points in one table, conf at 0 / 4 / 8 / 12 bytes past a 16-byte boundary (both paths of keep_mask), thresholds equal to
           a value, +inf and 0.0 (with -0.0 and the smallest negative subnormal), NaN confidences, a workgroup that keeps all 1024 points next to one
           that keeps none, 1 / 7 / 4096 colours and 4097 refused, ids outside the table, rotated cameras, subnormal and infinite coordinates
  voxel    insert, count, scan, rank, accumulate, vote, emit by hand, with and without the wave-level merge: cell faces on both sides of zero and the
           last cells in range, a table at load factor 1 / 2 whose probe chains wrap from the last slot to slot 0 (cells and pairs), runs across the
           wave, workgroup and rank-group edges, vote ties, void-only voxels, offset sums beyond 2^32, colour clamps and NaN
  vcc rank vcc_count, scan, vcc_rank on a hand-written root[]: 1 .. 2049 rows around the 64-lane, 256-row wave and 1024-row workgroup edges; no root, all
           roots, roots in lane 63 / lane 0 alone, alternating, random, a full workgroup next to an empty one; rows >= C of the table keep a canary
  keep     surface_keep_count, scan, surface_keep_emit on a hand-written component[] / size[]: 1 .. 513 faces around the 64 and 256 edges, the same
           patterns, component -1, sizes 0, min_faces - 1, min_faces; outputs beyond `kept` keep a canary

Every index a kernel reads stays inside a tensor of the test; the only refusals exercised are the launchers' own, made on the host before any launch."""
import functools

import numpy as np
import pytest
import torch

import geom_stage_cases as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
CANARY_I, CANARY_F = -12345, -777.0


def _hip():
    from panst3r_amd import hip
    hip.lib()
    return hip


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


def _filled(shape, dtype):
    return torch.full(shape, CANARY_F if dtype == torch.float32 else CANARY_I, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t == (CANARY_F if t.dtype == torch.float32 else CANARY_I)).all())


def _assert_same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    assert G.same_bits(got.reshape(ref.shape), ref), '%s: %s' % (what, G.first_difference(got.reshape(ref.shape), ref))


# ---------------------------------------------------------------------------------------------------------------------------------------------- scan
def _scan(hip, counts):
    n = len(counts)
    buf = _filled((n + 1 + 64,), torch.int32)
    hip.cloud_scan(_dev(counts), buf[:n + 1])
    torch.cuda.synchronize()
    assert _untouched(buf[n + 1:]), 'cloud_scan wrote past base[n]'
    return buf[:n + 1]


@pytest.mark.parametrize('n', G.SCAN_N)
def test_scan(n):
    hip = _hip()
    for seed in (0, 1):
        counts = G.scan_counts(n, seed)
        _assert_same(_scan(hip, counts), G.scan_ref(counts), 'base (n = %d)' % n)


def test_scan_total_just_below_2_31():
    counts = G.scan_big()
    _assert_same(_scan(_hip(), counts), G.scan_ref(counts), 'base')


def test_scan_refuses_nothing_to_scan():
    hip = _hip()
    counts, base = _dev(np.ones(4, np.int32)), _filled((8,), torch.int32)
    with pytest.raises(RuntimeError, match='cloud_scan'):
        hip.cloud_scan(counts[:0], base[:1])
    for n in (0, -1):
        with pytest.raises(RuntimeError, match='cloud_scan'):
            hip._call('pst_cloud_scan', counts.data_ptr(), n, base.data_ptr())
    torch.cuda.synchronize()
    assert _untouched(base)


# -------------------------------------------------------------------------------------------------------------------------------------------- median
def _median(hip, pts, pan, M, id2row, S):
    """-> (count [S], median [S, 3]) of the rows [0, M) of the device tensors pts / pan"""
    count, median = _filled((S,), torch.int32), _filled((S, 3), torch.float32)
    hip.cloud_segment_median(pts, pan, _dev(np.asarray([M], np.int32)), id2row, S, count, median)
    torch.cuda.synchronize()
    return count.cpu().numpy(), median.cpu().numpy()


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_median_every_case_on_every_axis(axis):
    """one segment; the case on `axis`, the next two cases (cut or repeated to its length) on the other axes: a swapped axis shows"""
    hip = _hip()
    cases = G.median_cases()
    names = list(cases)
    id2row = _dev(np.asarray([-1, 0], np.int32))
    for i, name in enumerate(names):
        n = len(cases[name])
        seg = np.empty((n, 3), F)
        for k in range(3):
            seg[:, (axis + k) % 3] = np.resize(cases[names[(i + k) % len(names)]], n)
        want = np.asarray([G.median_ref(seg[:, a]) for a in range(3)], F)
        count, med = _median(hip, _dev(seg), _dev(np.ones(n, np.int32)), n, id2row, 1)
        assert count[0] == n, name
        _assert_same(med[0], want, 'median of %s on axis %d' % (name, axis))


@pytest.mark.parametrize('M', [32768, 32769])
@pytest.mark.parametrize('S', [1, 8, 9, 17])
def test_median_segments(S, M):
    hip = _hip()
    pts, pan, id2row, want_count, want_med = G.median_segments(S, M)
    d_pts, d_pan, d_tab = _dev(pts), _dev(pan), _dev(id2row)
    count, med = _median(hip, d_pts, d_pan, M, d_tab, S)
    _assert_same(count, want_count, 'count')
    _assert_same(med, want_med, 'median')
    count2, med2 = _median(hip, d_pts, d_pan, M, d_tab, S)
    assert count2.tobytes() == count.tobytes() and med2.tobytes() == med.tobytes(), 'two calls differ'


@pytest.mark.parametrize('M', [32768, 32769])
def test_median_ignores_the_rows_past_m(M):
    """buffers of 2 M rows whose tail holds live ids and large values: only the rows [0, *m_ptr) count"""
    hip = _hip()
    S = 9
    pts, pan, id2row, want_count, want_med = G.median_segments(S, M)
    g = np.random.Generator(np.random.PCG64(5))
    live = np.nonzero(id2row >= 0)[0].astype(np.int32)
    tail_pts = (g.standard_normal((M, 3)) * 1e9).astype(F)
    tail_pts[::7] = np.nan
    pts2, pan2 = np.concatenate([pts, tail_pts]), np.concatenate([pan, live[g.integers(0, len(live), M)]])
    count, med = _median(hip, _dev(pts2), _dev(pan2), M, _dev(id2row), S)
    _assert_same(count, want_count, 'count')
    _assert_same(med, want_med, 'median')


def test_median_of_no_rows():
    hip = _hip()
    S = 9
    pts, pan, id2row, _, _ = G.median_segments(S, 32768)
    count, med = _median(hip, _dev(pts), _dev(pan), 0, _dev(id2row), S)
    assert (count == 0).all() and np.isnan(med).all()


# --------------------------------------------------------------------------------------------------------------------------------------------- cloud
@functools.lru_cache(maxsize=None)
def _cloud_case(thr, ncolors):
    case = G.cloud_case(thr, ncolors)
    return case, G.cloud_reference(case)


def _cloud_inputs(hip, case, shift):
    """the device table of the case's views, conf of view v starting 4 ((v + shift) mod 4) bytes past a 16-byte boundary of one allocation"""
    off, total = G.cloud_offsets(shift)
    conf_flat = torch.full((total + 4,), float('nan'), dtype=torch.float32, device=DEV)
    assert conf_flat.data_ptr() % 16 == 0
    flat = lambda key, dtype=None: _dev(np.concatenate([np.asarray(x[key]).reshape(-1) for x in case['x_out']]), dtype)
    pts, loc = flat('pts3d'), flat('pts3d_local')
    img = _dev(np.concatenate([i.reshape(-1) for i in case['imgs']]))
    pan = _dev(np.concatenate([p.reshape(-1) for p in case['pan']]), torch.int32)
    views, at = [], 0
    for v, (n, o) in enumerate(zip(G.CLOUD_NPIX, off)):
        c = conf_flat[o:o + n]
        c.copy_(_dev(case['x_out'][v]['conf'].reshape(-1)))
        assert c.data_ptr() % 16 == 4 * ((v + shift) % 4)
        views.append((c, pts[3 * at:3 * (at + n)], loc[3 * at:3 * (at + n)], img[3 * at:3 * (at + n)], pan[at:at + n]))
        at += n
    table, nwg, N = hip.cloud_view_table(views, [c[:3, :4] for c in case['cams']], DEV)
    assert N == at and nwg == sum((n + G.WG - 1) // G.WG for n in G.CLOUD_NPIX)
    return table, nwg, N, (conf_flat, pts, loc, img, pan, views)


def _cloud_outputs(N, pad=64):
    f3 = lambda: _filled((N + pad, 3), torch.float32)
    return {'points': f3(), 'points_local': f3(), 'rgb': f3(), 'pan': _filled((N + pad,), torch.int32), 'colors': f3(), 'index': _filled((N + pad,), torch.int64)}


def _compact(hip, case, table, nwg, N, base, colors, out):
    w1, w2 = float(F(1.0 - case['opacity'])), float(F(case['opacity']))
    hip.cloud_compact(table, len(G.CLOUD_NPIX), nwg, case['thr'], base, colors, w1, w2, out['points'][:N], out['points_local'][:N], out['rgb'][:N], out['pan'][:N],
                      out['colors'][:N], out['index'][:N])
    torch.cuda.synchronize()


@pytest.mark.parametrize('ncolors', G.CLOUD_NCOLORS)
@pytest.mark.parametrize('thr', list(G.CLOUD_THRESHOLDS))
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_cloud_count_compact(shift, thr, ncolors):
    hip = _hip()
    case, ref = _cloud_case(thr, ncolors)
    table, nwg, N, alive = _cloud_inputs(hip, case, shift)
    counts, base = _filled((nwg,), torch.int32), _filled((nwg + 1,), torch.int32)
    hip.cloud_count(table, len(G.CLOUD_NPIX), nwg, case['thr'], counts)
    hip.cloud_scan(counts, base)
    want = G.cloud_wg_counts(case)
    _assert_same(counts, want, 'counts')
    _assert_same(base, G.scan_ref(want), 'base')
    out = _cloud_outputs(N)
    _compact(hip, case, table, nwg, N, base, _dev(case['colors']), out)
    M = int(want.sum())
    assert M == len(ref['pan'])
    for k in G.CLOUD_FIELDS:
        _assert_same(out[k][:M], ref[k], k)
        assert _untouched(out[k][M:]), k + ': rows past M were written'
    del alive


def test_cloud_compact_refuses_4097_colours():
    hip = _hip()
    case, ref = _cloud_case('present', 7)
    table, nwg, N, alive = _cloud_inputs(hip, case, 0)
    base = _dev(G.scan_ref(G.cloud_wg_counts(case)))
    out = _cloud_outputs(N)
    colors = torch.zeros(hip.CLOUD_MAX_COLORS + 1, 3, dtype=torch.float32, device=DEV)
    assert hip.CLOUD_MAX_COLORS == 4096
    with pytest.raises(RuntimeError, match='colour table of 4097 rows'):
        _compact(hip, case, table, nwg, N, base, colors, out)
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in out.values())
    del alive


# --------------------------------------------------------------------------------------------------------------------------------------------- voxel
def voxelize_by_hand(hip, case, merge):
    """the steps of engine.voxels.voxelize_cloud, one wrapper each: insert, count, scan, rank, accumulate, vote, emit -> (fields as numpy, status [2])"""
    points, rgb, pan, index = _dev(case['points']), _dev(case['rgb']), _dev(case['pan'], torch.int32), _dev(case['index'], torch.int64)
    M = pan.numel()
    ids = case['segment_ids']
    ntab = max(ids + [0]) + 1
    row = np.full(ntab, -1, dtype=np.int32)
    row[ids] = np.arange(len(ids), dtype=np.int32)
    id2row, ctab = _dev(row), _dev(case['colors'])
    vs = float(case['voxel_size'])
    inv = float(F(1.0 / vs))
    w1, w2 = float(F(1.0 - case['opacity'])), float(F(case['opacity']))
    ws = hip.voxel_workspace(M, DEV)
    assert ws['cap'] == hip.voxel_capacity(M) and ws['cap'] >= 2 * M
    nwg = (M + hip.CLOUD_WG - 1) // hip.CLOUD_WG
    counts, base = _filled((nwg,), torch.int32), _filled((nwg + 1,), torch.int32)
    point_voxel = _filled((M,), torch.int32)
    f3 = lambda: _filled((M, 3), torch.float32)
    out = {'points': f3(), 'rgb': f3(), 'colors': f3(), 'pan': _filled((M,), torch.int32), 'votes': _filled((M,), torch.int32), 'first_index': _filled((M,), torch.int64)}
    hip.voxel_insert(points, inv, ws, merge=merge)
    hip.voxel_count(ws, counts)
    hip.cloud_scan(counts, base)
    hip.voxel_rank(ws, base)
    hip.voxel_accumulate(points, rgb, pan, inv, id2row, ws, point_voxel, merge=merge)
    hip.voxel_vote(ws)
    mv = base[nwg:]
    hip.voxel_emit(points, index, mv, inv, vs, ws, ctab, w1, w2, out['points'], out['rgb'], out['pan'], out['colors'], out['votes'], out['first_index'])
    torch.cuda.synchronize()
    Mv = int(mv.cpu()[0])
    assert 0 <= Mv <= M
    for k, t in out.items():
        assert _untouched(t[Mv:]), k + ': rows past Mv were written'
    res = {k: t[:Mv].cpu().numpy() for k, t in out.items()}
    res['count'], res['point_voxel'] = ws['cnt'][:Mv].cpu().numpy(), point_voxel.cpu().numpy()
    return res, ws['status'].cpu().numpy()


@pytest.mark.parametrize('merge', [0, 1])
@pytest.mark.parametrize('name', list(G.voxel_cases()))
def test_voxel_stages(name, merge):
    hip = _hip()
    case, ref = G.voxel_cases()[name], G.voxel_reference(name)
    if name == 'load_half':
        assert hip.voxel_capacity(len(case['pan'])) == case['cap'] == 2 * len(case['pan'])
    got, status = voxelize_by_hand(hip, case, merge)
    assert status[0] == 0, 'a table ran full'
    assert status[1] == ref['dropped'] == case['dropped']
    for k in G.VOXEL_FIELDS:
        _assert_same(got[k], ref[k], '%s of %s (merge=%d)' % (k, name, merge))


# ------------------------------------------------------------------------------------------------------- the workgroup rank: components and surface keep
@pytest.mark.parametrize('Mv', G.VCC_MV)
def test_vcc_count_and_rank(Mv):
    hip = _hip()
    for pattern in G.RANK_PATTERNS:
        c = G.vcc_rank_case(Mv, pattern)
        w = c['want']
        ws = hip.vcc_workspace(Mv, DEV)
        for k in ('root', 'size', 'points', 'lo', 'hi'):
            ws[k].copy_(_dev(c[k]))
        ws['rank_of'].fill_(CANARY_I)
        nwg = (Mv + hip.CLOUD_WG - 1) // hip.CLOUD_WG
        counts, base, component = _filled((nwg,), torch.int32), _filled((nwg + 1,), torch.int32), _filled((Mv,), torch.int32)
        table = {k: _filled((Mv, 3) if k.startswith('cell') else (Mv,), torch.int64 if k == 'points' else torch.int32) for k in w['table']}
        hip.vcc_count(ws, counts)
        hip.cloud_scan(counts, base)
        hip.vcc_rank(_dev(c['pan']), ws, base, component, table)
        torch.cuda.synchronize()
        what = ' (Mv = %d, %s)' % (Mv, pattern)
        _assert_same(counts, w['counts'], 'counts' + what)
        _assert_same(base, w['base'], 'base' + what)
        rank_of = ws['rank_of'].cpu().numpy()
        _assert_same(rank_of[w['roots']], w['rank_of'][w['roots']], 'rank_of at the roots' + what)
        assert (rank_of[~c['is_root']] == CANARY_I).all(), 'rank_of was written at a row that is no root' + what
        _assert_same(component, w['component'], 'component' + what)
        for k, t in table.items():
            _assert_same(t[:w['C']], w['table'][k], k + what)
            assert _untouched(t[w['C']:]), k + ': rows past C were written' + what
        assert int(ws['status'][0]) == 0


@pytest.mark.parametrize('F_', G.KEEP_F)
def test_surface_keep_count_and_emit(F_):
    hip = _hip()
    for pattern in G.RANK_PATTERNS:
        c = G.keep_case(F_, pattern)
        w = c['want']
        ws = hip.surface_workspace(c['M'], DEV)
        ws['size'].copy_(_dev(c['size']))
        ws['parent'].fill_(CANARY_I)                                         # not read by the two kernels
        component = _dev(c['component'])
        nwg = (F_ + hip.SURFACE_WG - 1) // hip.SURFACE_WG
        counts, base = _filled((nwg,), torch.int32), _filled((nwg + 1,), torch.int32)
        out = {'faces': _filled((F_, 3), torch.int32), 'face_ids': _filled((F_,), torch.int32), 'quad': _filled((F_,), torch.int64)}
        hip.surface_keep_count(component, ws, c['min_faces'], counts)
        hip.cloud_scan(counts, base)
        hip.surface_keep_emit(_dev(c['faces']), _dev(c['face_ids']), _dev(c['quad']), component, ws, c['min_faces'], base, out['faces'], out['face_ids'], out['quad'])
        torch.cuda.synchronize()
        what = ' (F = %d, %s)' % (F_, pattern)
        _assert_same(counts, w['counts'], 'counts' + what)
        _assert_same(base, w['base'], 'base' + what)
        for k, t in out.items():
            _assert_same(t[:w['kept']], w[k], k + what)
            assert _untouched(t[w['kept']:]), k + ': rows past kept were written' + what
        assert int(ws['status'][0]) == 0 and _untouched(ws['parent'])
