"""Stage-level parity of csrc/surface.hip (rows, count, emit, link, components), csrc/simplify.hip and csrc/components.hip (with the union-find of
csrc/union_find.h and the table of csrc/voxel_table.h): every `hip.surface_*`, `hip.simplify_*` and `hip.vcc_*` wrapper called by hand, chained as
panst3r_amd/engine/surface.py, engine/simplify.py and engine/voxels.py chain them, fed the hand-written cases of tests/topo_stage_cases.py and
compared after each stage with the restatement.  No tolerance and no cap on compared elements.  tests/test_topo_stage_checks.py asserts without a
GPU that every case holds what it was built for and which case catches which planted mistake; test_hip_surface.py, test_hip_simplify.py and
test_hip_vcc.py hold the same kernels end to end on scenes.

  quads     eleven views in one table under k = float32(1.1), +inf and 1.0, the z of an absent pixel NaN in one run and +inf in the next.
            BYTES: row, counts, base, faces, face_ids, quad (rows beyond F keep the canary).  An empty index: row all -1, counts all 0.
  islands   hand-written faces (strips of 1 .. 4097 faces in three orders, a star, interleaved components, duplicates, equal corners, unused rows,
            M = 1), corners equal to M and -1 (the RANGE bit), a planted two-cycle in parent (the LOOP bit).
            BYTES: component, size (0 away from the roots), status.  INVARIANT: parent - 0 <= parent[v] <= v and the chain from v ends at the root.
  keep      surface_keep_count / scan / surface_keep_emit after the islands of the interleaved case: the chain of engine/surface.py to its end.
  simplify  used, mask, remap, count, scan, emit on hand-written clusters, with and without dedupe, merge 0 and 1.
            BYTES: used, masked (NaN where unused, the bits of NaN, +inf and -0.0 where used), status[0 .. 4], counts, base, the kept faces, face_ids,
            quad, src_face (rows beyond F' keep the canary).  INVARIANT: face_slot - -1 / -2 exactly where the restatement says, else keys[slot] is
            the face's key (0 without dedupe); the table - the non-empty keys are the expected set, each found by the restated probe before an empty
            slot, winner[slot] = the smallest face of the key.
            Dropped: Mv at SIMPLIFY_MAX_KEYED.  `hip.simplify_remap` takes Mv <= M = the length of `cluster`, so a cluster that may name row
            2^21 - 3 has more than two million entries; the refusal of Mv above the limit sits behind the same test.
  vcc       cells; build, link, flatten, count, scan, rank, votes, voxel_vote, apply on hand-written voxels at connectivity 6, 18 and 26, merge 0 and 1.
            BYTES: cells, parent after build, root, size, points, lo, hi, component, the compacted table (rows beyond C keep the canary), best,
            out_pan, out_colors, status[0 .. 2].  INVARIANT: parent after link (-1 exactly at void rows, else as the islands); keys / rows after
            build and pair_keys / pair_cnt after votes (as the face table).  The status bits RANGE (a cell one step beyond), DUPLICATE, FULL (eight
            slots pre-filled with foreign keys) and LOOP (a planted two-cycle) with what stands beside them.
Outputs sit in canary-padded allocations; read-only operands keep their bytes; every launch sequence runs twice (once per merge setting where there
is one) with equal bytes.  Every index a kernel reads stays inside a tensor of the test; the refusals exercised are the launchers' own, made on the
host before any launch; the out-of-range corners and cells and the planted cycles exercise documented status bits, every loop bounded by M."""
import numpy as np
import pytest
import torch

import geom_stage_cases as G
import topo_stage_cases as C
import voxel_ref
from test_hip_tsdf_stages import CANARY, DEV, Padded, dev, padded_of, raw, same

pytestmark = pytest.mark.gpu
F = np.float32
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _hip():
    from panst3r_amd import hip
    hip.lib()
    return hip


def host(t):
    return t.cpu().numpy()


def keeps_canary(p, k):
    return bool((p.rows_from(k) == CANARY).all())


def check_parent(parent, root, void=None):
    """the invariant of a parent[] after a link: -1 exactly at void rows, 0 <= parent[v] <= v elsewhere, the chain from v ends at the restatement's root"""
    p = host(parent).astype(np.int64)
    v = np.arange(len(p))
    void = np.zeros(len(p), dtype=bool) if void is None else void
    assert np.array_equal(p == -1, void) and ((p[~void] >= 0) & (p[~void] <= v[~void])).all()
    r = np.where(void, v, p)
    for _ in range(len(p) + 1):
        nxt = r[r]
        if np.array_equal(nxt, r):
            break
        r = nxt
    assert np.array_equal(r[~void], np.asarray(root, dtype=np.int64)[~void])


def check_table(keys, values, expected, what):
    """the invariant of an open-addressing table after a build: the non-empty keys are exactly `expected`'s, each is found by the restated probe from
    its home slot before any empty slot, and values[slot] is the expected value"""
    k = host(keys).view(np.uint64)
    val = host(values)
    filled = np.nonzero(k != C.EMPTY)[0]
    assert sorted(int(x) for x in k[filled]) == sorted(expected), what
    for key, want in expected.items():
        slot = C.probe(k, key)
        assert slot >= 0 and int(val[slot]) == want, (what, key, slot)
    return k


# ============================================================================================================================================ quads
def quad_chain(hip, case, k):
    """rows -> count -> scan -> emit as engine/surface.py, compared after each stage -> the bytes of the outputs"""
    ref = C.v_surface(case, k)
    V, N = len(case['shapes']), case['N']
    locs, views = [], []
    for d in case['depths']:
        n = d.size
        loc = np.full((n, 3), 7.0, dtype=F)
        loc[:, 2] = d.reshape(-1)
        t = padded_of(loc, F32)
        locs.append(t)
        views.append((dev(np.zeros(n, dtype=F)), t.t.view(-1), t.t.view(-1), t.t.view(-1), dev(np.zeros(n, dtype=np.int32))))
    eye = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    table, _, total = hip.cloud_view_table(views, [eye] * V, DEV)
    dims, nwg = hip.surface_dims(case['shapes'], DEV)
    want_dims, want_nwg = C.surface_dims(case['shapes'])
    assert total == N and nwg == want_nwg
    same(dims, want_dims, np.int32, 'dims')
    index, vertex_ids = padded_of(case['index'], I64), padded_of(case['vertex_ids'], I32)
    row, counts, base = Padded((N,), I32), Padded((nwg,), I32), Padded((nwg + 1,), I32)
    cap = 2 * hip.SURFACE_WG * nwg
    faces, face_ids, quad = Padded((cap, 3), I32), Padded((cap,), I32), Padded((cap,), I64)
    kk = float(C.K[k])
    hip.surface_rows(index.t, N, row.t)
    same(row.t, ref['row'], np.int32, 'row')
    hip.surface_count(table, dims, V, nwg, row.t, kk, counts.t)
    same(counts.t, ref['counts'], np.int32, 'counts')
    hip.cloud_scan(counts.t, base.t)
    same(base.t, ref['base'], np.int32, 'base')
    hip.surface_emit(table, dims, V, nwg, row.t, kk, vertex_ids.t, base.t, faces.t, face_ids.t, quad.t)
    torch.cuda.synchronize()
    Fn = int(ref['base'][-1])
    assert 0 < Fn <= cap
    same(faces.t[:Fn], ref['faces'], np.int32, 'faces')
    same(face_ids.t[:Fn], ref['face_ids'], np.int32, 'face_ids')
    same(quad.t[:Fn], ref['quad'], np.int64, 'quad')
    assert all(keeps_canary(p, Fn) for p in (faces, face_ids, quad))                      # an empty workgroup's early return among them
    assert all(p.intact() for p in [index, vertex_ids, row, counts, base, faces, face_ids, quad] + locs)
    same(row.t, ref['row'], np.int32, 'row (an input of count and emit)')
    same(index.t, case['index'], np.int64, 'index (an input)')
    same(vertex_ids.t, case['vertex_ids'], np.int32, 'vertex_ids (an input)')
    for t, d in zip(locs, case['depths']):
        same(t.t[:, 2], d.reshape(-1), F, 'pts3d_local (an input)')
    return raw(row.t, counts.t, base.t, faces.t[:Fn], face_ids.t[:Fn], quad.t[:Fn])


@pytest.mark.parametrize('k', list(C.K))
def test_quads(k):
    hip = _hip()
    runs = [quad_chain(hip, C.quad_case(absent), k) for absent in ('nan', 'inf', 'nan')]
    assert runs[0] == runs[1] == runs[2]                                                   # whatever stands at an absent pixel; two launch sequences


def test_quads_without_a_point():
    """an empty index: every pixel absent, no workgroup counts a face"""
    hip = _hip()
    case = C.quad_case('inf', ('sq17', 'strip258'))
    N = case['N']
    row = Padded((N,), I32)
    hip.surface_rows(torch.empty(0, dtype=I64, device=DEV), N, row.t)
    assert bool((row.t == -1).all()) and row.intact()
    views = [(dev(np.zeros(d.size, dtype=F)),) + (dev(np.repeat(d.reshape(-1, 1), 3, axis=1)).view(-1),) * 3 + (dev(np.zeros(d.size, dtype=np.int32)),) for d in case['depths']]
    eye = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    table, _, _ = hip.cloud_view_table(views, [eye] * 2, DEV)
    dims, nwg = hip.surface_dims(case['shapes'], DEV)
    counts = Padded((nwg,), I32)
    hip.surface_count(table, dims, 2, nwg, row.t, float('inf'), counts.t)
    torch.cuda.synchronize()
    assert nwg == 3 and host(counts.t).tolist() == [0, 0, 0] and counts.intact()


# ========================================================================================================================================== islands
def island_chain(hip, faces, M, ref, plant=None):
    """link -> components as engine/surface.py -> (component, size, status, workspace, faces on the device)"""
    fd = padded_of(faces, I32)
    ws = hip.surface_workspace(M, DEV)
    parent, size = Padded((M,), I32), Padded((M,), I32)
    ws['parent'], ws['size'] = parent.t, size.t
    component = Padded((len(faces),), I32)
    hip.surface_link(fd.t, ws)
    if plant is None:
        check_parent(parent.t, ref['root'])
    else:                                                                                  # two rows of one component name each other
        r, w = plant
        parent.t[r], parent.t[w] = w, r
    assert bool((size.t == 0).all())
    before = raw(parent.t)
    hip.surface_components(fd.t, ws, component.t)
    torch.cuda.synchronize()
    assert parent.intact() and size.intact() and component.intact() and fd.intact() and raw(parent.t) == before
    same(fd.t, faces, np.int32, 'faces (an input)')
    return component, size, ws, fd, parent


@pytest.mark.parametrize('name', list(C.island_cases()))
def test_islands(name):
    hip = _hip()
    faces, M = C.island_cases()[name]
    ref = C.v_islands(faces, M)
    runs = []
    for _ in range(2):
        component, size, ws, _, _ = island_chain(hip, faces, M, ref)
        same(component.t, ref['component'], np.int32, 'component')
        same(size.t, ref['size'], np.int32, 'size')
        assert ws['status'].tolist() == [0]
        runs.append(raw(component.t, size.t))
    assert runs[0] == runs[1]


def test_islands_keep_after_link():
    """the chain of drop_small to its end: the faces of the first of two interleaved components survive min_faces = its size, the second (one face
    removed) does not"""
    hip = _hip()
    faces, M = C.island_cases()['interleaved']
    faces = faces[:-1]
    Fn = len(faces)
    ref = C.v_islands(faces, M)
    component, size, ws, fd, _ = island_chain(hip, faces, M, ref)
    same(component.t, ref['component'], np.int32, 'component')
    face_ids, quad = dev((np.arange(Fn) % 7).astype(np.int32)), dev((np.arange(Fn, dtype=np.int64) << 33) + 5)
    nwg = C.wgs(Fn)
    counts, base = Padded((nwg,), I32), Padded((nwg + 1,), I32)
    out_f, out_i, out_q = Padded((Fn, 3), I32), Padded((Fn,), I32), Padded((Fn,), I64)
    min_faces = int(ref['size'][0])
    hip.surface_keep_count(component.t, ws, min_faces, counts.t)
    hip.cloud_scan(counts.t, base.t)
    hip.surface_keep_emit(fd.t, face_ids, quad, component.t, ws, min_faces, base.t, out_f.t, out_i.t, out_q.t)
    torch.cuda.synchronize()
    keep = ref['component'] == 0
    assert ref['size'][1] == min_faces - 1 and int(base.t[nwg]) == keep.sum() == min_faces
    same(out_f.t[:min_faces], faces[keep], np.int32, 'kept faces')
    same(out_q.t[:min_faces], host(quad)[keep], np.int64, 'kept quad')
    assert all(keeps_canary(p, min_faces) and p.intact() for p in (out_f, out_i, out_q))


def test_islands_corners_outside_the_rows():
    """the documented RANGE bit: such a face is united with nothing (the two strips it would bridge stay two components), has component -1 and is
    counted nowhere; nothing is written through the bad corner (the canaries around parent and size)"""
    hip = _hip()
    faces, M = C.range_case()
    ref = C.v_islands(faces, M)
    for _ in range(2):
        component, size, ws, _, _ = island_chain(hip, faces, M, ref)
        same(component.t, ref['component'], np.int32, 'component')
        same(size.t, ref['size'], np.int32, 'size')
        assert ws['status'].tolist() == [hip.VCC_RANGE]
    assert sorted(set(ref['component'].tolist())) == [-1, 0, 8]


def test_islands_planted_cycle():
    """the documented LOOP bit of surface_components, its loop bounded by M = 205"""
    hip = _hip()
    faces, M, plant = C.loop_case()
    ref = C.v_islands(faces, M)
    looped = ref['component'] == plant[0]
    want_size = ref['size'].copy()
    want_size[plant[0]] = 0
    for _ in range(2):
        component, size, ws, _, _ = island_chain(hip, faces, M, ref, plant)
        same(component.t, np.where(looped, -1, ref['component']), np.int32, 'component')
        same(size.t, want_size, np.int32, 'size')
        assert ws['status'].tolist() == [hip.VCC_LOOP]
    assert 0 < looped.sum() < len(faces) and M <= 257


# ========================================================================================================================================= simplify
def simplify_chain(hip, case, dedupe, merge):
    ref = C.v_simplify(case, dedupe)
    faces, M, Mv = case['faces'], case['M'], case['Mv']
    Fn = len(faces)
    fd, cluster, quad, ids, vertices = padded_of(faces, I32), padded_of(case['cluster'], I32), padded_of(case['quad'], I64), padded_of(case['ids'], I32), padded_of(case['vertices'], F32)
    ws = hip.simplify_workspace(M, Fn, DEV)
    used, face_slot, status = padded_of(host(ws['used']), I32), Padded((Fn,), I32), padded_of(host(ws['status']), I32)
    ws['used'], ws['face_slot'], ws['status'] = used.t, face_slot.t, status.t
    masked = Padded((M, 3), F32)
    hip.simplify_used(fd.t, ws)
    same(used.t, ref['used'], np.int32, 'used')
    assert status.t.tolist()[:5] == [C.RANGE if ((faces < 0) | (faces >= M)).any() else 0, 0, 0, 0, 0]
    hip.simplify_mask(vertices.t, ws, masked.t)
    same(masked.t, ref['masked'], F, 'masked')
    assert int(status.t[1]) == ref['status'][1]
    keys = winner = None
    if dedupe:
        hip.simplify_table(ws)
        assert ws['cap'] == C.capacity(Fn) == case.get('cap', ws['cap'])
        keys, winner = padded_of(host(ws['keys']), I64), padded_of(host(ws['winner']), I32)
        ws['keys'], ws['winner'] = keys.t, winner.t
    hip.simplify_remap(fd.t, cluster.t, Mv, dedupe, ws, merge)
    assert status.t.tolist() == ref['status'].tolist() + [0, 0, 0]
    slot = host(face_slot.t)
    cand = ref['klass'] == 0
    assert np.array_equal(slot[~cand], ref['klass'][~cand]) and (slot[cand] >= 0).all()
    if dedupe:
        k = check_table(keys.t, winner.t, ref['winner'], 'the face table')
        assert np.array_equal(k[slot[cand]], ref['key'][cand])
        if 'chain' in case:                                                                # the probe that starts in the last slot went on to slot 0
            assert k[-1] != C.EMPTY and k[0] != C.EMPTY
    else:
        assert (slot[cand] == 0).all()
    nwg = C.wgs(Fn)
    counts, base = Padded((nwg,), I32), Padded((nwg + 1,), I32)
    out_f, out_i, out_q, src = Padded((Fn, 3), I32), Padded((Fn,), I32), Padded((Fn,), I64), Padded((Fn,), I32)
    table_before = raw(keys.t, winner.t) if dedupe else None
    hip.simplify_count(dedupe, ws, counts.t)
    same(counts.t, ref['counts'], np.int32, 'counts')
    hip.cloud_scan(counts.t, base.t)
    same(base.t, ref['base'], np.int32, 'base')
    hip.simplify_emit(fd.t, quad.t, cluster.t, ids.t, Mv, dedupe, ws, base.t, out_f.t, out_i.t, out_q.t, src.t)
    torch.cuda.synchronize()
    Fo = len(ref['faces'])
    same(out_f.t[:Fo], ref['faces'], np.int32, 'faces')
    same(out_i.t[:Fo], ref['face_ids'], np.int32, 'face_ids')
    same(out_q.t[:Fo], ref['quad'], np.int64, 'quad')
    same(src.t[:Fo], ref['src_face'], np.int32, 'src_face')
    assert all(keeps_canary(p, Fo) for p in (out_f, out_i, out_q, src))
    padded = [fd, cluster, quad, ids, vertices, used, face_slot, status, masked, counts, base, out_f, out_i, out_q, src] + ([keys, winner] if dedupe else [])
    assert all(p.intact() for p in padded)
    for p, a, dt in ((fd, faces, np.int32), (cluster, case['cluster'], np.int32), (quad, case['quad'], np.int64), (ids, case['ids'], np.int32), (vertices, case['vertices'], F)):
        same(p.t, a, dt, 'an input')
    assert status.t.tolist() == ref['status'].tolist() + [0, 0, 0] and (not dedupe or raw(keys.t, winner.t) == table_before)
    return raw(used.t, masked.t, status.t, counts.t, base.t, out_f.t[:Fo], out_i.t[:Fo], out_q.t[:Fo], src.t[:Fo])


@pytest.mark.parametrize('name', list(C.SIMPLIFY_CASES))
def test_simplify(name):
    hip = _hip()
    case = C.simplify_case(name)
    with_table = [simplify_chain(hip, case, True, merge) for merge in (0, 1)]
    assert with_table[0] == with_table[1]
    without = [simplify_chain(hip, case, False, merge) for merge in (0, 1)]
    assert without[0] == without[1]
    assert with_table[0][:3] == without[0][:3]                                             # used, masked and the counts do not depend on dedupe


def test_simplify_refuses_on_the_host():
    """Mv above M, Mv = 0, dedupe without a table: refused before any launch, nothing written"""
    hip = _hip()
    case = C.simplify_case('identity')
    fd, cluster = dev(case['faces']), dev(case['cluster'])
    ws = hip.simplify_workspace(case['M'], len(case['faces']), DEV)
    face_slot = Padded((len(case['faces']),), I32)
    ws['face_slot'] = face_slot.t
    for Mv, dedupe in ((case['M'] + 1, False), (0, False), (case['Mv'], True)):
        with pytest.raises(RuntimeError, match='simplify_remap'):
            hip.simplify_remap(fd, cluster, Mv, dedupe, ws)
    torch.cuda.synchronize()
    assert face_slot.untouched() and ws['status'].tolist() == [0] * hip.SIMPLIFY_STATUS_WORDS and hip.SIMPLIFY_MAX_KEYED == 2 ** 21 - 2


# ============================================================================================================================================== vcc
def vcc_expected(case, connectivity, min_voxels, ncolors):
    return C.v_vcc(case, connectivity, min_voxels, ncolors)


def vcc_workspace(hip, Mv, pair_cap):
    """hip.vcc_workspace with its outputs moved into canary-padded allocations -> (workspace, {name: Padded})"""
    ws = hip.vcc_workspace(Mv, DEV, pair_cap)
    assert ws['cap'] == C.capacity(Mv)
    pads = {}
    for name in ('keys', 'rows', 'parent', 'root', 'size', 'points', 'lo', 'hi', 'rank_of', 'status') + (('pair_keys', 'pair_cnt', 'best') if pair_cap else ()):
        if name in ('rows', 'parent', 'root', 'rank_of'):                                  # (torch.empty: nothing to keep)
            pads[name] = Padded(tuple(ws[name].shape), ws[name].dtype)
        else:
            pads[name] = padded_of(host(ws[name]), ws[name].dtype)
        ws[name] = pads[name].t
    return ws, pads


def vcc_chain(hip, case, connectivity=26, min_voxels=C.MIN_VOXELS, ncolors=7, merge=None, pair_cap=None, ref=None, plant=None, status0=0, in_table=None):
    """build -> link -> flatten -> count -> scan -> rank -> votes -> voxel_vote -> apply as engine/voxels.py, compared after each stage"""
    ref = vcc_expected(case, connectivity, min_voxels, ncolors) if ref is None else ref
    Mv = len(case['pan'])
    in_table = np.ones(Mv, dtype=bool) if in_table is None else in_table
    pair_cap = hip.vcc_pair_capacity(Mv, 26) if pair_cap is None else pair_cap
    assert pair_cap == case.get('pair_cap', C.capacity(26 * Mv))
    cells, pan, count, rgb = padded_of(case['cells'], I32), padded_of(case['pan'], I32), padded_of(case['count'], I32), padded_of(case['rgb'], F32)
    colors = padded_of(case['colors'][:ncolors], F32)
    ws, pads = vcc_workspace(hip, Mv, pair_cap)
    void = case['pan'] <= 0
    hip.vcc_build(cells.t, pan.t, ws)
    same(ws['parent'], np.where(void, -1, np.arange(Mv)), np.int32, 'parent after build')
    check_table(ws['keys'], ws['rows'], {int(k): int(v) for k, v in zip(G.vx_key(case['cells'][in_table]), np.nonzero(in_table)[0])}, 'the cell table')
    assert ws['status'].tolist() == [status0, 0, 0, 0]
    table_before = raw(ws['keys'], ws['rows'])
    hip.vcc_link(cells.t, pan.t, connectivity, ws)
    if plant is None:
        check_parent(ws['parent'], ref['root'], void)
    else:
        r, w = plant
        ws['parent'][r], ws['parent'][w] = w, r
    hip.vcc_flatten(count.t, cells.t, ws, merge)
    same(ws['root'], ref['root'], np.int32, 'root')
    same(ws['size'], ref['size'], np.int32, 'size')
    same(ws['points'], ref['points'], np.int64, 'points')
    same(ws['lo'], ref['lo'], np.int32, 'lo')
    same(ws['hi'], ref['hi'], np.int32, 'hi')
    nwg = C.wgs(Mv, G.WG)
    counts, base, component = Padded((nwg,), I32), Padded((nwg + 1,), I32), Padded((Mv,), I32)
    table = {'root': Padded((Mv,), I32), 'pan': Padded((Mv,), I32), 'size': Padded((Mv,), I32), 'points': Padded((Mv,), I64), 'cell_lo': Padded((Mv, 3), I32),
             'cell_hi': Padded((Mv, 3), I32)}
    hip.vcc_count(ws, counts.t)
    hip.cloud_scan(counts.t, base.t)
    hip.vcc_rank(pan.t, ws, base.t, component.t, {k: p.t for k, p in table.items()})
    Cn = ref['C']
    assert int(base.t[nwg]) == Cn
    same(component.t, ref['component'], np.int32, 'component')
    for k, p in table.items():
        same(p.t[:Cn], ref['table'][k], np.int64 if k == 'points' else np.int32, 'table ' + k)
        assert keeps_canary(p, Cn) and p.intact(), k
    hip.vcc_votes(cells.t, pan.t, connectivity, min_voxels, ws)
    pk = check_table(ws['pair_keys'], ws['pair_cnt'], ref['pairs'], 'the pair table')
    if 'planted' in case:                                                                  # the probe that starts in the last slot went on to slot 0
        assert pk[-1] != C.EMPTY and pk[0] != C.EMPTY and (pk != C.EMPTY).sum() == len(case['planted'])
    hip.voxel_vote({'cap': ws['pair_cap'], 'pair_keys': ws['pair_keys'], 'pair_cnt': ws['pair_cnt'], 'best': ws['best']})
    same(host(ws['best']).view(np.uint64), ref['best'], np.uint64, 'best')
    out_pan, out_colors = Padded((Mv,), I32), Padded((Mv, 3), F32)
    w1, w2 = float(F(1.0 - C.OPACITY)), float(F(C.OPACITY))
    hip.vcc_apply(pan.t, min_voxels, rgb.t, colors.t, w1, w2, ws, out_pan.t, out_colors.t)
    torch.cuda.synchronize()
    same(out_pan.t, ref['out_pan'], np.int32, 'out_pan')
    same(out_colors.t, ref['out_colors'], F, 'out_colors')
    assert ws['status'].tolist() == [status0, ref['moved'], ref['gone'], 0]
    every = list(pads.values()) + [cells, pan, count, rgb, colors, counts, base, component, out_pan, out_colors]
    assert all(p.intact() for p in every) and raw(ws['keys'], ws['rows']) == table_before
    for p, a, dt in ((cells, case['cells'], np.int32), (pan, case['pan'], np.int32), (count, case['count'], np.int32), (rgb, case['rgb'], F),
                     (colors, case['colors'][:ncolors], F)):
        same(p.t, a, dt, 'an input')
    return raw(ws['root'], ws['size'], ws['points'], ws['lo'], ws['hi'], component.t, ws['best'], out_pan.t, out_colors.t, ws['status'], *[table[k].t[:Cn] for k in table])


@pytest.mark.parametrize('name', list(C.VCC_CASES))
def test_vcc(name):
    hip = _hip()
    case = C.vcc_case(name)
    for connectivity in ((6, 18, 26) if len(case['pan']) <= 257 or name in ('line', 'runs') else (26,)):
        runs = [vcc_chain(hip, case, connectivity, merge=merge, pair_cap=case.get('pair_cap')) for merge in (0, 1)]
        assert runs[0] == runs[1], connectivity
    if 'cap' in case:                                                                      # the wrapped chain of the cell table
        ws, _ = vcc_workspace(hip, len(case['pan']), 0)
        hip.vcc_build(dev(case['cells']), dev(case['pan']), ws)
        k = host(ws['keys']).view(np.uint64)
        assert ws['cap'] == case['cap'] and k[-1] != C.EMPTY and k[0] != C.EMPTY


@pytest.mark.parametrize('ncolors', C.NCOLORS)
def test_vcc_min_voxels_and_colours(ncolors):
    """min_voxels at a component's size, one above it and 1 (nothing is small); 1, 7 and 4096 colours: a winner equal to ncolors - 1 is read, one
    equal to ncolors is not"""
    hip = _hip()
    case = C.vcc_case('speckle')
    for min_voxels in (1, C.MIN_VOXELS, C.MIN_VOXELS + 1):
        for connectivity in (6, 26):
            vcc_chain(hip, case, connectivity, min_voxels, ncolors)


def test_vcc_apply_refuses_4097_colours():
    hip = _hip()
    case = C.vcc_case('ids')
    Mv = len(case['pan'])
    ws, _ = vcc_workspace(hip, Mv, 16)
    ws['root'].fill_(-1)
    out_pan, out_colors = Padded((Mv,), I32), Padded((Mv, 3), F32)
    with pytest.raises(RuntimeError, match='vcc_apply'):
        hip.vcc_apply(dev(case['pan']), 3, dev(case['rgb']), torch.zeros(4097, 3, dtype=F32, device=DEV), 0.7, 0.3, ws, out_pan.t, out_colors.t)
    torch.cuda.synchronize()
    assert out_pan.untouched() and out_colors.untouched() and ws['status'].tolist() == [0, 0, 0, 0]


def test_vcc_cell_one_step_beyond_the_range():
    """the documented RANGE bit: the voxel is in no table and stays its own root; every other voxel is labelled as without it"""
    hip = _hip()
    case = C.beyond_case()
    inner = C.v_vcc(C.vcc_case('ids'))
    Mv = len(case['pan'])
    ref = C.v_vcc(dict(case, cells=np.concatenate([case['cells'][:-1], [[50, 50, 50]]])))  # the same voxels with the last one far away, inside the range
    for k in ('lo', 'hi'):
        ref[k][Mv - 1] = case['cells'][-1]
        ref['table']['cell_' + k][-1] = case['cells'][-1]
    assert np.array_equal(ref['root'][:-1], inner['root']) and ref['root'][-1] == Mv - 1 and ref['size'][-1] == 1
    in_table = np.arange(Mv) < Mv - 1
    runs = [vcc_chain(hip, case, 26, merge=merge, ref=ref, status0=hip.VCC_RANGE, in_table=in_table) for merge in (0, 1)]
    assert runs[0] == runs[1]


def test_vcc_two_voxels_in_one_cell():
    """the documented DUPLICATE bit: the table holds the cell once, parent is written for every row"""
    hip = _hip()
    case = C.duplicate_case()
    Mv = len(case['pan'])
    for _ in range(2):
        ws, pads = vcc_workspace(hip, Mv, 0)
        hip.vcc_build(dev(case['cells']), dev(case['pan']), ws)
        torch.cuda.synchronize()
        assert ws['status'].tolist() == [hip.VCC_DUPLICATE, 0, 0, 0] and all(p.intact() for p in pads.values())
        k = host(ws['keys']).view(np.uint64)
        assert sorted(k[k != C.EMPTY].tolist()) == sorted(set(G.vx_key(case['cells']).tolist()))
        slot = C.probe(k, int(G.vx_key(case['cells'][-1:])[0]))
        assert int(ws['rows'][slot]) in (3, Mv - 1)
        same(ws['parent'], np.where(case['pan'] <= 0, -1, np.arange(Mv)), np.int32, 'parent')


def test_vcc_full_table():
    """eight slots pre-filled with foreign keys: every probe ends after eight steps, the FULL bit, nothing claimed and no row written"""
    hip = _hip()
    cells = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5)], dtype=np.int32)
    foreign = G.vx_key(np.array([(100 + i, -7, 3) for i in range(8)])).view(np.int64)
    for _ in range(2):
        ws, pads = vcc_workspace(hip, 4, 0)
        assert ws['cap'] == 8
        ws['keys'].copy_(dev(foreign))
        hip.vcc_build(dev(cells), dev(np.ones(4, dtype=np.int32)), ws)
        torch.cuda.synchronize()
        assert ws['status'].tolist() == [hip.VCC_FULL, 0, 0, 0] and all(p.intact() for p in pads.values())
        same(ws['keys'], foreign, np.int64, 'keys')
        assert pads['rows'].untouched()
        same(ws['parent'], np.arange(4), np.int32, 'parent')


def test_vcc_planted_cycle():
    """the documented LOOP bit of vcc_flatten, its loop bounded by Mv = 257: root -1 for the voxels of that component only, which count nowhere"""
    hip = _hip()
    case, plant = C.vcc_loop_case()
    ref = C.v_vcc(case)
    r = plant[0]
    looped = ref['root'] == r
    assert 2 <= looped.sum() < (ref['root'] >= 0).sum() and len(case['pan']) <= 257
    for merge in (0, 1):
        cells, pan, count = dev(case['cells']), dev(case['pan']), dev(case['count'])
        ws, pads = vcc_workspace(hip, len(case['pan']), 0)
        hip.vcc_build(cells, pan, ws)
        hip.vcc_link(cells, pan, 26, ws)
        check_parent(ws['parent'], ref['root'], case['pan'] <= 0)
        ws['parent'][plant[0]], ws['parent'][plant[1]] = plant[1], plant[0]
        hip.vcc_flatten(count, cells, ws, merge)
        torch.cuda.synchronize()
        assert ws['status'].tolist() == [hip.VCC_LOOP, 0, 0, 0] and all(p.intact() for p in pads.values())
        same(ws['root'], np.where(looped, -1, ref['root']), np.int32, 'root')
        want = {k: ref[k].copy() for k in ('size', 'points', 'lo', 'hi')}
        want['size'][r], want['points'][r], want['lo'][r], want['hi'][r] = 0, 0, C.INT_MAX, C.INT_MIN
        for k, dt in (('size', np.int32), ('points', np.int64), ('lo', np.int32), ('hi', np.int32)):
            same(ws[k], want[k], dt, k)


def test_vcc_cells():
    """the cell of every voxel's first point: rows [0, *mv_ptr) written, the rest keep the canary; both sides of zero and the last legal cells"""
    hip = _hip()
    g = np.random.default_rng(21)
    L = C.LIM - 1
    cell = np.concatenate([C.vcc_case('blob_257')['cells'], [[L, -L, 0], [-L, L, L], [0, 0, 0], [-1, -1, -1]]]).astype(np.int64)
    M = len(cell) + 40
    points = np.concatenate([((cell + g.integers(0, 8, cell.shape) / 8) * 0.25), g.standard_normal((40, 3)) * 100]).astype(F)
    first_row = g.permutation(M).astype(np.int32)
    Mv = len(cell)
    want = voxel_ref.cells(points, 0.25)[1][first_row[:Mv]].astype(np.int32)
    assert want.max() == L and want.min() == -L and (want == -1).any()
    for _ in range(2):
        cells = Padded((M, 3), I32)
        hip.vcc_cells(dev(points), dev(first_row), dev(np.array([Mv], dtype=np.int32)), 4.0, cells.t)
        torch.cuda.synchronize()
        same(cells.t[:Mv], want, np.int32, 'cells')
        assert keeps_canary(cells, Mv) and cells.intact()
