"""Stage-level parity of the seven kernels of csrc/tsdf.hip: every `hip.tsdf_*` wrapper called by hand, chained as panst3r_amd/engine/tsdf.py chains
them (workspace from `hip.tsdf_workspace`, ranks through `hip.voxel_count` / `cloud_scan` / `voxel_rank`), fed the hand-written cases of
tests/tsdf_stage_cases.py and compared BIT FOR BIT, after each stage, with the restatement (tests/tsdf_ref.py: NodeTable, integrate_planes, extract).
No tolerance and no cap on compared elements.  tests/test_tsdf_stage_checks.py asserts without a GPU that every case holds what it was built for and
which case catches which planted mistake; tests/test_hip_tsdf.py holds the same kernels end to end on rendered scenes.

  nodes      bands 1 .. 4: one cell, shuffled rows with overlapping bands, both sides of zero, the last legal cells; one step beyond them (the RANGE
             bit, pair_slot == -1 for exactly those pairs, every other pair placed); a table at its smallest capacity whose probes wrap from the last
             slot to slot 0; 8 .. 2049 and 4913 nodes
  integrate  1 .. 2049 nodes against seven hand-written planes: s == -tau and the float32 below it, s == tau and the float32 above it, d = +0.0 and
             -0.0, zc == near, the four borders at u + 0.5 == 0 and == W, |u| beyond 2^20, a node behind the camera, views with H W == npix + 1,
             H == 0 and negative dims, offsets that are no multiple of 4 floats; 67 one-pixel views whose sum order and quotient show
  extraction cells -> scan -> vertices -> face_count -> scan -> face_emit on hand-written fields: the checkerboard (all twelve edges of a cell, mask 7,
             full lanes, F near 6 Nv), +0.0 / -0.0 / subnormal sign changes, 2^-20 against 1, lone nodes, a corner one weight short, the label
             fall-back's ties and "no voxel at all", every face-id pattern, random fields over 4913 nodes, and face-bearing nodes placed across the
             lane, wave and workgroup edges and in the last, partial lane
Outputs sit in canary-padded allocations; rows beyond F keep the canary; status stays 0; keys, first and slot_rank keep their bytes through the
read-only kernels; every launch sequence runs twice with equal bytes; the closed fields pass the topology and winding checks on the reference first,
then on the GPU result.  Every index a kernel reads stays inside a tensor of the test; the only refusals exercised are the launchers' own, made on the
host before any launch; the out-of-range cells exercise the documented status bit."""
import numpy as np
import pytest
import torch

import geom_stage_cases as G
import tsdf_ref as T
import tsdf_stage_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
PAD, CANARY = 256, 0xA5


def _hip():
    from panst3r_amd import hip
    hip.lib()
    return hip


class Padded:
    """a tensor of `shape` in the middle of a byte buffer whose PAD bytes on either side hold the canary; the tensor itself starts as canaries too"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((PAD + n + PAD,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(dtype).view(*shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all()) and bool((self.buf[PAD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())

    def rows_from(self, k):
        """the bytes of the rows [k, end) of the tensor"""
        return self.t[k:].contiguous().view(-1).view(torch.uint8)


def padded_of(a, dtype):
    p = Padded(np.asarray(a).shape, dtype)
    p.t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(dtype))
    return p


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


def same(got, ref, dtype, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.ascontiguousarray(np.asarray(ref).astype(dtype, copy=False))
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert G.same_bits(got, ref), '%s: %s' % (what, G.first_difference(got, ref))


def raw(*tensors):
    return [t.cpu().numpy().tobytes() for t in tensors]


# -------------------------------------------------------------------------------------------------------------------------------------------- nodes
def insert_and_rank(hip, cells, band):
    """insert -> count -> scan -> rank, as engine/tsdf.py -> (cells on the device, workspace, Nn)"""
    cd = dev(np.asarray(cells, dtype=np.int32))
    ws = hip.tsdf_workspace(len(cells), band, DEV)
    nwg, counts, base = hip.scan_buffers(DEV, hip.tsdf_pairs(len(cells), band))
    hip.tsdf_insert(cd, band, ws)
    hip.voxel_count(ws, counts)
    hip.cloud_scan(counts, base)
    hip.voxel_rank(ws, base)
    return cd, ws, int(base[nwg])


def node_table(hip, cells, band, tab):
    """... -> nodes, against the NodeTable `tab` -> (workspace, nodes, voxel_row: Padded)"""
    cd, ws, Nn = insert_and_rank(hip, cells, band)
    assert Nn == len(tab) and ws['cap'] == C.capacity(len(cells) * (2 * band) ** 3)
    assert int(ws['point_slot'].min()) >= 0 and ws['status'].tolist() == [0, 0, 0, 0]
    nodes, voxel_row = Padded((Nn, 3), torch.int32), Padded((Nn,), torch.int32)
    voxel_row.t.fill_(-1)
    hip.tsdf_nodes(cd, band, Nn, ws, nodes.t, voxel_row.t)
    torch.cuda.synchronize()
    assert nodes.intact() and voxel_row.intact() and ws['status'].tolist() == [0, 0, 0, 0]
    same(nodes.t, tab.nodes, np.int32, 'nodes')
    same(voxel_row.t, tab.voxel_row, np.int32, 'voxel_row')
    # the table itself: every node's key sits in the slot whose rank is the node's
    keys = ws['keys'].cpu().numpy().view(np.uint64)
    slot = np.nonzero(keys != np.uint64(2 ** 64 - 1))[0]
    assert len(slot) == Nn
    rank = ws['slot_rank'].cpu().numpy()[slot]
    assert np.array_equal(np.sort(rank), np.arange(Nn)) and np.array_equal(keys[slot], G.vx_key(tab.nodes[rank]))
    return ws, nodes, voxel_row


@pytest.mark.parametrize('band', C.BANDS)
def test_nodes(band):
    hip = _hip()
    for name, cells in C.node_cases(band).items():
        tab = C.node_table(band, name)
        first = node_table(hip, cells, band, tab)
        again = node_table(hip, cells, band, tab)                                          # two launch sequences, equal bytes
        assert raw(first[1].t, first[2].t) == raw(again[1].t, again[2].t), name
        if name == 'wrap':                                                                 # the probe that starts in the last slot went on to slot 0
            keys = first[0]['keys'].cpu().numpy().view(np.uint64)
            cap = first[0]['cap']
            chain = np.nonzero(G.home_slot(keys[keys != np.uint64(2 ** 64 - 1)], cap) == cap - 1)[0]
            assert len(chain) >= 2 and keys[cap - 1] != np.uint64(2 ** 64 - 1) and keys[0] != np.uint64(2 ** 64 - 1)


@pytest.mark.parametrize('band', C.BANDS)
def test_nodes_one_step_beyond_the_range(band):
    """the documented status bit, not an error path of the hardware: an out-of-range pair touches no slot"""
    hip = _hip()
    cells, out = C.range_case(band)
    outs = []
    for _ in range(2):
        cd = dev(cells.astype(np.int32))
        ws = hip.tsdf_workspace(len(cells), band, DEV)
        hip.tsdf_insert(cd, band, ws)
        torch.cuda.synchronize()
        assert ws['status'].tolist() == [hip.TSDF_RANGE, 0, 0, 0]
        slot = ws['point_slot'].cpu().numpy()
        assert np.array_equal(slot == -1, out) and (slot[~out] >= 0).all() and (slot[~out] < ws['cap']).all()
        keys = ws['keys'].cpu().numpy().view(np.uint64)
        assert np.array_equal(keys[slot[~out]], G.vx_key(C.pairs_of(cells, band)[~out]))   # every other pair is placed
        assert (keys != np.uint64(2 ** 64 - 1)).sum() == len(np.unique(C.pairs_of(cells, band)[~out], axis=0))
        first = ws['first'].cpu().numpy()
        inv = np.full(ws['cap'], 2 ** 31 - 1, dtype=np.int64)
        np.minimum.at(inv, slot[~out], np.nonzero(~out)[0])
        assert np.array_equal(first, inv.astype(np.int32))
        outs.append(slot == -1)
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------------------------- integrate
def integrate(hip, case):
    """hip.tsdf_integrate on the case's planes -> (sdf, weight: Padded).  The view table is the one `consist_view_table` builds for planes of npix
    pixels; dims are the case's own, which is what the kernel tests against npix."""
    V = len(case['dims'])
    planes = [dev(np.zeros(n, dtype=F)) for n in case['npix']]
    points = [dev(np.zeros(3 * n, dtype=F)) for n in case['npix']]
    views = [(c, p, p, None) for c, p in zip(planes, points)]
    eye = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    table, camd, _, _, N = hip.consist_view_table(views, [eye] * V, np.ascontiguousarray(case['cams'], dtype=F), [(1, n) for n in case['npix']], DEV)
    assert N == sum(case['npix'])
    dims = dev(np.asarray(case['dims'], dtype=np.int32).reshape(V, 2))
    depth = padded_of(np.concatenate(case['depths']).astype(F), torch.float32)
    nodes = dev(case['nodes'])
    Nn = len(case['nodes'])
    sdf, weight = Padded((Nn,), torch.float32), Padded((Nn,), torch.int32)
    hip.tsdf_integrate(nodes, float(case['vs']), case['band'], table, camd, dims, V, depth.t, sdf.t, weight.t)
    torch.cuda.synchronize()
    assert sdf.intact() and weight.intact() and depth.intact()
    same(depth.t, np.concatenate(case['depths']), F, 'depth (an input)')
    return sdf, weight


def check_integrate(hip, case, what):
    ref_sdf, ref_w = C.integrate_ref(case)
    a, b = integrate(hip, case), integrate(hip, case)
    same(a[1].t, ref_w, np.int32, 'weight of %s' % what)
    same(a[0].t, ref_sdf, F, 'sdf of %s' % what)
    assert raw(a[0].t, a[1].t) == raw(b[0].t, b[1].t), what


@pytest.mark.parametrize('Nn', C.INTEGRATE_NN)
def test_integrate(Nn):
    hip = _hip()
    for band in C.BANDS:
        check_integrate(hip, C.integrate_case(band, Nn), 'band %d, %d nodes' % (band, Nn))


def test_integrate_single_views_and_many_views():
    hip = _hip()
    case = C.integrate_case(2, 1025)
    for v in C.VIEWS:                                                                      # each view alone: D, E and G alone write zeros
        check_integrate(hip, C.one_view(case, v), 'view %s alone' % v)
    check_integrate(hip, C.many_views(), '%d views' % C.MANY_V)


# --------------------------------------------------------------------------------------------------------------------------------------- extraction
def extract(hip, case, ref):
    """cells -> scan -> vertices -> face_count -> scan -> face_emit on the case's field, compared with `ref` after each stage -> dict of arrays"""
    tab, mw = case['tab'], case['min_weight']
    ws, nodes, voxel_row = node_table(hip, case['cells'], case['band'], tab)
    Nn, Mv = len(tab), len(case['cells'])
    table_before = raw(ws['keys'], ws['first'], ws['slot_rank'])
    sdf, weight = padded_of(case['sdf'], torch.float32), padded_of(case['weight'], torch.int32)
    count, pan, colors = dev(case['count']), dev(case['pan']), dev(case['colors'])
    nwg = (Nn + C.WG - 1) // C.WG
    cell_vertex, face_mask = Padded((Nn,), torch.int32), Padded((Nn,), torch.int32)
    counts, base = Padded((nwg,), torch.int32), Padded((nwg + 1,), torch.int32)
    hip.tsdf_cells(nodes.t, ws, sdf.t, weight.t, mw, cell_vertex.t, counts.t)
    same(cell_vertex.t, ref['is_cell'], np.int32, 'the 0 / 1 flags')
    same(counts.t, ref['cell_counts'], np.int32, 'the cells per workgroup')
    hip.cloud_scan(counts.t, base.t)
    Nv = int(base.t[nwg])
    assert Nv == len(ref['vertices']) > 0
    vertices, vertex_ids, vcolors = Padded((Nv, 3), torch.float32), Padded((Nv,), torch.int32), Padded((Nv, 3), torch.float32)
    hip.tsdf_vertices(nodes.t, ws, sdf.t, weight.t, mw, voxel_row.t, count, pan, colors, float(case['vs']), base.t, cell_vertex.t, vertices.t, vertex_ids.t, vcolors.t)
    same(cell_vertex.t, ref['cell_vertex'], np.int32, 'cell_vertex')
    same(vertices.t, ref['vertices'], F, 'vertices')
    same(vertex_ids.t, ref['vertex_ids'], np.int32, 'vertex_ids')
    same(vcolors.t, ref['colors'], F, 'colors')
    fcounts, fbase = Padded((nwg,), torch.int32), Padded((nwg + 1,), torch.int32)
    hip.tsdf_face_count(nodes.t, ws, sdf.t, weight.t, mw, cell_vertex.t, face_mask.t, fcounts.t)
    same(face_mask.t, ref['face_mask'], np.int32, 'face_mask')
    same(fcounts.t, ref['face_counts'], np.int32, 'the faces per workgroup')
    hip.cloud_scan(fcounts.t, fbase.t)
    Fn = int(fbase.t[nwg])
    assert Fn == len(ref['faces']) <= 6 * Nv
    faces, face_ids, edge = Padded((6 * Nv, 3), torch.int32), Padded((6 * Nv,), torch.int32), Padded((6 * Nv,), torch.int64)
    hip.tsdf_face_emit(nodes.t, ws, sdf.t, cell_vertex.t, face_mask.t, vertex_ids.t, fbase.t, faces.t, face_ids.t, edge.t)
    torch.cuda.synchronize()
    same(faces.t[:Fn], ref['faces'].reshape(-1, 3), np.int32, 'faces')
    same(face_ids.t[:Fn], ref['face_ids'], np.int32, 'face_ids')
    same(edge.t[:Fn], ref['edge'], np.int64, 'edge')
    for p in (faces, face_ids, edge):                                                      # the rows beyond F keep their canary
        assert bool((p.rows_from(Fn) == CANARY).all())
    for name, p in (('nodes', nodes), ('voxel_row', voxel_row), ('sdf', sdf), ('weight', weight), ('cell_vertex', cell_vertex), ('face_mask', face_mask),
                    ('counts', counts), ('base', base), ('vertices', vertices), ('vertex_ids', vertex_ids), ('colors', vcolors), ('fcounts', fcounts),
                    ('fbase', fbase), ('faces', faces), ('face_ids', face_ids), ('edge', edge)):
        assert p.intact(), name
    same(sdf.t, case['sdf'], F, 'sdf (an input)')
    same(weight.t, case['weight'], np.int32, 'weight (an input)')
    same(nodes.t, tab.nodes, np.int32, 'nodes (an input)')
    same(voxel_row.t, tab.voxel_row, np.int32, 'voxel_row (an input)')
    assert ws['status'].tolist() == [0, 0, 0, 0]
    assert raw(ws['keys'], ws['first'], ws['slot_rank']) == table_before                   # the read-only kernels left the table as it was
    out = dict(vertices=vertices.t, vertex_ids=vertex_ids.t, colors=vcolors.t, cell_vertex=cell_vertex.t, face_mask=face_mask.t, faces=faces.t[:Fn],
               face_ids=face_ids.t[:Fn], edge=edge.t[:Fn])
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('name', list(C.EXTRACT))
def test_extraction(name):
    hip = _hip()
    case, ref = C.extract_case(name), C.extract_ref(name)
    if name in C.CLOSED:                                                                   # the mesh is sane on the reference first ...
        assert T.topology(ref['faces'], len(ref['vertices'])) == (True, 1, 2) and (C.winding(case, ref) > 0).all()
    a, b = extract(hip, case, ref), extract(hip, case, ref)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                                         # two launch sequences, equal bytes
    if name in C.CLOSED:                                                                   # ... then on the GPU result
        assert T.topology(a['faces'], len(a['vertices'])) == (True, 1, 2) and (C.winding(case, a) > 0).all()


# ----------------------------------------------------------------------------------------------------------------------------- launcher refusals
def test_launchers_refuse_what_the_end_to_end_module_does_not_try():
    """band 0 and 5 for nodes and integrate, Nn > Mv (2 band)^3, nviews 0 and 65536, voxel_size 0, negative and inf for vertices, min_weight 0 for
    face_count: refused on the host before any launch, nothing written"""
    hip = _hip()
    Mv, band, Nn = 2, 1, 12
    p = lambda t: t.data_ptr()
    ws = hip.tsdf_workspace(Mv, band, DEV)
    cells = dev(np.array([(0, 0, 0), (1, 0, 0)], dtype=np.int32))
    i32 = lambda *shape: Padded(shape, torch.int32)
    f32 = lambda *shape: Padded(shape, torch.float32)
    nodes, voxel_row, cell_vertex, face_mask, counts, base, weight, vertex_ids = i32(Nn, 3), i32(Nn), i32(Nn), i32(Nn), i32(1), i32(2), i32(Nn), i32(4)
    sdf, vertices, colors, depth, cams = f32(Nn), f32(4, 3), f32(4, 3), f32(8), f32(1, 16)
    dims = i32(1, 2)
    table = Padded((256,), torch.uint8)
    outputs = (nodes, voxel_row, cell_vertex, face_mask, counts, base, weight, vertex_ids, sdf, vertices, colors, depth, cams, dims, table)
    before = raw(ws['keys'], ws['first'], ws['slot_rank'], ws['point_slot'], ws['first_row'], ws['status'])

    def refused(match, what, *args):
        with pytest.raises(RuntimeError, match=match):
            hip._call(what, *args)
    node_args = lambda band, Nn: (p(cells), Mv, band, p(ws['first_row']), Nn, p(ws['keys']), ws['cap'], p(ws['slot_rank']), p(nodes.t), p(voxel_row.t), p(ws['status']))
    for b in (0, 5):
        refused('bad shape', 'pst_tsdf_nodes', *node_args(b, Nn))
    refused('bad shape', 'pst_tsdf_nodes', *node_args(1, Mv * 8 + 1))
    integ = lambda band, nviews: (p(nodes.t), Nn, 0.25, band, p(table.t), p(cams.t), p(dims.t), nviews, p(depth.t), p(sdf.t), p(weight.t))
    for b in (0, 5):
        refused('bad shape', 'pst_tsdf_integrate', *integ(b, 1))
    for nviews in (0, 65536):
        refused('bad shape', 'pst_tsdf_integrate', *integ(1, nviews))
    for vs in (0.0, -0.25, float('inf')):
        refused('voxel size', 'pst_tsdf_vertices', p(nodes.t), Nn, p(ws['keys']), ws['cap'], p(ws['slot_rank']), p(sdf.t), p(weight.t), 1, p(voxel_row.t), p(counts.t),
                p(counts.t), p(colors.t), 1, vs, p(base.t), p(cell_vertex.t), p(vertices.t), p(vertex_ids.t), p(colors.t), p(ws['status']))
    refused('min_weight', 'pst_tsdf_face_count', p(nodes.t), Nn, p(ws['keys']), ws['cap'], p(ws['slot_rank']), p(sdf.t), p(weight.t), 0, p(cell_vertex.t), p(face_mask.t),
            p(counts.t), p(ws['status']))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outputs)
    assert raw(ws['keys'], ws['first'], ws['slot_rank'], ws['point_slot'], ws['first_row'], ws['status']) == before
