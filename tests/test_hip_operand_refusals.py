"""The operand checks of the wrappers of panst3r_amd.hip, engine and model path, one wrapper per section: a valid call on a handful of elements reaches the
library exactly once with the operands' own addresses; the same call with ONE operand replaced - a buffer one element short, a view of the right shape
whose column stride is 2, a wrong dtype, a CPU tensor, and for a 2-D operand one row fewer and one column narrower - raises RuntimeError before anything
reaches the library.  The valid call of every row-view operand of the model path uses a padded view (leading dimension > columns).  `hip._call` is replaced by a recorder, so
NOTHING RUNS ON THE DEVICE: a bad operand can only fail on the host.  Workspace entries are operands like any other.

Three kinds of operand have no "one element short" (nor a row fewer, nor a column narrower):
  * an operand whose own length or shape is a size of the call (qubo_argmax's sel, voxel_accumulate's id2row, pointmap_activate's raw; x of l2norm_rows,
    ids / tok / pos of token_embed): a smaller one is another valid call, unless a second operand is sized by it exactly - then that one is refused,
    and the case is run (rope2d_'s x against pos, layernorm's gamma against beta);
  * an operand read at indices that only the device knows and whose length the entry point does not take (pp_finalize's seg_id, read at best_q;
    retrieval_scores' word lists, read up to the last offset);
  * depth_table's pred, whose contract is its storage and not its shape: it also has no "non-contiguous", row fewer or column narrower (a stride is what it is given for).
They are named in each case with `free=`; the other three substitutions are made for them all the same.  An [n, k] operand whose row count is a size of
the call (points, faces, colour tables) is refused when it is flat or a column narrower, but one row fewer is another valid call: `own=`."""
import pytest
import torch

from panst3r_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64, I32, I64, U8, F16 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.float16
WRONG = {F32: F64, F64: F32, I32: I64, I64: I32, U8: I32, F16: torch.int16}


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def pv(dtype, rows, cols):
    """a padded row view: [rows, cols] at a leading dimension of cols + 4, the storage ending with the last row's padding"""
    return z(dtype, rows, cols + 4)[:, :cols]


def substitutes(t):
    """(kind, tensor) for every way an operand can be wrong"""
    n = t.numel()
    if n > 0:
        yield 'short', torch.zeros(n - 1, dtype=t.dtype, device=t.device)
    if n > 1:
        dense, s = [], 1
        for d in reversed(t.shape):
            dense.insert(0, s)
            s *= d
        v = torch.zeros(2 * n, dtype=t.dtype, device=t.device).as_strided(tuple(t.shape), [2 * s for s in dense])
        assert v.shape == t.shape and not v.is_contiguous()
        yield 'strided', v
    if t.dim() == 2:
        yield 'rows', t[:-1]
        yield 'cols', t[:, :-1]
    yield 'dtype', t.to(WRONG[t.dtype])
    yield 'cpu', t.cpu()


@pytest.fixture
def recorder(monkeypatch):
    rec = []
    monkeypatch.setattr(hip, '_call', lambda what, *args: rec.append((what, args)))
    return rec


def hold(recorder, call, ops, free=(), loose=(), own=()):
    """call(ops) with the operands ops = {name: tensor}: valid once, then refused for every substitute of every operand (`free`: no 'short', 'rows',
    'cols'; `own`: an [n, k] operand whose n sizes the call, no 'rows'; `loose`: no 'strided')"""
    call(ops)
    assert len(recorder) == 1, recorder
    sent = set(a for a in recorder[0][1] if isinstance(a, int))
    assert all(t.data_ptr() in sent for t in ops.values()), [k for k, t in ops.items() if t.data_ptr() not in sent]
    tried = 0
    for name, t in ops.items():
        for kind, bad in substitutes(t):
            if (kind in ('short', 'rows', 'cols') and name in free) or (kind == 'strided' and name in loose) or (kind == 'rows' and name in own):
                continue
            del recorder[:]
            with pytest.raises(RuntimeError):
                call(dict(ops, **{name: bad}))
                pytest.fail('%s with a %s %s was accepted' % (recorder[0][0] if recorder else 'the call', kind, name))
            assert not recorder, (name, kind)
            tried += 1
    assert tried >= 3 * len(ops)


def ws_ops(ws, *names):
    return {'ws.' + k: ws[k] for k in names}


def ws_of(ops, **rest):
    return dict({k[3:]: t for k, t in ops.items() if k.startswith('ws.')}, **rest)


def test_pp_finalize(recorder):
    n, Q = 6, 3
    ops = dict(best_q=z(I32, n), best_m=z(F32, n), seg_id=z(I32, Q), pan=z(I32, n), conf=z(F32, n))
    hold(recorder, lambda o: hip.pp_finalize(o['best_q'], o['best_m'], o['seg_id'], n, 0.5, 0.0, o['pan'], o['conf']), ops, free=('seg_id',))


def test_pointmap_activate(recorder):
    ops = dict(raw=z(F32, 5, 7), pts3d=z(F32, 5, 3), pts3d_local=z(F32, 5, 3), conf=z(F32, 5))
    hold(recorder, lambda o: hip.pointmap_activate(o['raw'], o['pts3d'], o['pts3d_local'], o['conf']), ops, free=('raw',))


def test_qubo_argmax(recorder):
    P = 6
    ops = dict(probs=z(F32, 2, P), sel=z(I32, 2), conf=z(F32, P), inst=z(I32, P))
    hold(recorder, lambda o: hip.qubo_argmax(o['probs'], o['sel'], P, o['conf'], o['inst']), ops, free=('sel',))


def test_retrieval_scores(recorder):
    ops = dict(q_off=z(I32, 3), q_word=z(I32, 3), q_bits=z(I32, 3, 1), db_off=z(I32, 2), db_word=z(I32, 2), db_bits=z(I32, 2, 1), S=z(F32, 2, 1))
    hold(recorder, lambda o: hip.retrieval_scores(o['q_off'], o['q_word'], o['q_bits'], o['db_off'], o['db_word'], o['db_bits'], 32, 3.0, 0.0, o['S'], 2), ops,
         free=('q_word', 'db_word'), own=('q_bits', 'db_bits'))


def test_cloud_compact(recorder):
    n = 5
    ops = dict(table=z(U8, hip._VIEW_BYTES), base=z(I32, 2), colors=z(F32, 2, 3), points=z(F32, n, 3), points_local=z(F32, n, 3), rgb=z(F32, n, 3), pan=z(I32, n),
               colors_out=z(F32, n, 3), index=z(I64, n))
    hold(recorder, lambda o: hip.cloud_compact(o['table'], 1, 1, 1.5, o['base'], o['colors'], 0.5, 0.5, o['points'], o['points_local'], o['rgb'], o['pan'],
                                               o['colors_out'], o['index']), ops, own=('colors',))


def test_voxel_accumulate(recorder):
    M = 5
    ws = hip.voxel_workspace(M, DEV)
    ops = dict(points=z(F32, M, 3), rgb=z(F32, M, 3), pan=z(I32, M), id2row=z(I32, 4), point_voxel=z(I32, M),
               **ws_ops(ws, 'point_slot', 'slot_rank', 'cnt', 'sums', 'pair_keys', 'pair_cnt', 'status'))
    hold(recorder, lambda o: hip.voxel_accumulate(o['points'], o['rgb'], o['pan'], 10.0, o['id2row'], ws_of(o, cap=ws['cap']), o['point_voxel']), ops,
         free=('id2row',))


def test_vcc_rank(recorder):
    Mv = 3
    ws = hip.vcc_workspace(Mv, DEV)
    tab = dict(root=z(I32, Mv), pan=z(I32, Mv), size=z(I32, Mv), points=z(I64, Mv), cell_lo=z(I32, Mv, 3), cell_hi=z(I32, Mv, 3))
    ops = dict(pan=z(I32, Mv), base=z(I32, 2), component=z(I32, Mv), **ws_ops(ws, 'root', 'size', 'points', 'lo', 'hi', 'rank_of'),
               **{'t.' + k: t for k, t in tab.items()})
    hold(recorder, lambda o: hip.vcc_rank(o['pan'], ws_of(o), o['base'], o['component'], {k[2:]: t for k, t in o.items() if k.startswith('t.')}), ops)


def test_render_resolve(recorder):
    n, M = 6, 5
    ops = dict(zbuf=z(I64, 1, 2, 3), rgb=z(F32, M, 3), colors=z(F32, M, 3), pan=z(I32, M), index=z(I64, n), depth=z(F32, n), out_pan=z(I32, n),
               out_rgb=z(F32, n, 3), out_colors=z(F32, n, 3))
    hold(recorder, lambda o: hip.render_resolve(*(o[k] for k in ('zbuf', 'rgb', 'colors', 'pan', 'index', 'depth', 'out_pan', 'out_rgb', 'out_colors'))), ops)


def test_consist_count(recorder):
    N = 6
    ops = dict(table=z(U8, hip._VIEW_BYTES), cams=z(F32, 1, hip.RENDER_CAM_FLOATS), dims=z(I32, 1, 2), depth=z(F32, N), agree=z(I32, N), violate=z(I32, N),
               same_label=z(I32, N))
    hold(recorder, lambda o: hip.consist_count(o['table'], o['cams'], o['dims'], 1, 1, 0.01, False, o['depth'], o['agree'], o['violate'], o['same_label']), ops)


def test_tsdf_vertices(recorder):
    Nn, Mv, Nv = 4, 3, 2
    ws = hip.tsdf_workspace(Mv, 1, DEV)
    ops = dict(nodes=z(I32, Nn, 3), sdf=z(F32, Nn), weight=z(I32, Nn), voxel_row=z(I32, Nn), vox_count=z(I32, Mv), vox_pan=z(I32, Mv), vox_colors=z(F32, Mv, 3),
               base=z(I32, 2), cell_vertex=z(I32, Nn), vertices=z(F32, Nv, 3), vertex_ids=z(I32, Nv), colors=z(F32, Nv, 3), **ws_ops(ws, 'keys', 'slot_rank', 'status'))
    hold(recorder, lambda o: hip.tsdf_vertices(o['nodes'], ws_of(o, cap=ws['cap']), o['sdf'], o['weight'], 1, o['voxel_row'], o['vox_count'], o['vox_pan'],
                                               o['vox_colors'], 0.1, o['base'], o['cell_vertex'], o['vertices'], o['vertex_ids'], o['colors']), ops)


def test_mesh_resolve(recorder):
    n = 6
    ops = dict(zbuf=z(I64, 1, 2, 3), vertices=z(F32, 4, 3), faces=z(I32, 2, 3), cams=z(F32, 1, hip.MESH_CAM_FLOATS), vertex_ids=z(I32, 4), face=z(I64, n),
               depth=z(F32, n), pan=z(I32, n))
    hold(recorder, lambda o: hip.mesh_resolve(o['zbuf'], o['vertices'], o['faces'], o['cams'], 0.05, o['vertex_ids'], None, o['face'], o['depth'], o['pan']), ops, own=('faces',))


def test_pq_match(recorder):
    S, P, G = 1, 2, 2
    ops = dict(counts=z(I32, S, P + 1, G + 1), cat_p=z(I32, P), cat_g=z(I32, G), pred_area=z(I32, S, P), gt_area=z(I32, S, G), match=z(I32, S, G),
               iou=z(F64, S, G), pred_state=z(I32, S, P))
    hold(recorder, lambda o: hip.pq_match(*(o[k] for k in ('counts', 'cat_p', 'cat_g', 'pred_area', 'gt_area', 'match', 'iou', 'pred_state'))), ops)


def test_surface_keep_emit(recorder):
    F, M = 2, 4
    ws = hip.surface_workspace(M, DEV)
    ops = dict(faces=z(I32, F, 3), face_ids=z(I32, F), quad=z(I64, F), component=z(I32, F), base=z(I32, 2), out_faces=z(I32, F, 3), out_face_ids=z(I32, F),
               out_quad=z(I64, F), **ws_ops(ws, 'size'))
    hold(recorder, lambda o: hip.surface_keep_emit(o['faces'], o['face_ids'], o['quad'], o['component'], ws_of(o, parent=ws['parent']), 1, o['base'],
                                                   o['out_faces'], o['out_face_ids'], o['out_quad']), ops)


def test_nn_query(recorder):
    Nq, M = 3, 5
    ws = hip.nn_workspace(M, DEV)
    ws['start'] = z(I32, ws['cap'])
    ops = dict(queries=z(F32, Nq, 3), targets=z(F32, M, 3), d2=z(F32, Nq), row=z(I32, Nq), **ws_ops(ws, 'keys', 'start', 'cell_count', 'rows', 'status'))
    hold(recorder, lambda o: hip.nn_query(o['queries'], o['targets'], 2.0, 0.25, ws_of(o, cap=ws['cap']), 64, o['d2'], o['row']), ops)


def test_meshdist_query(recorder):
    Nq, P = 3, 7
    ws = hip.meshdist_workspace(P, DEV)
    ws['start'] = z(I32, ws['cap'])
    ops = dict(queries=z(F32, Nq, 3), vertices=z(F32, 4, 3), faces=z(I32, 2, 3), d2=z(F32, Nq), face=z(I32, Nq), closest=z(F32, Nq, 3), status=z(I32, 4),
               **ws_ops(ws, 'keys', 'start', 'cell_count', 'rows'))
    hold(recorder, lambda o: hip.meshdist_query(o['queries'], o['vertices'], o['faces'], 2.0, 0.25, ws_of(o, cap=ws['cap'], P=P), 64, o['d2'], o['face'],
                                                o['closest'], o['status']), ops, own=('vertices', 'faces'))


def test_depth_errors_and_its_table(recorder):
    H, W = 2, 3
    planes = dict(pred=z(F32, H, W), gt=z(F32, H, W), conf=z(F32, H, W))
    table = hip.depth_table([(planes['pred'], 1, planes['gt'], planes['conf'])], [0], DEV)
    assert table.host[0, :5].tolist() == [planes['pred'].data_ptr(), 1, planes['gt'].data_ptr(), planes['conf'].data_ptr(), H * W]
    for name, t in planes.items():                          # the planes whose addresses the table stores
        for kind, bad in substitutes(t):
            if name == 'pred' and kind in ('strided', 'rows', 'cols'):          # views of the same storage: still its contract
                continue
            p = dict(planes, **{name: bad})
            with pytest.raises(RuntimeError, match='depth_table: '):
                hip.depth_table([(p['pred'], 1, p['gt'], p['conf'])], [0], DEV)
    ws = hip.depth_workspace(table, DEV)
    ops = dict(align=z(F64, 1, 2), **ws_ops(ws, 'partials', 'out'))
    hold(recorder, lambda o: hip.depth_errors(table, 0.0, 10.0, 1.0, o['align'], (1.25,), ws_of(o)), ops)


def test_depth_table_refuses_a_stride_that_reaches_past_the_storage():
    H, W = 2, 3
    gt = z(F32, H, W)
    full = z(F32, H * W, 3)
    assert hip.depth_table([(full[:, 2], 3, gt, None)], [0], DEV).host[0, 0] == full.data_ptr() + 8          # z of a whole pointmap, read in place
    cut = full[:-1].clone()                                   # the last pixel sliced off: 15 elements of storage
    with pytest.raises(RuntimeError, match='depth_table: .*storage'):
        hip.depth_table([(cut[:, 2], 3, gt, None)], [0], DEV)
    with pytest.raises(RuntimeError, match='depth_table'):
        hip.depth_table([(full[:, 2], 0, gt, None)], [0], DEV)


# ---------------------------------------------------------------------------------------------------------------- the model path
def test_layernorm(recorder):
    rows, D = 3, 8
    ops = dict(x=pv(F32, rows, D), gamma=z(F32, D), beta=z(F32, D), out=pv(F16, rows, D))
    hold(recorder, lambda o: hip.layernorm(o['x'], o['gamma'], o['beta'], o['out'], 1e-6, rows=rows), ops)


def test_layernorm_remapped_rows_with_an_addend(recorder):
    """grp = (3, 4, 1): row 5, the last of 6, is read at (5 // 3) * 4 + 1 + 5 % 3 = 7, so x and add hold 8 rows - 'rows' leaves 7: enough for the 6 rows
    of the call, one short of the remapped last row"""
    rows, D = 6, 8
    ops = dict(x=pv(F32, 8, D), gamma=z(F32, D), beta=z(F32, D), add=pv(F32, 8, D), out=pv(F32, rows, D))
    hold(recorder, lambda o: hip.layernorm(o['x'], o['gamma'], o['beta'], o['out'], 1e-6, rows=rows, grp=(3, 4, 1), add=o['add']), ops)
    del recorder[:]
    hip.layernorm(ops['x'][:7], ops['gamma'], ops['beta'], ops['out'], 1e-6, rows=rows, add=ops['add'][:6])      # without the remap 6 rows do
    assert len(recorder) == 1


def test_layernorm_batch(recorder):
    n, rows, D = 2, 3, 8
    ops = dict(x_all=z(F32, n, rows, D + 4)[:, :, :D], gamma_all=z(F32, n, D), beta_all=z(F32, n, D), out_all=z(F16, n, rows, D + 4)[:, :, :D])
    hold(recorder, lambda o: hip.layernorm_batch(o['x_all'], o['gamma_all'], o['beta_all'], o['out_all'], 1e-6, rows=rows), ops)
    for name in ('x_all', 'out_all'):                       # one row fewer in every problem, one column narrower
        for bad in (ops[name][:, :-1], ops[name][:, :, :-1]):
            del recorder[:]
            with pytest.raises(RuntimeError):
                hip.layernorm_batch(*(dict(ops, **{name: bad})[k] for k in ('x_all', 'gamma_all', 'beta_all', 'out_all')), 1e-6, rows=rows)
            assert not recorder


def test_rowstats(recorder):
    rows, D = 3, 64
    ops = dict(x=pv(F32, rows, D), xcopy=pv(F16, rows, D), stats=z(F32, rows, 1, 2))
    hold(recorder, lambda o: hip.rowstats(o['x'], o['xcopy'], o['stats']), ops, free=('x',))
    for bad in (z(F32, rows - 1, 1, 2), z(F32, rows, 0, 2), z(F32, rows, 1, 1)):
        del recorder[:]
        with pytest.raises(RuntimeError):
            hip.rowstats(ops['x'], ops['xcopy'], bad)
        assert not recorder


def test_add_cast(recorder):
    rows, D = 3, 8
    ops = dict(a=pv(F16, rows, D), out=pv(F32, rows, D), b=pv(F32, rows, D))
    hold(recorder, lambda o: hip.add_cast(o['a'], o['out'], b=o['b']), ops, free=('out',))
    del recorder[:]
    hip.add_cast(ops['a'], ops['out'], b=ops['b'][:2], b_mod=2)          # b_mod rows of b do
    with pytest.raises(RuntimeError):
        hip.add_cast(ops['a'], ops['out'], b=ops['b'][:1], b_mod=2)
    assert len(recorder) == 1


def test_split3(recorder):
    ops = dict(x=pv(F32, 3, 8), out=pv(F16, 3, 24))
    hold(recorder, lambda o: hip.split3(o['x'], o['out']), ops, free=('x',))


def test_split_operand(recorder):
    ops = dict(x=pv(F32, 3, 8), out=pv(F16, 3, 3 * 64))
    hold(recorder, lambda o: hip.split_operand(o['x'], 0, out=o['out']), ops, free=('x',))


def test_rope2d_(recorder):
    rows, nheads, hd = 3, 2, 16
    ops = dict(x=pv(F16, rows, nheads * hd), pos=z(I32, rows, 2), table=z(F32, 5, hd // 4, 2))
    hold(recorder, lambda o: hip.rope2d_(o['x'], o['pos'], o['table'], nheads, hd), ops)


def test_patchify(recorder):
    ops = dict(img=z(F32, 1, 3, 4, 4), out=pv(F16, 4, 12))
    hold(recorder, lambda o: hip.patchify(o['img'], o['out'], 2), ops)
    del recorder[:]
    with pytest.raises(RuntimeError, match='patchify: out.*storage'):    # every row is filled up to the leading dimension: the last row's padding too
        hip.patchify(ops['img'], z(F16, 4 * 16 - 1).as_strided((4, 12), (16, 1)), 2)
    assert not recorder


def test_token_embed(recorder):
    B, L, D = 2, 3, 8
    ops = dict(ids=z(I32, B, L), tok=z(F32, 5, D), pos=z(F32, 4, D), out=pv(F32, B * L, D), status=z(I32, 1))
    hold(recorder, lambda o: hip.token_embed(o['ids'], o['tok'], o['pos'], o['out'], o['status']), ops, free=('ids', 'tok', 'pos'))
    for bad in (dict(tok=z(F32, 5, D - 4)), dict(pos=z(F32, 4, D + 4)), dict(ids=z(I32, B * L))):
        del recorder[:]
        with pytest.raises(RuntimeError):
            o = dict(ops, **bad)
            hip.token_embed(o['ids'], o['tok'], o['pos'], o['out'], o['status'])
        assert not recorder


def test_l2norm_rows(recorder):
    ops = dict(x=pv(F32, 3, 8), out=pv(F16, 3, 8))
    hold(recorder, lambda o: hip.l2norm_rows(o['x'], o['out'], 1e-7), ops, free=('x',))


def test_mean4(recorder):
    ops = dict(F=z(F16, 1, 8, 8, 4), Fm=z(F16, 1, 4))
    hold(recorder, lambda o: hip.mean4(o['F'], o['Fm'], 1, 8, 8, 4), ops)


def test_resize_bilinear(recorder):
    ops = dict(F=z(F16, 1, 2, 2, 4), Fd=z(F16, 1, 3, 3, 4))
    hold(recorder, lambda o: hip.resize_bilinear(o['F'], o['Fd'], 1, 2, 2, 3, 3, 4), ops)


def test_attn_mask_from_logits(recorder):
    ops = dict(logits=pv(F32, 3, 5), mask=pv(U8, 3, 5))
    hold(recorder, lambda o: hip.attn_mask_from_logits(o['logits'], o['mask']), ops, free=('logits',))


def test_loftup_guidance_gn(recorder):
    n, h, w, nf = 1, 4, 4, 2
    P, ch = (h // 2) * (w // 2), 10 * nf + 3
    ops = dict(img=z(F32, n, 3, h, w), biases=z(F32, 2, 5, nf), gamma=z(F32, ch), beta=z(F32, ch), scratch=z(F32, n * (3 * P + 6)),
               stats=hip.stats_buffer(n, 1, DEV), out=pv(F16, n * P, ch), mm=z(F32, n, 3, 2))
    hold(recorder, lambda o: hip.loftup_guidance_gn(o['img'], o['biases'], o['gamma'], o['beta'], 1e-5, o['scratch'], o['stats'], o['out'], nf, mm=o['mm']), ops)


def test_minmax_merge(recorder):
    ops = dict(mm=z(F32, 2, 3, 2), scope=z(I32, 2), out=z(F32, 2, 3, 2))
    hold(recorder, lambda o: hip.minmax_merge(o['mm'], o['scope'], o['out']), ops)
    del recorder[:]
    with pytest.raises(RuntimeError, match='minmax_merge: out of place'):
        hip.minmax_merge(ops['mm'], ops['scope'], ops['mm'])
    assert not recorder


def test_groupnorm_stats(recorder):
    nimg, P, Cc, G = 2, 3, 8, 2
    ops = dict(x=pv(F16, nimg * P, Cc), stats=hip.stats_buffer(nimg, G, DEV))
    hold(recorder, lambda o: hip.groupnorm_stats(o['x'], o['stats'], nimg, P, Cc, G), ops)


def test_groupnorm_apply(recorder):
    nimg, P, Cc, G = 2, 3, 8, 2
    ops = dict(x=pv(F16, nimg * P, Cc), stats=z(F32, nimg, G, 2), gamma=z(F32, Cc), beta=z(F32, Cc), out=pv(F16, nimg * P, Cc))
    hold(recorder, lambda o: hip.groupnorm_apply(o['x'], o['stats'], o['gamma'], o['beta'], o['out'], nimg, P, Cc, G, 1e-5, True), ops)
    split = dict(ops, out=pv(F16, nimg * P, 3 * Cc))
    hold(recorder, lambda o: hip.groupnorm_apply(o['x'], o['stats'], o['gamma'], o['beta'], o['out'], nimg, P, Cc, G, 1e-5, True, split=True), split)


def test_loftup_lr_pe(recorder):
    nimg, h, w, col0 = 1, 2, 3, 8
    ops = dict(biases=z(F32, 2, 2, 5), out=pv(F16, nimg * h * w, col0 + 20))
    hold(recorder, lambda o: hip.loftup_lr_pe(o['biases'], o['out'], col0, nimg, h, w), ops)
