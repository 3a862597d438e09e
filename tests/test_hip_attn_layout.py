"""Every attention variant under the strides, paddings and base offsets the model really uses (tests/attn_layout_cases.py): q | k column slices of one
buffer with Tp > T rows per batch, V^T batches side by side, outputs inside wider guarded buffers, shared / key-padding masks, negative batch strides and a
caller-owned split-K workspace of exactly pst_attn_workspace_bytes - with NaN in everything the operand contract of include/panst3r_hip.h says is not read,
large finite values in the V^T columns it says are read and multiplied by 0, and a sentinel in everything that may be written.

Per case and format:
  (a) pst_attn_variant / pst_attn_pair_variant / pst_attn_x3_variant names the case's kernel for the padded and the tight parameters;
  (b) the logical O of the padded call equals the tight call bit for bit - strides change addresses, not arithmetic;
  (c) every other element of the O buffer, and of the workspace buffer outside [offset, offset + pst_attn_workspace_bytes), still holds the sentinel;
  (d) the logical O holds no NaN or Inf: no poisoned pad reached a score, a sum or an output, no element was left unwritten;
  (e) the anchor cases are held to errbound.attn_bound against the float64 softmax of the same operands, as tests/test_hip_ops.py::check_attention,
      test_hip_fp32.py and test_hip_x3_producers.py do (a PST_X3H output: plus the split's own 2^-22 |ref| + 2^-25).
The padded launch runs twice (fresh buffers) and the two results are compared byte for byte; each output of a pair is compared with its own single launch.
A negative k_rs or v_ds is refused by every entry point before anything is launched."""
import pytest
import torch

import errbound as EB
import gemm_layout_cases as G
import attn_layout_cases as A

pytestmark = pytest.mark.gpu
PST_EINVAL = -1


def dev():
    return torch.device('cuda:0')


def _ptr(buf):
    return buf.alloc.data_ptr() + buf.base * buf.alloc.element_size()


def _params(hip, s):
    """(pst_attn_params, the tensors it points into) of a built set on the device"""
    p = s['p']
    code = hip._TC[s['q'].alloc.dtype]
    m, ws = s['mask'], s['ws']
    prm, keep = hip._attn_struct(code, _ptr(s['q']), _ptr(s['k']), _ptr(s['vt']), s['o'].alloc[s['o'].base:], p['B'], p['H'], p['Nq'], p['Nk'], p['hd'],
                                 s['q'].strides, s['k'].strides, s['vt'].strides, s['o'].strides, p['scale'], None if m is None else m.alloc[m.base:],
                                 (0, 0) if m is None else m.strides, p['nsplit'], None if ws is None else ws.alloc[ws.base: ws.base + ws.idx.numel()], p['pre'])
    if ws is not None:
        assert prm.ws_bytes == hip.lib().pst_attn_workspace_bytes(p['B'], p['H'], p['Nq'], p['hd'], p['nsplit']) == A.ws_bytes(p) and prm.ws == _ptr(ws)
    return prm, keep


def _x3_extra(hip, s):
    """(Q_lo, K_lo, Vt_lo, out_type, out_block) of pst_attn_x3: the lo planes at the offsets of the hi planes"""
    lo = lambda b: s['allocs'][b.name + '_lo'].data_ptr() + b.base * 2
    return lo(s['q']), lo(s['k']), lo(s['vt']), (hip.X3H if s['p']['out'] == 'x3h' else hip._TC[torch.float32]), s['out_block']


def _name(hip, what, *params):
    """the entry point's answer as it is: None for NULL (refused), '' for a pair that is not fused"""
    r = getattr(hip.lib(), what)(*params)
    return None if r is None else r.decode()


def _variant(hip, c, sets):
    ps = [_params(hip, s)[0] for s in sets]
    what = {'fwd': 'pst_attn_variant', 'pair': 'pst_attn_pair_variant', 'x3': 'pst_attn_x3_variant'}[c['kind']]
    return _name(hip, what, *ps)


def _launch(hip, c, sets, single=False):
    keep = [_params(hip, s) for s in sets]
    if c['kind'] == 'x3':
        hip._call('pst_attn_x3', keep[0][0], *_x3_extra(hip, sets[0]))
    elif c['kind'] == 'pair' and not single:
        hip._call('pst_attn_pair', keep[0][0], keep[1][0])
    else:
        for prm, _ in keep:
            hip._call('pst_attn_fwd', prm)
    return keep


def _anchor(c, s, fmt):
    """(e): the padded call against the float64 reference of the same operands, under the bound of the kernel's arithmetic"""
    p, v = s['p'], s['vals']
    d = dev()
    q, k, vv = v['q'].to(d), v['k'].to(d), v['v'].to(d)
    if c['kind'] == 'x3':
        # errbound's references are float64 evaluations of the operands the kernel GETS: here the planes, hi + lo (exact in float64).  The bound's x3 terms
        # model a plane pair as 2^-22 relative; an fp32 value in f16's subnormal range (|x| < 2^-14) is only carried to 2^-25 absolute, and a row that a
        # mask leaves a single key returns that key's V as it is (x3_h64_b128_q129: v = -4.298e-6 comes back as -4.292e-6, 40 x the bound on the fp32 value)
        hl = lambda b: (s['allocs'][b.name][b.idx.to(d)].double() + s['allocs'][b.name + '_lo'][b.idx.to(d)].double())
        q, k, vv = hl(s['q']), hl(s['k']), hl(s['vt']).transpose(-1, -2).contiguous()
    m = v['mask'].to(d) if v['mask'] is not None else None
    ref = EB.attn_ref(q, k, vv, m, p['pre'])
    what = '%s [%s] B%d H%d Nq%d Nk%d hd%d' % (c['name'], fmt, p['B'], p['H'], p['Nq'], p['Nk'], p['hd'])
    if c['kind'] == 'x3':
        bound = EB.attn_bound(q, k, vv, m, p['pre'], torch.float32, torch.float32, nsplit=p['nsplit'], mode='x3')
        if p['out'] == 'x3h':
            bound = bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25
    elif s['f32ops']:
        bound = EB.attn_bound(q, k, vv, m, p['pre'], torch.float32, torch.float32, mode='fp32')
    else:
        d16 = A.fmt_dtype(fmt)
        bound = EB.attn_bound(q, k, vv, m, p['pre'], d16, d16, nsplit=p['nsplit'])
    return EB.check(A.logical_out(s), ref, bound, what)


@pytest.mark.parametrize('name,fmt', A.PARAMS)
def test_attn_layout(name, fmt):
    from panst3r_amd import hip
    c = A.BY_NAME[name]
    d = dev()
    tight = [A.to_device(s, d) for s in A.build(c, fmt, False)]
    cpu = A.build(c, fmt, True)
    padded = [A.to_device(s, d) for s in cpu]
    again = [A.to_device(s, d, like) for s, like in zip(cpu, padded)]
    single = [A.to_device(s, d, like) for s, like in zip(cpu, padded)] if c['kind'] == 'pair' else None
    del cpu
    got_p, got_t = _variant(hip, c, padded), _variant(hip, c, tight)
    print('\n%s [%s]: padded -> %r, tight -> %r' % (A.describe(c), fmt, got_p, got_t))
    assert got_p == c['variant'], (got_p, hip.lib().pst_last_error())                                   # (a)
    assert got_t == c['tight_variant'], (got_t, hip.lib().pst_last_error())
    keep = [_launch(hip, c, tight), _launch(hip, c, padded), _launch(hip, c, again)]
    if single:
        keep.append(_launch(hip, c, single, single=True))
    torch.cuda.synchronize()
    del keep
    for i, (t, p, q) in enumerate(zip(tight, padded, again)):
        for (k, bt), (_, bp), (_, bq) in zip(A.outputs(t), A.outputs(p), A.outputs(q)):
            what = '%s [%s] problem %d %s' % (name, fmt, i, k)
            G.check_outside(what, bp)                                                                   # (c)
            G.check_same_bytes(what, bp, bq)
            G.check_outside(what + ' (tight)', bt)
            if k == 'o':
                G.check_no_nan(what, bp)                                                                # (d)
                assert bool(torch.isfinite(bp.logical().float()).all()), what + ': Inf in the logical region'
                G.check_bits(what, bt, bp)                                                              # (b)
                if single:
                    G.check_bits(what + ' (pair against its own single launch)', single[i]['o'], bp)
                    G.check_outside(what + ' (single launch)', single[i]['o'])
    if c['anchor'] and not (c['kind'] == 'x3' and fmt != 'f16'):
        for s in padded:
            print('  anchor: worst |err| / bound = %.3f' % _anchor(c, s, fmt))                          # (e)


# ------------------------------------------------------------------------------------------------------------------------------------- refusals
def _sentinel_everywhere(buf):
    return bool((G.bits(buf.alloc) == G.SENTINEL[buf.alloc.dtype]).all())


@pytest.mark.parametrize('field', ['k_rs', 'v_ds'])
@pytest.mark.parametrize('name,fmt', [('h64_b64_open', 'bf16'), ('h96_b64_split_mask', 'f16'), ('f32_h64_open', 'f32'), ('x3_h64_f32_direct', 'f16'),
                                      ('x3_h96_x3h_split', 'f16')])
def test_negative_row_strides_are_refused(name, fmt, field):
    """k_rs and v_ds enter the 16-bit kernels' full-tile offsets as 32-bit unsigned numbers: every entry point (the fp32-operand kernel too: one contract)
    returns PST_EINVAL naming the field BEFORE anything is launched, its *_variant returns NULL, and O and the workspace keep the sentinel everywhere"""
    from panst3r_amd import hip
    c = A.BY_NAME[name]
    s = A.to_device(A.build(c, fmt, True)[0], dev())
    prm, keep = _params(hip, s)
    x3 = c['kind'] == 'x3'
    variant = 'pst_attn_x3_variant' if x3 else 'pst_attn_variant'
    assert _name(hip, variant, prm) == c['variant']                  # admitted as built
    setattr(prm, field, -getattr(prm, field))
    assert getattr(prm, field) < 0
    L = hip.lib()
    if x3:
        rc = L.pst_attn_x3(prm, *_x3_extra(hip, s), hip._stream())
    else:
        rc = L.pst_attn_fwd(prm, hip._stream())
    msg = L.pst_last_error().decode()
    assert rc == PST_EINVAL and field in msg and 'negative' in msg, (rc, msg)
    assert _name(hip, variant, prm) is None
    if not x3:
        good, _ = _params(hip, s)
        for a, b in ((prm, good), (good, prm)):
            assert L.pst_attn_pair(a, b, hip._stream()) == PST_EINVAL and field in L.pst_last_error().decode()
            assert _name(hip, 'pst_attn_pair_variant', a, b) is None
    torch.cuda.synchronize()
    assert _sentinel_everywhere(s['o']) and (s['ws'] is None or _sentinel_everywhere(s['ws'])), name + ': a refused call wrote'
