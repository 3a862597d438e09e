"""Every GEMM variant under the leading dimensions and base offsets the model really uses (tests/gemm_layout_cases.py): column slices as A, strided
residuals, outputs inside larger buffers, C rows that are 8-byte but not 16-byte aligned, and layouts one step outside a persistent / row-streaming class.

Per case and 16-bit format:
  (a) pst_gemm_variant / pst_gemm_pair_variant names the case's kernel for the padded parameters (and the case's `tight_variant` for the tight ones);
  (b) every output (C, xcopy, statistics, both outputs of a pair) of the padded call equals the tight call bit for bit in its logical region - a leading
      dimension changes addresses, not arithmetic;
  (c) every other element the test owns - pad columns, rows past M, rows a remap skips, guard rows, the bytes before the offset - still holds the sentinel;
  (d) the logical region holds no NaN: no poisoned padding of an input reached an accumulator or an epilogue, no element was left unwritten;
  (e) the anchor cases are held to the float64 reference under errbound.gemm_bound / gemm_bound_from / ln_fold_bound, as tests/test_hip_ops.py does.
The padded launch runs twice (fresh buffers) and the two results are compared byte for byte.

The ring-depth cases (PST_TUNE_DEEP_RING 6 / 8) are no proof of dispatch: pst_gemm_variant returns "gemm_kernel<2,2,false>" for every depth, so (a) cannot
tell the 6- or 8-slab instantiation from the 4-slab one.  The cases set the knob on a shape that meets the launcher's precondition (at most one tile per CU,
K >= 512; restated and asserted in tests/test_gemm_layout_checks.py) and hold whatever then runs to (b) - (e)."""
import contextlib

import pytest
import torch

from conftest import rel_l2
import errbound as EB
import gemm_layout_cases as G

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@contextlib.contextmanager
def tuned(hip, knobs):
    prev = {}
    try:
        for k, v in knobs.items():
            prev[k] = hip.tune(k, v)
        yield
    finally:
        for k, v in prev.items():
            hip.tune(k, v)


def _params(hip, sets):
    out = []
    for s in sets:
        a, w, o, kw = G.call_args(s)
        out.append(hip._gemm_params(a, w, o, **kw)[0])
    return out


def _variant(hip, c, sets):
    ps = _params(hip, sets)
    return hip._variant('pst_gemm_pair_variant' if c['kind'] == 'pair' else 'pst_gemm_variant', None, *ps)


def _launch(hip, c, sets):
    hip._call('pst_gemm_pair' if c['kind'] == 'pair' else 'pst_gemm', *_params(hip, sets))


def _anchor(c, s):
    """(e): the padded call against the float64 reference of the same operands, under the bound of the kernel's arithmetic"""
    p, v = s['p'], s['vals']
    d = dev()
    got = s['c'].logical()
    out_fmt = got.dtype
    ref = G.reference(p, v, d)
    g = lambda k: v[k].to(d) if k in v else None
    what = '%s (%dx%dx%d)' % (c['name'], p['M'], p['N'], p['K'])
    if p['ln']:
        ref2, bound = EB.ln_fold_bound(g('a'), g('w'), g('colsum'), g('bias'), g('x'), 1e-6, out_fmt, p['act'])
        assert rel_l2(ref, ref2) < 1e-12                                   # the module's restatement is errbound's
    elif p['conv']:
        cc = p['conv'][0]
        acc = 2 * (9 * cc / 32 + 2) * EB.U32 * G.core(p, v, d, absolute=True)   # implicit im2col: zero-padded taps add nothing
        bound = EB.gemm_bound_from(G.core(p, v, d), acc, out_fmt, bias=g('bias'), act=p['act'])
    elif p['batch']:
        bound = torch.stack([EB.gemm_bound(g('a')[b], g('w')[b], out_fmt, bias=g('bias')[b], act=p['act']) for b in range(p['batch'])])
    else:
        bound = EB.gemm_bound(g('a'), g('w'), out_fmt, bias=g('bias'), act=p['act'], gamma=g('gamma'), res=g('res'), mode='fp32' if p['f32'] else 'mfma16')
    return EB.check(got, ref, bound, what)


GEMM_PARAMS = [(c['name'], fmt) for c in G.CASES for fmt in c['fmts']]


@pytest.mark.parametrize('name,fmt', GEMM_PARAMS)
def test_gemm_layout(name, fmt):
    from panst3r_amd import hip
    c = G.BY_NAME[name]
    d = dev()
    tight = [G.to_device(s, d) for s in G.build(c, fmt, False)]
    cpu = G.build(c, fmt, True)
    padded = [G.to_device(s, d) for s in cpu]
    again = [G.to_device(s, d, like) for s, like in zip(cpu, padded)]
    del cpu
    with tuned(hip, c['tune']):
        got_p, got_t = _variant(hip, c, padded), _variant(hip, c, tight)
        print('\n%s [%s]: padded -> %s, tight -> %s' % (G.describe(c), fmt, got_p, got_t))
        assert got_p == c['variant'], (got_p, hip.lib().pst_last_error())                               # (a)
        assert got_t == c['tight_variant'], (got_t, hip.lib().pst_last_error())
        _launch(hip, c, tight)
        _launch(hip, c, padded)
        _launch(hip, c, again)
        torch.cuda.synchronize()
    for i, (t, p, q) in enumerate(zip(tight, padded, again)):
        for (k, bt), (_, bp), (_, bq) in zip(G.outputs(t), G.outputs(p), G.outputs(q)):
            what = '%s [%s] problem %d %s' % (name, fmt, i, k)
            G.check_outside(what, bp)                                                                   # (c)
            G.check_no_nan(what, bp)                                                                    # (d)
            G.check_bits(what, bt, bp)                                                                  # (b)
            G.check_same_bytes(what, bp, bq)
            G.check_outside(what + ' (tight)', bt)
    if c['anchor']:
        for s in padded:
            print('  anchor: worst |err| / bound = %.3f' % _anchor(c, s))                               # (e)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('mc', G.MASK_HEAD_CASES, ids=lambda m: m['name'])
def test_mask_head_layout(mc, fmt):
    """pst_mask_head with lde = C + 8, f_view_stride = P C + 64, out_view_stride = Q P + 64 (through the C ABI: the Python wrapper takes contiguous tensors)"""
    from panst3r_amd import hip
    d = dev()
    code = hip._TC[G.fmt_dtype(fmt)]

    def run(padded):
        b = G.build_mask_head(mc, fmt, padded)
        e, f, o = b['e'].to(d), b['f'].to(d), b['out'].to(d)
        hip._call('pst_mask_head', e.view().data_ptr(), b['lde'], f.view().data_ptr(), b['fvs'], o.view().data_ptr(), b['ovs'], mc['n'], mc['Q'], mc['P'], mc['C'], code)
        torch.cuda.synchronize()
        return b, o
    (_, t), (b, p), (_, q) = run(False), run(True), run(True)
    print('\n%s [%s]: mask_head_kernel C=%d Q=%d P=%d n=%d lde=%d f_view_stride=%d out_view_stride=%d' % (mc['name'], fmt, mc['C'], mc['Q'], mc['P'], mc['n'],
                                                                                                         b['lde'], b['fvs'], b['ovs']))
    what = '%s [%s]' % (mc['name'], fmt)
    G.check_outside(what, p)
    G.check_no_nan(what, p)
    G.check_bits(what, t, p)
    G.check_same_bytes(what, p, q)
    E, Fv = b['E'].to(d), b['F'].to(d)
    got = p.logical()
    for i in range(mc['n']):                                # a K = C dot product per pixel: the GEMM model, as test_mask_head_streaming_kernel
        EB.check(got[i], E.double() @ Fv[i].double().T, EB.gemm_bound(E, Fv[i], torch.float32), what + ' view %d' % i)


@pytest.mark.parametrize('fmt', ['bf16', 'f16'])
@pytest.mark.parametrize('rc', G.ROWSTATS_CASES, ids=lambda r: r['name'])
def test_rowstats_layout(rc, fmt):
    """pst_rowstats, the twin of the fold producer: ldx = D + 4, ldxc = D + 8, stats_ld = D / 64 + 1"""
    from panst3r_amd import hip
    d = dev()
    d16 = G.fmt_dtype(fmt)

    def run(padded):
        b = G.build_rowstats(rc, fmt, padded)
        x, xc, st = b['x'].to(d), b['xcopy'].to(d), b['stats'].to(d)
        hip._call('pst_rowstats', x.view().data_ptr(), x.ld, hip._TC[torch.float32], xc.view().data_ptr(), xc.ld, st.view().data_ptr(), b['sld'], rc['rows'], rc['D'],
                  hip._TC[d16])
        torch.cuda.synchronize()
        return b, xc, st
    (_, txc, tst), (b, pxc, pst_), (_, qxc, qst) = run(False), run(True), run(True)
    print('\n%s [%s]: rowstats_kernel rows=%d D=%d ldx=%d ldxc=%d stats_ld=%d' % (rc['name'], fmt, rc['rows'], rc['D'], b['x'].ld, pxc.ld, b['sld']))
    for k, t, p, q in (('xcopy', txc, pxc, qxc), ('stats', tst, pst_, qst)):
        what = '%s [%s] %s' % (rc['name'], fmt, k)
        G.check_outside(what, p)
        G.check_no_nan(what, p)
        G.check_bits(what, t, p)
        G.check_same_bytes(what, p, q)
    x = b['X']
    assert torch.equal(pxc.logical().cpu(), x.to(d16))                        # the anchors of test_gemm_layernorm_fold_consumer
    g = x.reshape(rc['rows'], rc['D'] // 64, 64)
    st = pst_.logical().cpu()
    assert rel_l2(st[..., 0], g.sum(-1)) < 1e-5 and rel_l2(st[..., 1], (g * g).sum(-1)) < 1e-5
