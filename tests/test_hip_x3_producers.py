"""The PST_X3H producers (ABI 18): pst_layernorm / pst_layernorm_add_batch, pst_groupnorm_apply and pst_attn_x3 (direct store and split-K combine) write
their result as the split A operand [hi | hi | lo] of the next 3 x f16 GEMM.  The header's contract is exact - "what pst_split_operand(side 0) would make of
its fp32 result" - so every producer is held to it twice:

 (i)  bit for bit: the same entry point on the same inputs with fp32 output, then pst_split_operand(side 0, kpad = block) of that, against the PST_X3H output
      written into a sentinel-filled buffer (guard rows before and after: nothing outside [rows, 3 x block] changes; pad columns as each kernel documents);
 (ii) an independent anchor: hi + lo against the float64 reference of the op under that op's fp32 bound of tests/errbound.py plus the split's own error
      2^-22 |ref| + 2^-25.  That term is derived: hi = rn16(v) leaves |v - hi| <= 2^-11 |v| (exact in fp32), lo = rn16(v - hi) rounds that remainder to 11
      more bits, |v - hi - lo| <= 2^-22 |v|; a lo (or a whole value) in f16's subnormal range is quantised to the 2^-24 spacing, i.e. 2^-25.
"""
import functools

import numpy as np
import pytest
import torch

import errbound as EB

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16 = torch.float32, torch.float16
SENT = -777.0             # exactly representable in f16 and never a result here
GUARD = 3                 # sentinel rows before and after every split output


def rn(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def rel64(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def d(t):
    return t.to(DEV)


def bits(t):
    return t.contiguous().view(torch.int16)


def guarded(rows, block, pad_from=None):
    """f16 [GUARD + rows + GUARD, 3 x block] full of SENT and its [rows, 3 x block] view; pad_from: columns [pad_from, block) of the three blocks start as
    zeros (a producer that does not promise to write them must leave them alone)"""
    buf = torch.full((rows + 2 * GUARD, 3 * block), SENT, dtype=F16, device=DEV)
    view = buf[GUARD:GUARD + rows]
    if pad_from is not None and pad_from < block:
        view.view(rows, 3, block)[:, :, pad_from:] = 0
    return buf, view


def assert_guards(buf, rows, what):
    sent = torch.full((), SENT, dtype=F16).view(torch.int16).item()
    g = torch.cat([bits(buf[:GUARD]), bits(buf[GUARD + rows:])])
    assert bool((g == sent).all()), what + ': wrote outside its [rows, 3 x block] output'


def split_term(ref):
    return 2.0 ** -22 * ref.double().abs() + 2.0 ** -25


def split_value(view, block, width):
    """hi + lo (float64: the sum is exact there) of the first `width` columns of a split output [rows, 3 x block]"""
    v = view.view(view.shape[0], 3, block)
    return v[:, 0, :width].double() + v[:, 2, :width].double()


def assert_is_split_operand(view, out32, block, what):
    from panst3r_amd import hip
    want = hip.split_operand(out32, 0, kpad=block)
    same = bits(view) == bits(want)
    if not bool(same.all()):
        bad = (~same).nonzero()
        r, c = int(bad[0, 0]), int(bad[0, 1])
        raise AssertionError('%s: %d of %d f16 values differ from split_operand(fp32 result); first at row %d, block %d, column %d: got %r want %r'
                             % (what, int((~same).sum()), same.numel(), r, c // block, c % block, float(view[r, c]), float(want[r, c])))


# ---------------------------------------------------------------------------------------------------------------- layernorm
def _ln_rows(D, remap):
    """(input rows [R, D], the rows the kernel normalises [74, D], grp)"""
    if not remap:
        x = rn(40, 74, D) * 3 + 1
        x[::9] = rn(47, x[::9].shape[0], D) * 0.01 + 1            # quiet rows, as tests/test_hip_ops.py::test_layernorm
        return x, (lambda t: t), None
    xs = rn(43, 2 * 38, D)
    return xs, (lambda t: t.reshape(2, 38, D)[:, 1:].reshape(74, D)), (37, 38, 1)     # skip a leading CLS row per 38-row group


@pytest.mark.parametrize('pad', [0, 16])
@pytest.mark.parametrize('in_fmt', [F32, F16], ids=['x32', 'x16'])
@pytest.mark.parametrize('D', [48, 384, 768, 1024])
def test_layernorm_split_output(D, in_fmt, pad):
    from panst3r_amd import hip
    rows, block, eps = 74, D + pad, 1e-6
    g, b = 1 + 0.1 * rn(41, D), 0.1 * rn(42, D)
    for remap in (False, True):
        what = 'layernorm X3H D=%d block=%d %s remap=%s' % (D, block, in_fmt, remap)
        x, pick, grp = _ln_rows(D, remap)
        x = x.to(in_fmt)
        out32 = torch.full((rows + 1, D), float('nan'), device=DEV)
        hip.layernorm(d(x), d(g), d(b), out32[:rows], eps, grp=grp)
        buf, view = guarded(rows, block, pad_from=D)
        hip.layernorm(d(x), d(g), d(b), view, eps, grp=grp, split=True)
        assert_is_split_operand(view, out32[:rows], block, what)             # (pad columns: zeros before, zeros in split_operand's output: untouched)
        assert_guards(buf, rows, what)
        xr = pick(x)
        ref = EB.layernorm_ref(xr, g, b, eps)
        EB.check(split_value(view, block, D).cpu(), ref, EB.rownorm_bound(xr, g, b, eps, F32) + split_term(ref), what)


@pytest.mark.parametrize('in_fmt', [F32, F16], ids=['x32', 'x16'])
def test_layernorm_add_batch_split_output(in_fmt):
    """three problems in one launch (gridDim.y = 3): own input, gamma / beta and output slice each, a shared addend; the 16-bit-wide output advances by a
    batch stride of its own (larger than rows x 3 D: guard rows between the problems stay untouched)"""
    from panst3r_amd import hip
    n, rows, D, eps = 3, 37, 768, 1e-6
    x = (rn(50, n, rows, D) * 2 + 0.5).to(in_fmt)
    add = rn(51, rows, D)
    g, b = 1 + 0.1 * rn(52, n, D), 0.1 * rn(53, n, D)
    out32 = torch.full((n, rows, D), float('nan'), device=DEV)
    hip.layernorm_batch(d(x), d(g), d(b), out32, eps, add=d(add))
    buf = torch.full((n, rows + GUARD, 3 * D), SENT, dtype=F16, device=DEV)
    out = buf[:, :rows]
    assert out.stride(0) > rows * 3 * D
    hip.layernorm_batch(d(x), d(g), d(b), out, eps, add=d(add), split=True)
    sent = torch.full((), SENT, dtype=F16).view(torch.int16).item()
    assert bool((bits(buf[:, rows:]) == sent).all()), 'layernorm_add_batch X3H: wrote between / behind the problems'
    for i in range(n):
        what = 'layernorm_add_batch X3H problem %d %s' % (i, in_fmt)
        assert_is_split_operand(out[i], out32[i], D, what)
        xa = x[i].float() + add                                    # the kernel's fp32 add: one rounding, the same as torch's
        ref = EB.layernorm_ref(xa, g[i], b[i], eps)
        EB.check(split_value(out[i], D, D).cpu(), ref, EB.rownorm_bound(xa, g[i], b[i], eps, F32) + split_term(ref), what)


# ---------------------------------------------------------------------------------------------------------------- groupnorm
@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('in_fmt', [F32, F16], ids=['x32', 'x16'])
@pytest.mark.parametrize('C,G,block', [(64, 1, 64), (104, 2, 128), (384, 8, 384)])
def test_groupnorm_apply_split_output(C, G, block, in_fmt, relu):
    """pad columns [C, block) of all three blocks come back as zeros ("zero beyond C"), whatever was there"""
    from panst3r_amd import hip
    P, nimg, eps = 150, 2, 1e-5
    what = 'groupnorm_apply X3H C=%d G=%d block=%d %s relu=%s' % (C, G, block, in_fmt, relu)
    x = (rn(84, nimg * P, C) * 2 + 0.3).to(in_fmt)
    g, b = 1 + 0.1 * rn(85, C), 0.1 * rn(86, C)
    st = hip.stats_buffer(nimg, G, DEV)
    hip.groupnorm_stats(d(x), st, nimg, P, C, G)
    out32 = torch.full((nimg * P, block), float('nan'), device=DEV)
    hip.groupnorm_apply(d(x), st, d(g), d(b), out32, nimg, P, C, G, eps, relu)
    buf, view = guarded(nimg * P, block)                        # the pad columns start as SENT
    hip.groupnorm_apply(d(x), st, d(g), d(b), view, nimg, P, C, G, eps, relu, split=True)
    assert_is_split_operand(view, out32[:, :C], block, what)
    if block > C:
        assert not bool(bits(view.view(nimg * P, 3, block)[:, :, C:]).any()), what + ': pad columns are not zero bits'
    assert_guards(buf, nimg * P, what)
    ref, bound = EB.groupnorm(x, nimg, P, G, g, b, eps, F32, relu=relu)
    EB.check(split_value(view, block, C).cpu(), ref, bound + split_term(ref), what)


# ---------------------------------------------------------------------------------------------------------------- attention on split operands
@functools.lru_cache(maxsize=None)
def _attn_case(B, H, Nq, Nk, hd, masked, pre):
    """operands (device layouts of tests/test_hip_fp32.py::test_attention_f32), its mask plus one fully blocked row, and the float64 reference"""
    from panst3r_amd import hip
    q, k, v = rn(20, B, H, Nq, hd) * (hd ** -0.5 * hip.LOG2E if pre else 1.0), rn(21, B, H, Nk, hd), rn(22, B, H, Nk, hd)
    mask, dead = None, None
    if masked:
        g = np.random.Generator(np.random.PCG64(5))
        mask = torch.from_numpy(g.uniform(size=(B, Nq, Nk)) < 0.6)
        mask[:, :, 0] = False
        mask[:, 0, min(64, Nk - 1):] = True                      # a row whose later tiles are fully blocked
        if Nq > 1:
            mask[:, 1, :Nk - 1] = True                           # a row whose only open key is the last one
            mask[:, 1, Nk - 1] = False
        if Nq > 2:
            dead = min(Nq - 1, 67)                               # a fully blocked row (in the second 64-query fragment where there is one)
            mask[:, dead] = True
    Nkp = (Nk + 7) // 8 * 8
    qd = d(q.permute(0, 2, 1, 3).reshape(B, Nq, H * hd).contiguous())
    kd = d(k.permute(0, 2, 1, 3).reshape(B, Nk, H * hd).contiguous())
    vt = torch.zeros(H * hd, B * Nkp + 8, dtype=F32)
    for bi in range(B):
        vt[:, bi * Nkp: bi * Nkp + Nk] = v[bi].permute(0, 2, 1).reshape(H * hd, Nk)
    vt = d(vt)
    md, ms = None, (0, 0)
    if masked:
        Nkm = (Nk + 3) // 4 * 4
        mm = torch.zeros(B, Nq, Nkm, dtype=torch.uint8)
        mm[:, :, :Nk] = mask.to(torch.uint8)
        md, ms = d(mm), (Nq * Nkm, Nkm)
    m64 = d(mask) if masked else None
    ops = (d(q), d(k), d(v), m64)
    return dict(qd=qd, kd=kd, vt=vt, Nkp=Nkp, md=md, ms=ms, dead=dead, ops=ops, ref=EB.attn_ref(*ops, pre))


@pytest.mark.parametrize('wide', [False, True], ids=['tight', 'padded'])
@pytest.mark.parametrize('nsplit', [None, 3], ids=['direct', 'combine'])
@pytest.mark.parametrize('pre', [False, True], ids=['scaled', 'prescaled'])
@pytest.mark.parametrize('masked', [False, True], ids=['open', 'masked'])
@pytest.mark.parametrize('B,H,Nq,Nk,hd', [(2, 3, 200, 333, 64), (3, 2, 50, 70, 96), (1, 2, 1, 5, 64)])
def test_attn_x3_split_output(B, H, Nq, Nk, hd, masked, pre, nsplit, wide):
    """nsplit None: the attention kernel's own split store (no key split at these sizes); 3: the partials go through the workspace and the combine kernel
    stores.  out_block = H hd, and H hd + 64 with zero pad columns the kernel must leave alone; strides of the split output in f16 elements."""
    from panst3r_amd import hip
    c = _attn_case(B, H, Nq, Nk, hd, masked, pre)
    D, rows = H * hd, B * Nq
    ob = D + (64 if wide else 0)
    what = 'attn_x3 X3H %s masked=%s pre=%s nsplit=%s out_block=%d' % ((B, H, Nq, Nk, hd), masked, pre, nsplit, ob)
    assert nsplit is not None or hip.auto_nsplit(B, H, Nq, Nk) == 1
    prev, hip.X3 = hip.X3, True
    try:
        kw = dict(q_strides=(Nq * D, hd, D), k_strides=(Nk * D, hd, D), v_strides=(c['Nkp'], hd * c['vt'].stride(0), c['vt'].stride(0)),
                  mask=c['md'], mask_strides=c['ms'], prescaled=pre, nsplit=nsplit)
        out32 = torch.full((rows, D), float('nan'), device=DEV)
        hip.attention(c['qd'], c['kd'], c['vt'], out32, B, H, Nq, Nk, hd, o_strides=(Nq * D, hd, D), **kw)
        buf, view = guarded(rows, ob, pad_from=D)
        hip.attention(c['qd'], c['kd'], c['vt'], view, B, H, Nq, Nk, hd, o_strides=(Nq * 3 * ob, hd, 3 * ob), **kw)
    finally:
        hip.X3 = prev
    assert_is_split_operand(view, out32, ob, what)
    assert_guards(buf, rows, what)
    if c['dead'] is not None:
        deadrows = view.view(B, Nq, 3 * ob)[:, c['dead']]
        assert not bool(bits(deadrows).any()), what + ': a fully masked row is not all-zero bits'
    got = split_value(view, ob, D).reshape(B, Nq, H, hd).permute(0, 2, 1, 3)
    q, k, v, m64 = c['ops']
    bound = EB.attn_bound(q, k, v, m64, pre, F32, F32, nsplit=nsplit or 1, mode='x3')
    EB.check(got, c['ref'], bound + split_term(c['ref']), what)


# ---------------------------------------------------------------------------------------------------------------- rejections
def _untouched(buf):
    sent = torch.full((), SENT, dtype=F16).view(torch.int16).item()
    return bool((bits(buf) == sent).all())


def test_split_output_rejections():
    """what the launchers refuse for a PST_X3H output raises and writes nothing"""
    from panst3r_amd import hip
    B, H, Nq, Nk, hd = 1, 2, 8, 16, 64
    D = H * hd
    # bf16 operand planes: the split output is f16 by definition (straight through the C entry point: the wrapper only ever passes its own plane format)
    planes = [torch.zeros(n, D, dtype=torch.bfloat16, device=DEV) for n in (Nq, Nq, Nk, Nk)] + [torch.zeros(D, Nk + 8, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    qh, ql, kh, kl, vh, vl = planes
    out = torch.full((Nq, 3 * D), SENT, dtype=F16, device=DEV)
    p, _ = hip._attn_struct(hip._TC[torch.bfloat16], qh.data_ptr(), kh.data_ptr(), vh.data_ptr(), out, B, H, Nq, Nk, hd, (0, hd, D), (0, hd, D),
                            (0, hd * vh.stride(0), vh.stride(0)), (0, hd, 3 * D), None, None, (0, 0), 1, None, False)
    with pytest.raises(RuntimeError, match='f16 planes'):
        hip._call('pst_attn_x3', p, ql.data_ptr(), kl.data_ptr(), vl.data_ptr(), hip.X3H, D)
    torch.cuda.synchronize()
    assert _untouched(out)
    # out_block < H hd
    prev, hip.X3 = hip.X3, True
    try:
        q, k, vt = rn(1, Nq, D).to(DEV), rn(2, Nk, D).to(DEV), torch.zeros(D, Nk + 8, device=DEV)
        small = torch.full((Nq, 3 * (D - 64)), SENT, dtype=F16, device=DEV)
        with pytest.raises(RuntimeError, match='out_block'):
            hip.attention(q, k, vt, small, B, H, Nq, Nk, hd, (0, hd, D), (0, hd, D), (0, hd * vt.stride(0), vt.stride(0)), (0, hd, 3 * (D - 64)))
    finally:
        hip.X3 = prev
    torch.cuda.synchronize()
    assert _untouched(small)
    # layernorm: a leading dimension that is no multiple of 12 (three blocks of whole 4-column groups)
    Dl = 48
    x, g, b = rn(3, 5, Dl).to(DEV), torch.ones(Dl, device=DEV), torch.zeros(Dl, device=DEV)
    odd = torch.full((5, 3 * Dl + 4), SENT, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match='split'):
        hip.layernorm(x, g, b, odd, 1e-6, split=True)
    torch.cuda.synchronize()
    assert _untouched(odd)
    # groupnorm: groups that are no multiple of 4 channels wide
    C, G, P = 24, 4, 10
    xg, gg, bg = rn(4, P, C).to(DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    st = torch.zeros(hip.stats_buffer(1, G, DEV).shape, device=DEV)
    og = torch.full((P, 3 * C), SENT, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match='split'):
        hip.groupnorm_apply(xg, st, gg, bg, og, 1, P, C, G, 1e-5, False, split=True)
    torch.cuda.synchronize()
    assert _untouched(og)
