"""The small row and pixel kernels at the bottom of csrc/misc.hip and the token gather of csrc/text.hip, called directly at the shapes where their loops
repeat, their lanes idle and their clamps act: l2norm_rows, resize_bilinear and dino_preprocess held element by element to the float64 references of
tests/smallops_ref.py under the bounds derived in tests/errbound.py; mean4, add_cast, patchify, token_embed and attn_mask_from_logits compared exactly.
tests/test_smallops_host.py shows on the CPU, on the same data, that a correct kernel meets each bound and that the planted mistakes do not.

Every output is a view of a larger buffer prefilled with a sentinel - one guard row behind it and, where the row stride exceeds the width, guard columns - which
must be untouched afterwards.  The grid-stride wrap of these kernels is tests/test_hip_large_launch.py's subject: none of its sizes is repeated here.
"""
import pytest
import torch

import errbound as EB
import smallops_ref as SR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32 = torch.float32
SENTINEL = 7.0


@pytest.fixture(params=['bf16', 'f16'])
def fmt(request):
    """the 16-bit storage format under test (PST_BF16 / PST_F16); the tests that take it also run fp32 where the kernel has it"""
    return torch.bfloat16 if request.param == 'bf16' else torch.float16


def guarded(rows, D, ld, dtype, col0=0):
    """-> (buffer [rows + 1, ld] full of the sentinel, its view [rows, D] from column col0 on)"""
    buf = torch.full((rows + 1, ld), 0xA5 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:rows, col0:col0 + D]


def guards_intact(buf, rows, D, col0=0):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:rows, col0:col0 + D] = False
    return bool((buf[keep] == (0xA5 if buf.dtype == torch.uint8 else SENTINEL)).all())


def raises():
    return pytest.raises(RuntimeError, match='failed')


# ------------------------------------------------------------------------------------------------------------------------------------------- l2norm_rows
@pytest.mark.parametrize('D', SR.L2_D)
def test_l2norm_rows(D, fmt):
    """x / (||x|| + eps): D below, at and above the wave width (the column loop takes 1 .. 18 steps, full and partly idle waves), 1 .. 257 rows (blocks with
    1 .. 4 live waves), input and output column slices of wider buffers, eps = 1e-7 (mask_transformer.py:225) and 0 (the class embeddings), a quiet row that
    tells where eps is added, a row with one element of 1e18.
    An all-zero row with eps = 0 is 0 * (1 / 0) = NaN, which is also what the reference's e / e.norm() gives: the product relies on every class embedding
    being non-zero (they are outputs of the text tower's head, or the checkpoint's stored vectors).  Held here as it is: the row is NaN, its neighbours are
    untouched."""
    from panst3r_amd import hip
    for rows in SR.L2_ROWS:
        x = SR.l2norm_case(rows, D)
        xb = torch.full((rows, D + 7), 3.0)
        xb[:, 3:3 + D] = x
        xd = xb.to(DEV)[:, 3:3 + D]
        for eps in (1e-7, 0.0):
            ref = SR.l2norm(x, eps)
            nan_rows = torch.isnan(ref).all(-1)
            assert int(nan_rows.sum()) == (1 if eps == 0.0 and rows >= 5 else 0) and bool(torch.isfinite(ref[~nan_rows]).all())
            for of in (fmt, F32):
                buf, out = guarded(rows, D, D + 5, of)
                hip.l2norm_rows(xd, out, eps)
                got = out.cpu()
                assert bool(torch.isnan(got[nan_rows]).all())
                what = '%d x %d eps %g %s' % (rows, D, eps, of)
                EB.check(got[~nan_rows], ref[~nan_rows], EB.l2norm_bound(ref[~nan_rows], D, of), 'l2norm_rows ' + what)
                # a correct rounding stays below half the bound, except into the format's subnormal range, where tiny(fmt) is the rounding's full size
                normal = (ref.abs() >= torch.finfo(of).tiny) & ~nan_rows[:, None]
                assert EB.check(got[normal], ref[normal], EB.l2norm_bound(ref[normal], D, of), 'l2norm_rows_normal ' + what) <= 0.5
                assert guards_intact(buf, rows, D)


# ------------------------------------------------------------------------------------------------------------------------------------------- attn_mask_from_logits
@pytest.mark.parametrize('Nk', SR.MASK_NK)
def test_attn_mask_from_logits(Nk):
    """mask = logits < 0 with fully blocked rows cleared, exactly: the 256-stride loops take 1 .. 17 steps; rows whose only open key is the last one, or lies
    in the loop's second trip, or is a NaN; -0.0, +-inf and subnormal logits; a logit row stride above Nk whose pad columns hold POSITIVE values (they must
    not keep a blocked row), a mask row stride above Nk.  A second launch into the same buffer gives the same bytes (any_open lives in LDS across a barrier)."""
    from panst3r_amd import hip
    ldl = (Nk + 3) // 4 * 4 + (0 if Nk % 4 else 4)
    ldm = (Nk + 3) // 4 * 4 + 4
    kinds = SR.MASK_KINDS
    cases = [[k] for k in kinds] + [list(kinds[3:9]), [kinds[i % len(kinds)] for i in range(200)]]          # Q = 1 (every kind), 6, 200
    for rows in cases:
        Q = len(rows)
        lg = SR.mask_case(Nk, rows)
        ref = SR.attn_mask(lg)
        lb = torch.full((Q, ldl), 5.0)
        lb[:, :Nk] = lg
        buf, m = guarded(Q, Nk, ldm, torch.uint8)
        hip.attn_mask_from_logits(lb.to(DEV)[:, :Nk], m)
        first = buf.clone()
        assert torch.equal(m.cpu(), ref), (Q, rows[:9])
        assert guards_intact(buf, Q, Nk)
        hip.attn_mask_from_logits(lb.to(DEV)[:, :Nk], m)
        assert torch.equal(buf, first)


# ------------------------------------------------------------------------------------------------------------------------------------------- resize_bilinear
@pytest.mark.parametrize('shape', SR.RESIZE_SHAPES, ids=lambda s: '%dx%d-%dx%d' % s)
def test_resize_bilinear(shape, fmt):
    """identity, a source one pixel high / wide, both axes shrinking / growing by non-integer factors, the older anisotropic shapes; C = 4 (one vector per
    pixel), 32, 100; the 16-bit format and fp32.  Every element under errbound.resize_bound; the identity is exact."""
    from panst3r_amd import hip
    Hs, Ws, Hd, Wd = shape
    n = 2
    for C in SR.RESIZE_C:
        for of in (fmt, F32):
            x = SR.resize_case(Hs, Ws, C, of, n=n)
            r = SR.resize(x, Hd, Wd)
            buf, out = guarded(n * Hd * Wd, C, C, of)
            hip.resize_bilinear(x.to(DEV), out, n, Hs, Ws, Hd, Wd, C)
            got = out.cpu().reshape(n, Hd, Wd, C)
            EB.check(got, r['ref'], SR.resize_bound(r, of), 'resize_bilinear %s C %d %s' % (shape, C, of))
            if (Hs, Ws) == (Hd, Wd):
                assert torch.equal(got, x)
            assert guards_intact(buf, n * Hd * Wd, C)


# ------------------------------------------------------------------------------------------------------------------------------------------- dino_preprocess
@pytest.mark.parametrize('shape', SR.DINO_SHAPES, ids=lambda s: '%dx%d-%dx%d' % s)
def test_dino_preprocess(shape):
    """[-1, 1] -> ImageNet normalise -> bilinear resize, up- and down-scaling, Wo % 4 == 0, Wo % 2 == 0 and odd: at float offsets 0, 1 and 2 of the output the
    launcher picks the widest store the width and the alignment allow (4 / 2 / 1 pixels per thread), all held to the same float64 reference element by
    element and to each other bit for bit"""
    from panst3r_amd import hip
    H, W, Ho, Wo = shape
    n = 2
    img = SR.dino_case(H, W, n=n)
    ref, tapmax, emax = SR.dino_preprocess(img, Ho, Wo)
    bound = EB.resize_bound(ref, tapmax, F32, dtaps=emax)
    N = n * 3 * Ho * Wo
    outs = []
    for off in (0, 1, 2):
        buf = torch.full((N + 8,), SENTINEL, device=DEV)
        out = buf[4 + off:4 + off + N].view(n, 3, Ho, Wo)
        hip.dino_preprocess(img.to(DEV), out)
        EB.check(out.cpu(), ref, bound, 'dino_preprocess %s offset %d' % (shape, off))
        assert bool((buf[:4 + off] == SENTINEL).all()) and bool((buf[4 + off + N:] == SENTINEL).all())
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------------------------------------------------- exact operations
def test_mean4(fmt):
    """0.25 (((a + b) + d) + e) in fp32, rounded once: exact in all three formats, from one float4 per token (C = 4) and one block per image (8 x 8) up"""
    from panst3r_amd import hip
    for of in (fmt, F32):
        for C in (4, 8, 100):
            for (Hm, Wm) in ((8, 8), (16, 24), (40, 8)):
                for nimg in (1, 3):
                    Fm = SR.rn(7000 + C + Hm, nimg, Hm, Wm, C).to(of)
                    T = nimg * (Hm // 8) * (Wm // 8)
                    buf, out = guarded(T, C, C, of)
                    hip.mean4(Fm.to(DEV), out, nimg, Hm, Wm, C)
                    assert torch.equal(out.cpu(), SR.mean4(Fm).reshape(T, C)), (of, C, Hm, Wm, nimg)
                    assert guards_intact(buf, T, C)
    with pytest.raises(RuntimeError, match='share one'):
        hip.mean4(torch.zeros(1, 8, 8, 4, dtype=fmt, device=DEV), torch.zeros(1, 4, device=DEV), 1, 8, 8, 4)


def test_add_cast(fmt):
    """rn(a + b[row % b_mod]) with one fp32 add, exactly: the eight combinations of (a, b, y) in {fp32, 16-bit}, b absent, b_mod 0 / 1 / 5 / rows, one
    vector per row up to 257; a, b and y are column slices of wider buffers with three different row strides"""
    from panst3r_amd import hip
    rows = SR.ADD_ROWS
    for D in SR.ADD_D:
        for fa in (fmt, F32):
            for fy in (fmt, F32):
                for fb in (fmt, F32, None):
                    a, b = SR.add_cast_case(D, fa, fb if fb is not None else F32)
                    ab = torch.full((rows, D + 8), 2.0, dtype=fa)
                    ab[:, 4:4 + D] = a
                    bb = torch.full((rows, D + 12), -2.0, dtype=b.dtype)
                    bb[:, 4:4 + D] = b
                    ad, bd = ab.to(DEV)[:, 4:4 + D], bb.to(DEV)[:, 4:4 + D]
                    for b_mod in (SR.ADD_BMOD if fb is not None else (0,)):
                        buf, y = guarded(rows, D, D + 16, fy, col0=8)
                        hip.add_cast(ad, y, b=bd if fb is not None else None, b_mod=b_mod)
                        assert torch.equal(y.cpu(), SR.add_cast(a, b if fb is not None else None, b_mod, fy)), (D, fa, fb, fy, b_mod)
                        assert guards_intact(buf, rows, D, col0=8)
    a8 = torch.zeros(rows, 8, dtype=fmt, device=DEV)
    with raises():                                                      # D = 6
        hip.add_cast(a8[:, :6], torch.zeros(rows, 8, device=DEV)[:, :6])
    with raises():                                                      # a row stride that is no multiple of 4
        hip.add_cast(torch.zeros(rows, 14, dtype=fmt, device=DEV)[:, :8], torch.zeros(rows, 8, device=DEV))
    with raises():
        hip.add_cast(a8, torch.zeros(rows, 8, device=DEV), b=torch.zeros(rows, 10, device=DEV)[:, :8], b_mod=0)
    with raises():
        hip.add_cast(a8, torch.zeros(rows, 10, device=DEV)[:, :8])


def test_patchify(fmt):
    """img [n, C, H, W] -> patch rows, column (c p + dy) p + dx, exactly: p = 14, 16 and 2, C = 3 and 1, rows without padding and with 8 pad columns
    (zero, written by the kernel's own thread class), the 16-bit format and fp32"""
    from panst3r_amd import hip
    n = 2
    for p in (14, 16, 2):
        for C in (3, 1):
            img = SR.rn(8000 + p + C, n, C, 2 * p, 3 * p)
            T, K = n * 6, C * p * p
            for of in (fmt, F32):
                for ld in (K, K + 8):
                    buf = torch.full((T + 1, ld), SENTINEL, dtype=of, device=DEV)
                    hip.patchify(img.to(DEV), buf[:T], p)
                    assert torch.equal(buf[:T, :K].cpu(), SR.patchify(img, p, of)), (p, C, of, ld)
                    assert int(torch.count_nonzero(buf[:T, K:])) == 0
                    assert bool((buf[T] == SENTINEL).all())
    with raises():                                                      # H no multiple of p
        hip.patchify(torch.zeros(1, 3, 17, 16, device=DEV), torch.zeros(1, 768, dtype=fmt, device=DEV), 16)


@pytest.mark.parametrize('D', SR.TOK_D)
def test_token_embed(D):
    """tok[ids] + pos[l] in fp32, exactly: D = 8 (two live lanes of 64), 256 (one full wave), 768 and 1024 (192 / 256 threads, one trip) and 1152 (the column
    loop's second trip); one token, several short and several full-length sequences; ids with 0, vocab - 1 and repeats; an output row stride above D.
    With ids -1 and `vocab` planted: those rows are zero, every other row is unchanged, status = PST_EINVAL; without, status stays 0."""
    from panst3r_amd import hip
    for (B, L) in SR.TOK_BL:
        ids, tok, pos = SR.token_case(B, L, D)
        ref, status = SR.token_embed(ids, tok, pos)
        assert status == 0
        buf, out = guarded(B * L, D, D + 4, F32)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        hip.token_embed(ids.to(DEV), tok.to(DEV), pos.to(DEV), out, st)
        assert torch.equal(out.cpu(), ref) and int(st.item()) == 0, (B, L)
        assert guards_intact(buf, B * L, D)
        bad = ids.clone()
        bad.view(-1)[0] = -1
        bad.view(-1)[B * L // 2 if B * L > 1 else 0] = SR.TOK_VOCAB
        ref_bad, status = SR.token_embed(bad, tok, pos)
        assert status == -1
        buf, out = guarded(B * L, D, D + 4, F32)
        hip.token_embed(bad.to(DEV), tok.to(DEV), pos.to(DEV), out, st)
        assert torch.equal(out.cpu(), ref_bad) and int(st.item()) == -1, (B, L)          # PST_EINVAL
        assert int(torch.count_nonzero(out[0])) == 0 and int(torch.count_nonzero(out[B * L // 2])) == 0
        assert guards_intact(buf, B * L, D)
    ids, tok, pos = SR.token_case(1, 1, D)
    with raises():                                                      # L > npos
        hip.token_embed(torch.zeros(1, SR.TOK_NPOS + 1, dtype=torch.int32, device=DEV), tok.to(DEV), pos.to(DEV), torch.zeros(SR.TOK_NPOS + 1, D, device=DEV))
