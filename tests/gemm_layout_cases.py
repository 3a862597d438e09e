"""Shared by tests/test_hip_gemm_layout.py (GPU) and tests/test_gemm_layout_checks.py (CPU): the GEMM family (csrc/gemm.hip, gemm256.hip, rowstream.hip,
gemm_f32.hip, maskhead.hip and pst_rowstats) under the leading dimensions and base offsets the model really uses.  Nothing here imports the code under test.

A case names the kernel variant it is meant to reach (the string pst_gemm_variant / pst_gemm_pair_variant returns), how that variant is forced, the epilogue
and store mode, the logical shape and a layout: pads of every leading dimension beyond the logical width and an element offset of every base pointer.
`build(case, fmt)` returns a TIGHT and a PADDED set of buffers with equal logical contents:
  - inputs: every element outside the logical region (pad columns, rows past M, everything before the offset) is NaN - a padding element that reaches a
    multiply-accumulate or an epilogue makes the output NaN;
  - outputs: every element is SENTINEL[dtype], a NaN with a fixed payload (compared as integers), including GUARD rows before and after; every buffer is
    allocated in full, so a small overrun lands in memory the test owns and is reported.
A buffer (`Buf`) knows the flat index of every logical element inside its allocation (`idx`, in GEMM coordinates [.., m, n]), so every store mode - row
remap, transposed, pixel shuffle, split store, strided batch - is compared in the same [M, N] coordinates as `reference(problem)`, the float64 restatement
of the operation (the expressions of tests/test_hip_ops.py).  `check_bits` / `check_outside` / `check_no_nan` are the checks (b), (c), (d) of the GPU
module; the CPU module runs them on a numpy emulation with planted mistakes.

Where the argument rules leave no room for the shape the table would like, the nearest admitted one is used: a 16-bit residual needs ldr % 8 == 0 in the
tight set too, so its cases use N = 104 / 264 for 100 / 260; the tight transposed store rounds M up to the next multiple of 8 (ldc % 8 of the persistent
class).  Where it is the padded layout itself that sends a problem to its variant (gemm256_kernel through 8-byte rows of C, the tiled kernels one step
outside a row-streaming class), the tight set necessarily runs on the class that was refused: the case names that kernel as `tight_variant`, and the
bit identity then also holds the two kernels to each other."""
import math

import torch
import torch.nn.functional as F

GUARD = 64                                   # guard rows before and after every padded output
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENTINEL = {F32: 0x7FD5A5A5, BF16: 0x7FB6, F16: 0x7E5A}       # NaNs with distinct payloads; never compared as floats
_INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
_SIZE = {F32: 4, BF16: 2, F16: 2}


def bits(t):
    """the storage bits of a float tensor, as integers of the same width"""
    return t.contiguous().view(_INT[t.dtype])


class Buf:
    """one operand inside its allocation: `alloc` 1-D (everything the test owns), the view handed to the kernel = alloc.as_strided(shape, strides, base),
    `idx` = flat index into alloc of every logical element (in GEMM coordinates), `out` = written by the kernel"""

    def __init__(self, alloc, base, shape, strides, idx, out, ld):
        self.alloc, self.base, self.shape, self.strides, self.idx, self.out, self.ld = alloc, base, tuple(shape), tuple(strides), idx, out, ld

    def view(self):
        return self.alloc.as_strided(self.shape, self.strides, self.base)

    def logical(self):
        return self.alloc[self.idx]

    def to(self, dev, idx=None):
        return Buf(self.alloc.to(dev, copy=True), self.base, self.shape, self.strides, self.idx.to(dev) if idx is None else idx, self.out, self.ld)

    def outside_mask(self):
        m = torch.ones(self.alloc.numel(), dtype=torch.bool, device=self.alloc.device)
        m[self.idx.reshape(-1)] = False
        return m


def _filled(n, dtype, out):
    if out:
        return torch.full((n,), SENTINEL[dtype], dtype=_INT[dtype]).view(dtype)
    return torch.full((n,), float('nan'), dtype=dtype)


def make_buf(values, idx, size, base, shape, strides, dtype, out, ld):
    """allocation of `size` elements, poisoned (input) or sentinel-filled (output), with `values` (or nothing) at idx"""
    alloc = _filled(size, dtype, out)
    assert int(idx.min()) >= 0 and int(idx.max()) < size
    if values is not None:
        alloc[idx.reshape(-1)] = values.to(dtype).reshape(-1)
    return Buf(alloc, base, shape, strides, idx, out, ld)


def rows_buf(values, rows, cols, ld, off, dtype, out, row_index=None, nrows_alloc=None, guard=0):
    """a row-major [rows_alloc, cols] operand with leading dimension ld whose first element sits `off` elements (plus `guard` rows) into its allocation;
    logical element (i, j) lives in row row_index[i] (identity by default).  A few poisoned / sentinel rows follow the last one."""
    nrows_alloc = rows if nrows_alloc is None else nrows_alloc
    base = guard * ld + off
    r = torch.arange(rows) if row_index is None else row_index
    idx = base + r[:, None] * ld + torch.arange(cols)[None]
    size = base + (nrows_alloc + max(guard, 8)) * ld
    return make_buf(values, idx, size, base, (nrows_alloc, cols), (ld, 1), dtype, out, ld)


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rope_table(npos, hd=64, base=100.0):
    """fp32 [npos, hd / 4, 2] (cos, sin) of RoPE-2D, as the model builds it"""
    D = hd // 2
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=F32) / D))
    ang = torch.outer(torch.arange(npos, dtype=F32), inv)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous()


def up(x, m):
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------------------------------------------------------------------- the cases
LAYOUT_KEYS = ('pad_a', 'pad_w', 'pad_c', 'pad_r', 'pad_x', 'pad_s', 'off_a', 'off_w', 'off_c', 'off_r', 'off_x')


def P(M, N, K, out='16', mode='plain', **kw):
    """one GEMM problem: out '16' / 'f32'; mode plain / trans / ps / conv / x3; epilogue bias / act / gamma / res ('f32' / '16') / inplace / grp / ln /
    producer (xcopy + stats: 'xs', stats only: 's') / rope; batch; the layout keys"""
    d = dict(M=M, N=N, K=K, out=out, mode=mode, bias=True, act=None, gamma=False, res=None, inplace=False, grp=None, ln=False, producer=None, rope=False,
             batch=0, ps=None, conv=None, x3_block=0, seed=1, f32=False)
    d.update({k: 0 for k in LAYOUT_KEYS})
    d.update(kw)
    return d


def case(name, variant, problem, kernel=0, tune=None, anchor=False, tight_variant=None, fmts=('bf16', 'f16'), kind='gemm', store=None):
    problems = problem if isinstance(problem, list) else [problem]
    for p in problems:
        p['kernel'] = kernel
    return dict(name=name, variant=variant, problems=problems, kernel=kernel, tune=tune or {}, anchor=anchor, tight_variant=tight_variant or variant, fmts=fmts, kind=kind,
                store=store or problems[0]['mode'] + ('-f32' if problems[0]['out'] == 'f32' else '-16'))


TUNE_DEEP_RING, TUNE_CUS = 8, 10             # PST_TUNE_* of include/panst3r_hip.h


def _tile_family(tag, variant, kernel, M, N, K, Np, Mg, grp):
    """the row-major epilogues every tile kernel must serve, at its smallest multi-tile shape (Np: the N of the fold producer, a multiple of 64; Mg, grp:
    the rows and the (grp_in, grp_out, grp_off) of the remap cases - more than one group, with a group boundary inside a tile)"""
    Nr = up(N, 8)                            # a 16-bit residual needs ldr % 8 == 0, in the tight set too
    pc16 = 4 if N % 8 == 0 else 8            # the 16-bit pad_c with ldc % 8 == 4
    pc16a = 8 if N % 8 == 0 else 4           # ... and with ldc % 8 == 0
    c = lambda n, p, **k: case('%s_%s' % (tag, n), variant, p, kernel=kernel, **k)
    return [
        c('plain16', P(M, N, K, bias=False, pad_a=8, pad_w=8, pad_c=pc16, off_a=8, off_w=8, off_c=4), anchor=True),
        c('plain16_ldc24', P(M, N, K, bias=False, pad_a=72, pad_c=24, off_w=8)),
        c('plain32', P(M, N, K, out='f32', bias=False, pad_a=72, pad_w=8, pad_c=4, off_a=8, off_c=4)),
        c('gelu16', P(M, N, K, act='gelu', pad_a=72, pad_w=8, pad_c=pc16a, off_w=8)),
        c('gelu32', P(M, N, K, out='f32', act='gelu', pad_a=8, pad_c=12, off_a=8, off_c=4)),
        c('gamma_res32_inplace', P(M, N, K, out='f32', gamma=True, res='f32', inplace=True, pad_a=8, pad_w=8, pad_c=4, off_c=4), anchor=True),
        c('gamma_res32_apart', P(M, N, K, out='f32', gamma=True, res='f32', pad_a=8, pad_c=12, pad_r=4, off_a=8, off_r=4)),
        c('gamma_res32_out16', P(M, N, K, gamma=True, res='f32', pad_a=8, pad_c=pc16, pad_r=4, off_a=8, off_c=4)),
        c('remap_res32_inplace', P(Mg, N, K, out='f32', res='f32', inplace=True, grp=grp, pad_a=8, pad_c=4, off_a=8, off_c=4)),
        # 16-bit, no residual, ldc % 8 == 0, 16-byte aligned C: the interior fast store of every tile kernel, with its incremental remap
        c('remap16', P(Mg, Np, K, act='gelu', grp=grp, pad_a=8, pad_w=8, pad_c=8, off_a=8, off_c=8)),
        c('rope_remap16', P(Mg, Np, K, rope=True, gamma=True, grp=grp, pad_a=8, pad_c=24, off_w=8, off_c=8)),
        c('res16_inplace', P(M, Nr, K, res='16', inplace=True, pad_a=8, pad_w=8, pad_c=8, off_a=8)),
        c('res16_apart', P(M, Nr, K, res='16', pad_a=72, pad_c=4, pad_r=8, off_c=4, off_r=8)),
        c('fold_consumer', P(M, N, K, ln=True, act='gelu', pad_a=8, pad_w=8, pad_c=pc16, off_a=8, off_c=4), anchor=True),
        c('fold_producer', P(M, Np, K, out='f32', res='f32', inplace=True, producer='xs', pad_a=8, pad_c=4, pad_x=4, pad_s=1, off_a=8, off_c=4, off_x=4)),
        c('fold_producer16', P(M, Np, K, res='16', inplace=True, producer='s', pad_a=8, pad_w=8, pad_c=8, pad_s=1, off_a=8, off_w=8)),
        c('fold_producer_x8', P(M, Np, K, out='f32', res='f32', inplace=True, producer='xs', pad_a=72, pad_w=8, pad_c=12, pad_x=8, pad_s=1, off_w=8)),
    ]


def _cases():
    cs = []
    cs += _tile_family('t64', 'gemm_kernel<2,2,false>', 0, 200, 100, 128, 128, 200, (100, 108, 3))
    cs += _tile_family('t128', 'gemm_kernel<4,4,false>', 128, 257, 260, 64, 320, 258, (129, 137, 3))
    # gemm256_kernel: everything the persistent classes refuse - a 16-bit C with ldc % 8 == 4, an fp32 C without a residual, a residual stream with
    # N % 256 != 0, 16-bit residuals, a row remap; and below N = 260.  Its interior fast store (16-bit, no residual, ldc % 8 == 0, 16-byte aligned C) is
    # reached where the persistent class refuses for another reason: a row remap (t256_remap16, t256_rope_remap16, t256_plain16_remap) or N % 64 != 0 (t256_n260)
    fam = _tile_family('t256', 'gemm256_kernel', 256, 513, 320, 128, 320, 513, (171, 179, 3))
    for c in fam:                             # the two entries the persistent class 1 would take: give them the 8-byte rows it refuses
        if c['name'] in ('t256_plain16_ldc24', 't256_gelu16'):
            c['problems'][0].update(pad_c=4, off_c=4)
        if c['name'] in ('t256_plain16', 't256_plain16_ldc24', 't256_gelu16', 't256_fold_consumer'):
            c['tight_variant'] = 'gemm256p_kernel'
    cs += fam
    cs.append(case('t256_n260', 'gemm256_kernel', P(513, 260, 128, act='gelu', pad_a=8, pad_w=8, pad_c=4, off_a=8, off_c=8), kernel=256, anchor=True))
    cs.append(case('t256_plain16_remap', 'gemm256_kernel', P(513, 320, 128, bias=False, grp=(171, 179, 3), pad_a=72, pad_c=24, off_w=8, off_c=8), kernel=256))
    # transposed store on the 64 / 128 tiles: ldc = roundup8(M) + 8
    cs.append(case('t64_trans', 'gemm_kernel<2,2,true>', P(200, 100, 128, mode='trans', pad_a=8, pad_w=8, pad_c=8, off_a=8, off_w=8, off_c=4), anchor=True))
    cs.append(case('t128_trans', 'gemm_kernel<4,4,true>', P(257, 260, 64, mode='trans', act='gelu', pad_a=72, pad_w=8, pad_c=8, off_a=8), kernel=128, anchor=True))
    cs.append(case('t128_trans_fold', 'gemm_kernel<4,4,true>', P(257, 260, 64, mode='trans', ln=True, pad_a=8, pad_c=8, off_c=4), kernel=128))
    # the deep LDS rings of the 64 x 64 tiles
    for depth in (6, 8):
        cs.append(case('t64_ring%d' % depth, 'gemm_kernel<2,2,false>', P(200, 128, 512, act='gelu', pad_a=72, pad_w=8, pad_c=4, off_a=8, off_w=8, off_c=4),
                       tune={TUNE_DEEP_RING: depth}, anchor=depth == 8))
        cs.append(case('t64_ring%d_res32' % depth, 'gemm_kernel<2,2,false>',
                       P(200, 128, 512, out='f32', res='f32', inplace=True, producer='xs', pad_a=8, pad_c=4, pad_x=8, pad_s=1, off_c=4), tune={TUNE_DEEP_RING: depth}))
    # the persistent 256 x 256 kernel, its three classes; 4 workgroups for 6 tiles (2 for 3): some of them walk to a second tile
    few = {TUNE_CUS: 4}
    cs.append(case('p256_plain16', 'gemm256p_kernel', P(513, 320, 128, act='gelu', pad_a=72, pad_w=8, pad_c=8, off_a=8, off_w=8, off_c=8), kernel=256, tune=few, anchor=True))
    cs.append(case('p256_fold_consumer', 'gemm256p_kernel', P(513, 320, 128, ln=True, act='gelu', pad_a=8, pad_c=8, off_a=8, off_c=8), kernel=256, tune=few, anchor=True))
    cs.append(case('p256_res32', 'gemm256p_kernel', P(513, 256, 128, out='f32', gamma=True, res='f32', inplace=True, producer='xs', pad_a=8, pad_w=8, pad_c=4, pad_x=8,
                                                      pad_s=1, off_a=8, off_c=4, off_x=8), kernel=256, tune={TUNE_CUS: 2}, anchor=True))
    cs.append(case('p256_res32_apart', 'gemm256p_kernel', P(513, 256, 128, out='f32', res='f32', producer='xs', pad_a=72, pad_c=12, pad_r=4, pad_x=8, pad_s=1, off_r=4),
                   kernel=256, tune={TUNE_CUS: 2}))
    cs.append(case('p256_trans', 'gemm256p_kernel', P(513, 320, 128, mode='trans', act='gelu', pad_a=8, pad_w=8, pad_c=8, off_a=8, off_c=8), kernel=256, tune=few, anchor=True))
    # the row-streaming kernel at its lower limit, and one step outside each of its classes (bit-identical on a tiled kernel)
    rs = lambda **k: P(16384, 384, 384, seed=7, **k)
    cs.append(case('rs_plain', 'rowgemm384_kernel', rs(act='gelu', pad_c=8, off_c=8), anchor=True))
    cs.append(case('rs_fold_consumer', 'rowgemm384_kernel', rs(ln=True, act='gelu', pad_c=8, off_w=8)))
    cs.append(case('rs_res16', 'rowgemm384_kernel', rs(res='16', producer='s', pad_c=8, pad_s=1, off_c=8, off_r=8), anchor=True))
    cs.append(case('rs_plain_lda392', 'gemm_kernel<4,4,false>', rs(act='gelu', pad_a=8, pad_c=8, off_c=8), tight_variant='rowgemm384_kernel'))
    cs.append(case('rs_plain_c8byte', 'gemm_kernel<4,4,false>', rs(act='gelu', pad_c=8, off_c=4), tight_variant='rowgemm384_kernel'))
    cs.append(case('rs_res16_ldr392', 'gemm_kernel<4,4,false>', rs(res='16', producer='s', pad_c=8, pad_r=8, pad_s=1, off_c=8, off_r=8), tight_variant='rowgemm384_kernel'))
    # two problems in one launch
    cs.append(case('pair64', 'gemm_pair_kernel<2,2>', [P(200, 128, 128, ln=True, act='gelu', pad_a=8, pad_w=8, pad_c=4, off_a=8, off_c=4),
                                                       P(200, 64, 128, mode='trans', ln=True, seed=2, pad_a=8, pad_w=8, pad_c=8, off_a=8, off_w=8)], kind='pair', anchor=True))
    cs.append(case('pair256p', 'gemm256p2_kernel', [P(26112, 1024, 1024, act='gelu', seed=3, pad_a=8, pad_w=8, pad_c=8, off_c=8),
                                                    P(38800, 1024, 1024, act='gelu', seed=4, pad_a=72, pad_c=24, off_a=8, off_w=8)], kind='pair', anchor=True))
    # strided batch: three problems further apart than one problem is long
    cs.append(case('batch_plain', 'gemm_kernel<2,2,false>', P(200, 100, 128, batch=3, act='gelu', pad_a=8, pad_w=8, pad_c=8, off_a=8, off_c=4), anchor=True, store='batch-16'))
    cs.append(case('batch_trans', 'gemm_kernel<2,2,true>', P(200, 100, 128, mode='trans', batch=3, pad_a=72, pad_w=8, pad_c=8, off_w=8), store='batch-trans'))
    # implicit 3 x 3 convolution, pixel-shuffle store, split store
    cs.append(case('conv3x3', 'gemm_kernel<2,2,false>', P(70, 100, 576, out='f32', mode='conv', conv=(64, 5, 7), pad_w=8, pad_c=4, off_a=8, off_w=8, off_c=4), anchor=True))
    cs.append(case('conv3x3_16', 'gemm_kernel<2,2,false>', P(70, 100, 576, mode='conv', conv=(64, 5, 7), act='relu', pad_w=8, pad_c=8, off_c=4)))
    cs.append(case('pixel_shuffle16', 'gemm_kernel<2,2,false>', P(30, 48, 64, mode='ps', ps=(2, 12, 3, 5), pad_a=8, pad_w=8, off_a=8, off_w=8, off_c=4), anchor=True))
    cs.append(case('pixel_shuffle32', 'gemm_kernel<4,4,false>', P(30, 48, 64, out='f32', mode='ps', ps=(2, 12, 3, 5), pad_a=72, pad_w=8, off_c=4), kernel=128))
    cs.append(case('split_store', 'gemm_kernel<2,2,false>', P(200, 100, 128, out='f32', mode='x3', x3_block=104, act='gelu', pad_a=8, pad_w=8, pad_c=8, off_a=8, off_c=8),
                   fmts=('f16',)))
    # fused RoPE
    cs.append(case('rope_t64', 'gemm_kernel<2,2,false>', P(200, 128, 128, rope=True, gamma=True, pad_a=8, pad_w=8, pad_c=8, off_a=8)))
    cs.append(case('rope_t64_c8byte', 'gemm_kernel<2,2,false>', P(200, 128, 128, rope=True, pad_a=72, pad_c=4, off_c=4)))
    cs.append(case('rope_t128', 'gemm_kernel<4,4,false>', P(257, 320, 64, rope=True, pad_a=8, pad_c=24, off_a=8, off_w=8), kernel=128))
    cs.append(case('rope_p256', 'gemm256p_kernel', P(513, 320, 128, rope=True, gamma=True, pad_a=8, pad_w=8, pad_c=8, off_a=8, off_c=8), kernel=256, tune=few))
    # fp32 operands: gemm_f32_validate wants lda / ldw / ldc / ldr % 4 and 16-byte aligned A, W, C, res
    cs.append(case('f32_plain', 'gemm_f32_kernel', P(200, 100, 64, out='f32', f32=True, act='gelu', pad_a=4, pad_w=4, pad_c=4, off_a=4, off_w=4, off_c=4),
                   fmts=('f32',), anchor=True))
    cs.append(case('f32_res_remap', 'gemm_f32_kernel', P(200, 100, 64, out='f32', f32=True, gamma=True, res='f32', inplace=True, grp=(100, 108, 3), pad_a=12, pad_c=12,
                                                         off_a=4, off_c=4), fmts=('f32',), anchor=True))
    cs.append(case('f32_res_apart', 'gemm_f32_kernel', P(200, 100, 64, out='f32', f32=True, res='f32', pad_a=4, pad_c=4, pad_r=12, off_r=4), fmts=('f32',)))
    return cs


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)

MASK_HEAD_CASES = [dict(name='mask_head_256', C=256, Q=130, P=64, n=3), dict(name='mask_head_384', C=384, Q=24, P=128, n=2)]
ROWSTATS_CASES = [dict(name='rowstats_%d' % D, D=D, rows=70) for D in (128, 384)]


def fmt_dtype(fmt):
    return {'bf16': BF16, 'f16': F16, 'f32': F32}[fmt]


def describe(c):
    out = []
    for p in c['problems']:
        lay = ' '.join('%s=%d' % (k, p[k]) for k in LAYOUT_KEYS if p[k])
        out.append('%dx%dx%d %s/%s%s [%s]' % (p['M'], p['N'], p['K'], p['mode'], p['out'], ' batch=%d' % p['batch'] if p['batch'] else '', lay))
    return '%s -> %s (kernel=%d tune=%s): %s' % (c['name'], c['variant'], c['kernel'], c['tune'], ' | '.join(out))


# -------------------------------------------------------------------------------------------------------------------------------------- the builder
def out_rows(p):
    """(row of C that GEMM row m is stored to, rows of the C buffer)"""
    M = p['M']
    m = torch.arange(M)
    if p['grp']:
        gi, go, goff = p['grp']
        return (m // gi) * go + goff + m % gi, (M // gi) * go
    return m, M


def logical_values(p, fmt):
    """the logical contents of every operand of a problem: the same for the tight and the padded set, whatever the layout (seeded by shape and p['seed'])"""
    d16 = fmt_dtype(fmt)
    op = F32 if p['f32'] else d16
    M, N, K, s = p['M'], p['N'], p['K'], 1000 * p['seed']
    nb = max(1, p['batch'])
    v = {}
    if p['ln']:
        x = rnd(s + 5, M, K) * 1.7 + 0.4
        x[:, 5] += 6.0                                             # an outlier channel, as ViT residual streams have
        v['x'] = x
        v['a'] = x.to(d16)
        g = x.reshape(M, K // 64, 64)
        v['ln_stats'] = torch.stack([g.sum(-1), (g * g).sum(-1)], -1).contiguous()
    elif p['conv']:
        cc, ch, cw = p['conv']
        v['a'] = rnd(s + 1, M, cc).to(op)                           # NHWC image stack, M = images * ch * cw
    else:
        v['a'] = rnd(s + 1, nb, M, K).to(op) if p['batch'] else rnd(s + 1, M, K).to(op)
    v['w'] = (rnd(s + 2, nb, N, K, scale=K ** -0.5) if p['batch'] else rnd(s + 2, N, K, scale=K ** -0.5)).to(op)
    if p['ln']:
        v['colsum'] = v['w'].float().sum(1).contiguous()
    if p['bias']:
        v['bias'] = rnd(s + 3, nb, N, scale=0.1) if p['batch'] else rnd(s + 3, N, scale=0.1)
    if p['gamma']:
        v['gamma'] = 1 + 0.1 * rnd(s + 4, N)
    if p['res']:
        v['res'] = rnd(s + 6, M, N).to(F32 if p['res'] == 'f32' else d16)
    if p['rope']:
        g = torch.Generator().manual_seed(s + 7)
        v['pos'] = torch.randint(0, 32, (M, 2), generator=g, dtype=torch.int32)
        v['table'] = rope_table(32)
    return v


def c_index(p, ldc, base, c_bs=0):
    """flat index of GEMM element (m, n) (x3: [block, m, n]; batch: [b, m, n]) inside the C allocation - the header's store rules"""
    M, N = p['M'], p['N']
    m, n = torch.arange(M)[:, None], torch.arange(N)[None]
    if p['mode'] == 'trans':
        idx = base + n * ldc + m
    elif p['mode'] == 'ps':
        pp, pc, ph, pw = p['ps']
        seg = pp * pc
        hw = ph * pw
        v_, t = m // hw, m % hw
        y, x = t // pw, t % pw
        dy, r = n // seg, n % seg
        idx = base + ((v_ * pp * ph + pp * y + dy) * pw + x) * seg + r          # C[v][p y + dy][(p x) c + r] of a contiguous [V, p h, p w, c]
    else:
        orow, _ = out_rows(p)
        idx = base + orow[:, None] * ldc + n
    if p['mode'] == 'x3':
        idx = torch.stack([idx, idx + p['x3_block'], idx + 2 * p['x3_block']])
    if p['batch']:
        idx = torch.stack([idx + b * c_bs for b in range(p['batch'])])
    return idx


def build_problem(p, fmt, padded, shared=None):
    """the buffers of one problem: dict of Buf (a, w, c, res, xcopy, stats) + plain tensors (bias, gamma, ln_stats, colsum, pos, table) + strides"""
    d16 = fmt_dtype(fmt)
    op = F32 if p['f32'] else d16
    L = {k: (p[k] if padded else 0) for k in LAYOUT_KEYS}
    guard = GUARD if padded else 0
    M, N, K, nb = p['M'], p['N'], p['K'], max(1, p['batch'])
    v = logical_values(p, fmt)
    if shared is not None:                                          # one A view for both problems of a pair (and its statistics, for a fold consumer)
        for k in ('x', 'a', 'ln_stats'):
            if k in shared['vals']:
                v[k] = shared['vals'][k]
    s = dict(p=p, fmt=fmt, padded=padded, vals=v)
    # ---- A
    if shared is not None:
        s['a'] = shared['a']
    elif p['conv']:
        cc = p['conv'][0]
        s['a'] = rows_buf(v['a'], M, cc, cc, L['off_a'], op, False)
    elif p['batch']:
        lda = K + L['pad_a']
        a_bs = M * lda + (64 if padded else 0)
        idx = L['off_a'] + torch.arange(nb)[:, None, None] * a_bs + torch.arange(M)[None, :, None] * lda + torch.arange(K)[None, None]
        s['a'] = make_buf(v['a'], idx, L['off_a'] + nb * a_bs + 8 * lda, L['off_a'], (M, K), (lda, 1), op, False, lda)
        s['a_bs'] = a_bs
    else:
        s['a'] = rows_buf(v['a'], M, K, K + L['pad_a'], L['off_a'], op, False)
    # ---- W
    ldw = K + L['pad_w']
    if p['batch']:
        w_bs = N * ldw + (64 if padded else 0)
        idx = L['off_w'] + torch.arange(nb)[:, None, None] * w_bs + torch.arange(N)[None, :, None] * ldw + torch.arange(K)[None, None]
        s['w'] = make_buf(v['w'], idx, L['off_w'] + nb * w_bs + 8 * ldw, L['off_w'], (N, K), (ldw, 1), op, False, ldw)
        s['w_bs'] = w_bs
    else:
        s['w'] = rows_buf(v['w'], N, K, ldw, L['off_w'], op, False)
    # ---- C
    cdt = F16 if p['mode'] == 'x3' else (F32 if p['out'] == 'f32' else d16)
    orow, nrows = out_rows(p)
    if p['mode'] == 'trans':
        ldc = up(M, 8) + L['pad_c']
        shape, crow = (N, ldc), N
    elif p['mode'] == 'ps':
        pp, pc, ph, pw = p['ps']
        ldc = pp * pw * pc                                          # one output pixel row; the kernel gets ldc = 0
        shape, crow = (M // (ph * pw) * pp * ph, ldc), M // (ph * pw) * pp * ph
    elif p['mode'] == 'x3':
        ldc = 3 * p['x3_block'] + L['pad_c']
        shape, crow = (nrows, 3 * p['x3_block']), nrows
    else:
        ldc = N + L['pad_c']
        shape, crow = (nrows, N), nrows
    cbase = guard * ldc + L['off_c']
    c_bs = crow * ldc + (64 if padded else 0) if p['batch'] else 0
    cidx = c_index(p, ldc, cbase, c_bs)
    size = cbase + (nb - 1) * c_bs + (crow + max(guard, 8)) * ldc
    init = None
    if p['res'] and p['inplace']:
        init = v['res']
    s['c'] = make_buf(init, cidx, size, cbase, shape, (ldc, 1), cdt, True, ldc)
    s['c_bs'] = c_bs
    if p['batch']:
        s['bias_bs'] = N + (4 if padded else 0)
        b = torch.full((nb * s['bias_bs'] + 8,), float('nan'))
        for i in range(nb):
            b[i * s['bias_bs']: i * s['bias_bs'] + N] = v['bias'][i]
        s['bias_alloc'] = b
    # ---- residual apart from C
    if p['res'] and not p['inplace']:
        rdt = F32 if p['res'] == 'f32' else d16
        s['res'] = rows_buf(v['res'], M, N, N + L['pad_r'], L['off_r'], rdt, False, row_index=orow, nrows_alloc=nrows)
    # ---- fold producer outputs
    if p['producer']:
        if 'x' in p['producer']:
            s['xcopy'] = rows_buf(None, M, N, N + L['pad_x'], L['off_x'], d16, True, row_index=orow, nrows_alloc=nrows, guard=guard)
        sld = N // 64 + L['pad_s']
        base = guard * sld * 2
        idx = base + orow[:, None, None] * (sld * 2) + torch.arange(N // 64)[None, :, None] * 2 + torch.arange(2)[None, None]
        s['stats'] = make_buf(None, idx, base + (nrows + max(guard, 8)) * sld * 2, base, (nrows, sld, 2), (sld * 2, 2, 1), F32, True, sld)
    return s


def build(c, fmt, padded):
    """the buffer sets of a case's problems (a pair shares one A between its problems, as the q|k and V^T projections do)"""
    sets = []
    for i, p in enumerate(c['problems']):
        share = sets[0] if (i == 1 and c['name'] == 'pair64') else None
        sets.append(build_problem(p, fmt, padded, share))
    return sets


def to_device(s, dev, like=None):
    """a fresh device copy of a buffer set (in-place residual cases are consumed by a launch); `like`: an earlier copy of the same set whose index tensors
    are shared"""
    d = dict(s)
    for k in ('a', 'w', 'c', 'res', 'xcopy', 'stats'):
        if k in s:
            d[k] = s[k].to(dev, None if like is None else like[k].idx)
    d['vals'] = {k: (t.to(dev) if k in ('bias', 'gamma', 'ln_stats', 'colsum', 'pos', 'table') else t) for k, t in s['vals'].items()}
    if 'bias_alloc' in s:
        d['bias_alloc'] = s['bias_alloc'].to(dev)
    return d


def call_args(s):
    """(a, w, out, kwargs) in the vocabulary of panst3r_amd.hip._gemm_params"""
    p, v = s['p'], s['vals']
    kw = dict(kernel=p['kernel'], act=p['act'])
    if p['bias']:
        kw['bias'] = s['bias_alloc'][:p['N']] if p['batch'] else v['bias']
    if p['gamma']:
        kw['gamma'] = v['gamma']
    if p['res']:
        kw['res'] = s['c'].view() if p['inplace'] else s['res'].view()
    if p['grp']:
        kw['grp'] = p['grp']
    if p['ln']:
        kw['ln'] = (v['ln_stats'], v['colsum'], 1e-6)
    if p['rope']:
        kw['rope'] = (v['pos'], v['table'])
    if p['mode'] == 'trans':
        kw['trans_out'] = True
    if p['mode'] == 'ps':
        kw['ps'] = p['ps']
    if p['mode'] == 'conv':
        kw['conv'] = p['conv']
    if p['mode'] == 'x3':
        kw['x3_block'] = p['x3_block']
    if p['batch']:
        kw['batch'] = (p['batch'], s['a_bs'], s['w_bs'], s['c_bs'], s['bias_bs'])
    if 'xcopy' in s:
        kw['xcopy'] = s['xcopy'].view()
    if 'stats' in s:
        kw['stats_out'] = s['stats'].view()
    return s['a'].view(), s['w'].view(), s['c'].view(), kw


def outputs(s):
    return [(k, s[k]) for k in ('c', 'xcopy', 'stats') if k in s]


# ------------------------------------------------------------------------------------------------------------------------------------ the reference
def ln_core(v, eps=1e-6):
    """LayerNorm folded into the consumer (include/panst3r_hip.h): rstd (x_c W^T - mean colsum), statistics of the fp32 rows"""
    x64 = v['x'].double()
    mean = x64.mean(-1, keepdim=True)
    var = (x64 * x64).mean(-1, keepdim=True) - mean * mean
    r = (var + eps).rsqrt()
    raw = v['a'].double() @ v['w'].double().T
    return r * raw - (mean * r) * v['colsum'].double()[None]


def core(p, v, dev='cpu', absolute=False):
    """float64 A W^T of a problem [.., M, N] (implicit convolution: of the image stack; fold consumer: ln_core); absolute: of |A| and |W|, the sum the
    accumulator's error bound scales with"""
    t = (lambda k: v[k].to(dev).double().abs()) if absolute else (lambda k: v[k].to(dev).double())
    if p['ln']:
        assert not absolute
        return ln_core({k: x.to(dev) for k, x in v.items() if k in ('x', 'a', 'w', 'colsum')})
    if p['conv']:
        cc, ch, cw = p['conv']
        x = t('a').reshape(-1, ch, cw, cc)
        wt = t('w').reshape(p['N'], 3, 3, cc).permute(0, 3, 1, 2)             # K is tap-major, channel-minor
        return F.conv2d(x.permute(0, 3, 1, 2), wt, padding=1).permute(0, 2, 3, 1).reshape(p['M'], p['N'])
    return t('a') @ t('w').transpose(-1, -2)


def reference(p, v, dev='cpu'):
    """float64 value of every GEMM element [.., M, N] (the stored value before the rounding to the output format; split store: the fp32 value whose
    (hi, lo) halves are stored).  RoPE: the value before the rotation."""
    t = lambda k: v[k].to(dev).double()
    y = core(p, v, dev)
    if p['bias']:
        y = y + (t('bias')[:, None, :] if p['batch'] else t('bias'))
    if p['act'] == 'gelu':
        y = F.gelu(y)
    elif p['act'] == 'relu':
        y = F.relu(y)
    if p['gamma']:
        y = y * t('gamma')
    if p['res']:
        y = y + t('res')
    return y


# ---------------------------------------------------------------------------------------------------------------------------------------- the checks
def _where(buf, flat):
    rel = int(flat) - buf.base
    return rel // buf.ld, rel % buf.ld


def _hex(b, i):
    return '%#x' % (int(b[i]) & ((1 << (8 * b.element_size())) - 1))


def check_bits(name, tight, padded):
    """(b) the logical region of the padded call equals that of the tight call, bit for bit"""
    a, b = bits(tight.logical()), bits(padded.logical())
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError('%s: %d logical elements differ between the tight and the padded call, first at %s: tight bits %s, padded bits %s'
                             % (name, len(bad), tuple(int(i) for i in bad[0]), _hex(a, tuple(bad[0])), _hex(b, tuple(bad[0]))))


def check_outside(name, buf):
    """(c) every element outside the logical region still holds the sentinel's bits"""
    b = bits(buf.alloc)
    bad = ((b != SENTINEL[buf.alloc.dtype]) & buf.outside_mask()).nonzero()
    if len(bad):
        row, col = _where(buf, bad[0, 0])
        raise AssertionError('%s: %d elements outside the logical region were written, first at (row %d, column %d) of the view (ld %d), bits %s'
                             % (name, len(bad), row, col, buf.ld, _hex(b, bad[0, 0])))


def check_no_nan(name, buf):
    """(d) no NaN in the logical region: neither poison that was read nor a sentinel that was never overwritten"""
    lg = buf.logical()
    nan = torch.isnan(lg)
    if bool(nan.any()):
        bad = nan.nonzero()
        left = int((bits(lg)[nan] == SENTINEL[lg.dtype]).sum())
        raise AssertionError('%s: %d NaN in the logical region (%d of them the untouched sentinel), first at %s'
                             % (name, len(bad), left, tuple(int(i) for i in bad[0])))


def check_same_bytes(name, first, second):
    """the same launch twice: the whole allocation, byte for byte"""
    assert torch.equal(bits(first.alloc), bits(second.alloc)), '%s: two launches of the same padded call differ' % name


# ------------------------------------------------------------------------------------------------------------- mask head and rowstats (no GEMM params)
def build_mask_head(mc, fmt, padded):
    """E [Q, C] (lde), F [n][P][C] (view stride), out fp32 [n][Q][P] (view stride) of pst_mask_head"""
    d16 = fmt_dtype(fmt)
    C, Q, Pn, n = mc['C'], mc['Q'], mc['P'], mc['n']
    lde = C + (8 if padded else 0)
    fvs = Pn * C + (64 if padded else 0)
    ovs = Q * Pn + (64 if padded else 0)
    off = 8 if padded else 0
    E, Fv = rnd(41, Q, C), rnd(42, n, Pn, C)
    e = rows_buf(E, Q, C, lde, off, d16, False)
    fidx = off + torch.arange(n)[:, None, None] * fvs + torch.arange(Pn)[None, :, None] * C + torch.arange(C)[None, None]
    f = make_buf(Fv, fidx, off + n * fvs + 64, off, (n, Pn, C), (fvs, C, 1), d16, False, C)
    obase = (GUARD * Pn + 4) if padded else 0
    oidx = obase + torch.arange(n)[:, None, None] * ovs + torch.arange(Q)[None, :, None] * Pn + torch.arange(Pn)[None, None]
    o = make_buf(None, oidx, obase + n * ovs + GUARD * Pn, obase, (n, Q, Pn), (ovs, Pn, 1), F32, True, Pn)
    return dict(e=e, f=f, out=o, lde=lde, fvs=fvs, ovs=ovs, E=E.to(d16), F=Fv.to(d16))


def build_rowstats(rc, fmt, padded):
    """x fp32 [rows, D] (ldx), xcopy 16-bit (ldxc), stats fp32 [rows][stats_ld][2] of pst_rowstats"""
    d16 = fmt_dtype(fmt)
    D, rows = rc['D'], rc['rows']
    x = rnd(51, rows, D) * 1.5 + 0.3
    guard = GUARD if padded else 0
    xb = rows_buf(x, rows, D, D + (4 if padded else 0), 4 if padded else 0, F32, False)
    xc = rows_buf(None, rows, D, D + (8 if padded else 0), 4 if padded else 0, d16, True, guard=guard)
    sld = D // 64 + (1 if padded else 0)
    base = guard * sld * 2
    idx = base + torch.arange(rows)[:, None, None] * (sld * 2) + torch.arange(D // 64)[None, :, None] * 2 + torch.arange(2)[None, None]
    st = make_buf(None, idx, base + (rows + max(guard, 8)) * sld * 2, base, (rows, sld, 2), (sld * 2, 2, 1), F32, True, sld)
    return dict(x=xb, xcopy=xc, stats=st, sld=sld, X=x)


# ------------------------------------------------------------------------------------------------------ the argument rules, restated from the source
def _aligned(buf, nbytes):
    return (buf.base * _SIZE[buf.alloc.dtype]) % nbytes == 0              # allocations themselves are at least 64-byte aligned


def validate(s):
    """gemm_validate / gemm_f32_validate of csrc/gemm.hip, gemm_f32.hip on a built set: None, or the rule that refuses it"""
    p = s['p']
    a, w, c = s['a'], s['w'], s['c']
    f32o = p['out'] == 'f32'
    if p['f32']:
        if p['K'] % 16 or p['N'] % 4 or w.ld % 4 or (not p['conv'] and a.ld % 4) or not (_aligned(a, 16) and _aligned(w, 16) and _aligned(c, 16)):
            return 'fp32 operands: K % 16, N % 4, lda / ldw % 4, 16-byte alignment'
        if p['mode'] == 'plain' and c.ld % 4:
            return 'ldc % 4'
        if p['res'] and (s.get('res', c).ld % 4 or not _aligned(s.get('res', c), 16)):
            return 'residual rows 16-byte aligned'
        return None
    if p['K'] % 64 or p['N'] % 4:
        return 'K % 64, N % 4'
    if not (_aligned(a, 16) and _aligned(w, 16)) or not _aligned(c, 16 if f32o else 8):
        return 'A / W 16-byte, C 8-byte (16-bit) / 16-byte (fp32) aligned'
    if w.ld % 8 or (not p['conv'] and a.ld % 8):
        return 'lda / ldw % 8'
    if p['mode'] != 'ps' and c.ld % 4:
        return 'ldc % 4'
    if p['res']:
        r = s.get('res', c)
        if r.ld % (8 if p['res'] == '16' else 4) or (p['res'] == '16' and not _aligned(r, 16)):
            return 'ldr % 4 (fp32) / 8 (16-bit), a 16-bit residual 16-byte aligned'
    if p['producer'] and (p['N'] % 64 or p['mode'] != 'plain' or p['batch'] or s['stats'].ld < p['N'] // 64):
        return 'fold producer: plain store, N % 64, stats_ld >= N / 64'
    if 'xcopy' in s and (not f32o or s['xcopy'].ld % 4 or not _aligned(s['xcopy'], 8)):
        return 'xcopy: fp32 C, ldxc % 4, 8-byte aligned'
    if p['mode'] == 'x3' and (p['x3_block'] < p['N'] or p['x3_block'] % 4 or c.ld < 3 * p['x3_block'] or s['fmt'] != 'f16'):
        return 'split store'
    if p['batch'] and ((s['a_bs'] | s['w_bs'] | s['c_bs']) % 8 or s['bias_bs'] % 4 or p['gamma'] or p['res']):
        return 'strided batch'
    if p['rope'] and (f32o or p['N'] % 64 or p['res'] or p['mode'] != 'plain'):
        return 'fused RoPE'
    return None


def persistent_class(s):
    """gemm256_persistent_class of csrc/gemm256.hip"""
    p, c = s['p'], s['c']
    if p['mode'] in ('ps', 'conv', 'x3') or p['grp'] or p['N'] % 64 or p['batch']:
        return 0
    if p['ln'] and ((p['K'] // 64) & 1 or p['K'] // 64 < 2 or p['K'] // 64 > 16):
        return 0
    if p['mode'] == 'trans':
        return 0 if (p['out'] == 'f32' or p['res'] or p['gamma'] or p['rope'] or p['producer'] or c.ld & 7 or not _aligned(c, 16)) else 3
    if p['rope'] and p['out'] == 'f32':
        return 0
    if p['out'] != 'f32':
        return 0 if (p['res'] or p['producer'] or c.ld & 7 or not _aligned(c, 16)) else 1
    if p['act'] or p['ln']:
        return 0
    r = s.get('res', c)
    if p['N'] % 256 or p['res'] != 'f32' or c.ld & 3 or r.ld & 3 or not (_aligned(c, 16) and _aligned(r, 16)):
        return 0
    if 'xcopy' in s and (s['xcopy'].ld & 7 or not _aligned(s['xcopy'], 16)):
        return 0
    return 2


def rowstream_class(s):
    """rowstream_class of csrc/rowstream.hip"""
    p, a, w, c = s['p'], s['a'], s['w'], s['c']
    if p['N'] != 384 or p['K'] != 384 or a.ld != 384 or w.ld != 384 or p['M'] % 32 or p['M'] < 16384 or p['out'] == 'f32' or p['kernel'] != 0:
        return 0
    if p['rope'] or p['mode'] != 'plain' or p['grp'] or p['batch'] or 'xcopy' in s:
        return 0
    if c.ld & 7 or not (_aligned(a, 16) and _aligned(w, 16) and _aligned(c, 16)):
        return 0
    if not p['res']:
        if p['producer'] or (p['ln'] and p['K'] // 64 != 6):
            return 0
        return 1
    r = s.get('res', c)
    if p['res'] != '16' or r.ld != 384 or not _aligned(r, 16) or p['ln'] or p['act']:
        return 0
    if p['producer'] and s['stats'].ld < 6:
        return 0
    return 2


def predicted_variant(s, deep_ring=4, cus=256):
    """pst_gemm_variant restated: gemm_choice of csrc/gemm.hip with the forced kernel (the table forces every tiled variant, or uses a shape far on one side
    of the automatic thresholds: fewer than 176 tiles of 128 x 128 -> 64 x 64 tiles, >= 256 of them and fewer than 176 of 256 x 256 -> 128 x 128)"""
    p = s['p']
    if p['f32']:
        return 'gemm_f32_kernel'
    if rowstream_class(s):
        return 'rowgemm384_kernel'
    nb = max(1, p['batch'])
    big = ((p['M'] + 127) // 128) * ((p['N'] + 127) // 128) * nb
    t256 = ((p['M'] + 255) // 256) * ((p['N'] + 255) // 256)
    small = p['kernel'] == 0 and big < (176 if p['K'] >= 2048 else 256)
    pc = persistent_class(s)
    one_round = 176 <= t256 <= 256
    if p['mode'] == 'trans':
        p3 = pc == 3 and nb == 1 and (p['kernel'] == 256 or (p['kernel'] == 0 and (t256 >= 384 or one_round) and p['K'] >= 512))
        return 'gemm256p_kernel' if p3 else ('gemm_kernel<2,2,true>' if small else 'gemm_kernel<4,4,true>')
    shape256 = p['N'] % 256 == 0 and p['K'] >= 1024 and (p['N'] >= 2048 or p['K'] >= 2048) and t256 >= 3 * 256 - 64
    shape256p = (t256 >= 384 or one_round) and ((pc == 1 and p['K'] >= 512) or (pc == 2 and (p['K'] >= 2048 or (p['K'] >= 768 and t256 <= 512))))
    if p['mode'] != 'conv' and nb == 1 and (p['kernel'] == 256 or (p['kernel'] == 0 and (shape256 or shape256p))):
        return 'gemm256p_kernel' if pc else 'gemm256_kernel'
    return 'gemm_kernel<2,2,false>' if small else 'gemm_kernel<4,4,false>'


def predicted_pair_variant(sets, cus=256):
    """pst_gemm_pair_variant restated (pair_split_256p / pair_fusable of csrc/gemm.hip, gemm256p_pair_split of csrc/gemm256.hip)"""
    a, b = sets
    pa, pb = a['p'], b['p']
    if pa['kernel'] or pb['kernel'] or pa['batch'] or pb['batch']:
        return ''
    va, vb = predicted_variant(a), predicted_variant(b)
    ca, cb = persistent_class(a), persistent_class(b)
    if va == vb == 'gemm256p_kernel' and ca == cb:
        tile_us = lambda p, cls: 1.94 * (p['K'] // 64 + (15 if cls == 2 else 8))
        ta = ((pa['M'] + 255) // 256) * ((pa['N'] + 255) // 256)
        tb = ((pb['M'] + 255) // 256) * ((pb['N'] + 255) // 256)
        sep = math.ceil(ta / cus) * tile_us(pa, ca) + math.ceil(tb / cus) * tile_us(pb, cb)
        best = min(max(math.ceil(ta / g) * tile_us(pa, ca), math.ceil(tb / (cus - g)) * tile_us(pb, cb)) for g in range(8, cus - 7))
        if ta >= 64 and tb >= 64 and best <= 0.95 * sep:
            return 'gemm256p2_kernel'
    if pa['mode'] != 'trans' and pb['mode'] == 'trans' and va == 'gemm_kernel<2,2,false>' and vb == 'gemm_kernel<2,2,true>':
        return 'gemm_pair_kernel<2,2>'
    return ''
