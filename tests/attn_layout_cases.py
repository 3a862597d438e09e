"""Shared by tests/test_hip_attn_layout.py (GPU) and tests/test_attn_layout_checks.py (CPU): every attention kernel (csrc/attention.hip, attn_f32.hip,
attn_x3.hip) under the strides, paddings and base offsets the model really uses, after tests/gemm_layout_cases.py (whose Buf, sentinels and checks are
reused).  Nothing here imports the code under test.

A case names the kernel variant it is meant to reach (the string pst_attn_variant / pst_attn_pair_variant / pst_attn_x3_variant returns), the logical shape,
mask, key split and softmax mode, and a layout.  `build(case, fmt, padded)` returns, per problem, a TIGHT set (the layout of tests/test_hip_ops.py::
test_attention: contiguous [B, N, H hd] rows, zeros in the V^T and mask pads, an output of exactly its logical size) or a PADDED set with equal logical
contents in the model's layout:
  - Q and K are column slices of ONE [rows, 2 D] or [rows, 3 D] buffer (D = H hd) that starts 2 rows + 8 elements into its allocation, Tp > max(Nq, Nk) rows
    per batch; with `neg_bs` the K / V^T pointers sit at the LAST batch and k_bs / v_bs are negative (the pair cross-attention of the memory build);
  - V^T has the row stride B Tp + vpad, the batches side by side (v_bs = Tp);
  - O is a column slice (8 columns in) of a buffer D + opad wide with GUARD rows before and after, Tp rows per batch; a PST_X3H output is three blocks
    of out_block = D + 64 columns;
  - the mask has m_rs = roundup4(Nk) + 4 (m_bs = 0: one mask for all batches; m_rs = 0: one row per batch, key padding); the fp32-operand kernel, which
    asks nothing of the mask, gets it at an odd base with odd strides;
  - a key split gets a caller-owned workspace of exactly pst_attn_workspace_bytes, 256 bytes into a larger buffer.
Everything the operand contract of include/panst3r_hip.h says is not read is poison: NaN in Q rows >= Nq, K rows >= Nk, the other columns of the shared
buffer, V^T columns >= roundup8(Nk) (fp32 operands: >= Nk); 0xFF in mask bytes >= Nk.  V^T columns [Nk, roundup8(Nk)), which the 16-bit and split-operand
kernels read and multiply by 0, hold finite values of magnitude 1e4.  O and the workspace are filled with SENTINEL.  The split-operand kernel gets (hi, lo)
planes made from the poisoned fp32 buffers, so the lo planes are poisoned exactly like the hi planes.

Operands are the recipes of tests/test_hip_ops.py (`rn`, `plant_keys`, restated here: that module needs a GPU): the last key and the first and last key of
every split carry a planted logit in one query row each, so a dropped or doubled key moves its row by O(|v|); full masks keep key 0 open in every row, block
every later tile of row 0 and leave row 1 only its last key.

Where the issue's shape and its variant disagree the variant wins: Nq = 113 (the last wave's second fragment holds one row) is one 128-query block, so
the `,2>` kernels need B H >= 256 there and the case uses B = 16, H = 16 instead of 8 x 16."""
import math

import numpy as np
import torch

import gemm_layout_cases as G
from gemm_layout_cases import BF16, F16, F32, GUARD, SENTINEL, Buf, up          # noqa: F401

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
WS_OFF, WS_GUARD = 64, 4096                  # floats before / after the workspace proper
X3H = 4                                      # PST_X3H


def rn(seed, *shape, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def split_keys(Nk, ns):
    """the last key and the first / last key of every key-range split (attn_body: tiles of 64 keys, tps = ceil(tiles / nsplit) per split)"""
    tiles = (Nk + 63) // 64
    tps = (tiles + ns - 1) // ns
    return sorted({Nk - 1} | {min(s_ * tps * 64, Nk - 1) for s_ in range(ns)} | {min((s_ + 1) * tps * 64, Nk) - 1 for s_ in range(ns)})


def plant_keys(qr, kr, Nk, ns):
    """tests/test_hip_ops.py::plant_keys: key i of split_keys gets a large logit in query row 2 i + 3"""
    keys = split_keys(Nk, ns)
    for i, key in enumerate(keys):
        kr[:, :, key] = qr[:, :, 2 * i + 3] * 1.5
    return keys


# --------------------------------------------------------------------------------------------------------------------------------------- the cases
def P(B, H, Nq, Nk, hd, masked=False, nsplit=1, pre=False, seed=1, scale=None, out='same', **lay):
    """one attention problem; out: 'same' (the operand format), 'f32' / 'x3h' (pst_attn_x3).  Layout keys (padded set only): W 2 / 3 (width of the shared q | k
    buffer in units of D), vpad, opad, neg_bs, m_bs0, m_rs0"""
    d = dict(B=B, H=H, Nq=Nq, Nk=Nk, hd=hd, masked=masked, nsplit=nsplit, pre=pre, seed=seed, scale=scale, out=out,
             W=2, vpad=8, opad=64, neg_bs=False, m_bs0=False, m_rs0=False)
    assert set(lay) <= set(d), lay
    d.update(lay)
    return d


def case(name, variant, problem, kind='fwd', fmts=('bf16', 'f16'), anchor=True, tight_variant=None):
    problems = problem if isinstance(problem, list) else [problem]
    return dict(name=name, variant=variant, tight_variant=variant if tight_variant is None else tight_variant, problems=problems, kind=kind, fmts=fmts,
                anchor=anchor)


def _cases():
    cs = []
    for hd in (64, 96):
        v1, v2 = 'attn_kernel<%d,1>' % hd, 'attn_kernel<%d,2>' % hd
        t = 'h%d' % hd
        # ---- 64-query blocks: one row past a block and one key past a tile (Nk % 8 == 1: the V^T chunk rule bites); a batch-shared mask; key padding
        for pre in (False, True):
            s = '_pre' if pre else ''
            cs.append(case('%s_b64_open%s' % (t, s), v1, P(2, 3, 65, 65, hd, pre=pre, W=3 if pre else 2, vpad=8 if pre else 24)))
            cs.append(case('%s_b64_mask_shared%s' % (t, s), v1, P(3, 2, 50, 70, hd, masked=True, pre=pre, m_bs0=True, W=2 if pre else 3)))
        cs.append(case('%s_b64_keypad' % t, v1, P(2, 3, 65, 65, hd, masked=True, pre=hd == 96, m_rs0=True, vpad=24)))
        # ---- 64-query blocks under a key split: tiles = 9, tps = 2 - split 4 is one key long, splits 5 - 7 are empty
        for masked in (False, True):
            for pre in (False, True):
                cs.append(case('%s_b64_split_%s%s' % (t, 'mask' if masked else 'open', '_pre' if pre else ''), v1,
                               P(1, 2, 65, 513, hd, masked=masked, nsplit=8, pre=pre, W=3 if masked else 2)))
        # ---- 128-query blocks where blocks and fragments end: 129 (the second block holds one row), 145 (there wave 0's first fragment is full and its
        # second holds one row), 113 (the last wave's first fragment is full, its second holds one row)
        for i, (B, Nq) in enumerate(((8, 129), (8, 145), (16, 113))):
            for masked in (False, True):
                pre = (i + masked) % 2 == 0
                cs.append(case('%s_b128_q%d_%s%s' % (t, Nq, 'mask' if masked else 'open', '_pre' if pre else ''), v2,
                               P(B, 16, Nq, 65, hd, masked=masked, pre=pre, W=2 + i % 2, vpad=24 if masked else 8)))
        # ---- 128-query blocks under a key split with 2 x 16 x 8 = 256: tiles = 17, tps = 3 - split 5 ends with the one-key tile, splits 6, 7 are empty;
        # and Nk = 513, where the last non-empty split is that one key alone
        for masked in (False, True):
            for pre in (False, True):
                cs.append(case('%s_b128_split_%s%s' % (t, 'mask' if masked else 'open', '_pre' if pre else ''), v2,
                               P(1, 16, 129, 1025, hd, masked=masked, nsplit=8, pre=pre, W=2 if masked else 3)))
        cs.append(case('%s_b128_split513_mask_pre' % t, v2, P(1, 16, 129, 513, hd, masked=True, nsplit=8, pre=True)))
        # ---- two problems in one launch, different shapes and different paddings; and two pairs that must fall back to two launches
        a2 = 'attn2_kernel<%d,2>' % hd
        cs.append(case('%s_pair' % t, a2, [P(8, 16, 129, 65, hd, pre=True, W=2, vpad=8, opad=64), P(4, 32, 200, 130, hd, pre=True, seed=2, W=3, vpad=24, opad=128)],
                       kind='pair'))
        cs.append(case('%s_pair_small_side' % t, '', [P(8, 16, 129, 65, hd, pre=True), P(2, 3, 65, 65, hd, pre=True, seed=2, W=3, vpad=24)], kind='pair', anchor=False))
        cs.append(case('%s_pair_two_scales' % t, '', [P(8, 16, 129, 65, hd), P(4, 32, 200, 130, hd, seed=2, scale=0.75 * hd ** -0.5, W=3, opad=128)],
                       kind='pair', anchor=False))
    # ---- the pair cross-attention of the memory build: each image attends to the other image's keys through a negative batch stride
    cs.append(case('h64_neg_batch_stride', 'attn_kernel<64,1>', P(2, 3, 65, 65, 64, neg_bs=True)))
    cs.append(case('h96_neg_batch_stride_mask', 'attn_kernel<96,1>', P(2, 2, 50, 70, 96, masked=True, pre=True, neg_bs=True, W=3, vpad=24)))
    # ---- fp32 operands (attn_f32_kernel): V^T columns past Nk are NaN - this kernel must not read them; the mask at an odd base with odd strides
    cs.append(case('f32_h64_open', 'attn_f32_kernel<64>', P(2, 3, 65, 65, 64, W=3), fmts=('f32',)))
    cs.append(case('f32_h96_keypad_pre', 'attn_f32_kernel<96>', P(3, 2, 50, 70, 96, masked=True, pre=True, m_rs0=True, vpad=24), fmts=('f32',)))
    cs.append(case('f32_h64_mask', 'attn_f32_kernel<64>', P(3, 2, 50, 70, 64, masked=True, vpad=24), fmts=('f32',)))
    # ---- split operands (pst_attn_x3): fp32 and PST_X3H outputs, direct and through the combine kernel; the error model of tests/errbound.py is the one of
    # f16 planes, so only those are anchored; a PST_X3H output exists for f16 planes only
    for hd, shape, kw in ((64, (2, 3, 65, 65), dict(W=3)), (96, (3, 2, 50, 70), dict(masked=True, pre=True, m_bs0=True, vpad=24))):
        for ns in (1, 3):
            for out in ('f32', 'x3h'):
                cs.append(case('x3_h%d_%s_%s' % (hd, out, 'split' if ns > 1 else 'direct'), 'attn_x3_kernel<%d,1>' % hd, P(*shape, hd, nsplit=ns, out=out, **kw),
                               kind='x3', fmts=('f16', 'bf16') if out == 'f32' else ('f16',)))
    cs.append(case('x3_h64_b128_q129', 'attn_x3_kernel<64,2>', P(8, 16, 129, 65, 64, masked=True, out='f32'), kind='x3', fmts=('f16', 'bf16')))
    cs.append(case('x3_h96_b128_q145', 'attn_x3_kernel<96,2>', P(8, 16, 145, 65, 96, pre=True, out='f32', W=3, vpad=24), kind='x3', fmts=('f16', 'bf16')))
    return cs


CASES = _cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PARAMS = [(c['name'], fmt) for c in CASES for fmt in c['fmts']]


def fmt_dtype(fmt):
    return {'bf16': BF16, 'f16': F16, 'f32': F32}[fmt]


def describe(c):
    out = []
    for p in c['problems']:
        lay = ' '.join('%s=%s' % (k, p[k]) for k in ('W', 'vpad', 'opad', 'neg_bs', 'm_bs0', 'm_rs0') if p[k] not in (False, 2, 8, 64))
        out.append('B%d H%d Nq%d Nk%d hd%d%s%s%s out=%s [%s]' % (p['B'], p['H'], p['Nq'], p['Nk'], p['hd'], ' masked' if p['masked'] else '',
                                                               ' nsplit=%d' % p['nsplit'] if p['nsplit'] > 1 else '', ' prescaled' if p['pre'] else '', p['out'], lay))
    return '%s -> %r: %s' % (c['name'], c['variant'], ' | '.join(out))


# -------------------------------------------------------------------------------------------------------------------------------------- the builder
def logical_values(p, kind, fmt):
    """q, k, v [B, H, N, hd] in the operand format (fp32 for the fp32-operand and the split-operand kernels), the mask as the kernel stores it
    (`mask_src` [B or 1, Nq or 1, Nk] bool) and as the reference sees it (`mask` [B, Nq, Nk])"""
    B, H, Nq, Nk, hd, s = p['B'], p['H'], p['Nq'], p['Nk'], p['hd'], 100 * p['seed']
    dt = F32 if (kind == 'x3' or fmt == 'f32') else fmt_dtype(fmt)
    qr, kr = rn(s + 20, B, H, Nq, hd), rn(s + 21, B, H, Nk, hd)
    planted = plant_keys(qr, kr, Nk, p['nsplit'])
    assert 2 * len(planted) + 3 <= Nq
    v = dict(q=(qr * (hd ** -0.5 * LOG2E if p['pre'] else 1.0)).to(dt), k=kr.to(dt), v=rn(s + 22, B, H, Nk, hd).to(dt), planted=planted, mask=None, mask_src=None)
    if p['masked']:
        g = np.random.Generator(np.random.PCG64(s + 5))
        nb, nr = (1 if p['m_bs0'] else B), (1 if p['m_rs0'] else Nq)
        m = torch.from_numpy(g.uniform(size=(nb, nr, Nk)) < (0.4 if p['m_rs0'] else 0.6))
        m[:, :, 0] = False                                        # every row keeps at least one key
        if p['m_rs0']:
            m[:, :, planted] = False                              # key padding: one row for all queries
        else:
            m[:, 0, 64:] = True                                   # a row whose later tiles are fully blocked
            m[:, 1, :Nk - 1] = True                               # a row whose only open key is the last one
            m[:, 1, Nk - 1] = False
            for i, key in enumerate(planted):
                m[:, 2 * i + 3, key] = False
        v['mask_src'] = m
        v['mask'] = m.expand(B, Nq, Nk).contiguous()
    return v


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


def index4(base, dims, strides, width):
    """flat index of element [a, b, c, w] of an operand with strides (s_a, s_b, s_c) and contiguous last axis"""
    (A, B_, C_), (sa, sb, sc) = dims, strides
    return base + _ar(A)[:, None, None, None] * sa + _ar(B_)[None, :, None, None] * sb + _ar(C_)[None, None, :, None] * sc + _ar(width)[None, None, None, :]


def _buf(name, alloc, base, idx, strides, out, ld):
    b = Buf(alloc, base, tuple(idx.shape), strides, idx, out, ld)
    b.name = name
    return b


def _alloc(n, dtype, out, tight_input=False):
    if tight_input:
        return torch.zeros(n, dtype=dtype)
    return G._filled(n, dtype, out)


def build_problem(p, kind, fmt, padded):
    """the buffers of one problem: `allocs` (name -> 1-D tensor; the split-operand kernel: name + '_lo' next to the hi plane), Bufs q, k, vt, o, mask, ws
    (idx in [B, H, N, hd] / [B, H, hd, Nk] / [B, Nq, Nk] coordinates) and the strides of pst_attn_params"""
    B, H, Nq, Nk, hd = p['B'], p['H'], p['Nq'], p['Nk'], p['hd']
    D = H * hd
    v = logical_values(p, kind, fmt)
    f32ops = fmt == 'f32' and kind != 'x3'
    dt = v['q'].dtype
    s = dict(p=p, kind=kind, fmt=fmt, padded=padded, vals=v, allocs={}, f32ops=f32ops)
    A = s['allocs']
    Nk8 = Nk if f32ops else up(Nk, 8)
    g = torch.Generator().manual_seed(7 + p['seed'])
    if padded:
        Tp = up(max(Nq, Nk), 8) + 8
        W = p['W'] * D
        base0 = 2 * W + 8
        A['qk'] = _alloc(base0 + (B * Tp + 2) * W, dt, False)
        qs = (Tp * W, hd, W)
        qb = base0 + (p['W'] - 2) * D
        ks, kb = qs, qb + D
        ldv = B * Tp + p['vpad']
        vs, vb = (Tp, hd * ldv, ldv), 8
        if p['neg_bs']:
            ks, kb = (-Tp * W, hd, W), kb + (B - 1) * Tp * W
            vs, vb = (-Tp, hd * ldv, ldv), vb + (B - 1) * Tp
        s['q'] = _buf('qk', A['qk'], qb, index4(qb, (B, H, Nq), qs, hd), qs, False, W)
        s['k'] = _buf('qk', A['qk'], kb, index4(kb, (B, H, Nk), ks, hd), ks, False, W)
        A['vt'] = _alloc(8 + D * ldv + 8, dt, False)
        s['vt'] = _buf('vt', A['vt'], vb, index4(vb, (B, H, hd), vs, Nk), vs, False, ldv)
        if Nk8 > Nk:                                              # the rest of the last 8-key chunk: read, multiplied by 0 - large and finite
            pad = index4(vb + Nk, (B, H, hd), vs, Nk8 - Nk)
            mag = (0.5 + torch.rand(pad.shape, generator=g)) * 1e4
            A['vt'][pad.reshape(-1)] = (mag * (1 - 2 * (torch.rand(pad.shape, generator=g) < 0.5).float())).to(dt).reshape(-1)
    else:
        Tp = Nq
        A['q'], A['k'] = _alloc(B * Nq * D, dt, False, True), _alloc(B * Nk * D, dt, False, True)
        qs, ks = (Nq * D, hd, D), (Nk * D, hd, D)
        s['q'] = _buf('q', A['q'], 0, index4(0, (B, H, Nq), qs, hd), qs, False, D)
        s['k'] = _buf('k', A['k'], 0, index4(0, (B, H, Nk), ks, hd), ks, False, D)
        Nkp = up(Nk, 8)
        ldv = B * Nkp + 8
        vs = (Nkp, hd * ldv, ldv)
        A['vt'] = _alloc(D * ldv, dt, False, True)
        s['vt'] = _buf('vt', A['vt'], 0, index4(0, (B, H, hd), vs, Nk), vs, False, ldv)
    A[s['q'].name][s['q'].idx.reshape(-1)] = v['q'].reshape(-1)
    A[s['k'].name][s['k'].idx.reshape(-1)] = v['k'].reshape(-1)
    A['vt'][s['vt'].idx.reshape(-1)] = v['v'].transpose(-1, -2).reshape(-1)
    # ---- O
    x3h = p['out'] == 'x3h'
    odt = F16 if x3h else (F32 if (p['out'] == 'f32' or f32ops) else dt)
    if x3h:
        ob = D + (64 if padded else 0)
        Wo = 3 * ob + (8 if padded else 0)
    else:
        ob = 0
        Wo = D + (p['opad'] if padded else 0)
    guard = GUARD if padded else 0
    obase = guard * Wo + (8 if padded else 0)
    os_ = (Tp * Wo, hd, Wo)
    oidx = index4(obase, (B, H, Nq), os_, hd)
    if x3h:
        oidx = torch.stack([oidx, oidx + ob, oidx + 2 * ob])
    A['o'] = _alloc((2 * guard + (B * Tp if padded else B * Nq)) * Wo, odt, True)
    s['o'] = _buf('o', A['o'], obase, oidx, os_, True, Wo)
    s['out_block'] = ob
    # ---- mask
    s['mask'] = None
    if p['masked']:
        src = v['mask_src']
        if padded:
            nb, nr = src.shape[:2]
            if f32ops:
                mbase, rowlen = 3, Nk + 1 + (Nk % 2)              # an odd base and odd strides
            else:
                mbase, rowlen = 4, up(Nk, 4) + 4
            m_rs = 0 if p['m_rs0'] else rowlen
            m_bs = 0 if p['m_bs0'] else nr * rowlen
            A['mask'] = torch.full((mbase + nb * nr * rowlen + 64,), 0xFF, dtype=torch.uint8)
            sidx = mbase + _ar(nb)[:, None, None] * (nr * rowlen) + _ar(nr)[None, :, None] * rowlen + _ar(Nk)[None, None]
            A['mask'][sidx.reshape(-1)] = src.to(torch.uint8).reshape(-1)
        else:                                                     # test_attention's: every batch and row spelled out, zeros up to a multiple of 4
            Nkm = up(Nk, 4)
            mbase, m_rs, m_bs = 0, Nkm, Nq * Nkm
            A['mask'] = torch.zeros(B * Nq * Nkm, dtype=torch.uint8)
            A['mask'].view(B, Nq, Nkm)[:, :, :Nk] = v['mask'].to(torch.uint8)
        midx = mbase + _ar(B)[:, None, None] * m_bs + _ar(Nq)[None, :, None] * m_rs + _ar(Nk)[None, None]
        s['mask'] = _buf('mask', A['mask'], mbase, midx, (m_bs, m_rs), False, max(m_rs, 1))
    # ---- split-K workspace: exactly pst_attn_workspace_bytes, caller-owned
    s['ws'] = None
    if p['nsplit'] > 1:
        need = p['nsplit'] * B * H * Nq * (hd + 2)
        off = WS_OFF if padded else 0
        A['ws'] = _alloc(off + need + (WS_GUARD if padded else 0), F32, True)
        s['ws'] = _buf('ws', A['ws'], off, off + _ar(need), (1,), True, hd + 2)
    # ---- the planes of the split-operand kernel
    if kind == 'x3':
        pf = fmt_dtype(fmt)
        for name in [n for n in A if n in ('qk', 'q', 'k', 'vt')]:
            hi = A[name].to(pf)
            A[name + '_lo'] = (A[name] - hi.float()).to(pf)
            A[name] = hi
        for key in ('q', 'k', 'vt'):
            s[key].alloc = A[s[key].name]
    return s


def build(c, fmt, padded):
    return [build_problem(p, c['kind'], fmt, padded) for p in c['problems']]


def to_device(s, dev, like=None):
    """a fresh device copy of a set: every allocation once; the index tensors of the outputs go along (or are shared with `like`)"""
    d = dict(s)
    d['allocs'] = {k: t.to(dev, copy=True) for k, t in s['allocs'].items()}
    for key in ('q', 'k', 'vt', 'o', 'mask', 'ws'):
        b = s[key]
        if b is None:
            continue
        idx = b.idx
        if b.out:
            idx = b.idx.to(dev) if like is None else like[key].idx
        d[key] = _buf(b.name, d['allocs'][b.name], b.base, idx, b.strides, b.out, b.ld)
    return d


def outputs(s):
    return [(k, s[k]) for k in ('o', 'ws') if s[k] is not None]


def logical_out(s):
    """the logical O [B, H, Nq, hd] as float64; a PST_X3H output: hi + lo (exact in float64), the value the [hi | hi | lo] row stands for"""
    o = s['o'].logical()
    if s['p']['out'] == 'x3h':
        return o[0].double() + o[2].double()
    return o.double()


# ------------------------------------------------------------------------------------------------------------------------------------ the reference
def reference(p, v):
    """float64 softmax attention of the logical operands [B, H, Nq, hd]; a row with every key blocked is 0.  For the default scale this is
    errbound.attn_ref (asserted in tests/test_attn_layout_checks.py); the pair with two scales has no other reference"""
    hd = p['hd']
    scale = LN2 if p['pre'] else (p['scale'] if p['scale'] is not None else hd ** -0.5)
    s = (v['q'].double() @ v['k'].double().transpose(-1, -2)) * scale
    if v['mask'] is not None:
        s = s.masked_fill(v['mask'][:, None], float('-inf'))
    dead = torch.isinf(s).all(-1, keepdim=True)
    pr = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    return pr @ v['v'].double()


# ------------------------------------------------------------------------------------------------------ the argument rules, restated from the source
def _elsize(buf):
    return buf.alloc.element_size()


def _aligned(buf, nbytes):
    return (buf.base * _elsize(buf)) % nbytes == 0               # allocations themselves are at least 64-byte aligned


def _rem(x, m):
    """C's x % m != 0 for the signed strides of pst_attn_params"""
    return abs(x) % m != 0


def ws_bytes(p):
    """pst_attn_workspace_bytes"""
    return p['nsplit'] * p['B'] * p['H'] * p['Nq'] * (p['hd'] + 2) * 4 if p['nsplit'] > 1 else 0


def validate(s):
    """attn_validate (csrc/attention.hip), attn_f32_validate (attn_f32.hip) and x3_validate (attn_x3.hip) on a built set: None, or the rule that refuses it"""
    p = s['p']
    q, k, vt, o, m, ws = (s[x] for x in ('q', 'k', 'vt', 'o', 'mask', 'ws'))
    if p['hd'] not in (64, 96):
        return 'head dim'
    if min(p['B'], p['H'], p['Nq'], p['Nk']) <= 0:
        return 'bad shape'
    if not p['pre'] and p['scale'] is not None and not p['scale'] > 0:
        return 'scale'
    k_rs, v_ds = k.strides[2], vt.strides[2]
    if s['f32ops']:
        if any(_rem(x, 4) for x in q.strides + k.strides + o.strides) or not (_aligned(q, 16) and _aligned(k, 16) and _aligned(o, 16)):
            return 'fp32 operands: Q / K / O rows 16-byte aligned'
        if not _aligned(vt, 4):
            return 'fp32 operands: Vt misaligned'
        if p['nsplit'] > 1:
            return 'fp32 operands: no split-K'
        if k_rs < 0:
            return 'k_rs'
        if v_ds < 0:
            return 'v_ds'
        return None
    x3 = s['kind'] == 'x3'
    if x3 and p['out'] == 'x3h' and (s['fmt'] != 'f16' or s['out_block'] < p['H'] * p['hd'] or s['out_block'] % 4 or s['out_block'] >= 1 << 30):
        return 'split output'
    if any(_rem(x, 8) for x in q.strides + k.strides + vt.strides):
        return 'Q/K/Vt strides % 8'
    if any(_rem(x, 4) for x in o.strides):
        return 'O strides % 4'
    if not (_aligned(q, 16) and _aligned(k, 16) and _aligned(vt, 16)) or not _aligned(o, 16 if x3 else 8):
        return 'alignment'
    if k_rs < 0:
        return 'k_rs'
    if v_ds < 0:
        return 'v_ds'
    if k_rs * 64 * 2 >= 1 << 31 or v_ds * p['hd'] * 2 >= 1 << 31:
        return 'row stride too large'
    if m is not None and (any(_rem(x, 4) for x in m.strides) or not _aligned(m, 4)):
        return 'mask rows 4-byte aligned'
    if p['nsplit'] > 1:
        if ws is None or ws.idx.numel() * 4 < ws_bytes(p) or not _aligned(ws, 16):
            return 'workspace'
        if p['nsplit'] > 64:
            return 'nsplit <= 64'
    return None


def attn_big(p):
    """attn_big (attention.hip) = x3_big (attn_x3.hip): 128-query blocks once blocks x splits fill the chip"""
    return ((p['Nq'] + 127) // 128) * p['H'] * p['B'] * max(1, p['nsplit']) >= 256


def pair_fusable(sa, sb):
    """attn_pair_fusable (attention.hip), PST_TUNE_PAIR_ATTN at its default"""
    a, b = sa['p'], sb['p']
    if sa['f32ops'] or sa['fmt'] != sb['fmt'] or a['hd'] != b['hd'] or a['pre'] != b['pre'] or a['nsplit'] > 1 or b['nsplit'] > 1:
        return False
    if not a['pre'] and (a['scale'] if a['scale'] is not None else a['hd'] ** -0.5) != (b['scale'] if b['scale'] is not None else b['hd'] ** -0.5):
        return False
    return attn_big(a) and attn_big(b)


def predicted_variant(c, sets):
    """pst_attn_variant / pst_attn_pair_variant / pst_attn_x3_variant restated"""
    p = sets[0]['p']
    if c['kind'] == 'pair':
        return 'attn2_kernel<%d,2>' % p['hd'] if pair_fusable(*sets) else ''
    if c['kind'] == 'x3':
        return 'attn_x3_kernel<%d,%d>' % (p['hd'], 2 if attn_big(p) else 1)
    if sets[0]['f32ops']:
        return 'attn_f32_kernel<%d>' % p['hd']
    return 'attn_kernel<%d,%d>' % (p['hd'], 2 if attn_big(p) else 1)
