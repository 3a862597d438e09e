"""The cases of tests/attn_layout_cases.py are what they claim (CPU only, no GPU), as tests/test_gemm_layout_checks.py shows for the GEMM cases.

Every case, tight and padded, satisfies the argument rules of attn_validate / attn_f32_validate / x3_validate and reaches the variant it names under attn_big /
attn_pair_fusable, all restated in Python - and every restated rule is found in the source text.  The table holds every variant name the three *_variant
entry points can return, in every format it supports, and every 16-bit forward variant {open, masked} x {direct, split} x {prescaled, not}.  Everything the
builders poison is disjoint from everything the operand contract of include/panst3r_hip.h says is read (computed from the strides with integer arithmetic),
every logical output element is disjoint from every guard, the padded sets hold the tight sets' logical contents, and the float64 reference is finite.
Planted mistakes - a store one row past Nq, a workspace row index over Nq + 1, a pad key let through - applied to an emulation are each reported by the
checks the GPU module runs; the same arithmetic shows that those mistakes stay inside the buffers a case owns."""
import os
import re

import pytest
import torch

import errbound as EB
import gemm_layout_cases as G
import attn_layout_cases as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'panst3r_amd', 'csrc')
HEADER = os.path.join(os.path.dirname(CSRC), '..', 'include', 'panst3r_hip.h')


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _func(src, head):
    """the text of the function whose definition starts with `head`"""
    i = src.index(head)
    return src[i: src.index('\n}\n', i)]


# ---------------------------------------------------------------------------------------------------------------- the rules and the sources
def test_restated_rules_match_the_sources():
    att, x3, f32 = _src('attention.hip'), _src('attn_x3.hip'), _src('attn_f32.hip')
    v16, vx3, vf32 = _func(att, 'static int attn_validate('), _func(x3, 'static int x3_validate('), _func(f32, 'int attn_f32_validate(')
    strides8 = r'\(p\.q_rs \| p\.q_hs \| p\.q_bs \| p\.k_rs \| p\.k_hs \| p\.k_bs \| p\.v_ds \| p\.v_hs \| p\.v_bs\) % 8'
    for v, tag in ((v16, 'attn'), (vx3, 'attn_x3')):
        assert re.search(r'p\.hd != 64 && p\.hd != 96', v) and re.search(strides8, v) and re.search(r'\(p\.o_rs \| p\.o_hs \| p\.o_bs\) % 4', v), tag
        assert re.search(r'p\.k_rs \* 64 \* 2 >= \(1ll << 31\) \|\| p\.v_ds \* \(int64_t\)p\.hd \* 2 >= \(1ll << 31\)', v), tag
        assert re.search(r'p\.mask && \(\(p\.m_rs \| p\.m_bs\) % 4 \|\| \(\(uintptr_t\)p\.mask & 3\)\)', v), tag
        assert re.search(r'need = \(int64_t\)p\.nsplit \* p\.B \* p\.H \* p\.Nq \* \(p\.hd \+ 2\) \* 4;', v) and re.search(r'p\.nsplit > 64', v), tag
        assert re.search(r'!p\.ws \|\| p\.ws_bytes < need \|\| \(\(uintptr_t\)p\.ws & 15\)', v), tag
    assert re.search(r'\(\(uintptr_t\)p\.Q \| \(uintptr_t\)p\.K \| \(uintptr_t\)p\.Vt\) & 15 \|\| \(\(uintptr_t\)p\.O & 7\)', v16)
    assert re.search(r'\(uintptr_t\)p\.Q \| \(uintptr_t\)p\.K \| \(uintptr_t\)p\.Vt \| \(uintptr_t\)Qlo \| \(uintptr_t\)Klo \| \(uintptr_t\)Vlo \| \(uintptr_t\)p\.O\) & 15', vx3)
    assert re.search(r'out_type == DT_X3H && \(p\.dtype16 != DT_F16 \|\| out_block < \(int64_t\)p\.H \* p\.hd \|\| out_block % 4 \|\| out_block >= \(1ll << 30\)\)', vx3)
    assert re.search(r'\(p\.q_rs \| p\.q_hs \| p\.q_bs \| p\.k_rs \| p\.k_hs \| p\.k_bs \| p\.o_rs \| p\.o_hs \| p\.o_bs\) % 4 \|\| '
                     r'\(\(\(uintptr_t\)p\.Q \| \(uintptr_t\)p\.K \| \(uintptr_t\)p\.O\) & 15\)', vf32)
    assert re.search(r'\(uintptr_t\)p\.Vt & 3', vf32) and re.search(r'p\.nsplit > 1', vf32) and 'mask' not in vf32          # it asks nothing of the mask
    # the refusal of negative row strides: in all three, naming the field, and in front of the 32-bit offsets' own bound
    for v, tag in ((v16, 'attn'), (vx3, 'attn_x3'), (vf32, r'attn \(fp32 operands\)')):
        for field in ('k_rs', 'v_ds'):
            assert re.search(r'if \(p\.%s < 0\) \{ set_error\("%s: %s must not be negative"\); return PST_EINVAL; \}' % (field, tag, field), v), (tag, field)
    assert v16.index('p.k_rs < 0') < v16.index('p.k_rs * 64 * 2') and vx3.index('p.v_ds < 0') < vx3.index('p.k_rs * 64 * 2')
    # ... because these are the 32-bit offsets (both 16-bit kernels), and nothing else narrows a stride
    for src in (att, x3):
        assert '(uint32_t)(k_key[j] * (int)p.k_rs + k_chunk[j] * 8) * 2u' in src and '(uint32_t)(v_row[j] * (int)p.v_ds + v_chunk[j] * 8) * 2u' in src
        assert len(re.findall(r'\(int\)p\.\w+_[bhrd]s', src)) == 2
    assert not re.search(r'\(int\)p\.\w+_[bhrd]s', f32)
    # every entry point validates before it launches, the variant queries included
    assert re.search(r'pst_attn_fwd\(const pst_attn_params\* pp, void\* stream\) \{\n  using namespace pst;\n  if \(int rc = attn_validate\(pp\)\) return rc;', att)
    assert re.search(r'if \(attn_validate\(pa\) \|\| attn_validate\(pb\)\) return nullptr;', att) and re.search(r'if \(attn_validate\(pp\)\) return nullptr;', att)
    assert re.search(r'pst_attn_x3\(.*\) \{\n  if \(int rc = x3_validate\(pp, Q_lo, K_lo, Vt_lo, out_type, out_block\)\) return rc;', x3)
    assert re.search(r'if \(!pp \|\| x3_validate\(pp, pp->Q, pp->K, pp->Vt, DT_F32, 0\)\) return nullptr;', x3)
    # dispatch
    big = r'\(long\)\(\(p\.Nq \+ 127\) / 128\) \* p\.H \* p\.B \* \(p\.nsplit > 1 \? p\.nsplit : 1\) >= 256'
    assert re.search(r'static bool attn_big\(const pst_attn_params& p\) \{ return ' + big, att) and re.search(r'static bool x3_big\(const pst_attn_params& p\) \{ return ' + big, x3)
    fus = _func(att, 'static bool attn_pair_fusable(')
    assert 'a.dtype16 == pst::DT_F32 || a.dtype16 != b.dtype16 || a.hd != b.hd || a.prescaled != b.prescaled || a.nsplit > 1 || b.nsplit > 1' in fus
    assert 'if (!a.prescaled && a.scale != b.scale) return false;' in fus and 'return attn_big(a) && attn_big(b);' in fus
    assert re.search(r'return nsplit > 1 \? \(int64_t\)nsplit \* B \* H \* Nq \* \(hd \+ 2\) \* 4 : 0;', att)
    # the reads the contract speaks of: 8-key V^T chunks and 4-byte mask words (16-bit, x3), scalars under a key predicate (fp32)
    for src in (att, x3):
        assert 'const int kcol = k0 + v_chunk[j] * 8;' in src and 'if (mrow && key < p.Nk) mb = *(const uint32_t*)(mrow + key);' in src
        assert re.search(r'min\(k0 \+ k_key\[j\], p\.Nk - 1\)', src) and re.search(r'min\(q_wave0 \+ a \* 16 \+ l16, p\.Nq - 1\)', src)
    assert 'Vs[key * PITCH + d] = (k0 + key < p.Nk) ? Vp[(int64_t)d * p.v_ds + k0 + key] : 0.f;' in f32
    assert 'if (key + r < p.Nk && Mp[(int64_t)qc * p.m_rs + key + r] != 0) mb |= 1u << r;' in f32
    head = open(HEADER).read()
    doc = head[head.index('The operand contract'): head.index('typedef struct pst_attn_params')]
    for phrase in ('k_rs and v_ds must be >= 0', '[Nk, roundup8(Nk))', 'FINITE', '[Nk, roundup4(Nk))', 'Q rows >= Nq, K rows >= Nk', 'pst_attn_workspace_bytes'):
        assert phrase in doc, phrase


def test_variant_names_of_the_sources_are_all_in_the_table():
    names = set()
    for f in ('attention.hip', 'attn_x3.hip'):
        src = _src(f)
        for fn in ('pst_attn_variant', 'pst_attn_pair_variant', 'pst_attn_x3_variant'):
            if 'const char* %s(' % fn in src:
                names |= set(re.findall(r'"(attn\w*_kernel<[\d,]+>)"', _func(src, 'extern "C" const char* %s(' % fn)))
    assert len(names) == 4 + 2 + 2 + 4, names
    have = {(c['variant'], fmt) for c in A.CASES for fmt in c['fmts']}
    for n in names:
        fmts = ('f32',) if n.startswith('attn_f32') else ('bf16', 'f16')
        for fmt in fmts:
            assert (n, fmt) in have, (n, fmt)
    assert any(c['variant'] == '' and c['kind'] == 'pair' for c in A.CASES)
    x3h = [c for c in A.CASES if c['problems'][0]['out'] == 'x3h']
    assert x3h and all(c['fmts'] == ('f16',) for c in x3h) and {c['problems'][0]['nsplit'] > 1 for c in x3h} == {False, True}


@pytest.mark.parametrize('variant', ['attn_kernel<%d,%d>' % (hd, qf) for hd in (64, 96) for qf in (1, 2)])
def test_every_16bit_variant_has_every_mode(variant):
    seen = {(p['masked'], p['nsplit'] > 1, p['pre']) for c in A.CASES if c['variant'] == variant and c['kind'] == 'fwd' for p in c['problems']}
    assert seen == {(m, s, pre) for m in (False, True) for s in (False, True) for pre in (False, True)}, (variant, sorted(seen))
    assert all(c['fmts'] == ('bf16', 'f16') for c in A.CASES if c['variant'] == variant)


def test_the_shapes_of_the_issue():
    shape = lambda n: tuple(A.BY_NAME[n]['problems'][0][k] for k in ('B', 'H', 'Nq', 'Nk', 'hd'))
    for hd in (64, 96):
        t = 'h%d' % hd
        assert shape(t + '_b64_open') == (2, 3, 65, 65, hd) and shape(t + '_b64_mask_shared') == (3, 2, 50, 70, hd) and A.BY_NAME[t + '_b64_mask_shared']['problems'][0]['m_bs0']
        assert A.BY_NAME[t + '_b64_keypad']['problems'][0]['m_rs0'] and shape(t + '_b64_keypad')[0] == 2
        assert shape(t + '_b64_split_open') == (1, 2, 65, 513, hd) and shape(t + '_b128_split_mask') == (1, 16, 129, 1025, hd)
        big = {shape(c['name'])[:4] for c in A.CASES if c['name'].startswith(t + '_b128_q')}
        assert big == {(8, 16, 129, 65), (8, 16, 145, 65), (16, 16, 113, 65)}
        for Nq in (129, 145, 113):                                 # open and masked, hd 96 too
            assert {c['problems'][0]['masked'] for c in A.CASES if c['name'].startswith('%s_b128_q%d_' % (t, Nq))} == {False, True}
        pair = A.BY_NAME[t + '_pair']['problems']
        assert [tuple(p[k] for k in ('B', 'H', 'Nq', 'Nk')) for p in pair] == [(8, 16, 129, 65), (4, 32, 200, 130)]
        assert all(pair[0][k] != pair[1][k] for k in ('W', 'vpad', 'opad'))                   # a stride taken from the wrong problem shows
    # the fragment edges the 128-query cases are about: rows of the last block's waves (32 rows per wave, two 16-row fragments)
    frag = lambda Nq, row0: (min(16, max(0, Nq - row0)), min(16, max(0, Nq - row0 - 16)))
    assert frag(129, 128) == (1, 0) and frag(145, 128) == (16, 1) and frag(113, 96) == (16, 1) and frag(65, 64) == (1, 0)
    # split tails: (tiles, tiles per split) -> keys of the last non-empty split, number of empty splits
    def tail(Nk, ns):
        tiles = (Nk + 63) // 64
        tps = (tiles + ns - 1) // ns
        live = [s for s in range(ns) if s * tps < tiles]
        return Nk - live[-1] * tps * 64, ns - len(live)
    assert tail(513, 8) == (1, 3) and tail(1025, 8) == (65, 2) and tail(65, 3) == (1, 1) and tail(70, 3) == (6, 1)
    neg = A.BY_NAME['h64_neg_batch_stride']['problems'][0]
    assert neg['B'] == 2 and neg['neg_bs']


# ---------------------------------------------------------------------------------------------------------------- every case, built
def _planes(s, buf):
    return [s['allocs'][buf.name]] + ([s['allocs'][buf.name + '_lo']] if s['kind'] == 'x3' else [])


def _read_sets(s):
    """per allocation name, the set of flat element indices the contract says are read, from the strides alone"""
    p = s['p']
    B, H, Nq, Nk, hd = p['B'], p['H'], p['Nq'], p['Nk'], p['hd']
    rd = {}

    def add(name, idx):
        rd.setdefault(name, []).append(idx.reshape(-1))
    q, k, vt, m = s['q'], s['k'], s['vt'], s['mask']
    add(q.name, A.index4(q.base, (B, H, Nq), q.strides, hd))
    add(k.name, A.index4(k.base, (B, H, Nk), k.strides, hd))
    add(vt.name, A.index4(vt.base, (B, H, hd), vt.strides, Nk if s['f32ops'] else G.up(Nk, 8)))
    if m is not None:
        w = Nk if s['f32ops'] else G.up(Nk, 4)
        add('mask', m.base + torch.arange(B)[:, None, None] * m.strides[0] + torch.arange(Nq)[None, :, None] * m.strides[1] + torch.arange(w)[None, None])
    return {n: torch.unique(torch.cat(v)) for n, v in rd.items()}


@pytest.mark.parametrize('name,fmt', A.PARAMS)
def test_case_is_admitted_laid_out_and_poisoned_as_declared(name, fmt):
    c = A.BY_NAME[name]
    tight, padded = A.build(c, fmt, False), A.build(c, fmt, True)
    for sets, want in ((padded, c['variant']), (tight, c['tight_variant'])):
        for s in sets:
            assert A.validate(s) is None, (name, s['padded'], A.validate(s))
        assert A.predicted_variant(c, sets) == want, (name, A.predicted_variant(c, sets), want)
    if ',2>' in c['variant']:
        assert all(A.attn_big(p) for p in c['problems'])
    for t, s in zip(tight, padded):
        p = s['p']
        B, H, Nq, Nk, hd = p['B'], p['H'], p['Nq'], p['Nk'], p['hd']
        D = H * hd
        Tp = G.up(max(Nq, Nk), 8) + 8
        # ---- the declared layout
        assert s['q'].name == s['k'].name == 'qk' and s['q'].strides == (Tp * p['W'] * D, hd, p['W'] * D) and Tp > max(Nq, Nk)
        assert s['q'].base > 0 and s['k'].base - s['q'].base == (D if not p['neg_bs'] else D + (B - 1) * Tp * p['W'] * D)
        assert s['k'].strides == ((-1 if p['neg_bs'] else 1) * Tp * p['W'] * D, hd, p['W'] * D)
        ldv = B * Tp + p['vpad']
        assert s['vt'].strides == ((-1 if p['neg_bs'] else 1) * Tp, hd * ldv, ldv) and p['vpad'] in (8, 24)
        assert t['q'].strides == (Nq * D, hd, D) and t['k'].strides == (Nk * D, hd, D) and t['o'].strides[:2] == (Nq * t['o'].strides[2], hd) and t['o'].base == 0
        if p['masked']:
            ms = s['mask'].strides
            assert (ms[0] == 0) == p['m_bs0'] and (ms[1] == 0) == p['m_rs0']
            if s['f32ops']:
                assert s['mask'].base % 4 and (ms[0] % 2 or ms[1] % 2)                        # the fp32-operand kernel asks nothing of the mask
            elif not p['m_rs0']:
                assert ms[1] == G.up(Nk, 4) + 4
            assert t['mask'].strides == (Nq * G.up(Nk, 4), G.up(Nk, 4))
        if p['nsplit'] > 1:
            assert s['ws'].base == A.WS_OFF > 0 and s['ws'].idx.numel() * 4 == A.ws_bytes(p) and s['ws'].alloc.numel() == A.WS_OFF + A.ws_bytes(p) // 4 + A.WS_GUARD
        # ---- equal logical contents; the mask as the reference sees it
        for key in ('q', 'k', 'vt'):
            for a, b in zip(_planes(t, t[key]), _planes(s, s[key])):
                assert torch.equal(G.bits(a[t[key].idx]), G.bits(b[s[key].idx])), (name, key)
        assert torch.equal(G.bits(s['q'].logical()), G.bits(s['vals']['q'].to(s['q'].alloc.dtype)))
        assert torch.equal(s['vt'].logical().float(), s['vals']['v'].transpose(-1, -2).to(s['vt'].alloc.dtype).float())
        if p['masked']:
            assert torch.equal(s['mask'].logical(), s['vals']['mask'].to(torch.uint8)) and torch.equal(t['mask'].logical(), s['mask'].logical())
        # ---- poison: everything outside the read set, nothing inside it (both planes alike)
        read = _read_sets(s)
        for n, idx in read.items():
            for plane in ([s['allocs'][n]] + ([s['allocs'][n + '_lo']] if s['kind'] == 'x3' and n != 'mask' else [])):
                poison = plane == 0xFF if n == 'mask' else torch.isnan(plane)
                inside = torch.zeros(plane.numel(), dtype=torch.bool)
                inside[idx] = True
                assert int(idx.min()) >= 0 and int(idx.max()) < plane.numel()
                if n == 'mask':                                                                # bytes [Nk, roundup4(Nk)) are read and ignored: poisoned too
                    lg = torch.zeros_like(inside)
                    lg[s['mask'].idx.reshape(-1)] = True
                    assert bool((poison == ~lg).all()), (name, n)
                else:
                    assert bool((poison == ~inside).all()), (name, n, int((poison & inside).sum()), int((~poison & ~inside).sum()))
        if not s['f32ops'] and Nk % 8:                                                         # the rest of the last 8-key chunk: finite, large
            pad = A.index4(s['vt'].base + Nk, (B, H, hd), s['vt'].strides, G.up(Nk, 8) - Nk)
            for plane in _planes(s, s['vt'])[:1]:
                assert 4e3 < float(plane[pad].float().abs().min()) and float(plane[pad].float().abs().max()) < 2e4
        # ---- outputs: the sentinel everywhere, guards before and after, logical elements distinct
        for k, b in A.outputs(s):
            assert bool((G.bits(b.alloc) == G.SENTINEL[b.alloc.dtype]).all()), (name, k)
            flat = b.idx.reshape(-1)
            assert torch.unique(flat).numel() == flat.numel()
            lo, hi = int(flat.min()), int(flat.max())
            guard = G.GUARD * b.ld if k == 'o' else A.WS_OFF
            assert lo >= guard and b.alloc.numel() - 1 - hi >= (guard if k == 'o' else A.WS_GUARD), (name, k)
        if s['p']['out'] == 'x3h':
            assert s['out_block'] == D + 64 and s['o'].ld == 3 * s['out_block'] + 8 and s['o'].idx.shape[0] == 3
        # ---- the mutations of the pull request's evidence stay inside these buffers: a store at row Nq of every (b, h) lands in the rows between the
        # batches or in the guard rows; a workspace row index over Nq + 1 ends B H - 1 rows late, (hd + 2) floats each at the most
        o = s['o']
        stray = A.index4(o.base, (B, H, 1), o.strides, hd) + Nq * o.strides[2]
        assert int(stray.min()) >= 0 and int(stray.max()) + 2 * s['out_block'] < o.alloc.numel() and Tp > Nq
        if p['nsplit'] > 1:
            assert (B * H - 1) * (hd + 2) <= A.WS_GUARD


@pytest.mark.parametrize('name', sorted({c['name'] for c in A.CASES}))
def test_reference_is_finite_and_the_one_of_errbound(name):
    c = A.BY_NAME[name]
    fmt = c['fmts'][0]
    for t, s in zip(A.build(c, fmt, False), A.build(c, fmt, True)):
        p = s['p']
        views = lambda x: dict(q=x['q'].logical() if x['kind'] != 'x3' else x['vals']['q'], k=x['k'].logical() if x['kind'] != 'x3' else x['vals']['k'],
                               v=(x['vt'].logical().transpose(-1, -2).contiguous() if x['kind'] != 'x3' else x['vals']['v']), mask=x['vals']['mask'])
        rp, rt = A.reference(p, views(s)), A.reference(p, views(t))
        assert torch.equal(rp, rt) and bool(torch.isfinite(rp).all()) and rp.shape == (p['B'], p['H'], p['Nq'], p['hd'])
        assert torch.equal(rp, A.reference(p, s['vals']))
        if p['scale'] is None:
            v = s['vals']
            eb = EB.attn_ref(v['q'], v['k'], v['v'], v['mask'], p['pre'])
            assert float((rp - eb).abs().max()) <= 1e-12 * float(eb.abs().max())
        if p['masked']:                                            # no row is fully blocked; row 0 loses its later tiles, row 1 keeps the last key only
            m = s['vals']['mask']
            assert not bool(m.all(-1).any())
            if not p['m_rs0']:
                assert bool(m[:, 0, 64:].all()) and int((~m[:, 1]).sum()) == p['B'] and not bool(m[:, 1, -1].any())
        # a planted key carries its row: dropping it would move the row by O(|v|)
        v = s['vals']
        keys = A.split_keys(p['Nk'], p['nsplit'])
        assert v['planted'] == keys and p['Nk'] - 1 in keys and 0 in keys
        if p['scale'] is None:
            sc = (v['q'].double() @ v['k'].double().transpose(-1, -2)) * (A.LN2 if p['pre'] else p['hd'] ** -0.5)
            if v['mask'] is not None:
                sc = sc.masked_fill(v['mask'][:, None], float('-inf'))
            pr = sc.softmax(-1)
            for i, key in enumerate(keys):
                assert float(pr[:, :, 2 * i + 3, key].min()) > 0.5, (name, key)
        dt = s['o'].alloc.dtype
        if p['out'] != 'x3h':
            assert not bool((G.bits(rp.to(dt)) == G.SENTINEL[dt]).any())


# ------------------------------------------------------------------------------------------------------------------------------ planted mistakes
def emulate(s, mistake=None):
    """a plain restatement of the kernel's addressing on the flat allocations of a built 16-bit set: operands read through the strides, O (and the split-K
    workspace rows) stored through them.  Mistakes: 'store_le' stores row Nq as well (`q <= p.Nq`), 'ws_row' indexes the workspace rows over Nq + 1,
    'pad_key' lets key Nk through (the row after the last K row, the column after the last V^T column)."""
    p = s['p']
    B, H, Nq, Nk, hd = p['B'], p['H'], p['Nq'], p['Nk'], p['hd']
    nk = Nk + (1 if mistake == 'pad_key' else 0)
    q = s['q'].alloc[A.index4(s['q'].base, (B, H, Nq), s['q'].strides, hd)].double()
    k = s['k'].alloc[A.index4(s['k'].base, (B, H, nk), s['k'].strides, hd)].double()
    v = s['vt'].alloc[A.index4(s['vt'].base, (B, H, hd), s['vt'].strides, nk)].double().transpose(-1, -2)
    sc = (q @ k.transpose(-1, -2)) * (A.LN2 if p['pre'] else hd ** -0.5)
    if s['mask'] is not None:
        m = s['mask']
        mb = m.alloc[m.base + torch.arange(B)[:, None, None] * m.strides[0] + torch.arange(Nq)[None, :, None] * m.strides[1] + torch.arange(nk)[None, None]]
        sc = sc.masked_fill(mb[:, None] != 0, float('-inf'))
    y = sc.softmax(-1) @ v
    o = s['o']
    out = G.Buf(o.alloc.clone(), o.base, o.idx.shape, o.strides, o.idx, True, o.ld)
    rows = Nq + (1 if mistake == 'store_le' else 0)
    if rows > Nq:
        y = torch.cat([y, y[:, :, -1:]], 2)
    out.alloc[A.index4(o.base, (B, H, rows), o.strides, hd).reshape(-1)] = y.to(o.alloc.dtype).reshape(-1)
    ws = None
    if s['ws'] is not None:
        w = s['ws']
        ws = G.Buf(w.alloc.clone(), w.base, w.idx.shape, w.strides, w.idx, True, w.ld)
        nq = Nq + (1 if mistake == 'ws_row' else 0)
        row = (torch.arange(B)[:, None, None] * H + torch.arange(H)[None, :, None]) * nq + torch.arange(Nq)[None, None]
        rows_all = B * H * Nq
        for sp in range(p['nsplit']):
            at = w.base + ((sp * rows_all + row) * hd).reshape(-1, 1) + torch.arange(hd)[None]
            ws.alloc[at.reshape(-1)] = 1.0
            ml = w.base + p['nsplit'] * rows_all * hd + ((sp * rows_all + row) * 2).reshape(-1, 1) + torch.arange(2)[None]
            ws.alloc[ml.reshape(-1)] = 1.0
    return out, ws


def _reported(name, tight, padded):
    caught = []
    for chk, args in ((G.check_bits, (name, tight, padded)), (G.check_outside, (name, padded)), (G.check_no_nan, (name, padded))):
        try:
            chk(*args)
        except AssertionError as e:
            caught.append(chk.__name__)
    return caught


@pytest.mark.parametrize('name', ['h64_b64_open', 'h96_b64_mask_shared', 'h64_b64_split_mask', 'h64_neg_batch_stride'])
def test_planted_mistakes_are_reported(name):
    c = A.BY_NAME[name]
    tight, padded = A.build(c, 'bf16', False)[0], A.build(c, 'bf16', True)[0]
    ref, ref_ws = emulate(tight)
    good, good_ws = emulate(padded)
    assert _reported(name, ref, good) == []                                            # the method passes a correct kernel
    if good_ws is not None:
        G.check_outside(name, good_ws)
        assert not bool((G.bits(good_ws.logical()) == G.SENTINEL[torch.float32]).any())
    bad, _ = emulate(padded, 'store_le')
    assert _reported(name, ref, bad) == ['check_outside']                              # (c): a row past Nq
    bad, _ = emulate(padded, 'pad_key')
    # (b), (d): the poison got in.  Under a mask the 0xFF of the mask pad blocks key Nk by itself: that mistake is the open cases' to find
    assert set(_reported(name, ref, bad)) == (set() if c['problems'][0]['masked'] else {'check_bits', 'check_no_nan'})
    if good_ws is not None:
        _, bad_ws = emulate(padded, 'ws_row')
        with pytest.raises(AssertionError, match='outside the logical region'):
            G.check_outside(name, bad_ws)                                              # (c) on the workspace
