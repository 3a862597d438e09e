"""The cases of tests/gemm_layout_cases.py are what they claim (CPU only, no GPU), as tests/test_geom_stage_checks.py shows for the geometry cases.

Every case satisfies the argument rules of gemm_validate / gemm_f32_validate and reaches the class it names under rowstream_class /
gemm256_persistent_class / gemm_choice, all restated in Python from the source: a case the device would refuse, or send elsewhere, fails here first.
Every declared pad and offset is really in the built tensors, the padded set's logical contents equal the tight set's, every input element outside the
logical region is NaN, every output element holds the sentinel, and the sentinel occurs nowhere in the float64 reference rounded to the output format.
The table holds, for every (variant, store mode) the layout tests are about, a case with a padded A, one with a padded C, one with a base offset and -
for 16-bit row-major stores - one whose rows of C are 8-byte but not 16-byte aligned.  Two planted mistakes - "store row m of C at m N" and "load row m of
A at m K" - applied to a numpy-style emulation of a padded case are each reported by the checks the GPU module runs."""
import pytest
import torch

import gemm_layout_cases as G

BIG = ('pair256p',)                          # built once, in one format: two problems of ~30 000 rows each
PARAMS = [(c['name'], fmt) for c in G.CASES for fmt in c['fmts'] if c['name'] not in BIG or fmt == 'bf16']


def _bufs(s):
    return [(k, s[k]) for k in ('a', 'w', 'c', 'res', 'xcopy', 'stats') if k in s]


@pytest.mark.parametrize('name,fmt', PARAMS)
def test_case_is_admitted_and_reaches_its_variant(name, fmt):
    c = G.BY_NAME[name]
    for padded, want in ((True, c['variant']), (False, c['tight_variant'])):
        sets = G.build(c, fmt, padded)
        for s in sets:
            assert G.validate(s) is None, (name, padded, G.validate(s))
        got = G.predicted_pair_variant(sets) if c['kind'] == 'pair' else G.predicted_variant(sets[0])
        assert got == want, (name, padded, got, want)
        if c['variant'] == 'gemm256p_kernel':
            assert G.persistent_class(sets[0]) == {'plain': 1 if sets[0]['p']['out'] == '16' else 2, 'trans': 3}[sets[0]['p']['mode']]
        if c['variant'] == 'gemm256_kernel' and padded:
            assert G.persistent_class(sets[0]) == 0
        if c['variant'] == 'rowgemm384_kernel':
            assert G.rowstream_class(sets[0]) == (2 if sets[0]['p']['res'] else 1)
        if c['tight_variant'] == 'rowgemm384_kernel' and c['variant'] != 'rowgemm384_kernel':
            assert G.rowstream_class(sets[0]) == (0 if padded else (2 if sets[0]['p']['res'] else 1))      # one step outside the class
        for knob, value in c['tune'].items():
            if knob == G.TUNE_DEEP_RING:         # the deep ring only takes a launch of at most one tile per CU with K >= 512
                p = sets[0]['p']
                assert value in (6, 8) and ((p['M'] + 63) // 64) * ((p['N'] + 63) // 64) <= 256 and p['K'] >= 512 and got == 'gemm_kernel<2,2,false>'
            if knob == G.TUNE_CUS:               # fewer workgroups than tiles: some walk to a second tile
                p = sets[0]['p']
                assert value < ((p['M'] + 255) // 256) * ((p['N'] + 255) // 256)


@pytest.mark.parametrize('name,fmt', PARAMS)
def test_layout_is_the_declared_one(name, fmt):
    c = G.BY_NAME[name]
    tight, padded = G.build(c, fmt, False), G.build(c, fmt, True)
    for t, s in zip(tight, padded):
        p = s['p']
        width = dict(a=p['K'] if not p['conv'] else p['conv'][0], w=p['K'], res=p['N'], xcopy=p['N'])
        for key, buf, pad, off in (('a', s['a'], 'pad_a', 'off_a'), ('w', s['w'], 'pad_w', 'off_w'), ('res', s.get('res'), 'pad_r', 'off_r'),
                                   ('xcopy', s.get('xcopy'), 'pad_x', 'off_x')):
            if buf is None:
                continue
            assert buf.ld == width[key] + p[pad] and buf.view().stride(0) == buf.ld and buf.view().stride(1) == 1, (name, key)
            assert buf.base % buf.ld == p[off] or buf.base == p[off], (name, key, buf.base)
            assert t[key].ld == width[key] and t[key].base == 0
        cb = s['c']
        if p['mode'] in ('plain', 'conv'):
            assert cb.ld == p['N'] + p['pad_c'] and t['c'].ld == p['N']
        elif p['mode'] == 'trans':
            assert cb.ld == G.up(p['M'], 8) + p['pad_c'] and p['pad_c'] == 8            # ldc = roundup8(M) + 8
        elif p['mode'] == 'x3':
            assert cb.ld == 3 * p['x3_block'] + p['pad_c']
        assert cb.base == G.GUARD * cb.ld + p['off_c'] and t['c'].base == 0 and cb.view().stride(0) == cb.ld
        if 'stats' in s:
            assert s['stats'].ld == p['N'] // 64 + p['pad_s'] and s['stats'].view().is_contiguous() and s['stats'].view().shape[1] == s['stats'].ld
        # every pad and offset the case declares is non-zero in the tensors, and the case declares at least one
        declared = [k for k in G.LAYOUT_KEYS if p[k]]
        assert declared, name
        for (k, bt), (_, bp) in zip(_bufs(t), _bufs(s)):
            assert bt.idx.shape == bp.idx.shape
            lt, lp = G.bits(bt.logical()), G.bits(bp.logical())
            assert torch.equal(lt, lp), (name, k)                                       # equal logical contents
            outside = bp.outside_mask()
            if bp.out:                                                                  # sentinel everywhere outside, and inside unless the residual sits there
                assert bool((G.bits(bp.alloc)[outside] == G.SENTINEL[bp.alloc.dtype]).all())
                if not (k == 'c' and p['inplace']):
                    assert bool((lp == G.SENTINEL[bp.alloc.dtype]).all())
                lo, hi = int(bp.idx.min()), int(bp.idx.max())
                assert lo >= G.GUARD * bp.ld and bp.alloc.numel() - 1 - hi >= G.GUARD * bp.ld - bp.ld, (name, k)       # guard rows before and after
            else:                                                                       # poison everywhere outside, none inside
                assert bool(torch.isnan(bp.alloc[outside]).all()) and int(outside.sum()) > 0, (name, k)
                assert not bool(torch.isnan(bp.logical()).any())


@pytest.mark.parametrize('name,fmt', [q for q in PARAMS if q[0] not in BIG])
def test_reference_never_holds_the_sentinel(name, fmt):
    c = G.BY_NAME[name]
    for s in G.build(c, fmt, False):
        ref = G.reference(s['p'], s['vals'])
        assert ref.shape[-2:] == (s['p']['M'], s['p']['N']) and bool(torch.isfinite(ref).all())
        dt = s['c'].alloc.dtype
        assert not bool((G.bits(ref.to(dt)) == G.SENTINEL[dt]).any())
        assert ref.shape == s['c'].idx.shape[-ref.dim():]


def test_sentinels_are_distinct_nans():
    for dt, v in G.SENTINEL.items():
        t = torch.tensor([v], dtype=G._INT[dt]).view(dt)
        assert bool(torch.isnan(t).all())
    assert len(set(G.SENTINEL.values())) == 3
    assert G.bits(torch.tensor([float('nan')], dtype=torch.float32))[0] != G.SENTINEL[torch.float32]


ROW16 = ['gemm_kernel<2,2,false>', 'gemm_kernel<4,4,false>', 'gemm256_kernel']
REQUIRED = [(v, st) for v in ROW16 for st in ('plain-16', 'plain-f32')] + \
           [('gemm_kernel<2,2,true>', 'trans-16'), ('gemm_kernel<4,4,true>', 'trans-16'), ('gemm256p_kernel', 'plain-16'), ('gemm256p_kernel', 'plain-f32'),
            ('gemm256p_kernel', 'trans-16'), ('rowgemm384_kernel', 'plain-16'), ('gemm_pair_kernel<2,2>', 'plain-16'), ('gemm256p2_kernel', 'plain-16'),
            ('gemm_kernel<2,2,false>', 'batch-16'), ('gemm_kernel<2,2,true>', 'batch-trans'), ('gemm_kernel<2,2,false>', 'conv-f32'),
            ('gemm_kernel<2,2,false>', 'ps-16'), ('gemm_kernel<2,2,false>', 'x3-f32'), ('gemm_f32_kernel', 'plain-f32')]


@pytest.mark.parametrize('variant,store', REQUIRED)
def test_table_covers_every_variant_and_store_mode(variant, store):
    ps = [p for c in G.CASES if c['variant'] == variant and c['store'] == store for p in c['problems']]
    assert ps, (variant, store)
    if store not in ('conv-f32',):                                                     # the implicit convolution's lda is conv_c by definition
        assert any(p['pad_a'] > 0 for p in ps) or variant == 'rowgemm384_kernel'       # (the row-streaming classes need lda = 384: their fallback cases pad it)
    if not store.startswith('ps'):                                                     # the pixel-shuffle store has no ldc
        assert any(p['pad_c'] > 0 for p in ps)
    assert any(p['off_a'] or p['off_w'] or p['off_c'] for p in ps)
    if variant in ROW16 and store == 'plain-16':                                       # rows of C that are 8-byte but not 16-byte aligned
        assert any((p['N'] + p['pad_c']) % 8 == 4 for p in ps)
        # ... and next to it the interior fast store: no residual, no statistics, ldc % 8 == 0 != pad_c, a 16-byte aligned padded C, a whole tile inside
        T = {'gemm_kernel<2,2,false>': 64, 'gemm_kernel<4,4,false>': 128, 'gemm256_kernel': 256}[variant]
        fast = [p for p in ps if not p['res'] and not p['producer'] and p['pad_c'] and (p['N'] + p['pad_c']) % 8 == 0 and p['off_c'] % 8 == 0
                and p['M'] >= T and p['N'] >= T]
        assert fast and any(p['grp'] for p in fast) and any(p['rope'] for p in fast) and any(p['off_c'] for p in fast), variant
    if variant == 'rowgemm384_kernel':
        assert any(c['tight_variant'] == variant and c['variant'] != variant and c['problems'][0]['pad_a'] for c in G.CASES)
    names = {c['variant'] for c in G.CASES}
    assert {'gemm_kernel<2,2,false>', 'gemm_kernel<4,4,false>', 'gemm256_kernel', 'gemm_kernel<2,2,true>', 'gemm_kernel<4,4,true>', 'gemm256p_kernel',
            'rowgemm384_kernel', 'gemm_pair_kernel<2,2>', 'gemm256p2_kernel', 'gemm_f32_kernel'} <= names


def test_remap_cases_cross_a_group_boundary_inside_a_tile():
    tile = {'gemm_kernel<2,2,false>': 64, 'gemm_kernel<4,4,false>': 128, 'gemm256_kernel': 256}
    seen = set()
    for c in G.CASES:
        for p in c['problems']:
            if p['grp'] and c['variant'] in tile:
                gi, go, goff = p['grp']
                assert p['M'] // gi >= 2 and p['M'] % gi == 0 and go > gi and goff > 0, c['name']          # several groups: the quot * grp_out step is taken
                assert gi % tile[c['variant']] != 0, c['name']                                              # ... in the middle of a tile
                seen.add(c['variant'])
    assert seen == set(tile)


def test_pads_of_the_issue_are_all_used():
    ps = [p for c in G.CASES for p in c['problems']]
    h = [p for p in ps if not p['f32']]
    assert {8, 72} <= {p['pad_a'] for p in h} and any(p['pad_w'] == 8 for p in h) and any(p['off_a'] == 8 for p in h) and any(p['off_w'] == 8 for p in h)
    c16 = [p for p in h if p['out'] == '16' and p['mode'] == 'plain']
    assert {4, 8, 24} <= {p['pad_c'] for p in c16} and any(p['off_c'] == 4 for p in c16)
    c32 = [p for p in h if p['out'] == 'f32' and p['mode'] == 'plain']
    assert {4, 12} <= {p['pad_c'] for p in c32} and any(p['off_c'] == 4 for p in c32)
    assert any(p['res'] == 'f32' and p['pad_r'] == 4 and not p['inplace'] for p in h) and any(p['res'] == '16' and p['pad_r'] == 8 and not p['inplace'] for p in h)
    assert any(p['res'] == 'f32' and p['inplace'] for p in h) and any(p['res'] == '16' and p['inplace'] for p in h)
    assert {4, 8} <= {p['pad_x'] for p in h if p['producer']} and any(p['pad_s'] == 1 for p in h)
    pair = G.BY_NAME['pair256p']['problems']
    assert all(pair[0][k] != pair[1][k] for k in ('pad_a', 'pad_c'))                   # a leading dimension taken from the wrong problem shows


# ------------------------------------------------------------------------------------------------------------------------------ planted mistakes
def emulate(s, mistake=None):
    """a plain restatement of the row-major GEMM on the flat allocations of a built set: row m of A is read at m lda, row m of C stored at m ldc
    (mistake 'ldc_is_n': at m N; 'lda_is_k': A read at m K)"""
    p = s['p']
    a, w, c = s['a'], s['w'], s['c']
    M, N, K = p['M'], p['N'], p['K']
    lda = K if mistake == 'lda_is_k' else a.ld
    ldc = N if mistake == 'ldc_is_n' else c.ld
    A = a.alloc[a.base + torch.arange(M)[:, None] * lda + torch.arange(K)[None]].double()
    W = w.alloc[w.base + torch.arange(N)[:, None] * w.ld + torch.arange(K)[None]].double()
    y = A @ W.T
    if p['bias']:
        y = y + s['vals']['bias'].double()
    out = G.Buf(c.alloc.clone(), c.base, c.shape, c.strides, c.idx, True, c.ld)
    out.alloc[c.base + torch.arange(M)[:, None] * ldc + torch.arange(N)[None]] = y.to(c.alloc.dtype)
    return out


def _reported(name, tight, padded):
    caught = []
    for chk, args in ((G.check_bits, (name, tight, padded)), (G.check_outside, (name, padded)), (G.check_no_nan, (name, padded))):
        try:
            chk(*args)
        except AssertionError as e:
            caught.append((chk.__name__, str(e)))
    return caught


@pytest.mark.parametrize('name', ['t128_plain16', 't64_plain32', 't256_plain16_ldc24'])
def test_planted_mistakes_are_reported(name):
    c = G.BY_NAME[name]
    tight, padded = G.build(c, 'bf16', False)[0], G.build(c, 'bf16', True)[0]
    ref = emulate(tight)
    assert _reported(name, ref, emulate(padded)) == []                                 # the method passes a correct kernel
    ldc = _reported(name, ref, emulate(padded, 'ldc_is_n'))
    assert 'check_outside' in [k for k, _ in ldc], ldc                                 # (c): names the first stray element
    assert 'row' in dict(ldc)['check_outside'] and 'column' in dict(ldc)['check_outside']
    lda = _reported(name, ref, emulate(padded, 'lda_is_k'))
    assert 'check_no_nan' in [k for k, _ in lda], lda                                  # (d): the poison got in
    assert 'check_bits' in [k for k, _ in lda]


def test_mask_head_and_rowstats_layouts():
    for mc in G.MASK_HEAD_CASES:
        b = G.build_mask_head(mc, 'bf16', True)
        assert (mc['C'], mc['Q'], mc['P'], mc['n']) in ((256, 130, 64, 3), (384, 24, 128, 2))
        assert b['lde'] == mc['C'] + 8 and b['fvs'] == mc['P'] * mc['C'] + 64 and b['ovs'] == mc['Q'] * mc['P'] + 64
        assert b['lde'] % 8 == 0 and b['fvs'] % 8 == 0 and b['ovs'] % 4 == 0 and all(G._aligned(b[k], 16) for k in ('e', 'f', 'out'))
        t = G.build_mask_head(mc, 'bf16', False)
        for k in ('e', 'f'):
            assert torch.equal(G.bits(t[k].logical()), G.bits(b[k].logical())) and bool(torch.isnan(b[k].alloc[b[k].outside_mask()]).all())
        assert bool((G.bits(b['out'].alloc) == G.SENTINEL[torch.float32]).all())
    for rc in G.ROWSTATS_CASES:
        b = G.build_rowstats(rc, 'f16', True)
        assert rc['rows'] == 70 and b['x'].ld == rc['D'] + 4 and b['xcopy'].ld == rc['D'] + 8 and b['sld'] == rc['D'] // 64 + 1
        assert G._aligned(b['x'], 16) and G._aligned(b['xcopy'], 8) and bool(torch.isnan(b['x'].alloc[b['x'].outside_mask()]).all())
