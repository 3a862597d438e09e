"""The checkpoint retriever's host side (panst3r_amd/model/retrieval.py): loader layouts, the parameter and key checks, and known-answer cases of
the float64 restatement (tests/retrieval_ref.py) that the GPU tests compare against, and the constructions of the kernel-level cases
(tests/test_hip_retrieval_kernels.py): that their float64 answers are the only admissible ones.  No GPU needed."""
import numpy as np
import pytest
import torch

import errbound
import retrieval_ref as R
from panst3r_amd.model.retrieval import RetrievalASMK, RetrievalSpecError


def small(**kw):
    kw.setdefault('k', 64)
    return R.make_dict(3, **kw)


@pytest.mark.parametrize('layout', ['dict', 'tensor', 'array'])
def test_loader_codebook_layouts(layout):
    ck = small(layout=layout)
    r = RetrievalASMK(ck)
    assert (r.k, r.D, r.d_in, r.nfeat) == (64, 128, 128, 40)
    assert torch.equal(r.centroids, torch.from_numpy(R.centroids_of(ck).astype(np.float32)))
    assert r.params == dict(ma_db=1, ma_q=5, alpha=3.0, tau=0.0)


def test_loader_reads_a_path(tmp_path):
    ck = small(hdims='96', prewhiten=True)
    f = tmp_path / 'retrieval.pth'
    torch.save(ck, str(f))
    r = RetrievalASMK(str(f))
    assert (r.k, r.D) == (64, 128) and [s[0] for s in r.stages] == ['white', 'proj']
    with pytest.raises(FileNotFoundError):
        RetrievalASMK(str(tmp_path / 'missing.pth'))


@pytest.mark.parametrize('hdims,pre,post,residual,d_out', [('', False, False, False, None), ('96', True, False, True, None), ('128_64', False, True, False, None),
                                                           ('', True, True, False, 96), ('96', True, True, False, 64)])
def test_loader_head_structures(hdims, pre, post, residual, d_out):
    ck = small(hdims=hdims, prewhiten=pre, postwhiten=post, residual=residual, d_out=d_out)
    r = RetrievalASMK(ck)
    assert r.D == R.centroids_of(ck).shape[1] == (d_out or 128) and r.d_in == 128
    kinds = (['white'] if pre else []) + (['proj'] if (hdims or residual or d_out) else []) + (['white'] if post else [])
    assert [s[0] for s in r.stages] == kinds


def test_defaults_when_params_are_absent():
    r = RetrievalASMK(small(params={}))
    assert r.params == dict(ma_db=1, ma_q=5, alpha=3.0, tau=0.0)


@pytest.mark.parametrize('path,value,match', [
    (('build_ivf', 'kernel', 'binary'), False, 'binary'),
    (('build_ivf', 'ivf', 'use_idf'), True, 'idf'),
    (('query_ivf', 'search', 'topk'), 10, 'top-k'),
    (('query_ivf', 'similarity', 'similarity_threshold'), -0.1, 'similarity_threshold'),
    (('query_ivf', 'similarity', 'alpha'), 0.0, 'alpha'),
    (('query_ivf', 'quantize', 'multiple_assignment'), 9, 'multiple_assignment'),
])
def test_unsupported_parameters_raise(path, value, match):
    params = {}
    d = params
    for p in path[:-1]:
        d = d.setdefault(p, {})
    d[path[-1]] = value
    with pytest.raises(RetrievalSpecError, match=match):
        RetrievalASMK(small(params=params))


def test_unsupported_head_and_codebook_raise():
    ck = small(d_out=48)                                    # D = 48: not a multiple of 32
    with pytest.raises(RetrievalSpecError, match='multiple of 32'):
        RetrievalASMK(ck)
    ck = small()
    ck['args'].featweights = 'gem'
    with pytest.raises(RetrievalSpecError, match='featweights'):
        RetrievalASMK(ck)
    ck = small()
    ck['asmk_codebook'] = {'weights': np.zeros((4, 128), np.float32), 'params': {}}
    with pytest.raises(RetrievalSpecError, match="'params', 'weights'"):
        RetrievalASMK(ck)
    ck = small()
    del ck['asmk_params']
    with pytest.raises(RetrievalSpecError, match='asmk_params'):
        RetrievalASMK(ck)


def test_mismatched_head_keys_raise():
    ck = small(hdims='96')
    ck['model']['projector.9.weight'] = torch.zeros(3, 3)
    with pytest.raises(RetrievalSpecError, match='unexpected keys projector.9.weight'):
        RetrievalASMK(ck)
    ck = small(hdims='96')
    del ck['model']['projector.1.bias']
    with pytest.raises(RetrievalSpecError, match='missing key projector.1.bias'):
        RetrievalASMK(ck)
    ck = small(hdims='96')
    ck['args'].hdims = '64'
    with pytest.raises(RetrievalSpecError, match='hdims'):
        RetrievalASMK(ck)
    ck = small(hdims='96', prewhiten=True)
    del ck['model']['prewhiten.p']
    with pytest.raises(RetrievalSpecError, match='prewhiten.p'):
        RetrievalASMK(ck)
    ck = small()
    ck['model']['postwhiten.m'] = torch.zeros(1, 64, dtype=torch.float64)
    ck['model']['postwhiten.p'] = torch.zeros(64, 64, dtype=torch.float64)
    with pytest.raises(RetrievalSpecError, match='outputs 64 dims, the codebook has 128'):
        RetrievalASMK(ck)
    ck = small()                                           # backbone.* keys are ignored
    ck['model']['backbone.enc_blocks.0.attn.qkv.weight'] = torch.zeros(2, 2)
    RetrievalASMK(ck)


# ---------------------------------------------------------------------------------------------------- restatement known answers
D = 32


def _basis(w):
    e = np.zeros(D)
    e[w] = 10.0
    return e


def _desc(w, signs, mag=0.1, second=None):
    """a descriptor at 10 e_w + residual with the given signs (second-nearest word steered by a larger residual on that axis)"""
    r = mag * np.asarray(signs, dtype=np.float64)
    if second is not None:
        r[second] = 0.5
    return _basis(w) + r


def test_restatement_known_answers():
    cent = np.stack([_basis(w) for w in range(3)])
    plus = np.ones(D)
    plus[[0, 1, 2]] = 1
    flip8 = plus.copy()
    flip8[8:16] = -1                                       # D / 4 of the signs flipped
    # view 0: one descriptor on word 0; view 1: the same signs on word 0, one on word 1; view 2: word 0 with D/4 signs flipped
    desc = np.stack([_desc(0, plus, second=1), _desc(0, plus, second=1), _desc(1, plus, second=2), _desc(0, flip8, second=2)])
    counts = [1, 2, 1]
    ids, dist = R.assign(desc, cent, 2)
    assert ids.tolist() == [[0, 1], [0, 1], [1, 2], [0, 2]]
    assert np.all(np.diff(dist, axis=1) >= 0)
    agg = R.aggregate(desc, cent, ids, counts, 1)
    assert [w for w, _ in agg[1]] == [0, 1]
    assert np.array_equal(agg[0][0][1] > 0, plus > 0) and np.array_equal(agg[2][0][1] > 0, flip8 > 0)
    S = R.scores(agg, agg, D, 3.0, 0.0)
    assert S[0, 1] == 1.0 and S[1, 0] == 1.0                # identical residual signs: kappa = 1
    assert S[0, 2] == 0.5 ** 3 and S[2, 0] == 0.5 ** 3      # D / 4 flipped bits: s = 0.5
    assert S[1, 1] == 2.0 and S[0, 0] == 1.0
    S = R.scores(agg, agg, D, 3.0, 0.6)                     # the flipped word is below tau
    assert S[0, 2] == 0.0 and S[0, 1] == 1.0
    # the fp32 emulation of the kernel gives the same exact values here
    words = [[w for w, _ in agg[v]] for v in range(3)]
    bits = [np.stack([s > 0 for _, s in agg[v]]) for v in range(3)]
    assert np.array_equal(R.scores_f32(words, bits, words, bits, D, 3.0, 0.0), R.scores(agg, agg, D, 3.0, 0.0).astype(np.float32))


def test_restatement_multiple_assignment_and_asymmetry():
    """query side with ma = 2: a descriptor also joins its second word, so S is not symmetric"""
    cent = np.stack([_basis(w) for w in range(3)])
    plus = np.ones(D)
    desc = np.stack([_desc(0, plus, second=1), _desc(1, plus, second=2)])
    ids, _ = R.assign(desc, cent, 2)
    q = R.aggregate(desc, cent, ids, [1, 1], 2)
    db = R.aggregate(desc, cent, ids, [1, 1], 1)
    S = R.scores(q, db, D, 3.0, 0.0)
    assert [w for w, _ in q[0]] == [0, 1] and [w for w, _ in db[1]] == [1]
    assert S[0, 1] != 0.0 and S[1, 0] == 0.0


def test_selection_ties_go_to_the_lower_token():
    ck = small(k=64, nfeat=2)
    x = np.zeros((4, 128))
    x[:, 0] = [1.0, 2.0, 2.0, 0.5]                          # identity head: rows 1 and 2 tie
    desc, counts, toks = R.descriptors(ck, [x])
    assert counts == [2] and toks[0].tolist() == [1, 2]
    ck = small(k=64, nfeat=10)                              # nfeat above T keeps every row
    assert R.descriptors(ck, [x])[1] == [4]


# ---------------------------------------------------------------------------------------------------- kernel-level cases
@pytest.mark.parametrize('nfeat', [1, 64, 300])
@pytest.mark.parametrize('D', [72, 128])
def test_select_case_has_one_admissible_order(nfeat, D):
    """neighbouring float64 norms differ by >= 1e-3 relative unless the two rows are bit-identical (then the token decides), so that lexsort is the
    only order a correct fp32 ranking can give; the planted ties are where the docstring says"""
    case = R.select_case(11, nfeat, D)
    x, Ts, counts = case['x'], case['Ts'], case['counts']
    assert Ts == [1, 5, 256, 257, 300, 700] and counts == [min(nfeat, T) for T in Ts] and x.dtype == np.float32 and x.shape == (sum(Ts), D)
    toks, rows = R.select_ref(x, Ts, counts)
    off, ooff = np.concatenate([[0], np.cumsum(Ts)]), np.concatenate([[0], np.cumsum(counts)])
    nties = 0
    for v, T in enumerate(Ts):
        h = x[off[v]:off[v + 1]].astype(np.float64)
        nrm = np.sqrt((h * h).sum(-1))
        order = np.lexsort((np.arange(T), -nrm))
        for a, b in zip(order[:-1], order[1:]):
            if nrm[a] == nrm[b]:
                assert np.array_equal(h[a].view(np.int64), h[b].view(np.int64)) and a < b        # same bits -> same fp32 key; the lower token first
                nties += 1
            else:
                assert nrm[a] - nrm[b] >= 1e-3 * nrm[a]
    assert nties == len(case['ties']) + 1                       # + the two all-zero rows
    sel = [set(toks[ooff[v]:ooff[v + 1]].tolist()) for v in range(len(Ts))]
    for v, lo, hi in case['ties']:
        a, b = x[off[v] + lo], x[off[v] + hi]
        assert lo < hi and np.array_equal(a.view(np.int32), b.view(np.int32)) and np.any(a != 0)
    assert [(v, lo, hi) for v, lo, hi in case['ties'] if (lo, hi) == (3, 260)] == [(4, 3, 260), (5, 3, 260)]
    for v, (T, n) in enumerate(zip(Ts, counts)):               # every cut view: a pair of which exactly the lower token is kept, as the last row
        if n < T:
            cut = [(lo, hi) for vv, lo, hi in case['ties'] if vv == v and lo in sel[v] and hi not in sel[v]]
            assert len(cut) == 1 and toks[ooff[v + 1] - 1] == cut[0][0]
    assert [v for v, _ in case['zeros']] == [1, 1] and all(not x[off[v] + t].any() for v, t in case['zeros'])
    (v, t), = case['tiny']
    assert 0 < np.linalg.norm(x[off[v] + t].astype(np.float64)) < 1e-12
    if counts[1] == Ts[1]:                                      # nsel == T: the zero rows are selected (last, lower token first) and come out as zeros
        z = sorted(t for _, t in case['zeros'])
        assert toks[ooff[2] - 2:ooff[2]].tolist() == z and not rows[ooff[2] - 2:ooff[2]].any()
        assert toks[ooff[2] - 3] == t and abs(np.linalg.norm(rows[ooff[2] - 3]) - 0.1) < 1e-3      # clamped: x / 1e-12, not unit length
    keep = np.ones(len(rows), bool)
    if counts[1] == Ts[1]:
        keep[ooff[2] - 3:ooff[2]] = False
    assert np.allclose(np.linalg.norm(rows[keep], axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize('D', [72, 128])
def test_select_bound_covers_the_fp32_steps(D):
    """an fp32 emulation of the kernel's steps (fma chains, butterfly, sqrt, clamp, division) stays below half of errbound.select_bound; a key that
    misses the lane tail (columns past the last multiple of 64) or a norm taken without the root does not"""
    case = R.select_case(11, 300, D)
    x = case['x']
    h = x.astype(np.float64)
    ref = h / np.maximum(np.sqrt((h * h).sum(-1)), 1e-12)[:, None]
    bound = errbound.select_bound(torch.from_numpy(ref), D)
    r = errbound.check(torch.from_numpy(R.select_f32(x)), torch.from_numpy(ref), bound, 'select emulation D=%d' % D)
    print('select fp32 emulation, D = %d: worst |err| / bound = %.3g' % (D, r))
    assert r <= 0.5
    if D % 64:
        f = np.float32
        key = (x[:, :D // 64 * 64].astype(np.float64) ** 2).sum(-1)
        bad = (x / np.maximum(np.sqrt(key), 1e-12)[:, None]).astype(f)
        with pytest.raises(AssertionError, match='exceed the error bound'):
            errbound.check(torch.from_numpy(bad), torch.from_numpy(ref), bound, 'dropped lane tail')
    bad = (h / np.maximum((h * h).sum(-1), 1e-12)[:, None]).astype(np.float32)
    with pytest.raises(AssertionError, match='exceed the error bound'):
        errbound.check(torch.from_numpy(bad), torch.from_numpy(ref), bound, 'no root')


def test_assign_case_pairs_and_splits():
    """the planted centroid pairs are bit-identical, each is the float64 top 2 of its descriptor row (lower index first), and they sit where the
    split arithmetic of retrieval_assign (chunk = ceil(tiles / nsplit) tiles of 64) puts them in the places the GPU test names"""
    k, pairs = R.ASSIGN_K, R.ASSIGN_PAIRS
    tiles = (k + 63) // 64
    assert tiles == 6 and k - 64 * (tiles - 1) == 1 and max(b for _, b in pairs) == k - 1
    for n in (1, 129):
        x, c, near = R.assign_case(5, n)
        assert x.shape == (n, R.ASSIGN_D) and c.shape == (k, R.ASSIGN_D) and x.dtype == c.dtype == np.float32
        for a, b in pairs:
            assert a < b and np.array_equal(c[a].view(np.int32), c[b].view(np.int32))
        assert len(near) == min(n, len(pairs)) and near[0][2] == k - 1
        ids, dist = R.assign(x.astype(np.float64), c.astype(np.float64), 3)
        for row, a, b in near:
            assert ids[row, :2].tolist() == [a, b] and dist[row, 0] == dist[row, 1] and dist[row, 2] - dist[row, 1] > 0.1
    split = lambda c_, ns: c_ // (-(-tiles // ns) * 64)
    a, b = pairs[0]
    assert a // 16 == b // 16 and (a % 16) // 4 != (b % 16) // 4                       # one 16-centroid subtile, two lane groups
    a, b = pairs[1]
    assert a // 64 != b // 64 and split(a, 2) == split(b, 2) and split(a, 4) != split(b, 4)
    a, b = pairs[2]
    assert all(split(a, ns) != split(b, ns) for ns in (2, 4, 5, 6))
    a, b = pairs[3]
    assert all(split(a, ns) == split(b, ns) for ns in (1, 2, 4, 5)) and split(a, 6) != split(b, 6)
    starts = lambda ns: [s * (-(-tiles // ns) * 64) for s in range(ns)]
    assert [s >= k for s in starts(4)] == [False, False, False, True] and [s >= k for s in starts(5)] == [False, False, False, True, True]
    assert k - starts(6)[-1] == 1                                                      # nsplit = 6: the last split holds one centroid, fewer than m = 5 or 8


def test_bit_packing_convention():
    b = np.zeros((2, 96), bool)
    b[0, 0] = b[0, 33] = b[1, 95] = True
    w = R.pack_bits(b)
    assert w.dtype == np.uint32 and w.tolist() == [[1, 2, 0], [0, 0, 1 << 31]]          # bit j of word w = component 32 w + j
    assert np.array_equal(R.unpack_bits(w), b) and np.array_equal(R.unpack_bits(w.view(np.int32)), b)


@pytest.mark.parametrize('D', [32, 96, 288, 1024])
def test_aggregate_case_planted_signs(D):
    case = R.aggregate_case(9, D)
    x, cent, member, gstart, gword = (case[k] for k in ('x', 'cent', 'member', 'gstart', 'gword'))
    s64, bound = R.aggregate_ref(x, cent, member, gstart, gword)
    sizes = np.diff(gstart).tolist()
    assert sizes == [1, 70, 70, 1, 70] and all(np.all(np.diff(member[gstart[g]:gstart[g + 1]]) > 0) for g in range(5))
    assert np.count_nonzero(member == 0) == 2 and np.count_nonzero(member == 5) == 2      # descriptors that belong to several groups
    for g, pat in case['patterns'].items():                    # decided far outside the bound: the bits are the pattern whatever the rounding
        assert np.array_equal(s64[g] > 0, pat) and np.all(np.abs(s64[g]) > 1e4 * bound[g]) and 0 < pat.sum() < D
    z = case['zero_group']
    assert not s64[z].any() and np.array_equal(x[member[gstart[z]]].view(np.int32), cent[gword[z]].view(np.int32))
    assert np.any(s64[1] > 0) and np.any(s64[1] < 0) and np.all(bound > 0)


@pytest.mark.parametrize('D', [32, 96, 1024])
def test_scores_case_planted_words_and_bits(D):
    case = R.scores_case(21, D)
    qw, qb, dw, db = case['qwords'], case['qbits'], case['dwords'], case['dbits']
    assert [len(w) for w in qw] == R.SCORES_Q and [len(w) for w in dw] == R.SCORES_DB
    assert all(np.all(np.diff(w) > 0) for w in qw + dw) and all(b.shape == (len(w), D) for w, b in zip(qw + dw, qb + db))
    lo, hi = min(w[0] for w in qw if len(w)), max(w[-1] for w in qw if len(w))
    first, last = qw[2][0], qw[2][-1]
    for w in dw:
        if len(w) >= 4:
            assert w[0] < lo and w[-1] > hi and first in w and last in w and 0.3 < np.isin(w, qw[2]).mean() < 0.8
    assert dw[1].tolist() == [first]
    ham = lambda j, w: int(np.count_nonzero(db[j][list(dw[j]).index(w)] != qb[2][list(qw[2]).index(w)]))
    assert sorted((R.SCORES_DB[j], w == first, h) for j, w, h in case['planted']) == [(1, True, D // 8), (130, False, D // 4 + 1), (130, True, D // 4), (300, False, D), (300, True, 0)]
    assert all(ham(j, w) == h for j, w, h in case['planted'])
    # s == tau exactly counts: the planted h = D / 4 group alone gives 0.5^3 under tau = 0.5, its h = D / 4 + 1 neighbour and the complement give 0
    one = lambda j, w: R.scores_f32([[w]], [qb[2][[list(qw[2]).index(w)]]], [[w]], [db[j][[list(dw[j]).index(w)]]], D, 3.0, 0.5)[0, 0]
    got = {(R.SCORES_DB[j], h): one(j, w) for j, w, h in case['planted']}
    assert got == {(1, D // 8): np.float32(0.421875), (130, D // 4): np.float32(0.125), (130, D // 4 + 1): 0.0, (300, D): 0.0, (300, 0): 1.0}
    S = R.scores_f32(qw, qb, dw, db, D, 3.0, 0.0)
    assert not S[0].any() and not S[:, 0].any() and np.all(S[2, 1:] != 0) and len(np.unique(S[2])) == 7
