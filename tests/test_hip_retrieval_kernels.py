"""The four kernels of csrc/retrieval.hip one by one, at the smallest shapes where their loops repeat, on planted ties and at their refusals, against the
float64 cases of tests/retrieval_ref.py (whose constructions tests/test_retrieval_host.py checks on the CPU).  tests/test_hip_retrieval.py pins the same
kernels at sizes where every loop runs once; a wrong second trip, a swapped half of the ballot word, a tie taken from the higher index or a dropped 65th
group passes there and fails here."""
import numpy as np
import pytest
import torch

import errbound
import retrieval_ref as R
from panst3r_amd import hip
from test_hip_retrieval import _assign_bound, _check_assign

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -12345.5                 # output sentinel (fp32); inputs are padded with NaN: a read past a row's D columns poisons the result
ISENT = 0x5A5A5A5A              # output sentinel (int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _slice_of_wider(a, left, right, extra, fill):
    """a [rows, cols] -> (buffer [rows + extra, left + cols + right] filled with `fill`, its view [rows, cols] holding a)"""
    rows, cols = a.shape
    buf = torch.full((rows + extra, left + cols + right), fill, dtype=a.dtype, device=DEV)
    view = buf[:rows, left:left + cols]
    view.copy_(a)
    return buf, view


def _bits32(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- select
def _select(x, Ts, counts, D, max_t):
    n, nout = sum(Ts), sum(counts)
    _, xv = _slice_of_wider(_dev(x), 8, 16, 3, float('nan'))                 # ldx = D + 24
    obuf = torch.full((nout + 3, D + 12), SENT, dtype=torch.float32, device=DEV)
    out = obuf[:nout, 4:4 + D]                                              # ldo = D + 12
    sbuf = torch.full((nout + 5,), -7, dtype=torch.int32, device=DEV)
    in_off = _dev(np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32))
    out_off = _dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    assert xv.shape == (n, D) and xv.stride(0) > D and out.stride(0) > D
    hip.retrieval_select(xv, in_off, out_off, out, max_t, sel_idx=sbuf[:nout])
    torch.cuda.synchronize()
    return obuf, out, sbuf


@pytest.mark.parametrize('D', [72, 128])
@pytest.mark.parametrize('nfeat', [1, 64, 300])
def test_select_order_rows_and_padding(nfeat, D):
    """hip.retrieval_select on its own, sel_idx read.  One launch of views with T = 1, 5, 256, 257, 300, 700 tokens: in the views of 257, 300 and 700
    tokens the ranking loop `for (t = threadIdx.x; t < T; t += blockDim.x)` takes a second (700: a third) trip, and with nfeat = 300 the gather loop
    `for (r = wave; r < nsel; r += 4)` runs 75 trips.  D = 72 leaves a lane tail in the key and in the gather (columns 64..71).  Bit-identical rows sit
    at tokens 3 and 260 (either side of 256) and across the selection cut of every cut view: the lower token must come first / be the one kept.  The
    5-token view holds two all-zero rows and one of norm 1e-13, which reach the 1e-12 clamp when nfeat >= 5 keeps them.  Input and output are column
    slices of wider buffers with rows to spare; nothing outside [out_off[v], out_off[v+1]) x [0, D) may change."""
    case = R.select_case(11, nfeat, D)
    x, Ts, counts = case['x'], case['Ts'], case['counts']
    toks, rows = R.select_ref(x, Ts, counts)
    nout = sum(counts)
    obuf, out, sbuf = _select(x, Ts, counts, D, max(Ts))
    sel = sbuf[:nout].cpu().numpy()
    assert np.array_equal(sel, toks), np.nonzero(sel != toks)[0][:8]
    ref = torch.from_numpy(rows)
    r = errbound.check(out, ref, errbound.select_bound(ref, D), 'retrieval_select nfeat=%d D=%d' % (nfeat, D))
    print('select nfeat = %d, D = %d: worst |out - x / max(||x||, 1e-12)| / bound = %.3g' % (nfeat, D, r))
    ooff = np.concatenate([[0], np.cumsum(counts)])
    if counts[1] == Ts[1]:                                      # the all-zero rows: exact zeros, not 0 / 0
        z = out[ooff[2] - 2:ooff[2]]
        assert bool((_bits32(z) == 0).all())
    mask = torch.ones_like(obuf, dtype=torch.bool)
    mask[:nout, 4:4 + D] = False
    assert bool((obuf[mask] == SENT).all()) and bool((sbuf[nout:] == -7).all())
    obuf2, out2, sbuf2 = _select(x, Ts, counts, D, max(Ts))
    assert torch.equal(_bits32(obuf2), _bits32(obuf)) and torch.equal(sbuf2, sbuf)


# ---------------------------------------------------------------------------------------------------- assign
def _assign(x, c, m, nsplit):
    """retrieval_assign with the split descriptors in a slice of a wider f16 buffer (ldx = K3 + 24, a multiple of 8; the padding would wreck a distance
    that read it) and sentinel rows behind ids / dist"""
    n = x.shape[0]
    c3 = hip.split_operand(_dev(c), 1)
    K3 = c3.shape[1]
    buf = torch.full((n + 2, K3 + 24), 30000.0, dtype=hip.X3_FMT, device=DEV)
    x3 = buf[:n, 8:8 + K3]
    hip.split_operand(_dev(x), 0, kpad=K3 // 3, out=x3)
    cn = (torch.from_numpy(c).double() ** 2).sum(1).float().to(DEV)
    ibuf = torch.full((n + 1, m), ISENT, dtype=torch.int32, device=DEV)
    dbuf = torch.full((n + 1, m), SENT, dtype=torch.float32, device=DEV)
    assert x3.stride(0) > K3 and x3.stride(0) % 8 == 0
    hip.retrieval_assign(x3, c3, cn, m, ibuf[:n], dbuf[:n], nsplit=nsplit)
    torch.cuda.synchronize()
    assert bool((ibuf[n] == ISENT).all()) and bool((dbuf[n] == SENT).all())
    return ibuf[:n], dbuf[:n]


def _check_order(x, c, m, ids, dist, near):
    """_check_assign as everywhere, and what it does not see: no -1 id, equal distances in ascending id order, the planted pairs on top of their rows
    with the lower index first, and the float64 ids wherever the neighbouring sorted distances are further away than the bound"""
    n, k = x.shape[0], c.shape[0]
    _check_assign(x, c, m, ids, dist, np.arange(n))
    i, d = ids.cpu().numpy(), dist.cpu().numpy()
    assert i.min() >= 0 and np.isfinite(d).all()
    tie = d[:, 1:] == d[:, :-1]
    assert np.all(i[:, 1:][tie] > i[:, :-1][tie])
    for row, a, b in near:
        assert i[row, 0] == a
        if m > 1:
            assert i[row, 1] == b and d[row, 0].view(np.int32) == d[row, 1].view(np.int32)
    d64, bmax = _assign_bound(x, c, np.arange(n))
    s = torch.sort(d64, 1).values
    inf = torch.full((n, 1), float('inf'), dtype=torch.float64, device=s.device)
    gap = torch.minimum(torch.cat([inf, s[:, 1:] - s[:, :-1]], 1), torch.cat([s[:, 1:] - s[:, :-1], inf], 1))[:, :m]
    sure = (gap > bmax[:, None]).cpu().numpy()
    rid, _ = R.assign(x.astype(np.float64), c.astype(np.float64), m)
    assert np.array_equal(i[sure], rid[sure]) and (n == 1 or sure.mean() > 0.5)        # n = 1, m = 1: the one id is a planted tie
    return sure.mean()


@pytest.mark.parametrize('n', [1, 129])
@pytest.mark.parametrize('m', [1, 5, 8])
def test_assign_ties_splits_and_strides(n, m):
    """k = 321 centroids are 6 tiles of 64, the last one holding centroid 320 alone, so the tile loop `for (c0 = c_begin; c0 < c_end; c0 += 64)` takes
    6 trips with nsplit = 1, 3 with 2, 2 with 4 and 5; n = 129 is a second row block with one row.  nsplit = 4 and 5 give chunks of 2 tiles: split 3
    (and 4) starts past k, runs no tile and hands the merge its (inf, -1) padding; nsplit = 6 leaves the last split one centroid, fewer than m = 5 or
    8, so real and padding entries meet in the merge.  Bit-identical centroid rows (retrieval_ref.ASSIGN_PAIRS) sit in one 16-centroid subtile on two
    lane groups, in two tiles of one split, in two splits, and at k - 1; a descriptor next to each pair must get both, equal to the bit, lower index
    first - through the lane merge, the tile order and the split merge alike - and the result may not depend on nsplit by a bit."""
    x, c, near = R.assign_case(5, n)
    ids1, dist1 = _assign(x, c, m, 1)
    frac = _check_order(x, c, m, ids1, dist1, near)
    print('assign n = %d, m = %d: %.0f%% of the ids decided by more than the bound' % (n, m, 100 * frac))
    for nsplit in (2, 4, 5, 6):
        ids, dist = _assign(x, c, m, nsplit)
        assert torch.equal(ids, ids1) and torch.equal(_bits32(dist), _bits32(dist1)), nsplit


@pytest.mark.parametrize('k,pairs', [(8, [(1, 7)]), (1, [])])
def test_assign_every_centroid_is_returned(k, pairs):
    """k = m: the whole codebook comes back in order, the tile's 64 - k clamped rows never enter a list (k = m = 8 with centroids 1 and 7 equal, k = m = 1)"""
    for n in (1, 129):
        x, c, near = R.assign_case(6, n, k=k, pairs=pairs)
        ids, dist = _assign(x, c, k, 1)
        _check_order(x, c, k, ids, dist, near)
        assert np.array_equal(np.sort(ids.cpu().numpy(), 1), np.tile(np.arange(k), (n, 1)))


# ---------------------------------------------------------------------------------------------------- aggregate
@pytest.mark.parametrize('D', [32, 96, 288, 1024])
def test_aggregate_words_tails_and_padding(D):
    """hip.retrieval_aggregate on its own.  D = 1024 takes four trips of `for (base = wave * 64; base < D; base += 256)` per wave, D = 288 = 256 + 32 a
    second trip for wave 0 only, which ends on an odd bit word (`base + 32 < D` false: the upper ballot half must be dropped, as for D = 32 and 96);
    the 70-member groups run the member loop 70 times.  Groups with planted signs (x = c + delta pattern) fix every bit, so a swapped word order or the
    wrong ballot half shows; a member equal to its centroid gives zero words; descriptor 0 belongs to two groups.  x and cent are column slices of
    wider NaN-filled buffers, bits and sums carry sentinel rows past G."""
    case = R.aggregate_case(9, D)
    x, cent, member, gstart, gword = (case[k] for k in ('x', 'cent', 'member', 'gstart', 'gword'))
    G, W = len(gword), D // 32
    _, xv = _slice_of_wider(_dev(x), 4, 4, 1, float('nan'))
    _, cv = _slice_of_wider(_dev(cent), 8, 4, 1, float('nan'))
    bbuf = torch.full((G + 2, W), ISENT, dtype=torch.int32, device=DEV)
    sbuf = torch.full((G + 2, D), SENT, dtype=torch.float32, device=DEV)
    assert xv.stride(0) > D and cv.stride(0) > D
    hip.retrieval_aggregate(xv, cv, _dev(member), _dev(gstart), _dev(gword), bbuf[:G], sbuf[:G])
    torch.cuda.synchronize()
    assert bool((bbuf[G:] == ISENT).all()) and bool((sbuf[G:] == SENT).all())
    words, sums = bbuf[:G].cpu().numpy(), sbuf[:G].cpu().numpy()
    assert not np.any(sums == np.float32(SENT)) and np.isfinite(sums).all()          # every sum written ...
    got = R.unpack_bits(words)
    assert np.array_equal(got, sums > 0)                                               # ... and every word: it is the sign of the kernel's own sums
    s64, bound = R.aggregate_ref(x, cent, member, gstart, gword)
    assert np.all(np.abs(sums - s64) <= bound), float((np.abs(sums - s64) / bound).max())
    sure = np.abs(s64) > bound
    assert np.array_equal(got[sure], (s64 > 0)[sure])
    for g, pat in case['patterns'].items():
        assert np.array_equal(got[g], pat), (g, np.nonzero(got[g] != pat)[0][:8])
    z = case['zero_group']
    assert not words[z].any() and not sums[z].view(np.int32).any()
    bonly = torch.full((G + 2, W), ISENT, dtype=torch.int32, device=DEV)               # without the optional sums: the same words
    hip.retrieval_aggregate(xv, cv, _dev(member), _dev(gstart), _dev(gword), bonly[:G])
    torch.cuda.synchronize()
    assert torch.equal(bonly, bbuf)


# ---------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize('D', [32, 96, 1024])
def test_scores_chunks_empty_views_and_the_threshold(D):
    """hip.retrieval_scores on synthetic sorted word lists and bits.  Seven database views make `for (j = wave; j < Vdb; j += 4)` repeat for waves 0 to
    2; they hold 0, 1, 63, 64, 65, 130 and 300 groups, so the chunk loop `for (base = b; base < e; base += 64)` runs 0, 1, 1, 1, 2, 3 and 5 trips (65:
    a second chunk of one group; 64: exactly one full chunk); the 600-word query view fills the LDS word list in three trips of 256 threads, and the
    binary search runs over 600 words.  Database words lie below and above every query word and on the first and the last one (the search's ends).
    Planted bit pairs: equal (kappa = 1), complementary (s = -1: nothing) and h = D / 4, s == tau = 0.5 exactly, which must count.  An empty query
    view gives a zero row, an empty database view a zero column, and no NaN of the prefill survives."""
    case = R.scores_case(21, D)
    qw, qb, dw, db = case['qwords'], case['qbits'], case['dwords'], case['dbits']
    q = [_dev(a.view(np.int32) if a.dtype == np.uint32 else a) for a in R.flat_groups(qw, qb, D)]
    d = [_dev(a.view(np.int32) if a.dtype == np.uint32 else a) for a in R.flat_groups(dw, db, D)]
    Vq, Vdb = len(qw), len(dw)
    for alpha, tau in ((3.0, 0.0), (3.0, 0.5), (2.5, 0.1)):
        S = torch.full((Vq, Vdb), float('nan'), dtype=torch.float32, device=DEV)
        hip.retrieval_scores(q[0], q[1], q[2], d[0], d[1], d[2], D, alpha, tau, S, max(len(w) for w in qw))
        S2 = torch.full((Vq, Vdb), float('nan'), dtype=torch.float32, device=DEV)
        hip.retrieval_scores(q[0], q[1], q[2], d[0], d[1], d[2], D, alpha, tau, S2, max(len(w) for w in qw))
        torch.cuda.synchronize()
        assert torch.equal(_bits32(S), _bits32(S2))
        S = S.cpu().numpy()
        assert np.isfinite(S).all()
        assert not S[0].view(np.int32).any() and not S[:, 0].view(np.int32).any()
        ref = R.scores_f32(qw, qb, dw, db, D, alpha, tau)
        ulps = 1 if float(alpha).is_integer() else 4          # the rule of test_scores_equal_the_fp32_restatement_to_one_ulp
        err = np.abs(S - ref) / np.spacing(np.abs(ref).astype(np.float32))
        print('scores D = %d, alpha = %g, tau = %g: worst |S - ref| = %.3g ulp' % (D, alpha, tau, np.nanmax(np.where(ref != 0, err, 0))))
        assert np.all(np.abs(S - ref) <= ulps * np.spacing(np.abs(ref).astype(np.float32))), (alpha, tau, np.abs(S - ref).max())
        assert np.all(ref[2, 1:] > 0) and len(np.unique(ref[2])) == Vdb


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(match, fn, *outputs):
    """fn raises the library's refusal and the sentinel-filled outputs are as they were.  In csrc/retrieval.hip every check of the four entry points
    stands before its hipLaunchKernelGGL (pst_retrieval_select :299-301, _assign :310-318, _aggregate :337-338, _scores :346-351), so nothing runs."""
    before = [o.clone() for o in outputs]
    with pytest.raises(RuntimeError, match=match):
        fn()
    torch.cuda.synchronize()
    for o, b in zip(outputs, before):
        assert torch.equal(_bits32(o.reshape(-1)), _bits32(b.reshape(-1)))


def test_select_refusals():
    D = 64
    x = torch.ones(8, D, dtype=torch.float32, device=DEV)
    in_off, out_off = _dev(np.array([0, 8], np.int32)), _dev(np.array([0, 4], np.int32))
    buf = torch.full((4 * D,), SENT, dtype=torch.float32, device=DEV)
    sel = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    out = buf.view(4, D)
    _refused('exceed the LDS ranking buffer', lambda: hip.retrieval_select(x, in_off, out_off, out, 16385, sel), buf, sel)
    narrow = buf.as_strided((4, D), (D - 8, 1))                 # ldo < D: the rows would overlap
    _refused('leading dimensions', lambda: hip.retrieval_select(x, in_off, out_off, narrow, 8, sel), buf, sel)
    xn = torch.ones(8 * D, dtype=torch.float32, device=DEV).as_strided((8, D), (D - 8, 1))
    _refused('leading dimensions', lambda: hip.retrieval_select(xn, in_off, out_off, out, 8, sel), buf, sel)
    hip.retrieval_select(x, in_off, out_off, out, 8, sel)       # the same call within the limits runs
    torch.cuda.synchronize()
    assert sel.tolist() == [0, 1, 2, 3] and bool((out == D ** -0.5).all())


def test_assign_refusals():
    n, k, D = 4, 70, 64                                         # 2 centroid tiles
    x, c, _ = R.assign_case(1, n, k=k, pairs=[])
    c3 = hip.split_operand(_dev(c), 1)
    x3 = hip.split_operand(_dev(x), 0)
    K3 = x3.shape[1]
    cn = (torch.from_numpy(c).double() ** 2).sum(1).float().to(DEV)
    ids = torch.full((n, 9), ISENT, dtype=torch.int32, device=DEV)
    dist = torch.full((n, 9), SENT, dtype=torch.float32, device=DEV)
    ws_d, ws_i = torch.full((3 * n * 9,), SENT, dtype=torch.float32, device=DEV), torch.full((3 * n * 9,), ISENT, dtype=torch.int32, device=DEV)
    outs = (ids, dist, ws_d, ws_i)
    out = lambda m: (ids.view(-1)[:n * m].view(n, m), dist.view(-1)[:n * m].view(n, m))

    def raw(m=2, nsplit=1, ws=(None, None), tc=2, a=x3, b=c3, kk=k):
        """pst_retrieval_assign itself, for the calls hip.retrieval_assign cannot express"""
        hip._call('pst_retrieval_assign', a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), cn.data_ptr(), n, kk, a.shape[1], m, nsplit,
                  ws[0], ws[1], ids.data_ptr(), dist.data_ptr(), tc)
    # a bf16 operand: the wrapper refuses the tensor, the entry point the type code
    _refused('unexpected dtype', lambda: hip.retrieval_assign(x3.view(torch.bfloat16), c3, cn, 2, *out(2)), *outs)
    _refused('must be f16', lambda: raw(tc=0), *outs)
    _refused('1 <= m <= 8', lambda: raw(m=0), *outs)
    _refused('1 <= m <= 8', lambda: hip.retrieval_assign(x3, c3, cn, 9, *out(9)), *outs)
    _refused('m <= k', lambda: hip.retrieval_assign(x3, c3[:4], cn[:4], 5, *out(5)), *outs)
    _refused('K3 % 64', lambda: hip.retrieval_assign(x3[:, :96], c3[:, :96], cn, 2, *out(2)), *outs)
    odd = torch.zeros(n, K3 + 4, dtype=hip.X3_FMT, device=DEV)[:, :K3]          # ldx % 8 == 4
    _refused('multiples of 8', lambda: hip.retrieval_assign(odd, c3, cn, 2, *out(2)), *outs)
    _refused('nsplit 0 outside', lambda: hip.retrieval_assign(x3, c3, cn, 2, *out(2), nsplit=0), *outs)
    _refused(r'nsplit 3 outside \[1, 2\]', lambda: hip.retrieval_assign(x3, c3, cn, 2, *out(2), nsplit=3), *outs)
    _refused('needs the workspace', lambda: raw(nsplit=2), *outs)
    _refused('needs the workspace', lambda: raw(nsplit=2, ws=(ws_d.data_ptr(), None)), *outs)
    raw(nsplit=2, ws=(ws_d.data_ptr(), ws_i.data_ptr()))        # the same call with its workspace runs
    torch.cuda.synchronize()
    _check_assign(x, c, 2, *out(2), np.arange(n))
    assert bool((ids.view(-1)[n * 2:] == ISENT).all())


def test_aggregate_and_scores_refusals():
    D = 40                                                      # not a multiple of 32
    x, cent = torch.ones(4, D, dtype=torch.float32, device=DEV), torch.zeros(2, D, dtype=torch.float32, device=DEV)
    member, gstart, gword = _dev(np.array([0, 1], np.int32)), _dev(np.array([0, 2], np.int32)), _dev(np.array([0], np.int32))
    bits = torch.full((1, D // 32), ISENT, dtype=torch.int32, device=DEV)
    sums = torch.full((1, D), SENT, dtype=torch.float32, device=DEV)
    _refused('D % 32', lambda: hip.retrieval_aggregate(x, cent, member, gstart, gword, bits, sums), bits, sums)
    off, word = _dev(np.array([0, 1], np.int32)), _dev(np.array([7], np.int32))
    S = torch.full((1, 1), SENT, dtype=torch.float32, device=DEV)
    _refused('D % 32', lambda: hip.retrieval_scores(off, word, bits, off, word, bits, D, 3.0, 0.0, S, 1), S, bits)
    one = torch.zeros(1, 1, dtype=torch.int32, device=DEV)
    call = lambda alpha, tau, max_q: hip.retrieval_scores(off, word, one, off, word, one, 32, alpha, tau, S, max_q)
    _refused('tau >= 0', lambda: call(3.0, -0.1, 1), S)
    _refused('alpha > 0', lambda: call(0.0, 0.0, 1), S)
    _refused('alpha > 0', lambda: call(-1.0, 0.0, 1), S)
    _refused('alpha > 0', lambda: call(float('nan'), 0.0, 1), S)
    _refused('exceed the LDS word list', lambda: call(3.0, 0.0, 16385), S)
    call(3.0, 0.0, 1)                                           # within the limits: one shared word, equal bits
    torch.cuda.synchronize()
    assert S.item() == 1.0
