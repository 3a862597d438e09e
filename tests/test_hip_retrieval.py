"""The checkpoint retriever on the GPU (csrc/retrieval.hip, panst3r_amd/model/retrieval.py, engine/retrieval.py) against the float64 restatement of
tests/retrieval_ref.py: the assign kernel to per-element error bounds, aggregate bits exact outside their bound, scores to 1 ulp of the kernel's fp32
arithmetic on the same bits, the whole retriever to rel 1e-5, and use_retrieval=True through the public entry point."""
import numpy as np
import pytest
import torch

import errbound
import retrieval_ref as R
import tiny
from panst3r_amd import hip
from panst3r_amd.engine import PanSt3RRetriever
from panst3r_amd.model.retrieval import RetrievalASMK
from panst3r_amd.schedule import keyframes_from_similarity

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U32 = 2.0 ** -24


def _unit(g, n, d):
    x = g.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _case(seed, n, k, D):
    """unit descriptors and centroids drawn near them (non-trivial nearest sets)"""
    g = np.random.Generator(np.random.PCG64(seed))
    x = _unit(g, n, D)
    c = x[g.integers(0, n, k)] + 0.3 * _unit(g, k, D)
    return x, c.astype(np.float32)


def _run_assign(x, c, m, nsplit=None):
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)
    c3 = hip.split_operand(cd, 1)
    x3 = hip.split_operand(xd, 0, kpad=c3.shape[1] // 3)
    cn = (torch.from_numpy(c).double() ** 2).sum(1).float().to(DEV)
    ids = torch.empty(x.shape[0], m, dtype=torch.int32, device=DEV)
    dist = torch.empty(x.shape[0], m, dtype=torch.float32, device=DEV)
    hip.retrieval_assign(x3, c3, cn, m, ids, dist, nsplit=nsplit)
    torch.cuda.synchronize()
    return ids, dist


def _assign_bound(x, c, rows):
    """float64 distances [rows, k] of the given descriptor rows and the per-row bound of _check_assign (the largest per-element bound of the row)"""
    xd, cd = torch.from_numpy(x[rows]).to(DEV).double(), torch.from_numpy(c).to(DEV).double()
    cn = (cd * cd).sum(1)
    d64 = cn[None] - 2 * xd @ cd.T
    absprod = xd.abs() @ cd.abs().T
    K = x.shape[1]
    bound = 2 * errbound.acc_bound(absprod, K, 'x3', xd.abs().sum(1, keepdim=True), cd.abs().sum(1)[None]) + 2 * U32 * (cn[None].abs() + d64.abs())
    return d64, bound.max(1).values


def _check_assign(x, c, m, ids, dist, rows):
    """every returned id's float64 distance within the bound of the true i-th smallest, the returned distance within the bound of its id's, ids
    distinct per row, ascending"""
    d64, bmax = _assign_bound(x, c, rows)
    true = torch.sort(d64, 1).values[:, :m]
    ids = ids[rows].long()
    got = torch.gather(d64, 1, ids)
    assert (ids >= 0).all() and (ids < c.shape[0]).all()
    assert torch.all((got - true).abs() <= bmax[:, None]), float(((got - true).abs() / bmax[:, None]).max())
    assert torch.all((dist[rows].double() - got).abs() <= bmax[:, None])
    s = torch.sort(ids, 1).values
    assert torch.all(s[:, 1:] != s[:, :-1])
    assert torch.all(dist[rows][:, 1:] >= dist[rows][:, :-1])
    return float(((got - true).abs() / bmax[:, None]).max())


@pytest.mark.parametrize('n,k,D', [(200, 1000, 64), (130, 65, 64), (257, 4096, 1024), (1, 70, 1024)])
def test_assign_shapes_and_tails(n, k, D):
    x, c = _case(n + k + D, n, k, D)
    rows = np.arange(n)
    for m in range(1, 9):
        if m > k:
            continue
        ids, dist = _run_assign(x, c, m)
        _check_assign(x, c, m, ids, dist, rows)
        ids1, dist1 = _run_assign(x, c, m, nsplit=1)          # the centroid split does not change the result
        assert torch.equal(ids1, ids) and torch.equal(dist1, dist)


def test_assign_full_size():
    n, k, D, m = 15000, 65536, 1024, 5
    x, c = _case(7, n, k, D)
    ids, dist = _run_assign(x, c, m)
    rows = np.random.Generator(np.random.PCG64(1)).choice(n, 256, replace=False)
    ratio = _check_assign(x, c, m, ids, dist, rows)
    print('assign full size: worst |d(id) - d_true| / bound = %.3g' % ratio)


def _grouped(ck_seed=4, V=5, T=40, m=5, k=1000, D=128):
    """descriptors of V views, their kernel assignments and (view, word) groups of the query (ma = m) and database (ma = 1) sides"""
    r = RetrievalASMK(R.make_dict(ck_seed, k=k))
    g = np.random.Generator(np.random.PCG64(ck_seed))
    cent = r.centroids.numpy()
    x = (cent[g.integers(0, 60, V * T)] + 0.2 * _unit(g, V * T, D)).astype(np.float32)      # 60 shared words: the views overlap
    xd = torch.from_numpy(x).to(DEV)
    ids, _ = r.assign(xd, m)
    view = torch.arange(V, device=DEV).repeat_interleave(T)
    return r, x, xd, ids, view, V


def _host_groups(grp):
    member, gstart, gword, voff = (t.cpu().numpy() for t in grp)
    return member, gstart, gword, voff


def test_aggregate_bits_exact_outside_the_bound():
    r, x, xd, ids, view, V = _grouped()
    cent = r.centroids.numpy().astype(np.float64)
    for ma in (1, 5):
        grp = r.groups(ids, view, ma, V)
        bits, sums = r.aggregate(xd, grp, sums=True)
        torch.cuda.synchronize()
        member, gstart, gword, voff = _host_groups(grp)
        ub = bits.cpu().numpy().view(np.uint32)
        got = ((ub[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(gword), -1).astype(bool)
        for gi in range(len(gword)):
            mem = member[gstart[gi]:gstart[gi + 1]]
            assert np.all(np.diff(mem) > 0)
            res = x[mem].astype(np.float64) - cent[gword[gi]]
            s64 = res.sum(0)
            bound = 2 * (len(mem) + 1) * U32 * np.abs(res).sum(0) + 2 * U32 * (np.abs(x[mem]).sum(0) + len(mem) * np.abs(cent[gword[gi]]))
            sure = np.abs(s64) > bound
            assert np.array_equal(got[gi][sure], (s64 > 0)[sure])
            assert np.all(np.abs(sums[gi].cpu().numpy() - s64) <= bound)


def test_scores_equal_the_fp32_restatement_to_one_ulp():
    r, x, xd, ids, view, V = _grouped()
    qg, dbg = r.groups(ids, view, 5, V), r.groups(ids, view, 1, V)
    qb, dbb = r.aggregate(xd, qg)[0], r.aggregate(xd, dbg)[0]
    for alpha, tau in ((3.0, 0.0), (3.0, 0.5), (2.5, 0.1)):
        r.params = dict(r.params, alpha=alpha, tau=tau)
        S = r.scores(qg, qb, dbg, dbb).cpu().numpy()

        def lists(grp, bits):
            _, _, gword, voff = _host_groups(grp)
            ub = bits.cpu().numpy().view(np.uint32)
            b = ((ub[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(gword), -1).astype(bool)
            return [gword[voff[v]:voff[v + 1]].tolist() for v in range(V)], [b[voff[v]:voff[v + 1]] for v in range(V)]
        qw, qbits = lists(qg, qb)
        dw, dbits = lists(dbg, dbb)
        ref = R.scores_f32(qw, qbits, dw, dbits, r.D, alpha, tau)
        ulps = 1 if float(alpha).is_integer() else 4          # powf against numpy's power: an ulp per term at most
        assert np.all(np.abs(S - ref) <= ulps * np.spacing(np.abs(ref).astype(np.float32))), (alpha, tau, np.abs(S - ref).max())
        if tau == 0.0:
            assert (S[~np.eye(V, dtype=bool)] > 0).all() and len(np.unique(S)) > V    # off-diagonal similarities, not all of them integers


# well-separated synthetic dicts (tests/retrieval_ref.make_dict with centroids around the token pool the views share; margins asserted below)
CONFIGS = [(0, dict(hdims='', k=1000, nfeat=20)), (0, dict(hdims='96', prewhiten=True, residual=True, k=4096, nfeat=40)),
           (0, dict(hdims='128_64', postwhiten=True, k=4096, nfeat=64)), (0, dict(hdims='96', prewhiten=True, postwhiten=True, k=1000, nfeat=20, d_out=96)),
           # every loop of csrc/retrieval.hip takes a second trip at once: views of more than 256 tokens (select's ranking loop, scores' LDS fill: 300 and
           # 260 descriptors x 5 query words), nfeat = 300 kept rows per view (more than 64 database groups: scores' chunk loop) and D = 288 = 256 + 32
           # (aggregate's second 256-column trip, ending on an odd bit word).  Seed 0 was the first one tried; its float64 margins (1.0, 3.0e-2, 2.5e-3)
           # are far above 5e-5 (seeds 1 to 3, also tried on the CPU, give the same margins to two digits).
           (0, dict(hdims='', k=4096, nfeat=300, d_out=288, Ts=[300, 260, 300], pool=512))]
TS = [48, 48, 30, 30, 48, 30]          # two token counts: a multi-aspect-ratio scene


@pytest.mark.parametrize('seed,cfg', CONFIGS, ids=['plain', 'pre-res-4096', 'deep-post', 'pre-post-96', 'second-trips-288'])
def test_retriever_end_to_end(seed, cfg):
    cfg = dict(cfg)
    xs, pool = R.tokens(100 + seed, cfg.pop('Ts', TS), pool=cfg.pop('pool', 64))
    ck = R.make_dict(seed, feats=[pool], **cfg)
    assert min(R.margins(ck, xs)) > 5e-5
    ref = R.similarity(ck, xs)
    ret = PanSt3RRetriever(ck, backbone=object(), device=DEV, verbose=False)
    xt = [torch.from_numpy(x).to(DEV)[None] for x in xs]
    S = ret(xt)
    assert S.shape == ref.shape and S.dtype == np.float32
    assert np.all(np.abs(S - ref) <= 1e-5 * np.abs(ref) + 1e-12), float(np.max(np.abs(S - ref) / np.maximum(np.abs(ref), 1e-30)))
    assert np.array_equal(ret(xt), S)                          # two calls: bit-identical
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(len(xs))
    Sp = ret([xt[i] for i in perm])
    assert np.array_equal(Sp, S[perm][:, perm])                # permuting the views permutes S bit for bit
    K = 3
    np.random.seed(11)
    kf = keyframes_from_similarity(S, K)
    np.random.seed(11)
    assert kf == keyframes_from_similarity(ref, K)


@pytest.fixture(scope='module')
def model():
    h = tiny.build(tiny.hip_ns(), 'v1').to(DEV)
    yield h
    h.clear_runners()


# single assignment on both sides: every view's own similarity is its word count, the row maximum the keyframe sampler needs
API_PARAMS = {'query_ivf': {'quantize': {'multiple_assignment': 1}}}


def _setup(h, V, H, W, seed=0):
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    x, _ = h.forward_must3r_encoder(imgs, ts, amp='fp16')
    toks = [t.float() for t in x]
    ck = R.make_dict(seed, k=16, nfeat=16, hdims='96', prewhiten=True, params=API_PARAMS)     # few words: every pair of views shares some
    return imgs, ts, toks, ck


def _same(a, b):
    pa, qa = a
    pb, qb = b
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(torch.equal(x, y) for x, y in zip(qa['pred_masks'], qb['pred_masks']))
    assert torch.equal(qa['out_queries'], qb['out_queries'])


def test_use_retrieval_through_the_entry_point(model, tmp_path):
    h = model
    V, K, H, W = 6, 3, 64, 96
    imgs, ts, toks, ck = _setup(h, V, H, W)
    h.retrieval = ck
    S = PanSt3RRetriever(ck, backbone=h.must3r_encoder, device=DEV, verbose=False)(toks)
    np.random.seed(3)
    kf = keyframes_from_similarity(S, K)
    for cache in (False, True):
        np.random.seed(3)
        got = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, use_retrieval=True, amp='fp16', cache_graphs=cache)
        want = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, keyframes=kf, amp='fp16', cache_graphs=cache)
        _same(got, want)
    h.clear_runners()
    f = tmp_path / 'retrieval.pth'
    torch.save(ck, str(f))
    h.retrieval = str(f)                                       # the dict given as a file path
    np.random.seed(3)
    got = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, use_retrieval=True, amp='fp16')
    _same(got, want)
    # sim_matrix= still takes precedence over the retriever
    sim = np.eye(V) * 0.5 + 0.5 * np.linspace(0, 1, V)[None] * np.linspace(1, 0, V)[:, None]
    np.fill_diagonal(sim, 1.0)
    np.random.seed(5)
    kf2 = keyframes_from_similarity(sim, K)
    np.random.seed(5)
    got = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, use_retrieval=True, sim_matrix=sim, amp='fp16')
    _same(got, h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, keyframes=kf2, amp='fp16'))
    h.retrieval = None
    with pytest.raises(NotImplementedError):
        h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, use_retrieval=True, amp='fp16')


def test_use_retrieval_multi_aspect_ratio(model):
    h = model
    K = 3
    a, tsa, ta, _ = _setup(h, 3, 64, 96)
    b, tsb, tb, _ = _setup(h, 3, 96, 64)
    imgs, ts = a + b, torch.cat([tsa, tsb])
    ck = R.make_dict(1, k=16, nfeat=16, params=API_PARAMS)
    h.retrieval = ck
    try:
        S = PanSt3RRetriever(ck, backbone=h.must3r_encoder, device=DEV, verbose=False)(ta + tb)
        np.random.seed(2)
        kf = keyframes_from_similarity(S, K)
        np.random.seed(2)
        got = h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, use_retrieval=True, amp='fp16')
        _same(got, h.forward_inference_multi_ar(imgs, ts, tiny.NAMES, num_keyframes=K, keyframes=kf, amp='fp16'))
        assert len(got[0]) == 6
    finally:
        h.retrieval = None
