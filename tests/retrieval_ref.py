"""float64 restatement of the checkpoint retriever (panst3r_amd/model/retrieval.py docstring, [3P-recalled, parity unpinned]) and a seeded maker of
retrieval dicts in the checkpoint layout.  Plain numpy / torch on the CPU, written step by step from the spec, not from the HIP path."""
from argparse import Namespace

import numpy as np
import torch

LN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------- head
def _gelu(x):
    return torch.nn.functional.gelu(torch.as_tensor(x)).numpy()


def head(ck, x):
    """x float64 [T, Denc] -> [T, D] (prewhiten, projector (+ residual), postwhiten)"""
    sd = {k: np.asarray(v.double() if torch.is_tensor(v) else v, dtype=np.float64) for k, v in ck['model'].items() if not k.startswith('backbone.')}
    args = ck['args']
    hd = args.hdims if isinstance(args, Namespace) else args['hdims']
    residual = (args.residual if isinstance(args, Namespace) else args.get('residual', False))
    h = np.asarray(x, dtype=np.float64)
    if 'prewhiten.m' in sd:
        h = (h - sd['prewhiten.m'].reshape(1, -1)) @ sd['prewhiten.p']
    if any(k.startswith('projector.') for k in sd):
        nh = len(hd.split('_')) if hd else 0
        p = h
        for li in range(nh):
            p = p @ sd['projector.%d.weight' % (3 * li)].T + sd['projector.%d.bias' % (3 * li)]
            mu = p.mean(-1, keepdims=True)
            var = ((p - mu) ** 2).mean(-1, keepdims=True)
            p = (p - mu) / np.sqrt(var + LN_EPS) * sd['projector.%d.weight' % (3 * li + 1)] + sd['projector.%d.bias' % (3 * li + 1)]
            p = _gelu(p)
        p = p @ sd['projector.%d.weight' % (3 * nh)].T + sd['projector.%d.bias' % (3 * nh)]
        h = h + p if residual else p
    if 'postwhiten.m' in sd:
        h = (h - sd['postwhiten.m'].reshape(1, -1)) @ sd['postwhiten.p']
    return h


def nfeat_of(ck):
    a = ck['args']
    return int(a.nfeat if isinstance(a, Namespace) else a['nfeat'])


def descriptors(ck, xs):
    """per view: the min(nfeat, T) rows of largest norm (ties to the lower token), in that order, L2-normalised -> (desc [n, D], counts, tokens)"""
    out, counts, toks = [], [], []
    for x in xs:
        h = head(ck, x)
        nrm = np.sqrt((h * h).sum(-1))
        order = np.lexsort((np.arange(len(nrm)), -nrm))[:min(nfeat_of(ck), len(nrm))]
        out.append(h[order] / np.maximum(nrm[order], 1e-12)[:, None])
        counts.append(len(order))
        toks.append(order)
    return np.concatenate(out, 0), counts, toks


# ---------------------------------------------------------------------------------------------------- ASMK
def params_of(ck):
    p = ck['asmk_params']

    def get(path, default):
        d = p
        for q in path:
            if not isinstance(d, dict) or q not in d:
                return default
            d = d[q]
        return d
    return dict(ma_db=get(('build_ivf', 'quantize', 'multiple_assignment'), 1), ma_q=get(('query_ivf', 'quantize', 'multiple_assignment'), 5),
                alpha=get(('query_ivf', 'similarity', 'alpha'), 3.0), tau=get(('query_ivf', 'similarity', 'similarity_threshold'), 0.0))


def centroids_of(ck):
    cb = ck['asmk_codebook']
    while isinstance(cb, dict):
        cb = cb[next(k for k in ('centroids', 'codebook', 'cdb', 'state') if k in cb)]
    return np.asarray(cb.float() if torch.is_tensor(cb) else cb, dtype=np.float32).astype(np.float64)


def distances(desc, cent):
    return (cent * cent).sum(-1)[None, :] - 2.0 * desc @ cent.T


def assign(desc, cent, m):
    """the m nearest centroids (ascending ||c||^2 - 2 x.c, ties to the lower index) -> (ids [n, m], float64 distances [n, m])"""
    d = distances(desc, cent)
    ids = np.argsort(d, axis=1, kind='stable')[:, :m]
    return ids, np.take_along_axis(d, ids, 1)


def aggregate(desc, cent, ids, counts, ma):
    """{view: [(word, float64 residual sum [D]), ...] ascending by word}; members summed in ascending descriptor order"""
    view = np.repeat(np.arange(len(counts)), counts)
    out = {}
    for v in range(len(counts)):
        groups = {}
        for r in np.nonzero(view == v)[0]:
            for w in ids[r, :ma]:
                groups.setdefault(int(w), []).append(r)
        lst = []
        for w in sorted(groups):
            s = np.zeros(desc.shape[1])
            for r in groups[w]:
                s = s + (desc[r] - cent[w])
            lst.append((w, s))
        out[v] = lst
    return out


def kappa(s, alpha, tau):
    return s ** alpha if s >= tau else 0.0


def scores(qagg, dbagg, D, alpha, tau):
    """S[i, j] = sum over the words of query view i and database view j of kappa(1 - 2 hamming / D) (float64)"""
    V, Vd = len(qagg), len(dbagg)
    S = np.zeros((V, Vd))
    for i in range(V):
        qb = {w: s > 0 for w, s in qagg[i]}
        for j in range(Vd):
            for w, s in dbagg[j]:
                if w in qb:
                    h = int(np.count_nonzero(qb[w] != (s > 0)))
                    S[i, j] += kappa(1.0 - 2.0 * h / D, alpha, tau)
    return S


def scores_f32(qwords, qbits, dbwords, dbbits, D, alpha, tau):
    """the kernel's arithmetic on given bits: per (i, j) an fp32 sum in ascending word order of kappa in fp32 (integer alpha: repeated products).
    qwords / dbwords: list per view of ascending words; *bits: list per view of bool arrays [groups, D]."""
    f = np.float32
    S = np.zeros((len(qwords), len(dbwords)), dtype=np.float32)
    ia = int(alpha) if float(alpha).is_integer() and alpha <= 8 else 0
    for i in range(len(qwords)):
        qi = {w: g for g, w in enumerate(qwords[i])}
        for j in range(len(dbwords)):
            acc = f(0)
            for g, w in enumerate(dbwords[j]):
                if w not in qi:
                    continue
                h = int(np.count_nonzero(qbits[i][qi[w]] != dbbits[j][g]))
                s = f(1) - f(2 * h) / f(D)
                if s >= f(tau):
                    if ia:
                        p = s
                        for _ in range(ia - 1):
                            p = f(p * s)
                    else:
                        p = f(np.power(s, f(alpha)))
                    acc = f(acc + p)
            S[i, j] = acc
    return S


def similarity(ck, xs):
    """the whole retriever in float64: per-view encoder tokens -> S [V, V]"""
    desc, counts, _ = descriptors(ck, xs)
    cent = centroids_of(ck)
    p = params_of(ck)
    ids, _ = assign(desc, cent, max(p['ma_q'], p['ma_db']))
    qagg = aggregate(desc, cent, ids, counts, p['ma_q'])
    dbagg = aggregate(desc, cent, ids, counts, p['ma_db'])
    return scores(qagg, dbagg, desc.shape[1], p['alpha'], p['tau'])


# ---------------------------------------------------------------------------------------------------- seeded retrieval dicts
def _white(g, d_in, d_out=None):
    d_out = d_in if d_out is None else d_out
    q, _ = np.linalg.qr(g.standard_normal((d_in, d_in)))
    p = q[:, :d_out] * g.uniform(0.5, 1.5, d_out)[None]
    return torch.from_numpy(g.standard_normal((1, d_in)) * 0.1), torch.from_numpy(p)


def make_dict(seed, denc=128, hdims='', prewhiten=False, postwhiten=False, residual=False, k=1000, nfeat=40, d_out=None, feats=None,
              params=None, layout='dict', backbone_keys=True):
    """A retrieval dict in the checkpoint layout (args Namespace, model state dict with backbone.* keys, asmk_codebook, asmk_params).
    With `feats` (list of [T, denc] arrays, e.g. the token pool of `tokens`) the centroids are placed around the normalised head outputs of every
    row, so that the assignments are not trivial and the views that share pool tokens share words."""
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    if backbone_keys:
        sd['backbone.patch_embed.proj.weight'] = torch.zeros(4, 4)
    if prewhiten:
        sd['prewhiten.m'], sd['prewhiten.p'] = _white(g, denc)
    hd = [int(h) for h in hdims.split('_')] if hdims else []
    d = denc
    if hd or d_out is not None or residual:
        dims = hd + [denc if residual else (d_out or denc)]
        for li, h in enumerate(dims):
            sd['projector.%d.weight' % (3 * li)] = torch.from_numpy(g.standard_normal((h, d)) / np.sqrt(d)).float()
            sd['projector.%d.bias' % (3 * li)] = torch.from_numpy(g.standard_normal(h) * 0.1).float()
            if li < len(hd):
                sd['projector.%d.weight' % (3 * li + 1)] = torch.from_numpy(1 + 0.1 * g.standard_normal(h)).float()
                sd['projector.%d.bias' % (3 * li + 1)] = torch.from_numpy(0.1 * g.standard_normal(h)).float()
            d = h
    if postwhiten:
        sd['postwhiten.m'], sd['postwhiten.p'] = _white(g, d)
    args = Namespace(prewhiten=prewhiten, hdims=hdims, residual=residual, postwhiten=postwhiten, featweights='l2norm', nfeat=nfeat, imsize=512,
                     freeze_backbone=True)
    ck = dict(args=args, model=sd, asmk_params=params if params is not None else
              {'build_ivf': {'kernel': {'binary': True}, 'ivf': {'use_idf': False}, 'quantize': {'multiple_assignment': 1}},
               'query_ivf': {'quantize': {'multiple_assignment': 5}, 'similarity': {'similarity_threshold': 0.0, 'alpha': 3.0}, 'search': {'topk': None}}})
    # centroids: with sample features, m + 1 centroids around every descriptor at distances 0.1 (j + 1) whose offsets have no small component
    # (well separated: the j-th nearest centroid of a descriptor is its j-th own one, residual components >= 0.05 / sqrt(D)), shuffled into
    # random directions; without, random directions only
    cent = g.standard_normal((k, d))
    cent = cent / np.linalg.norm(cent, axis=1, keepdims=True)
    if feats is not None:
        ck['asmk_codebook'] = np.zeros((1, d), np.float32)
        desc = np.concatenate([h / np.linalg.norm(h, axis=1, keepdims=True) for h in (head(ck, f) for f in feats)], 0)
        p = params_of(ck)
        m = max(p['ma_q'], p['ma_db']) + 1
        if m * desc.shape[0] > k:
            raise ValueError('need k >= %d for %d descriptors' % (m * desc.shape[0], desc.shape[0]))
        u = g.choice([-1.0, 1.0], (desc.shape[0], m, d)) * g.uniform(0.5, 1.5, (desc.shape[0], m, d))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        own = desc[:, None, :] + 0.1 * (1 + np.arange(m))[None, :, None] * u
        cent[:m * desc.shape[0]] = own.reshape(-1, d)
        cent = cent[g.permutation(k)]
    cent = cent.astype(np.float32)
    ck['asmk_codebook'] = {'centroids': cent} if layout == 'dict' else (torch.from_numpy(cent) if layout == 'tensor' else cent)
    return ck


def tokens(seed, Ts, denc=128, pool=64):
    """seeded per-view encoder tokens of lengths Ts (float32 values): every view takes distinct rows of a shared pool of `pool` tokens plus 1e-3
    noise, so that views overlap the way neighbouring frames of a scene do.  Returns (list of [T, denc] arrays, the pool)."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = g.standard_normal((pool, denc)) * g.uniform(0.5, 2.0, (pool, 1))
    xs = [(base[g.choice(pool, T, replace=False)] * (1 + 1e-3 * g.standard_normal((T, denc)))).astype(np.float32) for T in Ts]
    return xs, base.astype(np.float32)


def margins(ck, xs):
    """how well separated a synthetic case is for the fp32 GPU path: (relative norm gap at the selection cut, smallest gap between the m-th and
    (m+1)-th nearest centroid, smallest |residual sum| component) - each a distance to a decision the ~1e-6 head error could flip"""
    p = params_of(ck)
    m = max(p['ma_q'], p['ma_db'])
    gaps = []
    for x in xs:
        h = head(ck, x)
        nrm = np.sort(np.sqrt((h * h).sum(-1)))[::-1]
        n = min(nfeat_of(ck), len(nrm))
        if n < len(nrm):
            gaps.append((nrm[n - 1] - nrm[n]) / nrm[n - 1])
    desc, counts, _ = descriptors(ck, xs)
    cent = centroids_of(ck)
    d = np.sort(distances(desc, cent), axis=1)[:, :m + 1]
    agap = float(np.min(np.diff(d, axis=1)))
    ids, _ = assign(desc, cent, m)
    smin = min(float(np.min(np.abs(s))) for ma in (p['ma_q'], p['ma_db']) for lst in aggregate(desc, cent, ids, counts, ma).values() for _, s in lst)
    return (min(gaps) if gaps else 1.0), agap, smin
