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


# ---------------------------------------------------------------------------------------------------- kernel-level cases (tests/test_hip_retrieval_kernels.py)
# Seeded inputs that make the loops of csrc/retrieval.hip repeat, with their float64 answers.  Everything is built from the contract in the docstrings of
# panst3r_amd/hip.py (retrieval_*) and panst3r_amd/model/retrieval.py; tests/test_retrieval_host.py checks the constructions themselves on the CPU.
SELECT_TS = [1, 5, 256, 257, 300, 700]      # one launch: a single row, a tiny view, the block width and one more, two views that need a second ranking trip
SELECT_STEP = 0.998                         # ratio of neighbouring row norms: a relative gap of 2e-3, far above the fp32 error of the ranking key


def _unit_rows(g, n, d):
    x = g.standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def select_case(seed, nfeat, D, Ts=SELECT_TS):
    """rows of len(Ts) views whose float64 norms form the ladder 2 SELECT_STEP^rank (rank -> token by a random permutation), with planted exceptions:
      ties    pairs of bit-identical rows at neighbouring ranks: tokens 3 and 260 of the 300- and 700-token views (either side of 256), and in every view
              that is cut (T > nsel) a pair at ranks (nsel - 1, nsel), so that exactly one of the two is selected;
      zeros   the two lowest ranks of the 5-token view are all-zero rows, the rank above them has norm 1e-13 (below the 1e-12 clamp).
    -> dict(x fp32 [sum T, D], Ts, counts, ties [(view, lower token, higher token)], zeros [(view, token)], tiny [(view, token)])"""
    g = np.random.Generator(np.random.PCG64(seed))
    xs, ties, zeros, tiny = [], [], [], []
    counts = [min(nfeat, T) for T in Ts]
    for v, (T, nsel) in enumerate(zip(Ts, counts)):
        perm = g.permutation(T)                                  # perm[rank] = token

        def place(rank, token):
            j = int(np.nonzero(perm == token)[0][0])
            perm[rank], perm[j] = perm[j], perm[rank]
        pairs = []                                               # ranks (r, r + 1) that share one row
        cut = nsel - 1 if nsel < T else None
        if T > 260:
            r = cut if (cut is not None and (T == 300 or nsel < 3)) else (10 if T == 300 else 0)
            place(r, 260), place(r + 1, 3)
            pairs.append(r)
        if cut is not None and cut not in pairs:
            pairs.append(cut)
        rows = (2.0 * SELECT_STEP ** np.arange(T))[:, None] * _unit_rows(g, T, D)
        if T == 5:
            rows[2] *= 1e-13 / np.linalg.norm(rows[2])
            rows[3:] = 0.0
            zeros += [(v, int(perm[3])), (v, int(perm[4]))]
            tiny.append((v, int(perm[2])))
        rows = rows.astype(np.float32)
        for r in pairs:
            rows[r + 1] = rows[r]
            ties.append((v, int(min(perm[r], perm[r + 1])), int(max(perm[r], perm[r + 1]))))
        x = np.empty_like(rows)
        x[perm] = rows
        xs.append(x)
    return dict(x=np.concatenate(xs, 0), Ts=list(Ts), counts=counts, ties=ties, zeros=zeros, tiny=tiny)


def select_ref(x, Ts, counts):
    """per view the counts[v] rows of largest float64 norm, ties to the lower token (the lexsort of `descriptors`), L2-normalised with the 1e-12 clamp
    -> (tokens int [sum counts], rows float64 [sum counts, D])"""
    toks, rows, t0 = [], [], 0
    for T, n in zip(Ts, counts):
        h = x[t0:t0 + T].astype(np.float64)
        nrm = np.sqrt((h * h).sum(-1))
        order = np.lexsort((np.arange(T), -nrm))[:n]
        toks.append(order)
        rows.append(h[order] / np.maximum(nrm[order], 1e-12)[:, None])
        t0 += T
    return np.concatenate(toks), np.concatenate(rows, 0)


def select_f32(x):
    """the select kernel's fp32 steps on rows x fp32 [n, D]: lane l of 64 adds the squares of columns l, l + 64, ... by fma, a six-step butterfly adds
    the lanes, one sqrt, the 1e-12f clamp, one division per element -> fp32 [n, D]"""
    f = np.float32
    n, D = x.shape
    pad = np.zeros((n, -(-D // 64) * 64), np.float64)
    pad[:, :D] = x
    s = np.zeros((n, 64), f)
    for c in range(0, pad.shape[1], 64):
        s = (pad[:, c:c + 64] * pad[:, c:c + 64] + s.astype(np.float64)).astype(f)      # fmaf: the product is exact in float64
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(f)
    nrm = np.maximum(np.sqrt(s[:, 0]).astype(f), f(1e-12))
    return (x / nrm[:, None]).astype(f)


ASSIGN_K, ASSIGN_D = 321, 64                # 6 centroid tiles of 64, the last one holding a single centroid
# bit-identical centroid rows (lower, higher): one 16-centroid subtile but two lane groups (4 centroids per lane); two 64-tiles that share a split for
# nsplit <= 2 and not above; two splits for every nsplit >= 2; the last centroid with one that shares its split up to nsplit = 5 and not for 6
ASSIGN_PAIRS = [(17, 22), (70, 140), (5, 250), (300, 320)]


def assign_case(seed, n, k=ASSIGN_K, D=ASSIGN_D, pairs=ASSIGN_PAIRS):
    """unit centroids with the rows of `pairs` made bit-identical, and n descriptors: row i < len(pairs) lies 0.05 from pair i (counted from the last
    pair, so that n = 1 meets the one with centroid k - 1), the others 0.3 from a random centroid -> (x fp32 [n, D], c fp32 [k, D], [(row, lower, higher)])"""
    g = np.random.Generator(np.random.PCG64(seed))
    c = _unit_rows(g, k, D).astype(np.float32)
    for a, b in pairs:
        c[b] = c[a]
    x = c[g.integers(0, k, n)].astype(np.float64) + 0.3 * _unit_rows(g, n, D)
    near = []
    for i, (a, b) in enumerate(reversed(pairs)):
        if i < n:
            x[i] = c[a].astype(np.float64) + 0.05 * _unit_rows(g, 1, D)[0]
            near.append((i, a, b))
    return x.astype(np.float32), c, near


def pack_bits(b):
    """bool [G, D] -> uint32 [G, D / 32], bit j of word w = component 32 w + j"""
    G, D = b.shape
    return (b.reshape(G, D // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(w):
    """uint32 [G, W] -> bool [G, 32 W]"""
    w = np.asarray(w).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1).astype(bool)


def aggregate_case(seed, D):
    """142 descriptors, 6 centroids and five groups (members ascending):
      0  one member, x = c + 0.5 pattern (a known +-1 pattern: every bit is decided)      1  70 members around their centroid (mixed signs)
      2  70 members: descriptor 0 of group 0 and 69 of group 1's (a descriptor in several groups)
      3  one member equal to its centroid bit for bit (zero sums, zero bits)               4  70 members, each c + (0.5 .. 1.5) pattern
    -> dict(x, cent, member, gstart, gword, patterns {group: bool [D]}, zero_group)"""
    g = np.random.Generator(np.random.PCG64(seed))
    cent = g.standard_normal((6, D)).astype(np.float32)
    x = np.empty((142, D), np.float32)
    pat = {0: g.random(D) < 0.5, 4: g.random(D) < 0.5}
    sgn = lambda p: np.where(p, 1.0, -1.0)
    x[0] = cent[0] + np.float32(0.5) * sgn(pat[0]).astype(np.float32)
    x[1:71] = cent[1] + 0.2 * g.standard_normal((70, D))
    x[71] = cent[3]
    x[72:] = cent[4] + g.uniform(0.5, 1.5, (70, D)) * sgn(pat[4])
    groups = [[0], list(range(1, 71)), [0] + list(range(2, 71)), [71], list(range(72, 142))]
    member = np.concatenate(groups).astype(np.int32)
    gstart = np.concatenate([[0], np.cumsum([len(m) for m in groups])]).astype(np.int32)
    return dict(x=x, cent=cent, member=member, gstart=gstart, gword=np.array([0, 1, 2, 3, 4], np.int32), patterns=pat, zero_group=3)


def aggregate_ref(x, cent, member, gstart, gword):
    """float64 residual sums [G, D] and the per-element bound of the kernel's fp32 sum (tests/test_hip_retrieval.py: every x - c rounds once, the
    running sum once per member, each allowed twice)"""
    u32 = 2.0 ** -24
    S, B = [], []
    for gi in range(len(gword)):
        mem = member[gstart[gi]:gstart[gi + 1]]
        c = cent[gword[gi]].astype(np.float64)
        res = x[mem].astype(np.float64) - c
        S.append(res.sum(0))
        B.append(2 * (len(mem) + 1) * u32 * np.abs(res).sum(0) + 2 * u32 * (np.abs(x[mem].astype(np.float64)).sum(0) + len(mem) * np.abs(c)))
    return np.stack(S), np.stack(B)


SCORES_Q = [0, 5, 600]                      # words per query view: none, a few, more than one 256-thread fill of the LDS word list
SCORES_DB = [0, 1, 63, 64, 65, 130, 300]    # groups per database view: 7 views (two trips of the 4-wave loop), either side of the 64-group chunk, 3 and 5 chunks


def scores_case(seed, D):
    """sorted word lists and sign bits of SCORES_Q query and SCORES_DB database views.  Every database view of >= 4 groups holds a word below and a
    word above every query word and the first and the last word of the 600-word query view; about half of its other words are that view's too.  The
    bits of a matching database group are the query's with h random flips, h uniform in [0, D]; planted against the 600-word view: h = 0 (first word)
    and h = D (last word) in the 300-group view, h = D / 4 (s = 0.5 exactly) and h = D / 4 + 1 in the 130-group view, h = D / 8 in the 1-group view.
    -> dict(qwords, qbits, dwords, dbits (lists per view; bits bool [groups, D]), planted [(db view, word, h)])"""
    g = np.random.Generator(np.random.PCG64(seed))
    uni = np.arange(100, 3000)
    qwords = [np.sort(g.choice(uni, n, replace=False)) for n in SCORES_Q]
    qbits = [g.random((n, D)) < 0.5 for n in SCORES_Q]
    big = qwords[2]
    lo, hi = min(int(w[0]) for w in qwords if len(w)), max(int(w[-1]) for w in qwords if len(w))
    first, last = int(big[0]), int(big[-1])
    pos = {int(w): i for i, w in enumerate(big)}
    dwords, dbits, planted = [], [], []
    for j, n in enumerate(SCORES_DB):
        cand = ([first] if n == 1 else [lo - 1 - j, hi + 1 + j, first, last]) if n else []
        for a, b in zip(g.permutation(big), g.permutation(np.arange(3000 + 10))):
            cand += [int(a), int(b)]
        words = []
        for w in cand:
            if len(words) < n and w not in words:
                words.append(w)
        words = np.sort(np.array(words, dtype=np.int64))
        bits = g.random((n, D)) < 0.5
        plant = {1: {first: D // 8}, 130: {first: D // 4, last: D // 4 + 1}, 300: {first: 0, last: D}}.get(n, {})
        for i, w in enumerate(words):
            if int(w) in pos:
                h = plant.get(int(w), int(g.integers(0, D + 1)))
                bits[i] = qbits[2][pos[int(w)]]
                flip = g.choice(D, h, replace=False)
                bits[i, flip] = ~bits[i, flip]
                if int(w) in plant:
                    planted.append((j, int(w), h))
        dwords.append(words)
        dbits.append(bits)
    return dict(qwords=qwords, qbits=qbits, dwords=dwords, dbits=dbits, planted=planted)


def flat_groups(words, bits, D):
    """lists per view -> (off int32 [V + 1], word int32 [G], packed bits uint32 [G, D / 32]) as retrieval_scores takes them"""
    off = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
    word = np.concatenate([np.asarray(w, dtype=np.int32) for w in words]).astype(np.int32)
    b = np.concatenate([np.asarray(x, dtype=bool).reshape(-1, D) for x in bits], 0)
    return off, word, pack_bits(b)
