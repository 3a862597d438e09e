"""The PanSt3R checkpoint's image retriever (`ckpt['retrieval']`, reference panst3r.py:311) on the HIP path: the retrieval head on pst_gemm /
pst_layernorm in fp32 mode and ASMK on csrc/retrieval.hip.  Feeds `schedule.keyframes_from_similarity` (reference panst3r.py:88-125).

[3P-recalled, parity unpinned]  The reference builds the retriever from must3r's `RetrievalModel` and asmk's `ASMKMethod` with a faiss-GPU index
(engine/retrieval.py:12-47); none of them is vendored.  What follows is the algorithm restated from the published code as recalled; a checkpoint that
asks for anything it does not cover raises (RetrievalSpecError) instead of being guessed at.

Checkpoint dict (or a path to a torch file holding one): `args`, `model`, `asmk_codebook`, `asmk_params`.
  args    prewhiten, hdims ('' or '1024' or '1024_512'), residual (default False), postwhiten, featweights, nfeat, imsize, freeze_backbone.
  model   state dict of the head; `backbone.*` keys are ignored (the backbone is the scene's must3r_encoder).
Head, per view, on x = the encoder's output tokens [T, Denc] as float32 (reference panst3r.py:180, outside autocast):
  1. prewhiten  (x - m) @ p, m [1, Denc] and p [Denc, Denc] float64 (`prewhiten.m` / `prewhiten.p`); present iff `prewhiten.m` is in the state dict.
  2. projector  from hdims: Linear -> LayerNorm(eps 1e-5) -> GELU(erf) for every hidden dim, then a final Linear (keys projector.0/1/3/4/6/...);
                no projector keys with hdims '' = identity.  residual: x + projector(x).
  3. postwhiten as 1. on the output dim D.
  4. attention  row L2 norm (featweights 'l2norm' only); the rows are L2-normalised.
  5. keep the min(nfeat, T) rows of largest attention, ties to the lower token index (in that order).
ASMK, binary kernel, over the V views (asmk_params; absent keys take the HOW / mast3r defaults of DEFAULTS):
  1. quantise   the ma nearest centroids of each descriptor in L2 (smallest ||c||^2 - 2 <x, c>, ties to the lower centroid index);
                ma = build_ivf.quantize.multiple_assignment for the database side, query_ivf.quantize.multiple_assignment for the query side.
  2. aggregate  per (view, word): sum of the residuals x - c_w over the descriptors assigned to w, in ascending descriptor order; bit = sum > 0.
  3. score      S[i, j] = sum over the words w held by query view i and database view j of kappa(1 - 2 popcount(b_i(w) XOR b_j(w)) / D),
                kappa(s) = s^alpha if s >= tau else 0.  No per-view normalisation: S is not symmetric.
Raised: binary=False, use_idf=True, a search topk that is not None, tau < 0, D not a multiple of 32, featweights other than 'l2norm'.
"""
import os

import numpy as np
import torch

from .. import hip
from .common import precision

LN_EPS = 1e-5        # nn.LayerNorm default (the projector's LayerNorms)
# HOW / mast3r defaults of the asmk parameters this restatement reads (used when the checkpoint's asmk_params leaves a key out)
DEFAULTS = {
    ('build_ivf', 'quantize', 'multiple_assignment'): 1,
    ('query_ivf', 'quantize', 'multiple_assignment'): 5,
    ('build_ivf', 'kernel', 'binary'): True,
    ('build_ivf', 'ivf', 'use_idf'): False,
    ('query_ivf', 'similarity', 'similarity_threshold'): 0.0,
    ('query_ivf', 'similarity', 'alpha'): 3.0,
    ('query_ivf', 'search', 'topk'): None,
}


class RetrievalSpecError(ValueError):
    """the checkpoint's retriever asks for something the restatement does not cover"""


def load_retrieval_ckpt(ckpt):
    """ckpt['retrieval'] as PanSt3RRetriever.__init__ accepts it: a dict, or a path to a torch file holding one"""
    if isinstance(ckpt, (str, os.PathLike)):
        if not os.path.isfile(ckpt):
            raise FileNotFoundError('retrieval checkpoint %s not found' % (ckpt,))
        ckpt = torch.load(ckpt, map_location='cpu', weights_only=False)
    if not isinstance(ckpt, dict):
        raise RetrievalSpecError('retrieval checkpoint must be a dict (or a path to one), got %s' % type(ckpt).__name__)
    missing = [k for k in ('args', 'model', 'asmk_codebook', 'asmk_params') if k not in ckpt]
    if missing:
        raise RetrievalSpecError('retrieval checkpoint lacks %s (has: %s)' % (', '.join(missing), ', '.join(sorted(map(str, ckpt)))))
    return ckpt


def _arg(args, name, default=KeyError):
    v = args.get(name, default) if isinstance(args, dict) else getattr(args, name, default)
    if v is KeyError:
        raise RetrievalSpecError('retrieval args lack %r' % name)
    return v


def parse_codebook(cb):
    """asmk_codebook -> float32 [k, D] tensor.  Layouts: a tensor / array, or a dict holding one under 'centroids' (asmk Codebook.state_dict), possibly
    nested under 'codebook' / 'cdb' / 'state'."""
    if isinstance(cb, (torch.Tensor, np.ndarray)):
        t = torch.as_tensor(np.asarray(cb) if isinstance(cb, np.ndarray) else cb)
        if t.dim() != 2 or not (t.dtype.is_floating_point):
            raise RetrievalSpecError('asmk codebook: need a floating-point [k, D] array, got %s %s' % (t.dtype, tuple(t.shape)))
        return t.float().contiguous()
    if isinstance(cb, dict):
        for key in ('centroids', 'codebook', 'cdb', 'state'):
            if key in cb:
                return parse_codebook(cb[key])
        raise RetrievalSpecError('asmk codebook: no centroid array under the keys %s (expected one of centroids / codebook / cdb / state)'
                                 % (sorted(map(str, cb)),))
    raise RetrievalSpecError('asmk codebook: unsupported layout %s' % type(cb).__name__)


def parse_params(params):
    """asmk_params -> dict(ma_db, ma_q, alpha, tau); raises on what the binary-kernel restatement does not cover"""
    if params is None:
        params = {}
    if not isinstance(params, dict):
        raise RetrievalSpecError('asmk_params must be a dict, got %s' % type(params).__name__)

    def get(path):
        d = params
        for p in path:
            if not isinstance(d, dict) or p not in d:
                return DEFAULTS[path]
            d = d[p]
        return d
    binary, use_idf, topk = get(('build_ivf', 'kernel', 'binary')), get(('build_ivf', 'ivf', 'use_idf')), get(('query_ivf', 'search', 'topk'))
    tau, alpha = get(('query_ivf', 'similarity', 'similarity_threshold')), get(('query_ivf', 'similarity', 'alpha'))
    ma_db, ma_q = get(('build_ivf', 'quantize', 'multiple_assignment')), get(('query_ivf', 'quantize', 'multiple_assignment'))
    if not binary:
        raise RetrievalSpecError('asmk: only the binary kernel is supported (build_ivf.kernel.binary=False)')
    if use_idf:
        raise RetrievalSpecError('asmk: idf weighting is not supported (build_ivf.ivf.use_idf=True)')
    if topk is not None:
        raise RetrievalSpecError('asmk: a search top-k is not supported (query_ivf.search.topk=%r; the full V x V matrix is needed)' % (topk,))
    if tau is None or float(tau) < 0:
        raise RetrievalSpecError('asmk: similarity_threshold must be >= 0 (got %r)' % (tau,))
    if alpha is None or not float(alpha) > 0:
        raise RetrievalSpecError('asmk: alpha must be > 0 (got %r)' % (alpha,))
    for name, ma in (('build_ivf', ma_db), ('query_ivf', ma_q)):
        if int(ma) != ma or not 1 <= int(ma) <= 8:
            raise RetrievalSpecError('asmk: %s.quantize.multiple_assignment must be an integer in 1..8 (got %r)' % (name, ma))
    return dict(ma_db=int(ma_db), ma_q=int(ma_q), alpha=float(alpha), tau=float(tau))


def parse_head(args, sd):
    """state dict of the head -> list of stages ('white', m, p) / ('proj', [layers], residual) in order, with key checks in the style of
    panst3r.check_checkpoint_keys: unknown or missing head keys raise."""
    sd = {k: v for k, v in sd.items() if not k.startswith('backbone.')}
    fw = _arg(args, 'featweights')
    if fw != 'l2norm':
        raise RetrievalSpecError("retrieval head: featweights %r is not supported (only 'l2norm')" % (fw,))
    hd = _arg(args, 'hdims')
    hd = '' if hd is None else str(hd)
    hdims = [int(h) for h in hd.split('_')] if hd else []
    residual = bool(_arg(args, 'residual', False))
    used, stages = set(), []

    def take(k):
        if k not in sd:
            raise RetrievalSpecError('retrieval head: missing key %s' % k)
        used.add(k)
        return sd[k]

    def white(name):
        if name + '.m' not in sd:
            return None
        m, p = take(name + '.m').double().reshape(1, -1), take(name + '.p').double()
        if p.dim() != 2 or p.shape[0] != m.shape[1]:
            raise RetrievalSpecError('retrieval head: %s.p %s does not match %s.m %s' % (name, tuple(p.shape), name, tuple(m.shape)))
        return ('white', m, p)
    w = white('prewhiten')
    if w is not None:
        stages.append(w)
    pidx = sorted({int(k.split('.')[1]) for k in sd if k.startswith('projector.')})
    if pidx:
        layers = []
        for li in range(len(hdims) + 1):
            W, b = take('projector.%d.weight' % (3 * li)), take('projector.%d.bias' % (3 * li))
            if W.dim() != 2:
                raise RetrievalSpecError('retrieval head: projector.%d is not a Linear' % (3 * li))
            if li < len(hdims):
                if W.shape[0] != hdims[li]:
                    raise RetrievalSpecError('retrieval head: projector.%d has %d outputs, hdims %r says %d' % (3 * li, W.shape[0], hd, hdims[li]))
                g, beta = take('projector.%d.weight' % (3 * li + 1)), take('projector.%d.bias' % (3 * li + 1))
                if g.dim() != 1 or g.shape[0] != W.shape[0]:
                    raise RetrievalSpecError('retrieval head: projector.%d is not a LayerNorm of width %d' % (3 * li + 1, W.shape[0]))
                layers.append(('lin_ln_gelu', W, b, g, beta))
            else:
                layers.append(('lin', W, b))
        for a, b_ in zip(layers, layers[1:]):
            if b_[1].shape[1] != a[1].shape[0]:
                raise RetrievalSpecError('retrieval head: projector widths do not chain (%s -> %s)' % (tuple(a[1].shape), tuple(b_[1].shape)))
        stages.append(('proj', layers, residual))
    elif hdims:
        raise RetrievalSpecError('retrieval head: hdims %r but no projector keys' % (hd,))
    elif residual:
        raise RetrievalSpecError('retrieval head: residual=True without a projector')
    w = white('postwhiten')
    if w is not None:
        stages.append(w)
    extra = sorted(set(sd) - used)
    if extra:
        raise RetrievalSpecError('retrieval head: unexpected keys %s (hdims %r)' % (', '.join(extra[:8]), hd))
    return stages


def stage_dims(stages, d_in):
    """(input dim, output dim) of the head; raises when the stages do not chain"""
    d = d_in
    for st in stages:
        if st[0] == 'white':
            if st[2].shape[0] != d:
                raise RetrievalSpecError('retrieval head: whitener of width %d on %d-dim features' % (st[2].shape[0], d))
            d = st[2].shape[1]
        else:
            layers, residual = st[1], st[2]
            if layers[0][1].shape[1] != d:
                raise RetrievalSpecError('retrieval head: projector input %d on %d-dim features' % (layers[0][1].shape[1], d))
            out = layers[-1][1].shape[0]
            if residual and out != d:
                raise RetrievalSpecError('retrieval head: residual projector %d -> %d' % (d, out))
            d = out
    return d


class RetrievalASMK:
    """The parsed retriever: head stages, codebook and ASMK parameters (host), packed onto a device on first use and kept there."""

    def __init__(self, ckpt):
        ck = load_retrieval_ckpt(ckpt)
        args = ck['args']
        self.nfeat = int(_arg(args, 'nfeat'))
        if self.nfeat < 1:
            raise RetrievalSpecError('retrieval args: nfeat must be >= 1 (got %d)' % self.nfeat)
        self.imsize = _arg(args, 'imsize', None)
        self.stages = parse_head(args, ck['model'])
        self.centroids = parse_codebook(ck['asmk_codebook'])
        self.params = parse_params(ck['asmk_params'])
        self.k, self.D = self.centroids.shape
        if self.D % 32:
            raise RetrievalSpecError('asmk: descriptor dim %d is not a multiple of 32 (binary signatures)' % self.D)
        if max(self.params['ma_db'], self.params['ma_q']) > self.k:
            raise RetrievalSpecError('asmk: multiple assignment %d exceeds the %d centroids' % (max(self.params['ma_db'], self.params['ma_q']), self.k))
        self.d_in = self._first_dim()
        if stage_dims(self.stages, self.d_in) != self.D:
            raise RetrievalSpecError('retrieval head outputs %d dims, the codebook has %d' % (stage_dims(self.stages, self.d_in), self.D))
        self._packed = {}

    def _first_dim(self):
        for st in self.stages:
            return st[2].shape[0] if st[0] == 'white' else st[1][0][1].shape[1]
        return self.D                       # no head at all: the encoder tokens are the descriptors

    # ------------------------------------------------------------------ device side
    def packed(self, device):
        device = torch.device(device)
        pk = self._packed.get(str(device))
        if pk is not None:
            return pk
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        ops = []
        for st in self.stages:
            if st[0] == 'white':             # (x - m) @ p = x @ p + (-m p): a GEMM with W = p^T and the bias folded in float64
                m, p = st[1], st[2]
                ops.append(('lin', f32(p.t()), f32((-m @ p).reshape(-1)), None))
            else:
                layers = []
                for L in st[1]:
                    if L[0] == 'lin_ln_gelu':
                        layers.append(('lin_ln_gelu', f32(L[1]), f32(L[2]), (f32(L[3]), f32(L[4]))))
                    else:
                        layers.append(('lin', f32(L[1]), f32(L[2]), None))
                ops.append(('proj', layers, st[2]))
        cent = f32(self.centroids)
        with torch.cuda.device(device):
            c3 = hip.split_operand(cent, 1)
        cnorm = (self.centroids.double() ** 2).sum(1).to(device=device, dtype=torch.float32)
        eye = {}
        for op in ops:                       # GELU after the LayerNorm: the act epilogue of an identity GEMM (exact in fp32 mode: x * 1 + 0 ...)
            if op[0] == 'proj':
                for L in op[1]:
                    if L[0] == 'lin_ln_gelu':
                        n = L[1].shape[0]
                        eye.setdefault(n, torch.eye(n, dtype=torch.float32, device=device))
        pk = dict(ops=ops, cent=cent, c3=c3, cnorm=cnorm, eye=eye)
        self._packed[str(device)] = pk
        return pk

    def head(self, x):
        """x fp32 [rows, d_in] on the device -> fp32 [rows, D] (before the row selection)"""
        pk = self.packed(x.device)
        rows = x.shape[0]
        h = x.contiguous()
        with precision('fp32_exact'):
            for op in pk['ops']:
                if op[0] == 'lin':
                    out = torch.empty(rows, op[1].shape[0], dtype=torch.float32, device=x.device)
                    h = hip.gemm(h, op[1], out, bias=op[2])
                    continue
                h0 = h
                for L in op[1]:
                    W, b = L[1], L[2]
                    out = torch.empty(rows, W.shape[0], dtype=torch.float32, device=x.device)
                    if L[0] == 'lin_ln_gelu':
                        hip.gemm(h, W, out, bias=b)
                        ln = torch.empty_like(out)
                        hip.layernorm(out, L[3][0], L[3][1], ln, LN_EPS)
                        hip.gemm(ln, pk['eye'][W.shape[0]], out, act='gelu')
                    else:
                        hip.gemm(h, W, out, bias=b, res=h0 if op[2] else None)
                    h = out
        return h

    def descriptors(self, xs):
        """xs: list of per-view fp32 [T_v, d_in] device tensors -> (descriptors fp32 [n, D] L2-normalised, rows per view)"""
        dev = xs[0].device
        Ts = [int(x.shape[0]) for x in xs]
        feat = self.head(torch.cat([x.float() for x in xs], 0) if len(xs) > 1 else xs[0].float())
        counts = [min(self.nfeat, T) for T in Ts]
        in_off = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=torch.int32, device=dev)
        out_off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
        desc = torch.empty(sum(counts), self.D, dtype=torch.float32, device=dev)
        hip.retrieval_select(feat, in_off, out_off, desc, max(Ts))
        return desc, counts

    def assign(self, desc, m):
        pk = self.packed(desc.device)
        x3 = hip.split_operand(desc, 0, kpad=pk['c3'].shape[1] // 3)
        ids = torch.empty(desc.shape[0], m, dtype=torch.int32, device=desc.device)
        dist = torch.empty(desc.shape[0], m, dtype=torch.float32, device=desc.device)
        hip.retrieval_assign(x3, pk['c3'], pk['cnorm'], m, ids, dist)
        return ids, dist

    def groups(self, ids, view, ma, V):
        """(view, word) groups of the first `ma` assignments (ATen glue: a stable sort on int keys, unique): members in ascending descriptor order"""
        n = ids.shape[0]
        key = (view.to(torch.int64)[:, None] * self.k + ids[:, :ma].to(torch.int64)).reshape(-1)
        skey, order = torch.sort(key, stable=True)
        member = (order // ma).to(torch.int32)
        gkey, counts = torch.unique_consecutive(skey, return_counts=True)
        gstart = torch.zeros(gkey.numel() + 1, dtype=torch.int32, device=ids.device)
        gstart[1:] = torch.cumsum(counts, 0).to(torch.int32)
        gword = (gkey % self.k).to(torch.int32)
        gview = gkey // self.k
        voff = torch.searchsorted(gview, torch.arange(V + 1, device=ids.device, dtype=torch.int64)).to(torch.int32)
        assert member.numel() == n * ma
        return member.contiguous(), gstart, gword.contiguous(), voff.contiguous()

    def aggregate(self, desc, grp, sums=False):
        member, gstart, gword, voff = grp
        pk = self.packed(desc.device)
        bits = torch.empty(gword.numel(), self.D // 32, dtype=torch.int32, device=desc.device)
        s = torch.empty(gword.numel(), self.D, dtype=torch.float32, device=desc.device) if sums else None
        hip.retrieval_aggregate(desc, pk['cent'], member, gstart, gword, bits, s)
        return bits, s

    def scores(self, qgrp, qbits, dbgrp, dbbits):
        qoff, dboff = qgrp[3], dbgrp[3]
        S = torch.empty(qoff.numel() - 1, dboff.numel() - 1, dtype=torch.float32, device=qbits.device)
        max_q = int((qoff[1:] - qoff[:-1]).max())
        hip.retrieval_scores(qoff, qgrp[2], qbits, dboff, dbgrp[2], dbbits, self.D, self.params['alpha'], self.params['tau'], S, max_q)
        return S

    def similarity(self, xs):
        """per-view encoder tokens (list of [T_v, d_in] device tensors, any float format) -> S fp32 [V, V] on the device"""
        V = len(xs)
        desc, counts = self.descriptors(xs)
        p = self.params
        ids, _ = self.assign(desc, max(p['ma_q'], p['ma_db']))
        view = torch.repeat_interleave(torch.arange(V, device=desc.device), torch.tensor(counts, device=desc.device))
        dbg = self.groups(ids, view, p['ma_db'], V)
        qg = dbg if p['ma_q'] == p['ma_db'] else self.groups(ids, view, p['ma_q'], V)
        dbb, _ = self.aggregate(desc, dbg)
        qb = dbb if qg is dbg else self.aggregate(desc, qg)[0]
        return self.scores(qg, qb, dbg, dbb)
