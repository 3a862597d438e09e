"""Shared by tests/test_hip_pp_stages.py, tests/test_hip_pointmap_stages.py (GPU) and tests/test_pp_stage_checks.py (CPU): the case tables, the float64
references of every stage of csrc/postprocess.hip and csrc/pointmap.hip, the checkers that compare a result with them, and float32 numpy emulations of the
kernels' arithmetic (with the planted mistakes the CPU module feeds to the checkers).  Nothing here imports the code under test.

Bilinear taps: positions and weights are part of the operation, taken as F.interpolate(mode='bilinear', align_corners=False) takes them for fp32 input -
scale = in / out and src = scale * (dst + 0.5) - 0.5 in float32 with every operation rounded, clamped at 0, neighbour clamped at the last row / column,
weight l = src - i0 and h = 1 - l in float32.  Sigmoid, blend, score product and every comparison are float64.

Decidedness: a comparison of the reference is decided when it clears its threshold (or the winner its runner-up) by more than the derived fp32 error bound
of the compared value (errbound.sigmoid_bound / blend_bound / product_bound).  Decided results must be reproduced exactly; undecided ones only widen an
integer interval or a candidate set.  CAP_WINNER / CAP_BAND limit how much may be undecided in a case; they are asserted on the reference alone."""
import math
import types

import numpy as np
import torch

import errbound as EB

CAP_WINNER = 1e-3        # share of the pixels of a case whose winner may be undecided
CAP_BAND = 8             # pixels of one query that may sit inside the error band around 0.5
F32 = np.float32

# (Q, Hm, Wm, H, W): production; two ragged-tile non-dyadic shapes; ratio 1 (CH = 3); 1.5 x down-sampling (CH = 1); every compaction pass (Q = 1024)
ARGMAX_SHAPES = [(200, 192, 256, 384, 512), (200, 25, 31, 75, 93), (257, 40, 56, 75, 93), (64, 48, 64, 48, 64), (24, 96, 128, 64, 85), (1024, 12, 16, 24, 32)]
DOWN4_SHAPE = (16, 96, 128, 24, 32)        # 4 x down-sampling: pp_argmax only, the fused kernel refuses the footprint
MASK_THR = 0.25


def shape_id(s):
    return 'Q%d_%dx%d_to_%dx%d' % s


def fused_geometry(Hm, Wm, H, W):
    """host restatement of pst_pp_argmax_logits' footprint rule (8 x 32 output tiles): rh, rw, CH (CH < 1: refused)"""
    rh = min(Hm, int(np.ceil(F32(8) * F32(Hm) / F32(H))) + 2)
    rw = min(Wm, int(np.ceil(F32(32) * F32(Wm) / F32(W))) + 2)
    return rh, rw, min(8, 1024 // (rh * rw))


def blob_scene(seed, Q, ncls, lowres, maxfrac=1.0):
    """class logits [1, Q, ncls] and per view mask logits [1, Q, h, w]: noise around -3 with one +6 rectangle per query (tests/test_hip_postprocess.py uses
    the same generator for its end-to-end scenes)"""
    g = np.random.Generator(np.random.PCG64(seed))
    logits = torch.from_numpy(g.standard_normal((1, Q, ncls)).astype(np.float32)) * 2
    masks = []
    for (h, w) in lowres:
        m = torch.from_numpy(g.standard_normal((1, Q, h, w)).astype(np.float32)) * 1.5 - 3.0
        for q in range(Q):
            y0, x0 = int(g.integers(0, h - 2)), int(g.integers(0, w - 2))
            y1 = int(g.integers(y0 + 2, min(h, y0 + max(2, int(h * maxfrac))) + 1))
            x1 = int(g.integers(x0 + 2, min(w, x0 + max(2, int(w * maxfrac))) + 1))
            m[0, q, y0:y1, x0:x1] += 6.0
        masks.append(m)
    return logits, masks


def blobs(seed, Q, h, w, maxfrac=0.2):
    """mask logits [Q, h, w] of one view of blob_scene"""
    return blob_scene(seed, Q, 2, [(h, w)], maxfrac=maxfrac)[1][0][0].contiguous()


def make_case(shape, seed=0):
    Q, Hm, Wm, H, W = shape
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    scores = torch.from_numpy((0.1 + 0.9 * g.random(Q)).astype(F32))
    return blobs(seed + Q + Hm, Q, Hm, Wm), scores


def keep_patterns(Q, CH):
    """name -> int32 keep flags: the chunk-boundary counts, the extremes, and kept queries only beyond the first compaction pass"""
    g = np.random.Generator(np.random.PCG64(Q))
    pats = {'all': np.ones(Q, np.int32), 'none': np.zeros(Q, np.int32)}
    last = np.zeros(Q, np.int32); last[Q - 1] = 1
    pats['last'] = last
    for nk in sorted({1, CH, CH + 1, 2 * CH - 1}):
        if nk <= Q:
            k = np.zeros(Q, np.int32)
            k[np.sort(g.choice(Q, nk, replace=False))] = 1
            pats['nk%d' % nk] = k
    if Q > 257:
        k = np.zeros(Q, np.int32)
        k[256 + np.sort(g.choice(Q - 256, min(Q - 256, 19), replace=False))] = 1
        pats['beyond256'] = k
    return pats


# ------------------------------------------------------------------------------------------------------------------------------------------- taps
def taps(n_in, n_out, mode='ref', n_dst=None):
    """i0, i1 (int64), l, h (float32) of one axis.  mode 'ref' as the module docstring; 'fma': the product unrounded before the subtraction (a contracted
    fma); 'align_corners': scale (in - 1) / (out - 1), src = scale * dst.  n_dst > n_out: also the destination indices beyond the image that a tile of
    the fused kernel holds, with the scale of the real size."""
    dst = np.arange(n_dst or n_out, dtype=F32)
    if mode == 'align_corners':
        src = (F32(n_in - 1) / F32(max(n_out - 1, 1))) * dst
    else:
        scale = F32(n_in) / F32(n_out)
        if mode == 'fma':
            src = (scale.astype(np.float64) * (dst + F32(0.5)).astype(np.float64) - 0.5).astype(F32)
        else:
            src = scale * (dst + F32(0.5)) - F32(0.5)
    src = np.maximum(src, F32(0)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
    return i0, i1, l, (F32(1) - l).astype(F32)


def exp32(x):
    """a correctly rounded expf (the emulations stand for the kernel's arithmetic, not for a libm)"""
    with np.errstate(over='ignore'):
        return np.exp(np.asarray(x, dtype=np.float64)).astype(F32)


class Grid:
    """per-pixel tap rows / columns and weights of an H x W output over an Hm x Wm input, flattened row-major"""

    def __init__(self, Hm, Wm, H, W, mode='ref'):
        y0, y1, ly, hy = taps(Hm, H, mode)
        x0, x1, lx, hx = taps(Wm, W, mode)
        rep = lambda a: np.repeat(a, W)
        til = lambda a: np.tile(a, H)
        self.y0, self.y1, self.ly, self.hy = rep(y0), rep(y1), rep(ly), rep(hy)
        self.x0, self.x1, self.lx, self.hx = til(x0), til(x1), til(lx), til(hx)
        self.n = H * W

    def sub(self, idx):
        g = object.__new__(Grid)
        for k in ('y0', 'y1', 'ly', 'hy', 'x0', 'x1', 'lx', 'hx'):
            setattr(g, k, getattr(self, k)[idx])
        g.n = len(idx)
        return g

    def blend64(self, s):
        """s [n, Hm, Wm] float64 torch -> [n, N] float64: hy (hx a + lx b) + ly (hx c + lx d)"""
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        y0, y1, x0, x1 = t(self.y0), t(self.y1), t(self.x0), t(self.x1)
        ly, hy, lx, hx = (t(a).double() for a in (self.ly, self.hy, self.lx, self.hx))
        return hy * (hx * s[:, y0, x0] + lx * s[:, y0, x1]) + ly * (hx * s[:, y1, x0] + lx * s[:, y1, x1])


def ref_m(logits, grid):
    """float64 blended probability m [n, N] of fp32 logits [n, Hm, Wm] and its fp32 error bound"""
    s = logits.double().sigmoid()
    m = grid.blend64(s)
    return m, EB.blend_bound(m, grid.blend64(EB.sigmoid_bound(s)))


# ------------------------------------------------------------------------------------------------------------------------------------------- argmax stage
def ref_argmax(logits, scores, keep, H, W, mask_thr=MASK_THR, chunk=8):
    """float64 reference of one view of pp_argmax / pp_argmax_logits with the decidedness of every comparison (module docstring).
    Fields: kept, q1, m1, dm1 (winner, its m and bound; q1 = -1 and m1 = 0 with nothing kept), decided [N], cand {pixel: [(q, m, dm)]} of the undecided pixels,
    orig_lo / orig_hi, mask_lo / mask_hi [Q] (the integer intervals), band [Q] (pixels inside the 0.5 band), undecided_share."""
    Q, Hm, Wm = logits.shape
    N = H * W
    grid = Grid(Hm, Wm, H, W)
    r = types.SimpleNamespace()
    r.kept = np.flatnonzero(np.asarray(keep))
    r.N, r.Q = N, Q
    r.orig_lo, r.band = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    r.mask_lo, mask_extra = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    p1 = torch.full((N,), -1.0, dtype=torch.float64)
    p2 = torch.full((N,), -math.inf, dtype=torch.float64)
    q1 = torch.full((N,), -1, dtype=torch.int64)
    m1, dm1, bmax = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    sc = scores.double()
    for c0 in range(0, len(r.kept), chunk):
        qs = torch.from_numpy(r.kept[c0:c0 + chunk])
        m, dm = ref_m(logits[qs], grid)
        r.orig_lo[qs.numpy()] = (m - 0.5 > dm).sum(1).numpy()
        r.band[qs.numpy()] = ((m - 0.5).abs() <= dm).sum(1).numpy()
        p = sc[qs, None] * m
        bmax = torch.maximum(bmax, EB.product_bound(sc[qs, None], m, dm).amax(0))
        for j in range(len(qs)):                                   # kept-query order; strict >: the first maximal query wins
            better = p[j] > p1
            p2 = torch.where(better, p1, torch.maximum(p2, p[j]))
            q1 = torch.where(better, qs[j], q1)
            m1, dm1 = torch.where(better, m[j], m1), torch.where(better, dm[j], dm1)
            p1 = torch.where(better, p[j], p1)
    r.orig_hi = r.orig_lo + r.band
    decided = (p1 - p2 > 2 * bmax) | (q1 < 0)
    r.q1, r.m1, r.dm1, r.decided = q1.numpy(), m1.numpy(), dm1.numpy(), decided.numpy()
    r.undecided_share = float((~decided).sum()) / N
    own = decided & (q1 >= 0)
    inside, edge = own & (m1 - mask_thr > dm1), own & ((m1 - mask_thr).abs() <= dm1)
    np.add.at(r.mask_lo, r.q1[inside.numpy()], 1)
    np.add.at(mask_extra, r.q1[edge.numpy()], 1)
    r.cand = {}
    und = np.flatnonzero(~r.decided)
    if len(und):
        gs = grid.sub(und)
        ms, dms = [], []
        for c0 in range(0, len(r.kept), 64):
            m, dm = ref_m(logits[torch.from_numpy(r.kept[c0:c0 + 64])], gs)
            ms.append(m); dms.append(dm)
        m, dm = torch.cat(ms), torch.cat(dms)
        p = sc[torch.from_numpy(r.kept), None] * m
        ok = (p + 2 * bmax[torch.from_numpy(und)] >= p1[torch.from_numpy(und)]).numpy()
        for k, pix in enumerate(und):
            js = np.flatnonzero(ok[:, k])
            r.cand[int(pix)] = [(int(r.kept[j]), float(m[j, k]), float(dm[j, k])) for j in js]
            for j in js:
                if float(m[j, k]) >= mask_thr - float(dm[j, k]):
                    mask_extra[r.kept[j]] += 1
    r.mask_hi = r.mask_lo + mask_extra
    return r


def assert_caps(r, what):
    """the conditions of a case, on the reference alone (before any result is looked at)"""
    assert r.undecided_share <= CAP_WINNER, '%s: %.3g of the pixels have an undecided winner (cap %.3g): change the seed' % (what, r.undecided_share, CAP_WINNER)
    assert int(r.band.max()) <= CAP_BAND, '%s: a query has %d pixels inside the 0.5 band (cap %d): change the seed' % (what, int(r.band.max()), CAP_BAND)


def check_best(r, best_q, best_m, what):
    """best_q equal and best_m within its bound on every decided pixel; on an undecided pixel the winner is one of the candidates, with that candidate's m.
    Returns the largest |best_m - m| / bound."""
    bq, bm = np.asarray(best_q).reshape(-1).astype(np.int64), np.asarray(best_m).reshape(-1).astype(np.float64)
    assert bq.shape == (r.N,) and bm.shape == (r.N,), what
    d = r.decided
    wrong = np.flatnonzero(d & (bq != r.q1))
    assert len(wrong) == 0, '%s: %d decided pixels have another winner, first pixel %d: got %d, reference %d' % (what, len(wrong), wrong[0], bq[wrong[0]], r.q1[wrong[0]])
    err = np.abs(bm - r.m1)[d]
    bound = np.where(r.q1 >= 0, r.dm1, 0.0)[d]
    bad = np.flatnonzero(err > bound)
    assert len(bad) == 0, '%s: best_m off its bound at %d decided pixels, first err %.3g bound %.3g' % (what, len(bad), err[bad[0]], bound[bad[0]])
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    for pix, cands in r.cand.items():
        hit = [c for c in cands if c[0] == bq[pix]]
        assert hit, '%s: undecided pixel %d: winner %d is not among the candidates %s' % (what, pix, bq[pix], [c[0] for c in cands])
        assert abs(bm[pix] - hit[0][1]) <= hit[0][2], '%s: undecided pixel %d: best_m %.9g, candidate %d has %.9g +- %.3g' % (what, pix, bm[pix], hit[0][0], hit[0][1], hit[0][2])
        ratio = max(ratio, abs(bm[pix] - hit[0][1]) / hit[0][2])
    return ratio


def check_counts(refs, cnt_orig, cnt_mask, orig0, mask0, what):
    """the counters after the views `refs` were accumulated on top of orig0 / mask0 lie in the intervals the decided pixels give"""
    co, cm = np.asarray(cnt_orig).astype(np.int64), np.asarray(cnt_mask).astype(np.int64)
    for name, got, start, lo, hi in (('cnt_orig', co, orig0, 'orig_lo', 'orig_hi'), ('cnt_mask', cm, mask0, 'mask_lo', 'mask_hi')):
        lo_ = np.asarray(start).astype(np.int64) + sum(getattr(r, lo) for r in refs)
        hi_ = np.asarray(start).astype(np.int64) + sum(getattr(r, hi) for r in refs)
        bad = np.flatnonzero((got < lo_) | (got > hi_))
        assert len(bad) == 0, '%s: %s of %d queries outside the interval, first query %d: got %d, interval [%d, %d]' % (what, name, len(bad), bad[0], got[bad[0]], lo_[bad[0]], hi_[bad[0]])


def emulate_argmax(logits, scores, keep, H, W, mask_thr=MASK_THR, variant=None):
    """float32 numpy emulation of pp_argmax_logits' arithmetic: sigmoid of the kept planes, the taps read through the 8 x 32 tile's clamped LDS footprint,
    unfused fp32 blend, strict > in kept order, counts over the valid pixels.  Returns best_q, best_m, d_orig, d_mask (this view's counts).
    variant: one planted mistake - 'rows_short' / 'cols_short' (footprint one row / column short, clamp in place), 'ge' (>= for >), 'reverse' (kept list walked
    backwards), 'drop_odd_last' (last query of an odd chunk dropped), 'no_valid' (0.5 count without the valid mask), 'align_corners', 'fma' (taps())."""
    lg = logits.numpy() if torch.is_tensor(logits) else logits
    sc = scores.numpy() if torch.is_tensor(scores) else scores
    Q, Hm, Wm = lg.shape
    rh, rw, CH = fused_geometry(Hm, Wm, H, W)
    rh, rw = rh - (variant == 'rows_short'), rw - (variant == 'cols_short')
    mode = variant if variant in ('align_corners', 'fma') else 'ref'
    Hp, Wp = -(-H // 8) * 8, -(-W // 32) * 32
    y0, y1, ly, hy = taps(Hm, H, mode, Hp)
    x0, x1, lx, hx = taps(Wm, W, mode, Wp)
    in_y0, in_x0 = np.repeat(y0[::8], 8), np.repeat(x0[::32], 32)
    ey0, ey1 = np.minimum(in_y0 + np.minimum(y0 - in_y0, rh - 1), Hm - 1), np.minimum(in_y0 + np.minimum(y1 - in_y0, rh - 1), Hm - 1)
    ex0, ex1 = np.minimum(in_x0 + np.minimum(x0 - in_x0, rw - 1), Wm - 1), np.minimum(in_x0 + np.minimum(x1 - in_x0, rw - 1), Wm - 1)
    rep, til = (lambda a: np.repeat(a, Wp)), (lambda a: np.tile(a, Hp))
    Y0, Y1, LY, HY, X0, X1, LX, HX = rep(ey0), rep(ey1), rep(ly), rep(hy), til(ex0), til(ex1), til(lx), til(hx)
    valid = (rep(np.arange(Hp)) < H) & (til(np.arange(Wp)) < W)
    kept = np.flatnonzero(np.asarray(keep))
    if variant == 'reverse':
        kept = kept[::-1]
    if variant == 'drop_odd_last' and len(kept) % CH % 2 == 1:
        kept = kept[:-1]
    n = Hp * Wp
    bp, bm, bq = np.full(n, -1, F32), np.zeros(n, F32), np.full(n, -1, np.int64)
    d_orig, d_mask = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    one = F32(1)
    for q in kept:
        s = (one / (one + exp32(-lg[q]))).astype(F32)
        m = HY * (HX * s[Y0, X0] + LX * s[Y0, X1]) + LY * (HX * s[Y1, X0] + LX * s[Y1, X1])
        d_orig[q] = int(((m >= F32(0.5)) & (valid | (variant == 'no_valid'))).sum())
        p = sc[q] * m
        better = (p >= bp) if variant == 'ge' else (p > bp)
        bp, bm, bq = np.where(better, p, bp), np.where(better, m, bm), np.where(better, q, bq)
    own = valid & (bq >= 0) & (bm >= F32(mask_thr))
    np.add.at(d_mask, bq[own], 1)
    return bq[valid].astype(np.int32), bm[valid].astype(F32), d_orig, d_mask


def tie_case(shape, seed, bump):
    """two kept queries (lo < hi) with identical logit planes: score 0.5 for lo (a power of two: 0.5 m is exact and fl(0.5 (1 + 2^-23) m) > 0.5 m for every
    normal m, so one ulp more decides every pixel); hi gets 0.5 (bump False) or the next float (bump True).  Returns logits, scores, lo, hi."""
    logits, scores = make_case(shape, seed)
    Q = shape[0]
    lo, hi = Q // 3, Q - 1 - Q // 5
    logits[hi] = logits[lo]
    scores[lo] = 0.5
    scores[hi] = float(np.nextafter(F32(0.5), F32(1))) if bump else 0.5
    return logits, scores, lo, hi


def check_tie(both, alone, lo, hi, bump, what):
    """both: (best_q, best_m, d_orig, d_mask) with lo and hi kept; alone: the same inputs with hi not kept.  Identical planes and scores: hi owns nothing and
    everything equals the run without it.  hi one ulp larger: hi owns exactly the pixels lo owned, with the same m."""
    bq, bm, do, dmk = (np.asarray(a) for a in both)
    aq, am, ao, amk = (np.asarray(a) for a in alone)
    assert np.array_equal(bm, am), what + ': best_m differs from the run without the twin'
    assert do[hi] == do[lo] == ao[lo], what + ': the twins count different 0.5 areas'
    if not bump:
        assert not (bq == hi).any(), '%s: the higher id owns %d pixels of an exact tie' % (what, int((bq == hi).sum()))
        assert np.array_equal(bq, aq) and dmk[lo] == amk[lo] and dmk[hi] == 0, what
    else:
        assert not (bq == lo).any(), '%s: the lower id keeps %d pixels although its twin scores one ulp more' % (what, int((bq == lo).sum()))
        assert np.array_equal(bq == hi, aq == lo) and np.array_equal(bq[bq != hi], aq[aq != lo]) and dmk[hi] == amk[lo] and dmk[lo] == 0, what


# ------------------------------------------------------------------------------------------------------------------------------------------- scores
SCORE_NCLS = [2, 63, 64, 65, 133, 1000]
SCORE_Q = [1, 200, 1024]


def scores_case(Q, ncls, seed):
    """class logits with planted exactly equal maxima: row 1 in different lanes (columns 3 and 7), row 2 in different strides of one lane (columns 5 and
    5 + 64 where they exist), row 0 with maximum exactly 0 (sigmoid 0.5, representable: the threshold sits on it)"""
    g = np.random.Generator(np.random.PCG64(seed * 7919 + Q * 31 + ncls))
    x = (g.standard_normal((Q, ncls)) * 2).astype(F32)
    x[0] = np.minimum(x[0], F32(-0.5)); x[0, ncls // 2] = 0
    if Q > 1 and ncls > 7:
        x[1, 3] = x[1, 7] = x[1].max() + F32(1)
    if Q > 2 and ncls > 69:
        x[2, 5] = x[2, 69] = x[2].max() + F32(1)
    return torch.from_numpy(x)


def check_scores(logits, mode, thr, temperature, scores, labels, keep, what):
    """mode 'sigmoid' (pp_scores) or 'softmax' (pp_scores_softmax) against float64.  Returns the largest score err / bound.
    Labels: softmax mode takes the argmax of the raw logits (exact: the lowest maximal column).  Sigmoid mode takes it over fp32 sigmoids, which saturate:
    the label must be a column whose float64 sigmoid is within two bounds of the largest, and the lowest such column when the raw logits tie exactly."""
    x = logits.double()
    sc, lb, kp = (np.asarray(a) for a in (scores, labels, keep))
    Q, N = x.shape
    if mode == 'softmax':
        lab = x.argmax(-1)                                          # torch: first maximal index
        arg = x - x.amax(-1, keepdim=True)
        ref = 1.0 / arg.exp().sum(-1)
        bound = EB.softmax_score_bound(arg, EB.R * EB.U32 * arg.abs(), N)
        assert np.array_equal(lb, lab.numpy()), what + ': labels'
        dec = (ref - thr).abs() > bound
        kref = (lab != N - 1) & (ref > thr)
    else:
        v = x.sigmoid()
        dv = EB.sigmoid_bound(v)
        best, lab = v.max(-1)
        tied_raw = x == x.amax(-1, keepdim=True)
        first = tied_raw.int().argmax(-1)
        near = v + dv + dv.gather(1, lab[:, None]) >= best[:, None]
        for q in range(Q):
            assert bool(near[q, lb[q]]), '%s: label %d of row %d is not a maximal column' % (what, lb[q], q)
            if int(near[q].sum()) == int(tied_raw[q].sum()):
                assert lb[q] == int(first[q]), '%s: row %d: label %d, the lowest maximal column is %d' % (what, q, lb[q], int(first[q]))
        dbest = dv.gather(1, lab[:, None])[:, 0]
        dec = (best - thr).abs() > dbest
        kref = best > thr
        if temperature:
            arg = (v - best[:, None]) / temperature
            darg = (dv + dbest[:, None] + EB.R * EB.U32 * (v - best[:, None]).abs()) / temperature + EB.R * EB.U32 * arg.abs()
            ref, bound = 1.0 / arg.exp().sum(-1), EB.softmax_score_bound(arg, darg, N)
        else:
            ref, bound = best, dbest
    exact = (ref == thr)                                            # a threshold exactly on a representable score: strict >, keep = 0 (both sides are exact there)
    assert np.array_equal(kp[dec.numpy()], kref.numpy()[dec.numpy()].astype(kp.dtype)), what + ': keep'
    return EB.check(torch.from_numpy(sc.astype(np.float64)), ref, bound, what), int(exact.sum())


def emulate_scores(logits, mode, thr, temperature):
    x = logits.numpy()
    one = F32(1)
    if mode == 'softmax':
        lab = x.argmax(-1)
        e = exp32(x - x.max(-1, keepdims=True))
        sc = one / _lane_sum(e)
        return sc, lab.astype(np.int32), ((lab != x.shape[1] - 1) & (sc > F32(thr))).astype(np.int32)
    v = (one / (one + exp32(-x))).astype(F32)
    lab, best = v.argmax(-1), v.max(-1)
    sc = best
    if temperature:
        sc = one / _lane_sum(exp32((v - best[:, None]) / F32(temperature)))
    return sc.astype(F32), lab.astype(np.int32), (best > F32(thr)).astype(np.int32)


def _lane_sum(e):
    """the kernel's order: 64 lanes, each over its stride, then the xor tree"""
    Q, N = e.shape
    pad = np.zeros((Q, -(-N // 64) * 64), F32); pad[:, :N] = e
    lanes = np.zeros((Q, 64), F32)
    for k in range(pad.shape[1] // 64):
        lanes = lanes + pad[:, 64 * k:64 * k + 64]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ off]
    return lanes[:, 0]


# ------------------------------------------------------------------------------------------------------------------------------------------- select / finalize
SELECT_Q = [1, 255, 256, 257, 1023, 1024]
# (cnt_mask, cnt_orig, threshold, selected): exactly at the threshold, one count below / above, zero counts, and a ratio that only double tells from 0.8
SELECT_PLANTS = [(1, 2, 0.5, 1), (3, 6, 0.5, 1), (2, 6, 0.5, 0), (4, 6, 0.5, 1), (4, 5, 0.8, 1), (3, 5, 0.8, 0), (5, 5, 0.8, 1), (0, 9, 0.5, 0), (7, 0, 0.5, 0),
                 (0, 0, 0.5, 0), (799999999, 1000000000, 0.8, 0), (800000000, 1000000000, 0.8, 1)]


def select_case(Q, thr, seed):
    """keep, cnt_orig, cnt_mask with the plants of this threshold in front (as far as Q allows) and keep == 0 rows with large counts"""
    g = np.random.Generator(np.random.PCG64(seed * 131 + Q))
    co = g.integers(0, 5000, Q).astype(np.int32)
    cm = (co * g.random(Q)).astype(np.int32)
    keep = (g.random(Q) < 0.7).astype(np.int32)
    plants = [p for p in SELECT_PLANTS if p[2] == thr][:Q]
    for i, (m, o, _, _) in enumerate(plants):
        cm[i], co[i], keep[i] = m, o, 1
    if Q > len(plants) + 1:
        keep[len(plants)], co[len(plants)], cm[len(plants)] = 0, 2000000000, 2000000000
    return keep, co, cm, plants


def ref_select(keep, co, cm, thr):
    """Python integers and Python's float division, as the model's post-processing does it"""
    sel, seg, run = [], [], 0
    for k, o, m in zip(keep.tolist(), co.tolist(), cm.tolist()):
        s = int(bool(k) and m > 0 and o > 0 and not (m / o < thr))
        run += s
        sel.append(s); seg.append(run if s else 0)
    return np.array(sel, np.int32), np.array(seg, np.int32)


def emulate_select(keep, co, cm, thr, variant=None):
    """variant 'fp32_ratio': cm / co < thr in float32; 'seg_all': seg_id numbered over all queries"""
    if variant == 'fp32_ratio':
        below = cm.astype(F32) / np.maximum(co, 1).astype(F32) < F32(thr)
    else:
        below = cm.astype(np.float64) / np.maximum(co, 1).astype(np.float64) < thr
    sel = ((keep != 0) & (cm > 0) & (co > 0) & ~below).astype(np.int32)
    seg = np.where(sel > 0, np.arange(1, len(sel) + 1) if variant == 'seg_all' else np.cumsum(sel), 0).astype(np.int32)
    return sel, seg


def check_select(keep, co, cm, thr, keep_out, seg_id, what):
    sel, seg = ref_select(keep, co, cm, thr)
    assert np.array_equal(np.asarray(keep_out), sel), what + ': keep_out'
    assert np.array_equal(np.asarray(seg_id), seg), what + ': seg_id'


FINALIZE_N = [1, 255, 256, 257, 384 * 512]


def finalize_case(n, Q, thr, seed):
    g = np.random.Generator(np.random.PCG64(seed + n))
    bq = g.integers(-1, Q, n).astype(np.int32)
    bm = g.random(n).astype(F32)
    bm[::5] = F32(thr)
    bm[1::5] = np.nextafter(F32(thr), F32(0))
    seg = np.arange(1, Q + 1, dtype=np.int32)
    seg[::3] = 0                                                    # winners that are not a segment: void confidence
    return bq, bm, seg


def ref_finalize(bq, bm, seg, thr, void):
    ok = (bq >= 0) & (bm.astype(np.float64) >= float(F32(thr)))
    pan = np.where(ok, seg[np.maximum(bq, 0)], 0).astype(np.int32)
    return pan, np.where(pan > 0, bm, F32(void)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------------------- QUBO
QUBO_Q = [1, 15, 16, 17, 200]
QUBO_P = [1, 255, 256, 257, 75 * 93, 384 * 512]


def qubo_probs(Q, P, seed):
    g = np.random.Generator(np.random.PCG64(seed * 17 + Q * 3 + P))
    return torch.from_numpy(g.random((Q, P)).astype(F32))


def ref_overlap(probs):
    """S[i][j] = sum_p min(p_i, p_j) in float64 and the bound of the kernel's chunked sums"""
    Q, P = probs.shape
    S = torch.empty(Q, Q, dtype=torch.float64)
    for i in range(Q):
        S[i] = torch.minimum(probs[i][None], probs).sum(1, dtype=torch.float64)       # the minimum of two fp32 values is exact
    return S, EB.chunked_sum_bound(S, -(-P // 256))


def emulate_overlap(probs):
    x = probs.numpy()
    Q, P = x.shape
    out = np.zeros((Q, Q), np.float64)
    for c0 in range(0, P, 256):
        mn = np.minimum(x[:, None, c0:c0 + 256], x[None, :, c0:c0 + 256])
        s = np.zeros((Q, Q), F32)
        for k in range(mn.shape[2]):
            s = s + mn[:, :, k]
        out += s.astype(np.float64)
    return out


def ref_qubo_argmax(probs, sel):
    """(max, position in sel of the first maximum) per pixel: fp32 values compared exactly"""
    sub = probs[torch.as_tensor(sel, dtype=torch.long)]
    conf, inst = sub.max(0)
    first = (sub == conf[None]).int().argmax(0)
    return conf, first.int()


# ------------------------------------------------------------------------------------------------------------------------------------------- pointmaps
ACT_NPIX = [1, 255, 257, 384 * 512, 12 * 384 * 512]
ACT_MAXNORM = 88.0        # expm1(88) = 1.65e38 is finite in fp32; 89 overflows


def activate_case(npix, seed):
    """raw [npix, 7]: random directions with |xyz| log-uniform in [1e-5, 88] and exactly 0, 1e-12, 1e-9, 1e-4, 88 planted; confidence logits in [-30, 80]"""
    g = np.random.Generator(np.random.PCG64(seed + npix))
    raw = np.empty((npix, 7), F32)
    for h in range(2):
        v = g.standard_normal((npix, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        mag = np.exp(g.uniform(np.log(1e-5), np.log(ACT_MAXNORM), npix))
        special = np.array([0.0, 1e-12, 1e-9, 1e-4, ACT_MAXNORM])
        k = np.arange(npix) % 16
        mag = np.where(k < 5, special[np.minimum(k, 4)], mag)
        raw[:, 3 * h:3 * h + 3] = (v * mag[:, None]).astype(F32)
    raw[:, 6] = g.uniform(-30, 80, npix).astype(F32)
    if npix >= 2:
        raw[0, 6], raw[1, 6] = -30, 80
    # keep fp32 |xyz| at or below ACT_MAXNORM after rounding
    n = np.linalg.norm(raw[:, :6].astype(np.float64).reshape(npix, 2, 3), axis=2, keepdims=True)
    raw[:, :6] = (raw[:, :6].reshape(npix, 2, 3) * np.where(n > ACT_MAXNORM, ACT_MAXNORM / np.maximum(n, 1e-300) * (1 - 1e-6), 1.0)).reshape(npix, 6).astype(F32)
    return torch.from_numpy(raw)


def ref_activate(raw):
    """float64: xyz / max(d, 1e-8) * expm1(d) for both triples, conf = 1 + exp(c); and the bounds"""
    r = raw.double()
    outs, bounds = [], []
    for h in range(2):
        xyz = r[:, 3 * h:3 * h + 3]
        d = xyz.norm(dim=-1, keepdim=True)
        ref = xyz / d.clamp_min(1e-8) * torch.expm1(d)
        outs.append(ref); bounds.append(EB.activate_bound(xyz, ref))
    return outs[0], outs[1], 1.0 + r[:, 6].exp(), bounds[0], bounds[1], EB.conf_bound(r[:, 6])


def emulate_activate(raw, variant=None, canary=-7.0):
    """fp32 numpy; variant 'expf_minus_1': expf(d) - 1 for expm1f(d); 'one_pass': the grid-stride loop stops after 8192 x 256 pixels (the rest keeps `canary`)"""
    x = raw.numpy()
    n = x.shape[0]
    outs = []
    for h in range(2):
        v = x[:, 3 * h:3 * h + 3]
        d = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F32)
        em = (exp32(d) - F32(1)) if variant == 'expf_minus_1' else np.expm1(d.astype(np.float64)).astype(F32)
        outs.append((v * (em / np.maximum(d, F32(1e-8)))[:, None]).astype(F32))
    conf = (F32(1) + exp32(x[:, 6])).astype(F32)
    if variant == 'one_pass' and n > 8192 * 256:
        for a in outs + [conf]:
            a[8192 * 256:] = canary
    return outs[0], outs[1], conf


FOCAL_HW = [(5, 7), (31, 33), (160, 96), (384, 512)]
FOCAL_ITERS = [0, 1, 10]


def focal_case(H, W, V, seed):
    """V pinhole views (focal 0.6 .. 1.1 of the larger side, own principal point) of a random depth map with 0.3 px noise, 10 % outliers, and planted
    points with z == 0, x == z == 0 and denormal z (fp32 x / z is not finite there: they contribute nothing)"""
    g = np.random.Generator(np.random.PCG64(seed * 11 + H * W))
    loc, pps = [], []
    for v in range(V):
        f = max(H, W) * (0.6 + 0.5 * g.random())
        pp = np.array([W / 2 + g.uniform(-2, 2), H / 2 + g.uniform(-2, 2)]).astype(F32)
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        z = 1.5 + 2.0 * g.random((H, W))
        px, py = xs - pp[0] + 0.3 * g.standard_normal((H, W)), ys - pp[1] + 0.3 * g.standard_normal((H, W))
        p = np.stack([px / f * z, py / f * z, z], -1).reshape(-1, 3)
        out = g.random(H * W) < 0.1
        p[out, :2] *= g.uniform(1.5, 4.0, (int(out.sum()), 1))
        n = H * W
        p[n // 2] = [0.3, -0.2, 0.0]
        p[n // 3] = [0.0, 0.4, 0.0]
        p[n // 5] = [1.0, 1.0, 1e-40]
        loc.append(p.astype(F32)); pps.append(pp)
    return torch.from_numpy(np.stack(loc)), torch.from_numpy(np.stack(pps))


def _focal_terms(loc_v, pp_v, H, W):
    """float64 u, w, qx, qy of one view with the kernel's nan_to_num rule (decided by the fp32 quotient)"""
    p = loc_v.double()
    with np.errstate(all='ignore'):
        u, w = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    fin = lambda t: torch.where(t.float().abs() <= 3.4e38, t, torch.zeros_like(t))        # NaN compares false
    u, w = fin(u), fin(w)
    i = torch.arange(H * W)
    return u, w, (i % W).double() - float(pp_v[0]), (i // W).double() - float(pp_v[1])


def _focal_step(f, u, w, qx, qy, variant=None):
    if f is None:
        wt = torch.ones_like(u)
    else:
        d2 = (qx - f * u) ** 2 + (qy - f * w) ** 2
        wt = 1.0 / d2.clamp_min(1e-8) if variant == 'weights_sq' else 1.0 / d2.sqrt().clamp_min(1e-8)
    return float((wt * (u * qx + w * qy)).sum() / (wt * (u * u + w * w)).sum())


def _focal_step_bound(f, u, w, qx, qy):
    """fp32 error of one step f' = a / b, every term in fp32 and the sums in double: u, w, qx, qy carry one rounding each; the residual dx = qx - f u two more,
    relative to |qx| + |f u| (cancellation: the weight 1 / d inherits (|dx| ddx + |dy| ddy) / d^2 plus the roundings of the squares, the root and the
    reciprocal); the products wt (u qx + w qy) and wt (u^2 + w^2) four roundings each; one rounding of f'."""
    Ru = EB.R * EB.U32
    ta, tb = u * qx + w * qy, u * u + w * w
    dta, dtb = 4 * Ru * ((u * qx).abs() + (w * qy).abs()), 4 * Ru * tb
    if f is None:
        wt, rel = torch.ones_like(u), torch.zeros_like(u)
    else:
        dx, dy = qx - f * u, qy - f * w
        d = (dx * dx + dy * dy).sqrt().clamp_min(1e-8)
        ddx, ddy = Ru * (qx.abs() + 3 * (f * u).abs()), Ru * (qy.abs() + 3 * (f * w).abs())
        rel = (dx.abs() * ddx + dy.abs() * ddy) / (d * d) + 4 * Ru
        wt = 1.0 / d
    a, b = float((wt * ta).sum()), float((wt * tb).sum())
    fn = a / b
    # first order: d f' = sum_i (d(wt_i ta_i) - f' d(wt_i tb_i)) / b; a weight's error multiplies ta_i - f' tb_i, which is small where the weight is large.
    # The roundings of different pixels are independent: the 5-sigma envelope of their sum (errbound.LAMBDA, as for attention's P rounding) where it is
    # smaller than the worst case, which would hide a wrong weight rule under sqrt(P) times the real error.
    e = wt * (dta + abs(fn) * dtb) + wt * (rel + Ru) * (ta - fn * tb).abs()
    return float(min(e.sum(), EB.LAMBDA * (e * e).sum().sqrt())) / abs(b) + Ru * abs(fn)


def ref_focal(loc, pp, H, W, iters, variant=None):
    """float64 Weiszfeld iteration per view and its bound: B_0 = the one-step bound of the closed-form start; B_{k+1} = L_k B_k + (one-step bound at f_k), L_k
    the Lipschitz factor of the float64 step at f_k by a central finite difference of width max(B_k, 1e-6 |f_k|).  Returns f [V], bound [V], max L."""
    fs, bs, Lmax = [], [], 0.0
    for v in range(loc.shape[0]):
        t = _focal_terms(loc[v], pp[v], H, W)
        f, B = _focal_step(None, *t), _focal_step_bound(None, *t)
        for _ in range(iters):
            h = max(B, 1e-6 * abs(f))
            L = abs(_focal_step(f + h, *t) - _focal_step(f - h, *t)) / (2 * h)
            Lmax = max(Lmax, L)
            B = L * B + _focal_step_bound(f, *t)
            f = _focal_step(f, *t, variant=variant)
        fs.append(f); bs.append(B)
    return torch.tensor(fs, dtype=torch.float64), torch.tensor(bs, dtype=torch.float64), Lmax


def emulate_focal(loc, pp, H, W, iters, variant=None):
    """fp32 terms, float64 sums, f rounded to fp32 after every step"""
    out = []
    for v in range(loc.shape[0]):
        p = loc[v].numpy()
        with np.errstate(all='ignore'):
            u, w = (p[:, 0] / p[:, 2]).astype(F32), (p[:, 1] / p[:, 2]).astype(F32)
            u, w = np.where(np.abs(u) <= F32(3.4e38), u, F32(0)), np.where(np.abs(w) <= F32(3.4e38), w, F32(0))
        i = np.arange(H * W)
        qx, qy = (i % W).astype(F32) - pp[v, 0].numpy(), (i // W).astype(F32) - pp[v, 1].numpy()
        ta, tb = (u * qx + w * qy).astype(F32), (u * u + w * w).astype(F32)
        f = F32(ta.astype(np.float64).sum() / tb.astype(np.float64).sum())
        for _ in range(iters):
            dx, dy = qx - f * u, qy - f * w
            d2 = (dx * dx + dy * dy).astype(F32)
            wt = (F32(1) / np.maximum(d2, F32(1e-8))) if variant == 'weights_sq' else (F32(1) / np.maximum(np.sqrt(d2), F32(1e-8)))
            f = F32((wt * ta).astype(np.float64).sum() / (wt * tb).astype(np.float64).sum())
        out.append(f)
    return np.array(out, F32)


MOMENT_P = [1, 35, 1024, 1025, 384 * 512]
MOMENT_V = [1, 50]


def moments_case(V, P, seed):
    """points of mixed sign, confidences in [0.2, 6): conf - 1 changes sign"""
    g = np.random.Generator(np.random.PCG64(seed * 13 + V * 7 + P))
    x, y = g.standard_normal((V, P, 3)).astype(F32) * 2, g.standard_normal((V, P, 3)).astype(F32) * 3 + 1
    return torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy((0.2 + 5.8 * g.random((V, P))).astype(F32))


def ref_moments(x, y, conf, off, variant=None):
    """the 16 moments [V, 16] in float64 numpy (sum w, sum w x, sum w y, sum w y x^T row-major [y][x]) and their bound; variant 'transposed': x y^T"""
    X, Y, w = x.double().numpy(), y.double().numpy(), conf.double().numpy() + float(off)
    V, P = w.shape
    yx = np.einsum('vp,vpr,vpc->vrc', w, X, Y) if variant == 'transposed' else np.einsum('vp,vpr,vpc->vrc', w, Y, X)
    ref = np.concatenate([w.sum(1)[:, None], np.einsum('vp,vpk->vk', w, X), np.einsum('vp,vpk->vk', w, Y), yx.reshape(V, 9)], 1)
    def absmom(a):
        return np.concatenate([a.sum(1)[:, None], np.einsum('vp,vpk->vk', a, np.abs(X)), np.einsum('vp,vpk->vk', a, np.abs(Y)),
                               np.einsum('vp,vpr,vpc->vrc', a, np.abs(Y), np.abs(X)).reshape(V, 9)], 1)
    # what the fp32 addition conf + off really loses, element by element (nothing with off = 0, nothing where Sterbenz applies)
    dw = np.abs((conf.numpy() + F32(off)).astype(F32).astype(np.float64) - w)
    bound = EB.moments_bound(torch.from_numpy(absmom(np.abs(w))), -(-P // 1024) + 6 + 16, torch.from_numpy(absmom(dw)))
    return torch.from_numpy(ref), bound


def emulate_moments(x, y, conf, off, variant=None):
    """fp32 w, double products and sums; variant 'transposed': x y^T; 'fp32_acc': products and sums in fp32"""
    acc = F32 if variant == 'fp32_acc' else np.float64
    w = (conf.numpy() + F32(off)).astype(F32).astype(acc)
    X, Y = x.numpy().astype(acc), y.numpy().astype(acc)
    V = w.shape[0]
    yx = np.einsum('vp,vpr,vpc->vrc', w, X, Y) if variant == 'transposed' else np.einsum('vp,vpr,vpc->vrc', w, Y, X)
    return np.concatenate([w.sum(1)[:, None], np.einsum('vp,vpk->vk', w, X), np.einsum('vp,vpk->vk', w, Y), yx.reshape(V, 9)], 1)
