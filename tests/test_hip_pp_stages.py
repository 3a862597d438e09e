"""Stage-level parity of csrc/postprocess.hip: every wrapper of panst3r_amd.hip called directly and compared with a float64 reference of the same stage
(tests/pp_stage_cases.py), so that a mistake is localised to a stage instead of hiding in the end-to-end pixel allowance of test_hip_postprocess.py.

No pixel allowance here.  Every comparison of the reference that clears its threshold / runner-up by more than the derived fp32 error bound (errbound
sigmoid_bound, blend_bound, product_bound, softmax_score_bound, chunked_sum_bound) is DECIDED and must be reproduced exactly: best_q equal and best_m within
its bound on every decided pixel, the counters inside the integer interval the decided pixels give, keep / labels / seg_id / pan equal.  How much may be
undecided is a condition of the case (at most 0.1 % of the pixels for the winner, at most 8 pixels per query in the 0.5 band), asserted on the reference
before the GPU result is looked at; tests/test_pp_stage_checks.py asserts the same caps without a GPU and proves that the checkers catch planted mistakes.

Every stage runs twice and must give the same bits (the file header of postprocess.hip promises determinism, integer atomics included), runs once more
through torch.ops.panst3r_hip where the stage has an op (a swapped argument in ops.py shows), and writes into canary-filled buffers larger than its output.

pp_sigmoid + pp_argmax and pp_argmax_logits must agree in every bit of all four outputs wherever both apply, and do: both kernels take the source
coordinate and the blend from one __device__ function each (pp_src, pp_blend), so the compiler cannot contract them differently.  Separately from path
identity, agreement with the REFERENCE needed a kernel change: the coordinate scale * (dst + 0.5) - 0.5 used to be contracted into one fma, which is not the
fp32 expression of the operation and moves a tap weight by up to 2e-6 at the non-dyadic ratios; the 'fma' variant of the CPU emulation fails check_best on the
40 x 56 -> 75 x 93 case.

Measured on the MI355X (profiles/output_kernel_margins.jsonl; PST_STAGE_LOG=<path> makes a run append its rows), largest observed error / derived bound:
pp_sigmoid 0.49, pp_scores 0.37, pp_scores_softmax 0.14, best_m of pp_argmax / pp_argmax_logits 0.28, qubo_upsample 0.31, qubo_overlap 0.03; every integer
output exact.  Undecided winners: 5.1e-6 of the pixels at 200 x (192 x 256 -> 384 x 512), none at the other shapes.  The two paths agreed in every bit at
every shape and keep pattern.  The 123 tests of this module take 27 s, 19 s of them the float64 reference of
qubo_overlap at 200 queries x 384 x 512 pixels.
"""
import json
import os

import numpy as np
import pytest
import torch

import errbound as EB
import pp_stage_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY_I, CANARY_F = -12345, -777.0


def _log(**kw):
    if os.environ.get('PST_STAGE_LOG'):
        with open(os.environ['PST_STAGE_LOG'], 'a') as f:
            f.write(json.dumps(kw) + '\n')


def _hip():
    from panst3r_amd import hip
    import panst3r_amd.ops                  # noqa: F401  (registers torch.ops.panst3r_hip)
    return hip


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t.to(dtype) if dtype is not None else t).to(DEV).contiguous()


class Padded:
    """an output of n elements inside a canary-filled buffer: nothing outside changes, everything inside does"""

    def __init__(self, n, dtype, pad=256):               # a multiple of 4 elements: the output keeps the 16-byte alignment the engine's buffers have
        self.n, self.pad = n, pad
        self.canary = CANARY_I if dtype == torch.int32 else CANARY_F
        self.buf = torch.full((n + 2 * pad,), self.canary, dtype=dtype, device=DEV)
        self.view = self.buf[pad:pad + n]

    def check(self, what, all_written=True):
        b = self.buf.cpu()
        assert bool((b[:self.pad] == self.canary).all()) and bool((b[self.pad + self.n:] == self.canary).all()), what + ': wrote outside its output'
        if all_written:
            assert not bool((b[self.pad:self.pad + self.n] == self.canary).any()), what + ': left part of its output unwritten'
        return b[self.pad:self.pad + self.n].clone()


# ------------------------------------------------------------------------------------------------------------------------------------------- scores
def _run_scores(hip, x, mode, thr, temp, via_ops=False):
    Q = x.shape[0]
    sc, lb, kp = Padded(Q, torch.float32), Padded(Q, torch.int32), Padded(Q, torch.int32)
    if mode == 'softmax':                                       # no torch op for this one: the engine calls the wrapper
        hip.pp_scores_softmax(x, thr, sc.view, lb.view, kp.view)
    elif via_ops:
        torch.ops.panst3r_hip.pp_scores(x, thr, float(temp or 0.0), sc.view, lb.view, kp.view)
    else:
        hip.pp_scores(x, thr, temp, sc.view, lb.view, kp.view)
    torch.cuda.synchronize()
    return sc.check('scores').numpy(), lb.check('labels').numpy(), kp.check('keep').numpy()


@pytest.mark.parametrize('ncls', [1] + C.SCORE_NCLS)
@pytest.mark.parametrize('Q', C.SCORE_Q)
def test_pp_scores(Q, ncls):
    """pp_scores (temperature None, 0.1, 1) and pp_scores_softmax (Ncls >= 2): planted equal maxima in different lanes and in different strides of one lane give
    the lowest column; the threshold 0.5 sits exactly on row 0's score sigmoid(0) (strict >: not kept)"""
    hip = _hip()
    x = C.scores_case(Q, ncls, 0)
    xd = _dev(x)
    for temp in (None, 0.1, 1.0):
        got = _run_scores(hip, xd, 'sigmoid', 0.5, temp)
        r, nexact = C.check_scores(x, 'sigmoid', 0.5, temp, *got, 'pp_scores Q=%d Ncls=%d T=%s' % (Q, ncls, temp))
        assert got[2][0] == 0 and (temp is not None or got[0][0] == 0.5)
        for again in (_run_scores(hip, xd, 'sigmoid', 0.5, temp), _run_scores(hip, xd, 'sigmoid', 0.5, temp, via_ops=True)):
            assert all(np.array_equal(a, b) for a, b in zip(got, again))
        _log(stage='pp_scores', Q=Q, ncls=ncls, temperature=temp, ratio=r)
    if ncls >= 2:
        got = _run_scores(hip, xd, 'softmax', 0.3, None)
        r, _ = C.check_scores(x, 'softmax', 0.3, None, *got, 'pp_scores_softmax Q=%d Ncls=%d' % (Q, ncls))
        assert all(np.array_equal(a, b) for a, b in zip(got, _run_scores(hip, xd, 'softmax', 0.3, None)))
        _log(stage='pp_scores_softmax', Q=Q, ncls=ncls, ratio=r)
    if ncls == 2:                                              # softmax of two equal logits is exactly 0.5: on the threshold, not kept; label 0
        got = _run_scores(hip, _dev(torch.full((Q, 2), 1.25)), 'softmax', 0.5, None)
        assert (got[0] == 0.5).all() and (got[1] == 0).all() and (got[2] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------------- sigmoid
@pytest.mark.parametrize('P', [4, 7, 1024, 1027, 64 * 256 * 4, 3 * 64 * 256 * 4 + 4, 3 * 64 * 256 * 4 + 5])
def test_pp_sigmoid(P):
    """P % 4 == 0 (float4 path) and != 0; below and far above one grid pass (64 blocks x 256 threads x 4); keep == 0 rows keep the canary"""
    hip = _hip()
    Q = 5
    g = np.random.Generator(np.random.PCG64(P))
    x = torch.from_numpy((g.standard_normal((Q, P)) * 6).astype(np.float32))
    x[0, :4] = torch.tensor([-104.0, -88.0, 0.0, 89.0])
    keep = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    outs = []
    for via_ops in (False, False, True):
        out = Padded(Q * P, torch.float32)
        (torch.ops.panst3r_hip.pp_sigmoid if via_ops else hip.pp_sigmoid)(_dev(x), _dev(keep), out.view, Q, P)
        torch.cuda.synchronize()
        outs.append(out.check('pp_sigmoid', all_written=False).view(Q, P))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    k = keep.bool()
    assert bool((outs[0][~k] == CANARY_F).all()), 'rows with keep == 0 were touched'
    s = x[k].double().sigmoid()
    r = EB.check(outs[0][k], s, EB.sigmoid_bound(s), 'pp_sigmoid P=%d' % P)
    _log(stage='pp_sigmoid', P=P, ratio=r)


# ------------------------------------------------------------------------------------------------------------------------------------------- argmax
def _run_argmax(hip, path, logits_d, scores_d, keep, shape, orig0=None, mask0=None, via_ops=False, cnt=None):
    """one view through 'fused' (pp_argmax_logits) or 'split' (pp_sigmoid + pp_argmax); returns numpy best_q, best_m, cnt_orig, cnt_mask (cumulative)"""
    Q, Hm, Wm, H, W = shape
    kd = _dev(keep, torch.int32)
    bq, bm = Padded(H * W, torch.int32), Padded(H * W, torch.float32)
    if cnt is None:
        cnt = (Padded(Q, torch.int32), Padded(Q, torch.int32))
        cnt[0].view.copy_(_dev(np.zeros(Q) if orig0 is None else orig0, torch.int32))
        cnt[1].view.copy_(_dev(np.zeros(Q) if mask0 is None else mask0, torch.int32))
    ns = torch.ops.panst3r_hip if via_ops else hip
    if path == 'fused':
        ns.pp_argmax_logits(logits_d, scores_d, kd, Q, Hm, Wm, H, W, C.MASK_THR, bq.view, bm.view, cnt[0].view, cnt[1].view)
    else:
        probs = torch.full((Q, Hm * Wm), CANARY_F, device=DEV)
        ns.pp_sigmoid(logits_d.view(Q, -1), kd, probs, Q, Hm * Wm)
        ns.pp_argmax(probs, scores_d, kd, Q, Hm, Wm, H, W, C.MASK_THR, bq.view, bm.view, cnt[0].view, cnt[1].view)
    torch.cuda.synchronize()
    return (bq.check(path + ' best_q').numpy(), bm.check(path + ' best_m').numpy(), cnt[0].check(path + ' cnt_orig').numpy(), cnt[1].check(path + ' cnt_mask').numpy()), cnt


@pytest.mark.parametrize('shape', C.ARGMAX_SHAPES, ids=C.shape_id)
def test_pp_argmax_stages(shape):
    """pp_argmax and pp_argmax_logits, every keep pattern, against the float64 reference; same bits from both paths, from a second run and through torch.ops;
    counters start non-zero and come out as start + this view"""
    hip = _hip()
    Q, Hm, Wm, H, W = shape
    assert hip.pp_fused_fits(Q, Hm, Wm, H, W)
    logits, scores = C.make_case(shape)
    ld, sd = _dev(logits), _dev(scores)
    CH = C.fused_geometry(Hm, Wm, H, W)[2]
    g = np.random.Generator(np.random.PCG64(11))
    o0, m0 = g.integers(1, 1000, Q), g.integers(1, 1000, Q)
    worst = und = 0.0
    for name, keep in C.keep_patterns(Q, CH).items():
        what = '%s %s' % (C.shape_id(shape), name)
        r = C.ref_argmax(logits, scores, keep, H, W)
        C.assert_caps(r, what)                                  # before the GPU result is looked at
        fused, _ = _run_argmax(hip, 'fused', ld, sd, keep, shape, o0, m0)
        split, _ = _run_argmax(hip, 'split', ld, sd, keep, shape, o0, m0)
        for path, got in (('pp_argmax_logits', fused), ('pp_sigmoid + pp_argmax', split)):
            worst = max(worst, C.check_best(r, got[0], got[1], what + ' ' + path))
            C.check_counts([r], got[2], got[3], o0, m0, what + ' ' + path)
        for k, a, b in zip(('best_q', 'best_m', 'cnt_orig', 'cnt_mask'), fused, split):
            assert np.array_equal(a, b), '%s: %s differs between pp_argmax_logits and pp_sigmoid + pp_argmax' % (what, k)
        if name == 'none':
            assert (fused[0] == -1).all() and (fused[1] == 0).all() and np.array_equal(fused[2], o0) and np.array_equal(fused[3], m0)
        if name in ('all', 'nk%d' % (CH + 1)):
            for path in ('fused', 'split'):
                again, _ = _run_argmax(hip, path, ld, sd, keep, shape, o0, m0)
                ops, _ = _run_argmax(hip, path, ld, sd, keep, shape, o0, m0, via_ops=True)
                assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(fused, again, ops)), what + ': second run / torch.ops differ'
        und = max(und, r.undecided_share)
    _log(stage='pp_argmax', shape=C.shape_id(shape), ratio_best_m=worst, undecided_share_max=und)


@pytest.mark.parametrize('shape', [C.ARGMAX_SHAPES[0], C.ARGMAX_SHAPES[1]], ids=C.shape_id)
def test_pp_argmax_two_views_accumulate(shape):
    """two views into the same non-zero counters: the result is start + view 1 + view 2, for both paths"""
    hip = _hip()
    Q, Hm, Wm, H, W = shape
    keep = np.ones(Q, np.int32)
    g = np.random.Generator(np.random.PCG64(5))
    o0, m0 = g.integers(1, 1000, Q), g.integers(1, 1000, Q)
    views = [C.make_case(shape, s) for s in (0, 1)]
    refs = [C.ref_argmax(lg, sc, keep, H, W) for lg, sc in views]
    for r in refs:
        C.assert_caps(r, C.shape_id(shape))
    res = {}
    for path in ('fused', 'split'):
        cnt = None
        for (lg, sc), r in zip(views, refs):
            got, cnt = _run_argmax(hip, path, _dev(lg), _dev(sc), keep, shape, o0, m0, cnt=cnt)
            C.check_best(r, got[0], got[1], path)
        C.check_counts(refs, got[2], got[3], o0, m0, path + ' two views')
        res[path] = got
    assert all(np.array_equal(a, b) for a, b in zip(res['fused'], res['split']))


@pytest.mark.parametrize('bump', [False, True])
@pytest.mark.parametrize('shape', [C.ARGMAX_SHAPES[3], C.ARGMAX_SHAPES[2]], ids=C.shape_id)
def test_pp_argmax_planted_ties(shape, bump):
    """two kept queries with identical planes: identical scores - the lower id owns every pixel either would own; the higher id one ulp larger - it owns them"""
    hip = _hip()
    Q, Hm, Wm, H, W = shape
    logits, scores, lo, hi = C.tie_case(shape, 0, bump)
    keep = np.ones(Q, np.int32)
    alone = keep.copy(); alone[hi] = 0
    for path in ('fused', 'split'):
        both, _ = _run_argmax(hip, path, _dev(logits), _dev(scores), keep, shape)
        ref_run, _ = _run_argmax(hip, path, _dev(logits), _dev(scores), alone, shape)
        C.check_tie(both, ref_run, lo, hi, bump, '%s %s' % (C.shape_id(shape), path))
        r = C.ref_argmax(logits, scores, alone, H, W)          # the run the twins are compared with is itself held to the float64 reference
        C.assert_caps(r, C.shape_id(shape) + ' without the twin')
        C.check_best(r, ref_run[0], ref_run[1], path + ' without the twin')
        C.check_counts([r], ref_run[2], ref_run[3], np.zeros(Q), np.zeros(Q), path + ' without the twin')
        assert (both[0] == (hi if bump else lo)).any()


def test_pp_argmax_down4_and_fused_refusal():
    """4 x down-sampling: pp_sigmoid + pp_argmax against the reference; pp_argmax_logits refuses the footprint with an argument error before any launch"""
    hip = _hip()
    shape = C.DOWN4_SHAPE
    Q, Hm, Wm, H, W = shape
    assert not hip.pp_fused_fits(Q, Hm, Wm, H, W)
    logits, scores = C.make_case(shape)
    keep = np.ones(Q, np.int32)
    r = C.ref_argmax(logits, scores, keep, H, W)
    C.assert_caps(r, C.shape_id(shape))
    got, _ = _run_argmax(hip, 'split', _dev(logits), _dev(scores), keep, shape)
    ratio = C.check_best(r, got[0], got[1], 'down4')
    C.check_counts([r], got[2], got[3], np.zeros(Q), np.zeros(Q), 'down4')
    bq, bm, co, cm = (Padded(H * W, torch.int32), Padded(H * W, torch.float32), Padded(Q, torch.int32), Padded(Q, torch.int32))
    with pytest.raises(RuntimeError, match='footprint'):
        hip.pp_argmax_logits(_dev(logits), _dev(scores), _dev(keep), Q, Hm, Wm, H, W, C.MASK_THR, bq.view, bm.view, co.view, cm.view)
    torch.cuda.synchronize()
    for p in (bq, bm, co, cm):
        p.check('refused call', all_written=False)
        assert bool((p.view == p.canary).all()), 'a refused call wrote its outputs'
    _log(stage='pp_argmax', shape=C.shape_id(shape), ratio_best_m=ratio, undecided_share_max=r.undecided_share)


# ------------------------------------------------------------------------------------------------------------------------------------------- select / finalize
@pytest.mark.parametrize('thr', [0.5, 0.8])
@pytest.mark.parametrize('Q', C.SELECT_Q)
def test_pp_select(Q, thr):
    """exact integer semantics (Python's int / int < thr in double), keep_out aliasing keep as the engine calls it, both counters zero afterwards, seg_id the
    running count in query order"""
    hip = _hip()
    keep, co, cm, plants = C.select_case(Q, thr, 0)
    res = []
    for via_ops in (False, False, True):
        kd, cod, cmd, seg = Padded(Q, torch.int32), Padded(Q, torch.int32), Padded(Q, torch.int32), Padded(Q, torch.int32)
        kd.view.copy_(_dev(keep)); cod.view.copy_(_dev(co)); cmd.view.copy_(_dev(cm))
        if via_ops:                                             # the op declares keep_out as written: a separate tensor there
            ko_t = Padded(Q, torch.int32)
            torch.ops.panst3r_hip.pp_select(kd.view, cod.view, cmd.view, Q, thr, ko_t.view, seg.view)
        else:
            ko_t = kd
            hip.pp_select(kd.view, cod.view, cmd.view, Q, thr, kd.view, seg.view)
        torch.cuda.synchronize()
        ko, sg = ko_t.check('keep_out').numpy(), seg.check('seg_id').numpy()
        assert not cod.check('cnt_orig').any() and not cmd.check('cnt_mask').any(), 'counters not re-armed'
        C.check_select(keep, co, cm, thr, ko, sg, 'pp_select Q=%d thr=%g' % (Q, thr))
        res.append((ko, sg))
    assert all(np.array_equal(res[0][i], res[j][i]) for i in (0, 1) for j in (1, 2))
    assert [int(v) for v in res[0][0][:len(plants)]] == [p[3] for p in plants]


@pytest.mark.parametrize('n', C.FINALIZE_N)
def test_pp_finalize(n):
    """exact: best_q == -1, best_m equal to the threshold and one ulp below it, winners whose seg_id is 0 get the void confidence"""
    hip = _hip()
    Q, thr, void = 40, 0.25, 0.1
    bq, bm, seg = C.finalize_case(n, Q, thr, 0)
    pan_r, conf_r = C.ref_finalize(bq, bm, seg, thr, void)
    for via_ops in (False, False, True):
        pan, conf = Padded(n, torch.int32), Padded(n, torch.float32)
        (torch.ops.panst3r_hip.pp_finalize if via_ops else hip.pp_finalize)(_dev(bq), _dev(bm), _dev(seg), n, thr, void, pan.view, conf.view)
        torch.cuda.synchronize()
        assert np.array_equal(pan.check('pan').numpy(), pan_r) and np.array_equal(conf.check('conf').numpy(), conf_r)


# ------------------------------------------------------------------------------------------------------------------------------------------- QUBO
@pytest.mark.parametrize('shape', [(200, 192, 256, 384, 512), (17, 25, 31, 75, 93), (1, 40, 56, 75, 93), (16, 96, 128, 64, 85), (15, 48, 64, 48, 64)], ids=C.shape_id)
def test_qubo_upsample(shape):
    """sigmoid + bilinear to the true shape against float64 m with the bound of the blended probability"""
    hip = _hip()
    Q, hm, wm, H, W = shape
    logits = C.blobs(3, Q, hm, wm)
    outs = []
    for via_ops in (False, False, True):
        out = Padded(Q * H * W, torch.float32)
        (torch.ops.panst3r_hip.qubo_upsample if via_ops else hip.qubo_upsample)(_dev(logits), out.view, Q, hm, wm, H, W)
        torch.cuda.synchronize()
        outs.append(out.check('qubo_upsample'))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    grid = C.Grid(hm, wm, H, W)
    worst = 0.0
    for q0 in range(0, Q, 8):
        m, dm = C.ref_m(logits[q0:q0 + 8], grid)
        worst = max(worst, EB.check(outs[0].view(Q, H * W)[q0:q0 + 8], m, dm, 'qubo_upsample %s' % C.shape_id(shape)))
    _log(stage='qubo_upsample', shape=C.shape_id(shape), ratio=worst)


@pytest.mark.parametrize('Q,P', [(q, p) for q in C.QUBO_Q for p in C.QUBO_P])
def test_qubo_overlap(Q, P):
    """W accumulated over two calls = twice the float64 sum within the chunked-sum bound; the diagonal is the sum of the probabilities; W equals its
    transpose bit for bit (min commutes and both triangles add the same partials in the same order)"""
    hip = _hip()
    probs = C.qubo_probs(Q, P, 0)
    S, bound = C.ref_overlap(probs)
    res = []
    for via_ops in (False, False, True):
        Wacc = torch.zeros(Q, Q, dtype=torch.float64, device=DEV)
        for _ in range(2):
            (torch.ops.panst3r_hip.qubo_overlap if via_ops else hip.qubo_overlap)(_dev(probs), Q, P, Wacc)
        torch.cuda.synchronize()
        res.append(Wacc.cpu())
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]) and torch.equal(res[0], res[0].T)
    r = EB.check(res[0], 2 * S, 2 * bound, 'qubo_overlap Q=%d P=%d' % (Q, P))
    EB.check(torch.diagonal(res[0]), 2 * probs.double().sum(1), 2 * EB.chunked_sum_bound(probs.double().sum(1), -(-P // 256)), 'qubo_overlap diagonal')
    _log(stage='qubo_overlap', Q=Q, P=P, ratio=r)


@pytest.mark.parametrize('Q', C.QUBO_Q)
@pytest.mark.parametrize('P', C.QUBO_P)
def test_qubo_argmax(Q, P):
    """sel of size 1, 2 and Q; planted equal probabilities: the first selected query wins; exact"""
    hip = _hip()
    probs = C.qubo_probs(Q, P, 1)
    probs[:, ::3] = probs[0, ::3].clone()                              # every query equal on a third of the pixels
    for sel in ([Q - 1], [0, Q - 1], list(range(Q))):
        sel = sorted(set(sel))
        conf_r, inst_r = C.ref_qubo_argmax(probs, sel)
        for via_ops in (False, False, True):
            conf, inst = Padded(P, torch.float32), Padded(P, torch.int32)
            (torch.ops.panst3r_hip.qubo_argmax if via_ops else hip.qubo_argmax)(_dev(probs), _dev(sel, torch.int32), P, conf.view, inst.view)
            torch.cuda.synchronize()
            assert torch.equal(conf.check('conf'), conf_r) and torch.equal(inst.check('inst'), inst_r), (Q, P, sel[:3])
