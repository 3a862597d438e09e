"""Stage-level parity of csrc/depth_eval.hip (sum, reduce, histogram, narrow) and csrc/evaluate.hip (count, areas, match, state): the wrappers
`hip.depth_table`, `hip.depth_median`, `hip.depth_moments`, `hip.depth_errors`, `hip.depth_workspace`, `hip.pq_count` (merge 0 and 1) and
`hip.pq_match` called by hand on the hand-written cases of tests/score_stage_cases.py and compared with its restatements BYTE FOR BYTE: integer
arithmetic, exact order statistics and fp64 sums in a fixed order leave no tolerance to choose.  tests/test_score_stage_checks.py asserts without a
GPU that every case holds what it was built for and which case catches which planted mistake; test_hip_depth_eval.py and test_hip_eval.py hold the
same kernels end to end through `depth_quality` and `panoptic_quality`.

  median    count, median after ONE call over all slabs of a case (ranks that part at every byte level, every pass-0 bin position of lanes 0 and 31,
            denormals and FLT_MAX, heavy ties, an all-invalid slab between valid ones, invalid pixels whose bits would move a median); the hist /
            prefix / rank workspace is all zero afterwards, and a second call on the SAME workspace gives the same bytes.
  reducer   partials and out of depth_moments and depth_errors for one slab of 255, 256, 257 and 513 one-pixel views followed by a one-view slab
            (the stride of the reducer, the end of a row range before nblocks, the binary search over a table of 514 views), and the medians of
            the same table.
  match     pred_area, gt_area, match, iou, pred_state of hand-made counts tables: 2 inter == union and union + 1, the void column that flips the
            decision, category and absence exclusions, areas that add to more than 2^31, 2 void == area and area + 1, and the launch edges of the
            four kernels (G + 1 = 1 .. 129, S P = 1 .. 257, S G = 255 .. 257, an empty side).
  count     counts of pixel streams under merge 0 and merge 1: N = 1 .. 1027, empty slabs and three boundaries inside one lane, the run heads
            (lane 0, lane 63, a run cut by one non-uniform lane, by a slab boundary, by N), ids at the edges of both tables.
Outputs sit in canary-padded allocations and start as canaries; read-only operands keep their bytes.  Every case is a valid call."""
import numpy as np
import pytest
import torch

import geom_stage_cases as G
import score_stage_cases as C
from test_hip_tsdf_stages import CANARY, DEV, Padded, dev, padded_of

pytestmark = pytest.mark.gpu
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
INF = float('inf')
MEDIAN, MATCH, COUNT = C.median_cases(), C.match_cases(), C.count_cases()


def _hip():
    from panst3r_amd import hip
    hip.lib()
    return hip


def same(got, ref, dtype, what):
    """equal BYTES - the median of an empty slab is the NaN 0x7fc00000 and no other"""
    got, ref = got.cpu().numpy(), np.ascontiguousarray(np.asarray(ref).astype(dtype, copy=False))
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert got.tobytes() == ref.tobytes(), '%s: %s' % (what, G.first_difference(got, ref))


def table_of(hip, case):
    """the DepthTable of a case and the device tensors it points into (whose bytes a call must leave alone)"""
    planes = [(dev(p, F32), dev(g, F32)) for views in case for p, g in views]
    slabs = [s for s, views in enumerate(case) for _ in views]
    return hip.depth_table([(p, 1, g, None) for p, g in planes], slabs, DEV), planes


def unchanged(planes, case):
    flat = [v for views in case for v in views]
    return all(p.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes() and g.cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes()
               for (p, g), (a, b) in zip(planes, flat))


def check_median(hip, case, table, what):
    S = len(case)
    want_n, want_m = C.median_ref(case)
    ws = hip.depth_median_workspace(table, DEV)
    first = None
    for again in (0, 1):                                                        # the second call runs on the workspace the first one left
        count, median = Padded((S,), I32), Padded((S, 2), F32)
        hip.depth_median(table, 0.0, INF, 0.0, count.t, median.t, ws=ws)
        torch.cuda.synchronize()
        same(count.t, want_n, np.int32, '%s: count (call %d)' % (what, again))
        same(median.t, want_m, np.float32, '%s: median (call %d)' % (what, again))
        assert count.intact() and median.intact() and bool((ws == 0).all()), (what, again)
        got = (count.t.cpu().numpy().tobytes(), median.t.cpu().numpy().tobytes())
        first = first or got
        assert got == first


# ============================================================================================================================================ median
@pytest.mark.parametrize('name', sorted(MEDIAN))
def test_median(name):
    hip, case = _hip(), MEDIAN[name]
    table, planes = table_of(hip, case)
    assert table.nslabs == len(case) and table.nviews == sum(len(v) for v in case)
    check_median(hip, case, table, name)
    assert unchanged(planes, case)


def test_median_under_bounds_that_cut_the_middle_pair_away():
    """the divergence slabs under a min_depth and a max_depth that are values of gt itself: equality is outside below and inside above, validity is
    decided on gt and the medians of BOTH quantities move"""
    hip, case = _hip(), MEDIAN['diverge']
    table, _ = table_of(hip, case)
    lo, hi = float(C.f32([0x3e9910ff])[0]), float(C.f32([0x41800000])[0])     # gt's lower middle value of slab 1 (g > lo), its upper one of slab 2 (g <= hi)
    want_n, want_m = C.median_ref(case, lo, hi)
    assert want_n.tolist() == [0, 7, 8, 14] and C.median_ref(case)[0].tolist() == [14] * 4
    count, median = Padded((len(case),), I32), Padded((len(case), 2), F32)
    hip.depth_median(table, lo, hi, 0.0, count.t, median.t)
    torch.cuda.synchronize()
    same(count.t, want_n, np.int32, 'count')
    same(median.t, want_m, np.float32, 'median')


# ============================================================================================================================================ reducer
@pytest.mark.parametrize('R', (255, 256, 257, 513))
def test_reducer_and_view_lookup(R):
    hip, case = _hip(), C.reducer_case(R)
    table, planes = table_of(hip, case)
    assert (table.nviews, table.nblocks, table.nslabs) == (R + 1, R + 1, 2) and table.slab_rows.tolist() == [0, R, R + 1]
    align = dev(np.array(C.ALIGN, dtype=np.float64))
    for what, ref, run in (('moments', C.moments_ref(case), lambda ws: hip.depth_moments(table, 0.0, INF, 0.0, ws)),
                           ('errors', C.errors_ref(case), lambda ws: hip.depth_errors(table, 0.0, INF, 0.0, align, C.THRESHOLDS, ws))):
        first = None
        for again in (0, 1):
            partials, out = Padded((table.nblocks, hip.DEPTH_MOMENTS), F64), Padded((table.nslabs, hip.DEPTH_MOMENTS), F64)
            assert set(hip.depth_workspace(table, DEV)) == {'partials', 'out'} and hip.depth_workspace(table, DEV)['partials'].shape == partials.t.shape
            run({'partials': partials.t, 'out': out.t})
            torch.cuda.synchronize()
            same(partials.t, ref[0], np.float64, '%s: partials of %d rows' % (what, R))
            same(out.t, ref[1], np.float64, '%s: out of %d rows' % (what, R))
            assert partials.intact() and out.intact()
            got = (partials.t.cpu().numpy().tobytes(), out.t.cpu().numpy().tobytes())
            first = first or got
            assert got == first
    check_median(hip, case, table, 'median of %d views' % R)
    assert unchanged(planes, case) and align.cpu().numpy().tolist() == [list(a) for a in C.ALIGN]


# ============================================================================================================================================ match / state
@pytest.mark.parametrize('name', sorted(MATCH))
def test_match_and_state(name):
    hip, case = _hip(), MATCH[name]
    counts, cat_p, cat_g = case['counts'], np.asarray(case['cat_p'], dtype=np.int32), np.asarray(case['cat_g'], dtype=np.int32)
    S, P, G = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    want = C.v_match(counts, cat_p, cat_g)
    for (s, p), v in case['states'].items():
        assert want['pred_state'][s, p] == v
    c, cp, cg = padded_of(counts, I32), dev(cat_p.reshape(P), I32), dev(cat_g.reshape(G), I32)
    first = None
    for again in (0, 1):
        out = {'pred_area': Padded((S, P), I32), 'gt_area': Padded((S, G), I32), 'match': Padded((S, G), I32), 'iou': Padded((S, G), F64),
               'pred_state': Padded((S, P), I32)}
        hip.pq_match(c.t, cp, cg, out['pred_area'].t, out['gt_area'].t, out['match'].t, out['iou'].t, out['pred_state'].t)
        torch.cuda.synchronize()
        for k, o in out.items():
            same(o.t, want[k], want[k].dtype, '%s: %s' % (name, k))
            assert o.intact(), (name, k)                                        # (an empty side: zero elements between two untouched pads)
        assert c.intact() and c.t.cpu().numpy().tobytes() == counts.tobytes()
        got = [o.t.cpu().numpy().tobytes() for o in out.values()]
        first = first or got
        assert got == first


# ============================================================================================================================================ count
@pytest.mark.parametrize('name', sorted(COUNT))
def test_count(name):
    hip, case = _hip(), COUNT[name]
    P, G, S = case['P'], case['G'], len(case['slab_off']) - 1
    want = C.count_ref(case)
    assert want.sum() == len(case['pred'])
    pred, gt, off = dev(case['pred'], I32), dev(case['gt'], I32), dev(case['slab_off'], I64)
    tp, tg = dev(case['tab_p'], I32), dev(case['tab_g'], I32)
    assert pred.data_ptr() % 16 == 0 and gt.data_ptr() % 16 == 0
    for merge in (0, 1, 1, 0):
        counts = padded_of(np.zeros((S, P + 1, G + 1), dtype=np.int32), I32)
        hip.pq_count(pred, gt, off, tp, tg, P, G, counts.t, merge=merge)
        torch.cuda.synchronize()
        same(counts.t, want, np.int32, '%s: counts, merge %d' % (name, merge))
        assert counts.intact(), (name, merge)
    assert pred.cpu().numpy().tobytes() == case['pred'].tobytes() and gt.cpu().numpy().tobytes() == case['gt'].tobytes()
    # counts ADD to what the caller left: a second call on the same table doubles it
    counts = padded_of(want, I32)
    hip.pq_count(pred, gt, off, tp, tg, P, G, counts.t, merge=1)
    torch.cuda.synchronize()
    same(counts.t, 2 * want, np.int32, '%s: counts on top of counts' % name)


def test_count_feeds_match():
    """the chain of engine/evaluate.py on the slab stream: count, then areas, match and state of THAT table, empty slabs included"""
    hip, case = _hip(), COUNT['slabs_uniform']
    P, G, S = case['P'], case['G'], len(case['slab_off']) - 1
    cat_p, cat_g = np.array([0, 1, 0], dtype=np.int32), np.array([0, 1, 0, 1], dtype=np.int32)
    want = C.v_match(C.count_ref(case), cat_p, cat_g)
    assert (want['match'] >= 0).any() and (want['gt_area'].sum(axis=1) == 0).any()
    counts = padded_of(np.zeros((S, P + 1, G + 1), dtype=np.int32), I32)
    hip.pq_count(dev(case['pred'], I32), dev(case['gt'], I32), dev(case['slab_off'], I64), dev(case['tab_p'], I32), dev(case['tab_g'], I32), P, G, counts.t)
    out = {'pred_area': Padded((S, P), I32), 'gt_area': Padded((S, G), I32), 'match': Padded((S, G), I32), 'iou': Padded((S, G), F64),
           'pred_state': Padded((S, P), I32)}
    hip.pq_match(counts.t, dev(cat_p), dev(cat_g), out['pred_area'].t, out['gt_area'].t, out['match'].t, out['iou'].t, out['pred_state'].t)
    torch.cuda.synchronize()
    for k, o in out.items():
        same(o.t, want[k], want[k].dtype, k)
        assert o.intact()
    assert CANARY == 0xA5
