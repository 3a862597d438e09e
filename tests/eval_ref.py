"""numpy restatement of the panoptic evaluation (panst3r_amd/engine/evaluate.py, csrc/evaluate.hip), the yardstick the kernels are held to bit for bit,
and a seeded generator of predicted / ground-truth map pairs.

Own design (the reference has no such stage); the rules are those of COCO panopticapi's pq_compute_single_core without iscrowd.  The contract of
include/panst3r_hip.h, with P = len(segments_info), G = len(gt_segments), N = total pixels < 2^31, ids unique and > 0 within each list:
  1 rows      a predicted id i maps to row id2row_p[i] if 0 < i < ntab_p and that entry is >= 0, else to the void row P; ground truth likewise to a
              column, or the void column G.  Ids <= 0, ids beyond the table and ids not listed are all void.
  2 slabs     scope='scene': S = 1 slab with every pixel of every view; scope='view': S = V slabs, a pixel belongs to its view's slab.
  3 counts    counts int32 [S, P+1, G+1] = the number of pixels of slab s with (row p, column g).  Integer adds: independent of order.
  4 areas     pa[s,p] = sum_g counts[s,p,g] (void column included), ga[s,g] = sum_p counts[s,p,g] (void row included); area 0 = the segment does not
              exist in that slab.
  5 match     for every g with ga > 0 and every p with pa > 0 of the SAME category: inter = counts[s,p,g], union = pa + ga - inter - counts[s,p,G]
              (the predicted pixels on void ground truth leave the union); a match iff 2 inter > union in int64 - equality is no match.  At most one
              p matches a g and at most one g a p (asserted here).  match[s,g] int32 = the row or -1, iou[s,g] float64 = inter / union (one IEEE
              division) or 0.
  6 misses    FN: an existing g without a match.  An existing p without a match is ignored if 2 counts[s,p,G] > pa[s,p], otherwise an FP.
              pred_state[s,p] int32: 0 absent, 1 matched, 2 FP, 3 ignored.
  7 category  on the host in float64, slabs ascending, then gt rows ascending: tp, fp, fn, iou_sum; pq = iou_sum / (tp + 0.5 fp + 0.5 fn),
              sq = iou_sum / tp (0 if tp = 0), rq = tp / (tp + 0.5 fp + 0.5 fn); a category with tp + fp + fn = 0 is left out; PQ / SQ / RQ = the mean
              over the others in ascending category order (0 if there is none); with `things` the same means over things and over stuff.
  8 semantic  rows and columns merged by category (void stays void), summed over the slabs in integers: iou_c = inter_c / (pred_c + gt_c - inter_c -
              pred_c-on-void); miou = the mean over categories with gt_c > 0; pixel_acc = sum_c inter_c / (non-void gt pixels) (0 without any)."""
import numpy as np

ABSENT, MATCHED, FP, IGNORED = 0, 1, 2, 3


def id_table(segs):
    """(id2row int32 [max id + 1], categories int32 [len(segs)]) of a segment list"""
    ids = [int(s['id']) for s in segs]
    assert len(set(ids)) == len(ids) and all(i > 0 for i in ids)
    tab = np.full(max(ids + [0]) + 1, -1, dtype=np.int32)
    tab[ids] = np.arange(len(ids), dtype=np.int32)
    return tab, np.array([int(s['category_id']) for s in segs], dtype=np.int32)


def rows_of(flat, tab, n):
    """step 1: the row of every pixel, n = void"""
    flat = np.asarray(flat).reshape(-1).astype(np.int64)
    r = np.full(len(flat), n, dtype=np.int64)
    ok = (flat > 0) & (flat < len(tab))
    r[ok] = tab[flat[ok]]
    r[r < 0] = n
    return r


def tables(pred_maps, segments_info, gt_maps, gt_segments, scope='scene'):
    """steps 1 - 6 -> dict(counts, pred_area, gt_area, match, iou, pred_state)"""
    assert scope in ('scene', 'view') and len(pred_maps) == len(gt_maps) > 0
    assert all(np.asarray(a).shape == np.asarray(b).shape for a, b in zip(pred_maps, gt_maps))
    tp_, cat_p = id_table(segments_info)
    tg_, cat_g = id_table(gt_segments)
    P, G, V = len(cat_p), len(cat_g), len(pred_maps)
    S = 1 if scope == 'scene' else V
    pr = rows_of(np.concatenate([np.asarray(m).reshape(-1) for m in pred_maps]), tp_, P)
    gr = rows_of(np.concatenate([np.asarray(m).reshape(-1) for m in gt_maps]), tg_, G)
    assert len(pr) < 2 ** 31
    slab = np.zeros(len(pr), dtype=np.int64) if S == 1 else np.repeat(np.arange(V), [np.asarray(m).size for m in pred_maps])
    counts = np.bincount((slab * (P + 1) + pr) * (G + 1) + gr, minlength=S * (P + 1) * (G + 1)).reshape(S, P + 1, G + 1).astype(np.int64)
    pa, ga = counts[:, :P, :].sum(axis=2), counts[:, :, :G].sum(axis=1)
    match, iou, state = np.full((S, G), -1, dtype=np.int32), np.zeros((S, G), dtype=np.float64), np.zeros((S, P), dtype=np.int32)
    for s in range(S):
        for g in range(G):
            if ga[s, g] == 0:
                continue
            for p in np.nonzero((pa[s] > 0) & (cat_p == cat_g[g]))[0]:
                inter = int(counts[s, p, g])
                union = int(pa[s, p]) + int(ga[s, g]) - inter - int(counts[s, p, G])
                if 2 * inter > union:
                    assert match[s, g] < 0 and state[s, p] == ABSENT, 'segments of one map are disjoint: a second match cannot happen'
                    match[s, g], state[s, p] = p, MATCHED
                    iou[s, g] = np.float64(inter) / np.float64(union)
        for p in range(P):
            if pa[s, p] > 0 and state[s, p] == ABSENT:
                state[s, p] = IGNORED if 2 * int(counts[s, p, G]) > int(pa[s, p]) else FP
    return {'counts': counts.astype(np.int32), 'pred_area': pa.astype(np.int32), 'gt_area': ga.astype(np.int32), 'match': match, 'iou': iou,
            'pred_state': state}


def tables_of_counts(counts, cat_p, cat_g):
    """steps 4 - 6 over a GIVEN counts table [S, P+1, G+1] (hand-made ones included, whose cells need not come from any pair of maps) ->
    dict(pred_area, gt_area, match, iou, pred_state).  Python integers, so nothing wraps; the first matching row of a column is kept."""
    c = np.asarray(counts).astype(np.int64)
    S, P, G = c.shape[0], c.shape[1] - 1, c.shape[2] - 1
    cat_p, cat_g = np.asarray(cat_p, dtype=np.int64).reshape(-1), np.asarray(cat_g, dtype=np.int64).reshape(-1)
    pa, ga = c[:, :P, :].sum(axis=2), c[:, :, :G].sum(axis=1)
    match, iou, state = np.full((S, G), -1, dtype=np.int32), np.zeros((S, G), dtype=np.float64), np.zeros((S, P), dtype=np.int32)
    for s in range(S):
        for g in range(G):
            if ga[s, g] == 0:
                continue
            for p in np.nonzero((pa[s] > 0) & (cat_p == cat_g[g]))[0]:
                inter = int(c[s, p, g])
                union = int(pa[s, p]) + int(ga[s, g]) - inter - int(c[s, p, G])
                if 2 * inter > union and match[s, g] < 0:
                    match[s, g], state[s, p] = p, MATCHED
                    iou[s, g] = np.float64(inter) / np.float64(union)
        for p in range(P):
            if pa[s, p] > 0 and state[s, p] == ABSENT:
                state[s, p] = IGNORED if 2 * int(c[s, p, G]) > int(pa[s, p]) else FP
    return {'pred_area': pa.astype(np.int32), 'gt_area': ga.astype(np.int32), 'match': match, 'iou': iou, 'pred_state': state}


def _mean(xs):
    return sum(xs) / len(xs) if xs else 0.0


def summarize(tab, segments_info, gt_segments, things=None):
    """steps 7 and 8 from the tables -> the result dict of panoptic_quality"""
    counts, match, iou, state, ga = tab['counts'].astype(np.int64), tab['match'], tab['iou'], tab['pred_state'], tab['gt_area']
    S, P, G = counts.shape[0], counts.shape[1] - 1, counts.shape[2] - 1
    cat_p, cat_g = [int(s['category_id']) for s in segments_info], [int(s['category_id']) for s in gt_segments]
    cats = sorted(set(cat_p) | set(cat_g))
    per = {c: {'tp': 0, 'fp': 0, 'fn': 0, 'iou_sum': 0.0, 'pq': None, 'sq': None, 'rq': None, 'iou': None} for c in cats}
    matches, ignored = [], []
    for s in range(S):
        for g in range(G):
            if match[s, g] >= 0:
                d = per[cat_g[g]]
                d['tp'] += 1
                d['iou_sum'] += float(iou[s, g])
                matches.append((s, int(segments_info[match[s, g]]['id']), int(gt_segments[g]['id']), float(iou[s, g])))
            elif ga[s, g] > 0:
                per[cat_g[g]]['fn'] += 1
        for p in range(P):
            if state[s, p] == FP:
                per[cat_p[p]]['fp'] += 1
            elif state[s, p] == IGNORED:
                ignored.append((s, int(segments_info[p]['id'])))
    for c in cats:
        d = per[c]
        den = d['tp'] + 0.5 * d['fp'] + 0.5 * d['fn']
        if den > 0:
            d['pq'], d['sq'], d['rq'] = d['iou_sum'] / den, (d['iou_sum'] / d['tp'] if d['tp'] else 0.0), d['tp'] / den
    out = {}
    groups = {'': lambda c: True}
    if things is not None:
        th = {int(t) for t in things}
        groups['_things'], groups['_stuff'] = (lambda c: c in th), (lambda c: c not in th)
    for suffix in ('', '_things', '_stuff'):
        for k in ('pq', 'sq', 'rq'):
            out[k + suffix] = _mean([per[c][k] for c in cats if groups[suffix](c) and per[c]['pq'] is not None]) if suffix in groups else None
    # step 8
    K = len(cats)
    col = {c: i for i, c in enumerate(cats)}
    rp, rg = np.array([col[c] for c in cat_p] + [K], dtype=np.int64), np.array([col[c] for c in cat_g] + [K], dtype=np.int64)
    sem = np.zeros((K + 1, K + 1), dtype=np.int64)
    np.add.at(sem, (rp[:, None], rg[None, :]), counts.sum(axis=0))
    ious, right = [], 0
    for c in cats:
        i = col[c]
        inter, pred, gt, pvoid = int(sem[i, i]), int(sem[i, :].sum()), int(sem[:, i].sum()), int(sem[i, K])
        right += inter
        if gt > 0:
            per[c]['iou'] = inter / (pred + gt - inter - pvoid)
            ious.append(per[c]['iou'])
    n, void = int(counts.sum()), int(counts[:, :, G].sum())
    out.update(miou=_mean(ious), pixel_acc=right / (n - void) if n > void else 0.0, per_class=per, matches=matches, ignored=ignored, n_pixels=n,
               void_pixels=void, tables=tab)
    return out


def panoptic_quality(pred_maps, segments_info, gt_maps, gt_segments, scope='scene', things=None):
    return summarize(tables(pred_maps, segments_info, gt_maps, gt_segments, scope), segments_info, gt_segments, things)


def totals(res):
    """(tp, fp, fn, ignored) over all categories"""
    return tuple(sum(d[k] for d in res['per_class'].values()) for k in ('tp', 'fp', 'fn')) + (len(res['ignored']),)


# ---------------------------------------------------------------- seeded pairs of maps
N_CATS = 4


def random_segments(shapes, P, G, seed, void=0.15, coherent=True):
    """-> (pred_maps, segments_info, gt_maps, gt_segments): int32 maps of the given shapes.  Ground truth ids are 2 k + 1 (sparse, scene-wide), predicted
    ids k + 1; categories cycle through N_CATS.
    coherent=True: the ground truth of a view is the Voronoi diagram of seeded sites that carry ids of the scene; the prediction is that diagram
    shifted by a seeded offset (boundary shifts) with gt segment k relabelled to predicted segment k mod (P - 1) (merges where G > P - 1), the right
    half of every third segment given another id (splits), and the second predicted segment carrying a foreign category (a category swap).  Then a box of about
    `void` of the view becomes void in the ground truth, the LAST predicted segment is painted inside that box and nowhere else (more than half of it on
    void: ignored), and boxes of the prediction get ids the table does not list, a negative id and a huge one; the ground truth gets an unlisted id too.
    coherent=False: independent uniform labels per pixel on both sides (every lane of a wave holds another key), void and unlisted ids among them,
    except the first four rows of a view: two of (first predicted, first gt segment) alone - a match - and two of the last predicted segment on void."""
    g = np.random.Generator(np.random.PCG64(seed))
    gt_segments = [{'id': 2 * k + 1, 'category_id': k % N_CATS} for k in range(G)]
    segments_info = [{'id': k + 1, 'category_id': (k + 1 if k == 1 and P > 3 else k) % N_CATS} for k in range(P)]
    preds, gts = [], []
    for H, W in shapes:
        if not coherent:
            gt = 2 * g.integers(1, G + 2, (H, W)) + 1                                             # rows 1 .. G - 1 (ids 3, 5, ...) and two unlisted ids
            gt[g.uniform(0, 1, (H, W)) < void] = 0
            pr = g.integers(-1, P + 2, (H, W))
            pr[(pr == 1) | (pr == P)] = 0                                                         # the first and the last id live in the header only
            if H >= 4:
                pr[0:2], gt[0:2] = (1 if P else 0), (1 if G else 0)
                pr[2:4], gt[2:4] = P, 0
            preds.append(pr.astype(np.int32))
            gts.append(gt.astype(np.int32))
            continue
        ys, xs = np.mgrid[0:H, 0:W]
        n = max(1, min(G, 3 + (H * W) // 256, 12))
        sites = np.stack([g.uniform(0, H, n), g.uniform(0, W, n)], axis=1)
        owner = g.choice(G, n, replace=False) if G else np.zeros(n, dtype=np.int64)
        cell = np.argmin((ys[..., None] - sites[:, 0]) ** 2 + (xs[..., None] - sites[:, 1]) ** 2, axis=-1)
        seg = owner[cell]                                                                         # gt row per pixel
        gt = 2 * seg + 1 if G else np.zeros((H, W), dtype=np.int64)
        dy, dx = g.integers(-1, 2), g.integers(1, 3)
        shifted = np.roll(seg, (dy, dx), axis=(0, 1))
        if P >= 2:
            pr = shifted % (P - 1) + 1
            split = (shifted % 3 == 2) & (np.roll(xs, (dy, dx), axis=(0, 1)) > sites[np.roll(cell, (dy, dx), axis=(0, 1)), 1])
            pr = np.where(split, (shifted + 1) % (P - 1) + 1, pr)
        else:
            pr = np.full((H, W), 1 if P else 0, dtype=np.int64)
        bh, bw = max(2, int(round(H * np.sqrt(void)))), max(2, int(round(W * np.sqrt(void))))
        y0, x0 = g.integers(0, H - bh + 1), g.integers(0, W - bw + 1)
        gt[y0:y0 + bh, x0:x0 + bw] = 0
        if P >= 2:
            pr[y0:y0 + bh - 1, x0:x0 + bw - 1] = P
        pr[0, :3], pr[H - 1, W - 2:], pr[H // 2, :2] = P + 5, -3, 2 ** 30
        gt[H - 1, :2] = 2 * G + 4
        preds.append(pr.astype(np.int32))
        gts.append(gt.astype(np.int32))
    return preds, segments_info, gts, gt_segments
