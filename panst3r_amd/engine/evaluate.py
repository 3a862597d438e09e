"""Panoptic quality of predicted maps against ground truth on the device (stage f7): PQ / SQ / RQ over all categories, over things and over stuff, and the
semantic mIoU / pixel accuracy.  It scores what the other stages leave on the device: `pan_preds[0]['pan']` of a panoptic post-processing,
`VoxelCloud.consistent_maps()` and `render_cameras(...)['pan']`.

The reference has no such stage: *restated, unpinned*.  The rules are those of COCO panopticapi's pq_compute_single_core without iscrowd, written
out in include/panst3r_hip.h and restated in numpy in tests/eval_ref.py; csrc/evaluate.hip is held to that bit for bit (a joint histogram of two
integer maps by int32 atomics, integer comparisons, one float64 division per match).  Two readings of the metric:
  scope='scene'  segments are matched across all views of the scene at once (the scene-level PQ of Panoptic Lifting, the paper's setting): an
                 instance whose id changes between views cannot match its ground truth in both, and is punished;
  scope='view'   the per-image COCO reading: every view is matched on its own and the counts are summed.
Contract, with P = len(segments_info), G = len(gt_segments), N = total pixels < 2^31, ids unique and > 0 within each list:
  1 rows      a predicted id i maps to row id2row_p[i] if 0 < i < ntab_p and that entry is >= 0, else to the void row P; ground truth likewise to a
              column, or the void column G.  Ids <= 0, ids beyond the table and ids not listed are all void, as in `voxelize_cloud`.
  2 slabs     'scene': S = 1 slab with every pixel; 'view': S = V slabs.
  3 counts    counts int32 [S, P+1, G+1] = pixels of slab s with (row p, column g).
  4 areas     pa[s,p] = sum_g counts[s,p,g], ga[s,g] = sum_p counts[s,p,g], void included; area 0 = the segment does not exist in that slab.
  5 match     g with ga > 0, p with pa > 0, same category: inter = counts[s,p,g], union = pa + ga - inter - counts[s,p,G]; a match iff 2 inter > union
              (int64; equality is no match); iou = inter / union in float64.
  6 misses    FN: an existing g without a match; an existing p without a match is ignored if 2 counts[s,p,G] > pa[s,p], else an FP.
  7 category  float64 on the host, slabs ascending then gt rows ascending: pq = iou_sum / (tp + 0.5 fp + 0.5 fn), sq = iou_sum / tp (0 if tp = 0),
              rq = tp / (tp + 0.5 fp + 0.5 fn); categories with tp + fp + fn = 0 are left out; the means run over the others in ascending category
              order (0 if there is none).
  8 semantic  rows and columns merged by category, void stays void, summed over slabs in integers: iou_c = inter_c / (pred_c + gt_c - inter_c -
              pred_c-on-void), miou over the categories with gt_c > 0, pixel_acc = sum_c inter_c / (non-void gt pixels) (0 without any)."""
import numpy as np
import torch

from .. import hip

ABSENT, MATCHED, FP, IGNORED = 0, 1, 2, 3


def _segment_table(segs, what):
    ids, cats = [], []
    for s in segs:
        if s.get('iscrowd'):
            raise ValueError('panoptic_quality: %s segment %r is a crowd region (iscrowd): crowd regions are not supported' % (what, s.get('id')))
        ids.append(int(s['id']))
        cats.append(int(s['category_id']))
    if len(set(ids)) != len(ids) or any(not 0 < i < hip.EVAL_MAX_ID for i in ids):
        raise ValueError('panoptic_quality: the ids of the %s segments must be unique and in (0, %d), got %s' % (what, hip.EVAL_MAX_ID, sorted(ids)[:8]))
    tab = np.full(max(ids + [0]) + 1, -1, dtype=np.int32)
    tab[ids] = np.arange(len(ids), dtype=np.int32)
    return ids, cats, tab


def _map_list(maps, what):
    if isinstance(maps, (torch.Tensor, np.ndarray)):
        if maps.ndim != 3:
            raise ValueError('panoptic_quality: stacked %s maps must be [V, H, W], got %s' % (what, tuple(maps.shape)))
        maps = list(maps)
    maps = list(maps)
    for m in maps:
        if m.ndim != 2:
            raise ValueError('panoptic_quality: a %s map must be [H, W], got %s' % (what, tuple(m.shape)))
        integer = not (m.dtype.is_floating_point or m.dtype == torch.bool) if isinstance(m, torch.Tensor) else np.asarray(m).dtype.kind in 'iu'
        if not integer:
            raise ValueError('panoptic_quality: a %s map holds integer ids, got %s' % (what, m.dtype))
    return maps


def _mean(xs):
    return sum(xs) / len(xs) if xs else 0.0


def _flat(maps, dev):
    out = []
    for m in maps:
        t = m if isinstance(m, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(m))
        out.append(t.to(device=dev, dtype=torch.int32).reshape(-1))
    flat = out[0].contiguous() if len(out) == 1 else torch.cat(out)
    return flat.clone() if flat.data_ptr() % 16 else flat                    # a view into a larger buffer: the kernel loads 16 bytes per lane


@torch.no_grad()
def panoptic_quality(pred_maps, segments_info, gt_maps, gt_segments, *, scope='scene', things=None):
    """Score V predicted panoptic maps (device int tensors [H_v, W_v], a list or a stacked [V, H, W] tensor; `segments_info` with 'id' and 'category_id'
    per entry, as every panoptic_inference_* returns it) against V ground-truth maps of the same shapes (tensors or numpy arrays; they are moved to
    the predictions' device) with `gt_segments` in the same form.  scope='scene' matches segments across all views at once, scope='view' per view.
    `things`: a collection of category ids, for the means over things and over stuff.  Returns a dict: pq, sq, rq; pq_things ... rq_stuff (None
    without `things`); miou, pixel_acc; per_class {category: tp, fp, fn, iou_sum, pq, sq, rq, iou} (None where undefined); matches [(slab, pred id,
    gt id, iou)]; ignored [(slab, pred id)]; n_pixels, void_pixels (pixels on void ground truth); tables: counts, pred_area, gt_area, match, iou,
    pred_state as numpy arrays.  One host sync.  GPU only: predicted maps on the CPU raise."""
    if scope not in ('scene', 'view'):
        raise ValueError("panoptic_quality: scope must be 'scene' or 'view', got %r" % (scope,))
    preds, gts = _map_list(pred_maps, 'predicted'), _map_list(gt_maps, 'ground-truth')
    V = len(preds)
    if V == 0 or len(gts) != V:
        raise ValueError('panoptic_quality: needs V >= 1 predicted maps and as many ground-truth maps, got %d and %d' % (V, len(gts)))
    sizes = []
    for v, (a, b) in enumerate(zip(preds, gts)):
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError('panoptic_quality: view %d: the predicted map is %s, the ground truth %s' % (v, tuple(a.shape), tuple(b.shape)))
        sizes.append(int(a.shape[0]) * int(a.shape[1]))
    N = sum(sizes)
    if not 0 < N < 2 ** 31:
        raise ValueError('panoptic_quality: the maps hold %d pixels; one call takes 1 .. 2^31 - 1' % N)
    ids_p, cat_p, tab_p = _segment_table(segments_info, 'predicted')
    ids_g, cat_g, tab_g = _segment_table(gt_segments, 'ground-truth')
    P, G = len(ids_p), len(ids_g)
    S = 1 if scope == 'scene' else V
    if 4 * S * (P + 1) * (G + 1) > hip.EVAL_MAX_TABLE_BYTES:
        raise ValueError('panoptic_quality: the counts table [%d, %d, %d] int32 is above hip.EVAL_MAX_TABLE_BYTES = %d bytes' % (S, P + 1, G + 1, hip.EVAL_MAX_TABLE_BYTES))
    for m in preds:
        if not (isinstance(m, torch.Tensor) and m.is_cuda):
            raise RuntimeError('panoptic_quality got predicted maps on %s: it runs on the GPU only (no CPU fallback)' % (m.device if isinstance(m, torch.Tensor) else 'the host'))
    dev = preds[0].device
    pred, gt = _flat(preds, dev), _flat(gts, dev)
    off = np.array([0, N] if S == 1 else np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int64)
    slab_off = torch.from_numpy(off).to(dev)
    blob = torch.from_numpy(np.concatenate([tab_p, tab_g, np.array(cat_p + cat_g, dtype=np.int32)])).to(dev)       # one copy: both id tables, both category tables
    id2row_p, id2row_g, cp, cg = torch.split(blob, [len(tab_p), len(tab_g), P, G])
    i32 = dict(dtype=torch.int32, device=dev)
    counts = torch.zeros(S, P + 1, G + 1, **i32)
    pa, ga, match, state = torch.empty(S, P, **i32), torch.empty(S, G, **i32), torch.empty(S, G, **i32), torch.empty(S, P, **i32)
    iou = torch.empty(S, G, dtype=torch.float64, device=dev)
    hip.pq_count(pred, gt, slab_off, id2row_p, id2row_g, P, G, counts)
    hip.pq_match(counts, cp, cg, pa, ga, match, iou, state)
    parts = [iou.view(torch.int32).reshape(-1), counts.reshape(-1), pa.reshape(-1), ga.reshape(-1), match.reshape(-1), state.reshape(-1)]
    res = torch.cat(parts).cpu().numpy()                                     # the only host sync
    cut = np.cumsum([p.numel() for p in parts])[:-1]
    iou_h, counts_h, pa_h, ga_h, match_h, state_h = np.split(res, cut)
    tables = {'counts': counts_h.reshape(S, P + 1, G + 1), 'pred_area': pa_h.reshape(S, P), 'gt_area': ga_h.reshape(S, G), 'match': match_h.reshape(S, G),
              'iou': iou_h.copy().view(np.float64).reshape(S, G), 'pred_state': state_h.reshape(S, P)}
    return _summarize(tables, ids_p, cat_p, ids_g, cat_g, things)


def _summarize(tables, ids_p, cat_p, ids_g, cat_g, things):
    """steps 7 and 8: float64 host arithmetic on the copied tables, in the contract's order"""
    counts, match, iou, state, ga = tables['counts'].astype(np.int64), tables['match'], tables['iou'], tables['pred_state'], tables['gt_area']
    S, P, G = counts.shape[0], len(ids_p), len(ids_g)
    cats = sorted(set(cat_p) | set(cat_g))
    per = {c: {'tp': 0, 'fp': 0, 'fn': 0, 'iou_sum': 0.0, 'pq': None, 'sq': None, 'rq': None, 'iou': None} for c in cats}
    matches, ignored = [], []
    for s in range(S):
        for g in range(G):
            p = int(match[s, g])
            if p >= 0:
                d = per[cat_g[g]]
                d['tp'] += 1
                d['iou_sum'] += float(iou[s, g])
                matches.append((s, ids_p[p], ids_g[g], float(iou[s, g])))
            elif ga[s, g] > 0:
                per[cat_g[g]]['fn'] += 1
        for p in np.nonzero(state[s] >= FP)[0]:
            if state[s, p] == FP:
                per[cat_p[p]]['fp'] += 1
            else:
                ignored.append((s, ids_p[p]))
    for d in per.values():
        den = d['tp'] + 0.5 * d['fp'] + 0.5 * d['fn']
        if den > 0:
            d['pq'], d['sq'], d['rq'] = d['iou_sum'] / den, (d['iou_sum'] / d['tp'] if d['tp'] else 0.0), d['tp'] / den
    scored = [c for c in cats if per[c]['pq'] is not None]
    out = {k: _mean([per[c][k] for c in scored]) for k in ('pq', 'sq', 'rq')}
    th = None if things is None else {int(t) for t in things}
    for name, keep in (('things', lambda c: c in th), ('stuff', lambda c: c not in th)):
        for k in ('pq', 'sq', 'rq'):
            out['%s_%s' % (k, name)] = None if th is None else _mean([per[c][k] for c in scored if keep(c)])
    K = len(cats)
    col = {c: i for i, c in enumerate(cats)}
    rp, rg = np.array([col[c] for c in cat_p] + [K], dtype=np.int64), np.array([col[c] for c in cat_g] + [K], dtype=np.int64)
    sem = np.zeros((K + 1, K + 1), dtype=np.int64)
    np.add.at(sem, (rp[:, None], rg[None, :]), counts.sum(axis=0))          # rows and columns merged by category, void stays void
    ious, right = [], 0
    for c in cats:
        i = col[c]
        inter, pred_c, gt_c, on_void = int(sem[i, i]), int(sem[i, :].sum()), int(sem[:, i].sum()), int(sem[i, K])
        right += inter
        if gt_c > 0:
            per[c]['iou'] = inter / (pred_c + gt_c - inter - on_void)
            ious.append(per[c]['iou'])
    n, void = int(counts.sum()), int(counts[:, :, G].sum())
    out.update(miou=_mean(ious), pixel_acc=right / (n - void) if n > void else 0.0, per_class=per, matches=matches, ignored=ignored, n_pixels=n,
               void_pixels=void, tables=tables)
    return out
