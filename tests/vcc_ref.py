"""numpy restatement of the connected components of the voxel cloud and of the label despeckling (panst3r_amd/engine/voxels.py, csrc/components.hip),
the yardstick the kernels are held to bit for bit.  [restated, parity unpinned]: own design, the reference has no such stage.

The contract (include/panst3r_hip.h): a voxel's cell is floor(float32(p * inv)) of its first point; two voxels are adjacent when their cells differ by
at most 1 on every axis and on exactly 1 (connectivity 6), 1 or 2 (18) or 1 to 3 (26) axes, and a neighbour cell with a coordinate outside
(-2^20, 2^20) does not exist; a component is a maximal set of voxels of one id > 0 connected through adjacent voxels of that id; root = its smallest
row, component = the rank of the root; the table per component; despeckling = one round of votes of the (voxel, adjacent voxel in a component that is
not small) pairs of every small component, most votes win, ties to the smallest id, no vote -> void.

Written independently of the kernels' method: the neighbour lookup is np.searchsorted on the sorted cell keys (no hash table), the components are
found by rounds of hooking the labels of all edges at once (np.minimum.at) and pointer jumping (no sequential union-find), the votes by np.unique."""
import numpy as np

import cloud_ref
import voxel_ref

F = np.float32
LIM = 1 << 20
AXES = {6: 1, 18: 2, 26: 3}


def cells_of(points, vox, voxel_size):
    """int32 [Mv, 3]: the cell of every voxel's first point; `points` the cloud's, `vox` voxel_ref.voxelize's dict"""
    t, c, keep = voxel_ref.cells(points, voxel_size)
    pv = vox['point_voxel']
    Mv = len(vox['pan'])
    first = np.full(Mv, len(pv), dtype=np.int64)
    np.minimum.at(first, pv[pv >= 0], np.nonzero(pv >= 0)[0])
    return c[first].astype(np.int32).reshape(Mv, 3)


def offsets(connectivity):
    """the (dx, dy, dz) != 0 of the neighbourhood"""
    n = AXES[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 0 < (dx != 0) + (dy != 0) + (dz != 0) <= n]


def _key(c):
    c = c.astype(np.int64) + LIM
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def pairs(cells, connectivity):
    """all ordered pairs (v, n) of adjacent voxels: two int64 arrays.  Neighbour cells outside (-2^20, 2^20) are never formed into a key."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    assert (np.abs(cells) < LIM).all()
    key = _key(cells)
    order = np.argsort(key, kind='stable')
    skey = key[order]
    assert (skey[1:] != skey[:-1]).all(), 'two voxels share a cell'
    vs, ns = [], []
    for d in offsets(connectivity):
        nc = cells + np.array(d, dtype=np.int64)
        ok = (np.abs(nc) < LIM).all(axis=1)
        v = np.nonzero(ok)[0]
        nk = _key(nc[ok])
        pos = np.searchsorted(skey, nk)
        hit = pos < len(skey)
        hit[hit] = skey[pos[hit]] == nk[hit]
        vs.append(v[hit])
        ns.append(order[pos[hit]])
    if not vs:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(vs), np.concatenate(ns)


def components(cells, pan, count, connectivity=26):
    """dict(component, root int32 [Mv]; per component roots, pan, size int32 [C], points int64 [C], cell_lo, cell_hi int32 [C, 3];
    pairs: the adjacent pairs it was built from)"""
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 3)
    pan, count = np.asarray(pan).reshape(-1).astype(np.int32), np.asarray(count).reshape(-1).astype(np.int64)
    Mv = len(pan)
    v, n = all_pairs = pairs(cells, connectivity)
    same = (pan[v] > 0) & (pan[v] == pan[n])
    v, n = v[same], n[same]
    # label[x] = a row of x's component that is <= x.  Per round: every edge whose ends carry different labels hooks the larger label under the smaller
    # (labels are fixed points after the jumping below, so no cycle can form), then pointer jumping until every label is a fixed point again.  It ends
    # when all edges agree: the label of a component is then a member that is <= every member - its smallest row.
    label = np.arange(Mv, dtype=np.int64)
    while True:
        lv, ln = label[v], label[n]
        open_ = lv != ln
        if not open_.any():
            break
        np.minimum.at(label, np.maximum(lv, ln)[open_], np.minimum(lv, ln)[open_])
        while True:
            j = label[label]
            if np.array_equal(j, label):
                break
            label = j
        v, n = v[open_], n[open_]                                    # an edge whose ends agree stays in one component
    solid = pan > 0
    root = np.where(solid, label, -1).astype(np.int32)
    roots = np.unique(root[solid])
    component = np.full(Mv, -1, dtype=np.int32)
    component[solid] = np.searchsorted(roots, root[solid]).astype(np.int32)
    C = len(roots)
    comp = component[solid]
    lo, hi = np.full((C, 3), np.iinfo(np.int32).max, dtype=np.int32), np.full((C, 3), np.iinfo(np.int32).min, dtype=np.int32)
    np.minimum.at(lo, comp, cells[solid])
    np.maximum.at(hi, comp, cells[solid])
    points = np.zeros(C, dtype=np.int64)
    np.add.at(points, comp, count[solid])
    return {'component': component, 'root': root, 'roots': roots.astype(np.int32), 'pan': pan[roots].astype(np.int32),
            'size': np.bincount(comp, minlength=C).astype(np.int32), 'points': points, 'cell_lo': lo, 'cell_hi': hi, 'pairs': all_pairs}


def boxes(comp, voxel_size):
    """the metric boxes, float64: (cell_lo * voxel_size, (cell_hi + 1) * voxel_size)"""
    vs = np.float64(voxel_size)
    return comp['cell_lo'].astype(np.float64) * vs, (comp['cell_hi'].astype(np.float64) + 1.0) * vs


def clean_pan(cells, pan, count, min_voxels, connectivity=26, comp=None):
    """(new pan int32 [Mv], relabelled, floaters): the despeckled ids and the number of voxels that took another id / became void"""
    pan = np.asarray(pan).reshape(-1).astype(np.int32)
    comp = components(cells, pan, count, connectivity) if comp is None else comp
    small_c = comp['size'] < min_voxels
    cv = comp['component']
    small = (cv >= 0) & small_c[np.maximum(cv, 0)]
    large = (cv >= 0) & ~small
    v, n = comp['pairs']
    vote = small[v] & large[n]                                       # (pan[n] > 0 is implied: n lies in a component)
    out = pan.copy()
    out[small] = 0                                                   # without a vote: a floater
    if vote.any():
        span = int(pan.max()) + 1
        key, votes = np.unique(cv[v[vote]].astype(np.int64) * span + pan[n[vote]], return_counts=True)
        c, pid = key // span, key % span
        o = np.lexsort((pid, -votes, c))                             # by component, then most votes, then smallest id
        head = np.ones(len(o), dtype=bool)
        head[1:] = c[o][1:] != c[o][:-1]
        winner = np.zeros(len(comp['size']), dtype=np.int32)
        winner[c[o[head]]] = pid[o[head]].astype(np.int32)
        out[small] = winner[cv[small]]
    return out, int((small & (out > 0)).sum()), int((small & (out == 0)).sum())


def clean(vox, cells, segments_info, colors, min_voxels, connectivity=26, opacity=0.5, comp=None):
    """voxel_ref.voxelize's dict with the despeckled pan, the re-blended colours, 'relabelled', 'floaters' and 'cells'; and its segment table"""
    colors = np.asarray(colors, dtype=F).reshape(-1, 3)
    out = dict(vox)
    out['pan'], out['relabelled'], out['floaters'] = clean_pan(cells, vox['pan'], vox['count'], min_voxels, connectivity, comp)
    known = (out['pan'] > 0) & (out['pan'] < len(colors))
    vis = np.zeros((len(out['pan']), 3), dtype=F)
    vis[known] = colors[out['pan'][known]]
    out['colors'] = cloud_ref.blend(vox['rgb'], vis, opacity)
    out['cells'] = np.asarray(cells, dtype=np.int32).reshape(-1, 3)
    return out, voxel_ref.segments(out, segments_info)
