"""The scene and the workspaces of the list-refusal tests (test_hip_score3d.py, test_hip_icp.py, test_hip_meshdist.py): the per-cell lists of
csrc/voxel_table.h are guarded once, where they are filled and before they are read, and these tests hand the kernels lists that are not their
build's.  They assert a refusal through the status words, never a fault: every tensor an index is read from (`targets`, `rows`, `vertices`, `faces`) is
the leading contiguous view of a tensor twice as long whose tail holds valid rows, so a kernel that lost a guard returns a wrong answer from memory
the test owns."""
import functools

import numpy as np
import torch

import nearest_ref as N
from panst3r_amd import hip

DEV = 'cuda:0'
F = np.float32
CELL = 0.25
LISTS = 2                                                                         # PST_NN_LISTS == PST_MESHDIST_LISTS
I32 = dict(dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def lattice():
    """300 targets on a 10 x 10 x 3 lattice of pitch 1/8 - 5 x 5 x 2 cells of edge 1/4 with 8 or 4 targets each, more than one workgroup of 256 - and
    300 queries, each a 32nd or less beside its target.  Row 0 lies in the cell (0, 0, 0): the cell the tests tamper with."""
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(3), indexing='ij'), -1).reshape(-1, 3)
    T = (g * 0.125 + 0.0625).astype(F)
    return (T + F([0.03125, 0.015625, 0.0078125])).astype(F), T


def check_lattice():
    """-> (touched, untouched): the queries whose 27 cells hold the cell of target 0, and those whose 27 cells do not"""
    Q, T = lattice()
    cq, ct = N.cells(Q, CELL)[0], N.cells(T, CELL)[0]
    assert len(T) == len(Q) == 300 > 256 and (ct[0] == 0).all() and (ct == ct[0]).all(1).sum() == 8      # a list of 8, and a second workgroup
    touched = np.abs(cq - ct[0]).max(1) <= 1
    want = N.nearest(Q, T, CELL)
    assert touched.sum() >= 8 and (~touched).sum() > 100 and (want['row'] == np.arange(300)).all()         # every query finds its own target
    assert (np.nonzero(~touched)[0] >= 256).any() and (np.nonzero(touched)[0] < 256).all()                # untouched readers in the other workgroup
    return touched, ~touched


def padded(a):
    """the array on the device as the leading view of a tensor that holds it twice: row len(a) is a valid row"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return torch.cat([t, t])[:len(t)]


def padded_rows(n):
    """(rows int32 [n] filled with -7, the tensor of 2 n it is the head of: the tail is zeros, the valid row or face 0)"""
    big = torch.cat([torch.full((n,), -7, **I32), torch.zeros(n, **I32)])
    return big[:n], big


def offsets(ws):
    ws['start'] = torch.cumsum(ws['cell_count'], 0, dtype=torch.int32) - ws['cell_count']


def nn_build(targets, tamper=None):
    """the build of `NearestIndex` by hand over padded rows; `tamper(ws)` runs between the offsets and the scatter"""
    ws = hip.nn_workspace(targets.shape[0], DEV)
    ws['rows'], ws['rows_big'] = padded_rows(targets.shape[0])
    hip.nn_insert(targets, float(N.radius_numbers(CELL)[1]), ws)
    offsets(ws)
    if tamper:
        tamper(ws)
    hip.nn_scatter(ws)
    return ws


def mesh_build(vertices, faces, tamper=None):
    """the build of `MeshIndex` by hand over padded rows -> the workspace, with `prefix` and the build's `status` in it"""
    inv = float(N.radius_numbers(CELL)[1])
    nf = faces.shape[0]
    counts, total, status = torch.empty(nf, **I32), torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(4, **I32)
    hip.meshdist_count(vertices, faces, inv, counts, total, status)
    prefix = torch.empty(nf + 1, **I32)
    hip.cloud_scan(counts, prefix)
    ws = hip.meshdist_workspace(int(total), DEV)
    ws['rows'], ws['rows_big'] = padded_rows(ws['P'])
    hip.meshdist_insert(vertices, faces, inv, prefix, ws, status)
    offsets(ws)
    if tamper:
        tamper(ws)
    hip.meshdist_scatter(prefix, ws, status)
    return dict(ws, prefix=prefix, status=status)


def fresh(ws):
    """a copy of a built workspace that shares no memory with it, its rows padded again, its status words zero"""
    out = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in ws.items()}
    out['rows'] = out['rows_big'][:ws['rows'].numel()]
    out['status'].zero_()
    return out


def move_list_out(ws, slot, total):
    """case (a): the list of `slot` ends one past rows[0, total)"""
    assert int(ws['cell_count'][slot]) >= 2
    ws['start'][slot] = total - int(ws['cell_count'][slot]) + 1


def first_entry_past_the_end(ws, slot, n):
    """case (b): the first entry of the list of `slot` names row (or face) n, one past the last"""
    ws['rows'][int(ws['start'][slot])] = n


def lists_of(ws):
    """slot -> the sorted entries of its list, for the occupied slots"""
    rows, start, cnt = ws['rows'].cpu().numpy(), ws['start'].cpu().numpy(), ws['cell_count'].cpu().numpy()
    return {int(s): sorted(rows[start[s]:start[s] + cnt[s]].tolist()) for s in np.nonzero(cnt > 0)[0]}


def assert_a_short_count_is_refused(good, build, slot_of, total):
    """case (c): the count of the slot `slot_of(ws)` lowered by one before the scatter.  The scatter sets the LISTS bit, every other list is the good
    build's, the slot's own list holds all but one of its entries and one row nobody wrote, nothing lands past rows[0, total), status[2] is no more
    than the longest list.  (Which slot a cell gets depends on arrival where two keys collide: the lists are compared by what they hold.)"""
    def lower(ws):
        ws['cell_count'][slot_of(ws)] -= 1
    bad = build(lower)
    assert bad['status'][0].item() == LISTS and 1 <= bad['status'][2].item() <= good['status'][2].item()
    slot = slot_of(bad)
    bad['cell_count'][slot] += 1                                                  # read the lists by the true counts
    want, got = lists_of(good), lists_of(bad)
    mine, short = want.pop(slot_of(good)), got.pop(slot)
    assert sorted(want.values()) == sorted(got.values())
    assert short.count(-7) == 1 and set(short) - {-7} < set(mine) and len(short) == len(mine) >= 2
    assert (bad['rows_big'][total:] == 0).all() and (bad['fill'].sort().values == good['fill'].sort().values).all()
