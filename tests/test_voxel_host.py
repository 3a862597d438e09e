"""Host side of the voxel fusion (panst3r_amd/engine/voxels.py): known answers of the numpy restatement the GPU tests compare against
(tests/voxel_ref.py), the exactness its contract rests on, and the product's side without a GPU - the C ABI, the refusals, the PLY writer, the
handling of the device status word.  No GPU needed."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi_header
import voxel_ref as R
from test_cloud_host import read_ply

F = np.float32
COLORS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]], dtype=F)
VOXEL_SYMBOLS = ['pst_voxel_accumulate', 'pst_voxel_count', 'pst_voxel_emit', 'pst_voxel_insert', 'pst_voxel_rank', 'pst_voxel_vote']


def vox(points, pan, voxel_size, rgb=None, ids=(1, 2, 3, 4), **kw):
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    rgb = np.zeros_like(points) if rgb is None else rgb
    return R.voxelize(points, rgb, pan, np.arange(len(points)) * 10, ids, voxel_size, COLORS, **kw)


def test_two_identical_views_halve_the_point_count():
    g = np.random.Generator(np.random.PCG64(1))
    one = (g.uniform(0, 50, (500, 3))).astype(F)
    pan = g.integers(1, 5, 500)
    single = vox(one, pan, 1e-4)
    assert len(single['pan']) == 500                                          # every point alone at this size
    v = vox(np.concatenate([one, one]), np.concatenate([pan, pan]), 1e-4)
    assert len(v['pan']) == 500 and v['dropped'] == 0
    assert np.array_equal(v['count'], np.full(500, 2)) and np.array_equal(v['votes'], v['count'])
    assert np.array_equal(v['pan'], pan) and np.array_equal(v['first_index'], np.arange(500) * 10)
    assert np.array_equal(v['point_voxel'], np.concatenate([np.arange(500), np.arange(500)]))
    assert np.array_equal(v['points'].view(np.uint32), single['points'].view(np.uint32))


def test_the_tie_goes_to_the_smaller_id_and_void_only_wins_alone():
    p = [[0.5, 0.5, 0.5]] * 4 + [[1.5, 0.5, 0.5]] * 3 + [[2.5, 0.5, 0.5]] * 2 + [[3.5, 0.5, 0.5]] * 5
    pan = [3, 2, 2, 3,   0, 0, 4,   0, -7,   1, 1, 99, 99, 99]             # 99 is outside the segment table: void
    v = vox(p, pan, 1.0)
    assert v['pan'].tolist() == [2, 4, 0, 1]
    assert v['votes'].tolist() == [2, 1, 2, 2] and v['count'].tolist() == [4, 3, 2, 5]
    assert v['colors'].tolist() == [[0, 0.5, 0], [0.5, 0.5, 0], [0, 0, 0], [0.5, 0, 0]]
    # an id inside the table's range that is not a listed segment is void too
    assert vox(p, pan, 1.0, ids=(1, 3, 4))['pan'].tolist() == [3, 4, 0, 1]
    assert R.point_labels(v, pan).tolist() == [2] * 4 + [4] * 3 + [0] * 2 + [1] * 5


def test_nan_infinite_and_far_points_are_dropped_and_counted():
    p = [[0.5, 0.5, 0.5], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [2.0 ** 20, 0, 0], [0, -(2.0 ** 20) - 1, 0], [2.0 ** 20 - 1, 0, 0], [-(2.0 ** 20) + 1, 0, 0],
         [3e38, 0, 0], [0.25, 0.75, 0.5]]
    pan = [1, 1, 1, 1, 1, 1, 2, 3, 1, 1]
    v = vox(p, pan, 1.0)
    assert v['dropped'] == 6 and v['point_voxel'].tolist() == [0, -1, -1, -1, -1, -1, 1, 2, -1, 0]
    assert v['count'].tolist() == [2, 1, 1] and v['pan'].tolist() == [1, 2, 3]
    assert R.point_labels(v, pan).tolist() == pan                              # a point left out keeps its own label
    assert vox(p, pan, 1e-39)['dropped'] == 10              # inv overflows to inf (the product refuses such a size): x * inf is inf, 0 * inf is NaN
    v = vox(p[1:6], pan[1:6], 1.0)
    assert v['dropped'] == 5 and len(v['pan']) == 0 and v['points'].shape == (0, 3)


def test_voxels_come_in_the_order_of_their_first_rows():
    p = [[5.5, 0, 0], [1.5, 0, 0], [5.6, 0, 0], [-3.5, 0, 0], [1.2, 0, 0], [9.0, 0, 0]]
    v = vox(p, [1] * 6, 1.0)
    assert v['point_voxel'].tolist() == [0, 1, 0, 2, 1, 3] and v['first_index'].tolist() == [0, 10, 30, 50]
    # means of the 16-bit in-cell offsets: 5.5 -> 32768, 5.6 -> 39321, 1.5 -> 32768, 1.2 -> 13107 (a position is known to voxel_size / 65536)
    assert v['points'][:, 0].tolist() == [float(F(5 + 36044.5 / 65536)), float(F(1 + 22937.5 / 65536)), -3.5, 9.0]


def exact_position(points, voxel_size):
    """step 2 in exact rational arithmetic from the restatement's own cell and offsets, rounded once per float64 operation by hand"""
    t, c, keep = R.cells(points, voxel_size)
    assert keep.all()
    q = [[int(np.floor(F(F(t[i, a] - c[i, a]) * F(65536)))) for a in range(3)] for i in range(len(t))]
    return t, c, q


@pytest.mark.parametrize('voxel_size', [0.3, 1.0, 0.0123, 7.0, 1e-3])
def test_step_two_is_exact_on_adversarial_values(voxel_size):
    """negative coordinates, values on cell borders, a voxel size that is not a power of two, checked in rational arithmetic: c <= t < c + 1; t - c is
    exact in float32 for t >= 0 and the correctly rounded difference for t < 0 (where it can need one bit more than float32 has, and rounds up to 1
    for a tiny negative t: q = 65536); the product with 65536 and the floor are exact.  One IEEE operation each, so every implementation agrees."""
    vs = voxel_size
    g = np.random.Generator(np.random.PCG64(5))
    k = g.integers(-1000, 1000, 200).astype(np.float64)
    border = (k * vs).astype(F)                                                # on (or an ulp off) cell borders
    vals = np.concatenate([border, np.nextafter(border, F(np.inf)), np.nextafter(border, F(-np.inf)), (g.standard_normal(400) * 30 * vs).astype(F),
                           np.array([0.0, -0.0, 1e-30, -1e-30, -1e-10 * vs, 1e-45, -1e-45], dtype=F)])
    pts = np.stack([vals, vals[::-1], np.roll(vals, 7)], axis=1)
    t, c, q = exact_position(pts, vs)
    inexact = top = 0
    for i in range(len(pts)):
        for a in range(3):
            tt, cc = Fraction(float(t[i, a])), Fraction(float(c[i, a]))
            assert cc <= tt < cc + 1
            d = F(t[i, a] - c[i, a])
            err = abs(Fraction(float(d)) - (tt - cc))
            if err:
                inexact += 1
                assert t[i, a] < 0 and err <= Fraction(float(np.spacing(d))) / 2
            assert 0 <= q[i][a] <= 65536 and q[i][a] == (Fraction(float(d)) * 65536).__floor__()
            if q[i][a] == 65536:
                top += 1
                assert d == F(1) and -1e-7 < t[i, a] < 0
    assert inexact > 0 and top > 0                                             # both cases are among the values
    # each point alone: pos = float32((c + q / 1 * 2^-16) * vs), the double rounding written out
    v = vox(pts, [1] * len(pts), vs)
    key = {}
    for i in range(len(pts)):
        key.setdefault(tuple(c[i]), []).append(i)
    assert len(v['pan']) == len(key)
    for r, (cell, members) in enumerate(key.items()):                          # dicts keep insertion order = order of first rows
        n = len(members)
        for a in range(3):
            s = sum(q[i][a] for i in members)
            want = F((float(cell[a]) + (float(s) / float(n)) * 2.0 ** -16) * float(vs))
            assert v['points'][r, a].tobytes() == want.tobytes()
        assert v['count'][r] == n


def test_colour_mean_is_taken_over_the_bytes():
    rgb = np.array([[0.0, 1.0, 0.5], [1.0, 1.0, 0.498], [2.0, -1.0, np.nan]], dtype=F)
    v = vox([[0.1, 0.1, 0.1]] * 3, [1, 1, 1], 1.0, rgb=rgb, opacity=0.0)
    want = np.array([(0 + 255 + 255) / 3 / 255.0, (255 + 255 + 0) / 3 / 255.0, (128 + 127 + 0) / 3 / 255.0]).astype(F)
    assert np.array_equal(v['rgb'][0], want) and np.array_equal(v['colors'][0], want)


def test_the_scene_generator_overlaps_and_the_vote_cleans_the_maps():
    """the behavioural claim, on the restatement alone: on views that see the same surfaces, the voted labels are right more often than the inputs"""
    import cloud_ref as C
    x, im, pan, info, cams, clean = R.overlapping_scene([(48, 64)] * 6, seed=11, flip=0.2)
    c = C.cloud(x, im, pan, info, cams, min_conf_thr=0.0, colors=np.zeros((len(info) + 1, 3), dtype=F))
    v = R.voxelize(c['points'], c['rgb'], c['pan'], c['index'], [s['id'] for s in c['segments']], 0.25, np.zeros((len(info) + 1, 3), dtype=F))
    assert len(v['pan']) < 0.5 * len(c['index']) and v['count'].max() >= 6      # the views do overlap
    maps = R.consistent_maps(v, c, pan)
    share = lambda m: np.mean([np.mean(a == b) for a, b in zip(m, clean)])
    assert 0.78 < share(pan) < 0.86 and share(maps) > share(pan) + 0.05


# ---------------------------------------------------------------- the product, without a GPU
def test_header_signatures_and_library_agree_on_the_voxel_symbols():
    from panst3r_amd import hip
    from panst3r_amd.build import build
    declared = sorted(p[0] for p in abi_header.prototypes() if p[0].startswith('pst_voxel_'))
    assert declared == VOXEL_SYMBOLS == sorted(s for s in hip.SIGNATURES if s.startswith('pst_voxel_'))
    lib = ctypes.CDLL(build(verbose=False))
    for s in declared:
        assert hasattr(lib, s), s
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']
    import panst3r_amd.ops as O
    for s in declared:
        assert s[4:] in O.registered_ops() and hasattr(torch.ops.panst3r_hip, s[4:]) and hasattr(hip, s[4:])
    assert [hip.voxel_capacity(m) for m in (1, 2, 3, 4, 5, 1000, 1024, 1025)] == [2, 4, 8, 8, 16, 2048, 2048, 4096]


def hand_cloud(n=4):
    from panst3r_amd.engine import PanopticCloud
    pts = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    return PanopticCloud(pts, pts, torch.zeros(n, 3), torch.ones(n, dtype=torch.int32), torch.zeros(n, 3), torch.arange(n), [0, n], [{'id': 1}])


def test_cpu_tensors_raise_and_a_bad_voxel_size_raises_first():
    from panst3r_amd.engine import voxelize_cloud
    c = hand_cloud()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        voxelize_cloud(c, 0.5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        c.voxelize(0.5)
    for bad in (0, -1.0, float('nan'), float('inf'), 1e-60, 1e60):
        with pytest.raises(ValueError, match='voxel_size'):
            voxelize_cloud(c, bad)


def test_a_full_table_reported_by_the_device_raises():
    from panst3r_amd.engine.voxels import check_status
    check_status(np.int32(0))
    with pytest.raises(RuntimeError, match='ran full'):
        check_status(np.int32(1))


def test_voxel_cloud_cpu_ply_round_trip_and_point_labels(tmp_path):
    from panst3r_amd.engine import VoxelCloud
    pts = torch.tensor([[1.5, -2.0, 3.25], [0.0, 1e-3, -7.0]])
    col = torch.tensor([[0.0, 1.0, 0.5], [0.498, 0.502, 2.0]])
    pan, count = torch.tensor([3, 0], dtype=torch.int32), torch.tensor([5, 70000], dtype=torch.int32)
    v = VoxelCloud(pts, col, pan, col, count, count, torch.tensor([0, 4]), torch.tensor([0, 0, -1, 1], dtype=torch.int32), [], None, [0, 9], 0.25, 1,
                   point_pan=torch.tensor([7, 7, 7, 7], dtype=torch.int32), point_index=torch.tensor([0, 2, 3, 4])).cpu()
    n, names, rows = read_ply(v.write_ply(str(tmp_path / 'v.ply')))
    assert n == 2 and names == ['x', 'y', 'z', 'red', 'green', 'blue', 'label', 'count']
    assert rows[0] == (1.5, -2.0, 3.25, 0, 255, 128, 3, 5) and rows[1][3:] == (127, 128, 255, 0, 70000)
    assert np.array_equal(np.array(rows[1][:3], dtype=F), pts[1].numpy())
    assert v.point_labels().tolist() == [3, 3, 7, 0] and len(v) == 2 and v.voxel_size == 0.25 and v.dropped == 1
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        v.consistent_maps()
