"""Host side of the panoptic point cloud (panst3r_amd/engine/cloud.py): known answers of the numpy restatement the GPU tests compare against
(tests/cloud_ref.py), the two numpy facts the kernel contract rests on, the default colour table, the PLY writer, the frusta, and the C ABI.
No GPU needed."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest
import torch

import abi_header
import cloud_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUD_SYMBOLS = ['pst_cloud_compact', 'pst_cloud_count', 'pst_cloud_scan', 'pst_cloud_segment_median']


def one_view(pts, conf, pan, c2w=None, img=None):
    """a 1 x n view from n points"""
    n = len(conf)
    pts = np.asarray(pts, dtype=F).reshape(1, n, 3)
    x = {'pts3d': pts, 'pts3d_local': pts.copy(), 'conf': np.asarray(conf, dtype=F).reshape(1, n)}
    img = np.zeros((3, 1, n), dtype=F) if img is None else np.asarray(img, dtype=F).reshape(3, 1, n)
    return [x], [img], [np.asarray(pan, dtype=np.int32).reshape(1, n)], [np.eye(4, dtype=F) if c2w is None else np.asarray(c2w, dtype=F)]


COLORS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F)
PTS3 = [[1, 2, 3], [4, 5, 6], [7, 8, 10]]


def test_three_points_under_the_identity():
    x, im, pan, cams = one_view(PTS3, [5, 5, 5], [1, 1, 1], img=[[-1, 0, 1], [1, 1, 1], [0, 0, 0]])
    c = R.cloud(x, im, pan, [{'id': 1}], cams, min_conf_thr=3.0, opacity=0.5, colors=COLORS)
    assert np.array_equal(c['points'], np.array(PTS3, dtype=F)) and np.array_equal(c['points_local'], np.array(PTS3, dtype=F))
    assert np.array_equal(c['rgb'], np.array([[0, 1, 0.5], [0.5, 1, 0.5], [1, 1, 0.5]], dtype=F))                # HWC order, img * 0.5 + 0.5
    assert np.array_equal(c['colors'], np.array([[0.5, 0.5, 0.25], [0.75, 0.5, 0.25], [1, 0.5, 0.25]], dtype=F))  # half rgb, half red
    assert c['index'].tolist() == [0, 1, 2] and c['pan'].tolist() == [1, 1, 1]
    assert len(c['segments']) == 1 and c['segments'][0]['count'] == 3 and c['segments'][0]['median'].tolist() == [4, 5, 6]


def test_three_points_under_a_quarter_turn():
    c2w = np.eye(4, dtype=F)
    c2w[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]          # 90 degrees about z: (x, y, z) -> (-y, x, z)
    c2w[:3, 3] = [10, 20, 30]
    x, im, pan, cams = one_view(PTS3, [5, 5, 5], [2, 2, 2], c2w=c2w)
    c = R.cloud(x, im, pan, [{'id': 2}], cams, colors=COLORS)
    assert np.array_equal(c['points'], np.array(PTS3, dtype=F))                                                   # pts3d is already in the world frame
    assert np.array_equal(c['points_local'], np.array([[8, 21, 33], [5, 24, 36], [2, 27, 40]], dtype=F))
    assert np.array_equal(R.cloud(x, im, pan, [{'id': 2}], cams, colors=COLORS, local_pointmaps=True)['points'], c['points_local'])
    assert c['segments'][0]['median'].tolist() == [5, 24, 36]


def test_segments_odd_even_single_and_skipped_and_the_threshold_is_inclusive():
    pts = [[1, 0, 0], [2, 0, 0], [4, 0, 0],       # segment 1: three points
           [1, 1, 0], [2, 3, 0], [4, 5, 0], [8, 7, 0],   # segment 2: four
           [9, 9, 9],                             # segment 3: one
           [5, 5, 5],                             # segment 4: below the threshold
           [6, 6, 6]]                             # void
    conf = [3, 3.5, 4, 3, 3, 3, 3, 3, 2.999, 10]
    pan = [1, 1, 1, 2, 2, 2, 2, 3, 4, 0]
    x, im, p, cams = one_view(pts, conf, pan)
    info = [{'id': i, 'query_id': 10 + i, 'category_id': 20 + i} for i in (1, 2, 3, 4)]
    c = R.cloud(x, im, p, info, cams, min_conf_thr=3.0, colors=np.zeros((5, 3)))
    assert c['index'].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9]                  # conf == 3.0 kept, 2.999 dropped, order kept
    seg = {s['id']: s for s in c['segments']}
    assert sorted(seg) == [1, 2, 3]                                            # 4 has no kept point: skipped
    assert seg[1]['median'].tolist() == [2, 0, 0] and seg[1]['count'] == 3
    assert seg[2]['median'].tolist() == [3, 4, 0] and seg[2]['count'] == 4
    assert seg[3]['median'].tolist() == [9, 9, 9] and (seg[3]['query_id'], seg[3]['category_id']) == (13, 23)
    assert c['colors'][-1].tolist() == [0.25, 0.25, 0.25] and c['pan'][-1] == 0  # void: half grey image, half black


@pytest.mark.parametrize('n', [1, 2, 3, 4, 7, 64, 1001, 4096])
def test_np_median_of_float32_is_the_two_order_statistic_form(n):
    g = np.random.Generator(np.random.PCG64(n))
    for scale in (1.0, 1e-30, 1e30, 3e38):
        with np.errstate(over='ignore', invalid='ignore'):               # 3e38: a few values and the sum of the two middle ones may overflow, identically
            x = (g.standard_normal(n) * scale).astype(F)
            got, want = R.median_two_stat(x), np.median(x)
        assert want.dtype == F and got.tobytes() == want.tobytes(), (n, scale)
    assert np.isnan(np.median(np.array([1, np.nan, 3][:max(n, 2)], dtype=F)))       # a NaN makes the median NaN


def test_blend_with_a_python_float_equals_the_float32_weights_form():
    g = np.random.Generator(np.random.PCG64(3))
    rgb, vis = g.uniform(0, 1, (5000, 3)).astype(F), g.uniform(0, 1, (5000, 3)).astype(F)
    for alpha in (0.0, 0.5, 0.3, 0.7, 1.0, 0.123456789):
        demo = (1.0 - alpha) * rgb + alpha * vis                      # tools/demo_panst3r.py:351-352 with a Python float from the slider
        assert demo.dtype == F and np.array_equal(demo, R.blend(rgb, vis, alpha)), alpha
        w1, w2 = F(1.0 - alpha), F(alpha)
        assert np.array_equal(demo, (w1 * rgb).astype(F) + (w2 * vis).astype(F))


def test_default_colour_table():
    from panst3r_amd.engine.cloud import default_colors
    a, b = default_colors(201), default_colors(201)
    assert a.dtype == F and a.shape == (201, 3) and np.array_equal(a, b)
    assert np.array_equal(default_colors(50), a[:50])                 # keyed by id, not by the table's length
    assert a[0].tolist() == [0, 0, 0]
    assert len({tuple(r) for r in a.tolist()}) == 201
    assert a[1:].min() >= 0.92 * (1 - 0.60) - 1e-6 and a[1:].max() <= 1.0       # pastel: value >= 0.92, saturation <= 0.60


def read_ply(path):
    """minimal reader of what write_ply writes: header fields by name, then fixed-size little-endian rows"""
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    n = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith('property')]
    fmt = '<' + ''.join({'float': 'f', 'uchar': 'B', 'int': 'i'}[t] for t, _ in props)
    assert len(body) == n * struct.calcsize(fmt)
    rows = [struct.unpack_from(fmt, body, i * struct.calcsize(fmt)) for i in range(n)]
    return n, [name for _, name in props], rows


def test_ply_round_trip(tmp_path):
    from panst3r_amd.engine.cloud import PanopticCloud
    pts = torch.tensor([[1.5, -2.0, 3.25], [0.0, 1e-3, -7.0], [4.0, 5.0, 6.0]])
    col = torch.tensor([[0.0, 1.0, 0.5], [0.498, 0.502, 2.0], [-1.0, 0.00196, 0.00197]])
    pan = torch.tensor([3, 0, 70000], dtype=torch.int32)
    cl = PanopticCloud(pts, pts, col, pan, col, torch.arange(3), [0, 3], [])
    n, names, rows = read_ply(cl.write_ply(str(tmp_path / 'c.ply')))
    assert n == 3 and names == ['x', 'y', 'z', 'red', 'green', 'blue', 'label']
    for r, p, c, l in zip(rows, pts.numpy(), col.numpy(), pan.tolist()):
        assert np.array_equal(np.array(r[:3], dtype=F), p) and r[6] == l
        assert list(r[3:6]) == [int(math.floor(min(max(float(v), 0.0), 1.0) * 255 + 0.5)) for v in c]
    assert rows[0][3:6] == (0, 255, 128) and rows[1][3:6] == (127, 128, 255) and rows[2][3:6] == (0, 0, 1)
    empty = PanopticCloud(pts[:0], pts[:0], col[:0], pan[:0], col[:0], torch.arange(0), [0, 3], [])
    assert read_ply(empty.write_ply(str(tmp_path / 'e.ply')))[0] == 0


def test_frusta():
    from panst3r_amd.engine.cloud import camera_frusta, quaternion_wxyz
    s = math.sqrt(0.5)
    assert np.allclose(quaternion_wxyz(np.eye(3)), [1, 0, 0, 0])
    assert np.allclose(quaternion_wxyz([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), [s, 0, 0, s])          # 90 degrees about z
    assert np.allclose(quaternion_wxyz([[1, 0, 0], [0, -1, 0], [0, 0, -1]]), [0, 1, 0, 0])         # 180 degrees about x (trace < 0 branch)
    assert np.allclose(quaternion_wxyz([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), [s, 0, s, 0])          # 90 degrees about y
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    f = camera_frusta([(384, 512)], [192.0], [c2w])[0]
    assert f['fov'] == pytest.approx(math.pi / 2) and f['aspect'] == pytest.approx(512 / 384) and f['position'].tolist() == [1, 2, 3]
    ref = R.frusta([(384, 512)], [192.0], [c2w.numpy()])[0]
    assert f['fov'] == pytest.approx(float(ref['fov'])) and f['aspect'] == ref['aspect']


def test_cpu_tensors_raise():
    from panst3r_amd.engine import panoptic_point_cloud
    x = [{'pts3d': torch.zeros(4, 4, 3), 'pts3d_local': torch.zeros(4, 4, 3), 'conf': torch.ones(4, 4)}]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        panoptic_point_cloud(x, [torch.zeros(3, 4, 4)], [[4, 4]], [torch.zeros(4, 4, dtype=torch.int32)], [], [torch.eye(4)])


def test_header_exports_and_library_agree_on_the_cloud_symbols():
    from panst3r_amd import hip
    from panst3r_amd.build import build
    declared = sorted(p[0] for p in abi_header.prototypes() if p[0].startswith('pst_cloud_'))
    assert declared == CLOUD_SYMBOLS == sorted(s for s in hip.EXPORTS if s.startswith('pst_cloud_'))
    lib = ctypes.CDLL(build(verbose=False))
    for s in declared:
        assert hasattr(lib, s), s
    assert hip.ABI_VERSION == 20
    names = [f[0] for f in abi_header.structs()['pst_cloud_view']]
    assert names == [f[0] for f in hip.CloudView._fields_] and ctypes.sizeof(hip.CloudView) == 104


def test_synthetic_scene_has_the_cases_the_gpu_test_needs():
    """tests/test_hip_cloud.py's scene, at a small size: single-point, even-count and never-kept segments; about half kept at the median confidence"""
    x, im, pan, info, cams = R.synthetic_scene([(48, 64), (64, 48), (48, 64)], seed=1)
    conf = np.concatenate([v['conf'].reshape(-1) for v in x])
    thr = float(np.sort(conf)[len(conf) // 2])
    from panst3r_amd.engine.cloud import default_colors
    c = R.cloud(x, im, pan, info, cams, min_conf_thr=thr, colors=default_colors(len(info) + 1))
    assert 0.3 <= len(c['index']) / len(conf) <= 0.7
    assert np.any(conf == F(thr))
    seg = {s['id']: s['count'] for s in c['segments']}
    assert seg[1] == 1 and seg[2] == 6 and 3 not in seg and len(info) not in seg and len(seg) >= 20
    assert max(seg.values()) >= 10 * min(v for k, v in seg.items() if k > 3)              # very unequal sizes
