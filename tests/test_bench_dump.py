"""bench.py --dump-outputs: the sample of a scene's outputs is float32, fixed from run to run, within 64 MB at the benchmark's own size, and the same
whatever rank holds a view.  Fake outputs in the shapes SceneRunner.results returns (no GPU, no model work)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)                  # top level defines functions / constants only
    return m


def _scene(views, H, W, Q=200, seed=0):
    g = torch.Generator().manual_seed(seed)
    res = {i: (torch.randn(1, H, W, 7, generator=g), torch.randn(1, Q, H // 2, W // 2, generator=g)) for i in views}
    return res, {'pred_logits': torch.randn(1, Q, 101, generator=g), 'out_queries': torch.randn(Q, 1, 768, generator=g)}


def test_small_scene_is_written_whole(tmp_path):
    b = _bench()
    res, scene = _scene(range(3), 64, 96)
    shapes = b.write_outputs(str(tmp_path), *b.output_sample(res, scene))
    assert shapes == {'pred_logits': [1, 200, 101], 'out_queries': [200, 1, 768], 'pointmaps': [3, 64 * 96, 7], 'pred_masks': [3, 200, 32 * 48]}
    pm = np.load(tmp_path / 'pointmaps.npy')
    assert pm.dtype == np.float32 and np.array_equal(pm[1], res[1][0].reshape(-1, 7).numpy())
    assert np.array_equal(np.load(tmp_path / 'pred_masks.npy')[2], res[2][1][0].reshape(200, -1).numpy())


def test_benchmark_size_sample_is_fixed_and_bounded(tmp_path):
    """50 views at 384 x 512 (2 GB of mask logits): a seeded pixel sample, within 64 MB, the same bytes from run to run and on any rank layout
    (the views share one tensor pair here: the sample size depends on the number of views only)"""
    b = _bench()
    V, H, W = 50, 384, 512
    one, scene = _scene([0], H, W)
    res = {i: one[0] for i in range(V)}
    blobs = []
    for layout in ([range(V)], [range(0, V, 2), range(1, V, 2)]):          # one rank | views split over two ranks
        views = {}
        for part in layout:
            views.update(b.output_sample({i: res[i] for i in part}, scene, n_views=V)[1])
        d = tmp_path / str(len(layout))
        b.write_outputs(str(d), b.output_sample({}, scene, n_views=V)[0], views)
        names = sorted(os.listdir(d))
        assert names == ['out_queries.npy', 'pointmaps.npy', 'pred_logits.npy', 'pred_masks.npy']
        assert sum(os.path.getsize(d / f) for f in names) <= 64 << 20
        arrays = {f: np.load(d / f) for f in names}
        assert all(a.dtype == np.float32 for a in arrays.values())
        pm, mk = arrays['pointmaps.npy'], arrays['pred_masks.npy']
        assert pm.shape[0] == V and pm.shape[2] == 7 and 1000 < pm.shape[1] < H * W
        assert mk.shape[:2] == (V, 200) and 100 < mk.shape[2] < H * W // 4
        blobs.append({f: open(d / f, 'rb').read() for f in names})
    assert blobs[0] == blobs[1]


def test_sample_positions_do_not_depend_on_values_or_layout():
    b = _bench()
    V, H, W = 50, 384, 512
    idx = torch.arange(H * W * 7, dtype=torch.float32).reshape(1, H, W, 7)           # value = flat position: the sample shows which positions it took
    midx = torch.arange(200 * (H // 2) * (W // 2), dtype=torch.float32).reshape(1, 200, H // 2, W // 2)
    _, scene = _scene([], H, W)
    a = b.output_sample({3: (idx, midx), 4: (idx, midx)}, scene, n_views=V)[1]
    c = b.output_sample({3: (idx * 1, midx * 1)}, scene, n_views=V)[1]
    assert np.array_equal(a[3][0], c[3][0]) and np.array_equal(a[3][1], c[3][1])      # view 3 alone or beside view 4: same positions
    assert not np.array_equal(a[3][0], a[4][0])                                          # other views: other pixels
    assert np.all(np.diff(a[3][0][:, 0]) > 0)                                            # sorted pixel order, all 7 channels of a pixel kept
    assert np.array_equal(a[3][0][:, 1:] - a[3][0][:, :1], np.tile(np.arange(1, 7, dtype=np.float32), (len(a[3][0]), 1)))
