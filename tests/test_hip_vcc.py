"""The connected components of the voxel cloud and the label despeckling on the GPU (csrc/components.hip, panst3r_amd/engine/voxels.py) against the numpy
restatement of tests/vcc_ref.py: every output BIT FOR BIT - the stage is integer arithmetic, so there is no tolerance to choose.  The voxel clouds
under test are the product's (`voxelize_cloud`, itself held to tests/voxel_ref.py by test_hip_voxel.py) and, for the adversarial grids, clouds built
by hand through the constructor with `cells`."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref as C
import eval_ref
import tiny
import vcc_ref as R
import voxel_ref as V
from panst3r_amd import hip
from panst3r_amd.engine import VoxelCloud, VoxelComponents, default_colors, voxel_components, clean_voxel_labels
from test_hip_cloud import bits, thresholds
from test_hip_voxel import device_cloud, SIZES, FIELDS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
CONNECTIVITIES = (6, 18, 26)
TABLE = ('pan', 'size', 'points', 'cell_lo', 'cell_hi')
SCENES = {'two_view': dict(shapes=[(24, 32), (24, 32)], seed=2, opacity=0.5, mid=0.5),
          'mixed': dict(shapes=[(48, 64), (64, 48), (37, 51), (48, 64), (30, 43)], seed=3, opacity=0.3, mid=0.25),
          # the two-view scene with id 3 left out of the segment table: its points vote void, so the cloud has void voxels
          'two_view_void': dict(shapes=[(24, 32), (24, 32)], seed=2, opacity=0.5, mid=0.5, drop_id=3)}


def assert_components(got, ref, voxel_size, connectivity):
    assert isinstance(got, VoxelComponents) and len(got) == len(ref['size']) and got.connectivity == connectivity and got.voxel_size == voxel_size
    for k in ('component', 'root') + TABLE:
        g, w = getattr(got, k), ref[k]
        assert tuple(g.shape) == w.shape and g.cpu().numpy().dtype == w.dtype, k
        assert np.array_equal(bits(g), bits(w)), k
    lo, hi = R.boxes(ref, voxel_size)
    assert got.box_lo.dtype == torch.float64 and np.array_equal(bits(got.box_lo), bits(lo)) and np.array_equal(bits(got.box_hi), bits(hi))


def assert_clean(got, ref, ref_segments, vox):
    """the cleaned cloud against the restatement: pan, colors, segments and the two counts; every other field is the input's, the same bytes"""
    assert (got.relabelled, got.floaters) == (ref['relabelled'], ref['floaters'])
    for k in ('pan', 'colors'):
        g, w = getattr(got, k), ref[k]
        assert tuple(g.shape) == w.shape and g.cpu().numpy().dtype == w.dtype and np.array_equal(bits(g), bits(w)), k
    for k in FIELDS + ('cells',):
        if k not in ('pan', 'colors'):
            assert np.array_equal(bits(getattr(got, k)), bits(getattr(vox, k))), k
    assert [s['id'] for s in got.segments] == [s['id'] for s in ref_segments]
    for a, b in zip(got.segments, ref_segments):
        assert a['count'] == b['count'] and (a.get('query_id'), a.get('category_id')) == (b.get('query_id'), b.get('category_id'))
        assert np.array_equal(bits(a['median']), bits(b['median'].astype(F))), (a['id'], a['median'], b['median'])


def assert_equal_clouds(a, b):
    for k in FIELDS + ('cells',):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert (a.relabelled, a.floaters) == (b.relabelled, b.floaters) and len(a.segments) == len(b.segments)
    for s, t in zip(a.segments, b.segments):
        assert (s['id'], s['count']) == (t['id'], t['count']) and np.array_equal(bits(s['median']), bits(t['median']))


@functools.lru_cache(maxsize=None)
def scene_case(name, which, size):
    """one scene at one keep ratio and voxel size: the restatement's cloud, voxels and cells, computed once and left unchanged, and the device voxels"""
    cfg = SCENES[name]
    scene = V.overlapping_scene(cfg['shapes'], seed=cfg['seed'])
    x, im, pan, info, cams, clean = scene
    if cfg.get('drop_id'):
        info = [s for s in info if s['id'] != cfg['drop_id']]
        scene = (x, im, pan, info, cams, clean)
    thr = thresholds(scene)[which]
    colors = default_colors(len(scene[3]) + 2)
    vs = cfg['mid'] if size == 'mid' else SIZES[size]
    rc = C.cloud(x, im, pan, info, cams, min_conf_thr=thr, opacity=cfg['opacity'], colors=colors)
    rv = V.voxelize(rc['points'], rc['rgb'], rc['pan'], rc['index'], [s['id'] for s in rc['segments']], vs, colors, cfg['opacity'])
    cells = R.cells_of(rc['points'], rv, vs)
    vox = device_cloud(scene, thr, cfg['opacity'], colors).voxelize(vs)
    return dict(scene=scene, info=info, colors=colors, vs=vs, opacity=cfg['opacity'], ref_cloud=rc, ref_vox=rv, cells=cells, vox=vox)


def check_scene(name, which, size, min_voxels_list=(1, 2, 4, 'all')):
    case = scene_case(name, which, size)
    rv, cells, vox = case['ref_vox'], case['cells'], case['vox']
    Mv = len(rv['pan'])
    assert len(vox) == Mv and tuple(vox.cells.shape) == (Mv, 3) and vox.cells.dtype == torch.int32
    assert np.array_equal(vox.cells.cpu().numpy(), cells)                      # voxelize_cloud fills the cells
    out = {}
    for conn in CONNECTIVITIES:
        ref = R.components(cells, rv['pan'], rv['count'], conn)
        comps = vox.components(conn)
        assert_components(comps, ref, case['vs'], conn)
        for mv in min_voxels_list:
            m = int(ref['size'].max()) + 1 if mv == 'all' and len(ref['size']) else 5 if mv == 'all' else mv       # 'all': everything is small
            want, want_segments = R.clean(rv, cells, case['ref_cloud']['segments'], case['colors'], m, conn, case['opacity'], comp=ref)
            got = vox.clean_labels(m, conn)
            assert_clean(got, want, want_segments, vox)
            assert np.array_equal(got.point_labels().cpu().numpy(), V.point_labels(want, case['ref_cloud']['pan']))
            maps, want_maps = got.consistent_maps(), V.consistent_maps(want, case['ref_cloud'], case['scene'][2])
            assert len(maps) == len(want_maps) and all(g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w) for g, w in zip(maps, want_maps))
            if mv == 1:
                for k in FIELDS:                                               # min_voxels = 1: the input, byte for byte
                    assert np.array_equal(bits(getattr(got, k)), bits(getattr(vox, k))), k
                assert (got.relabelled, got.floaters) == (0, 0) and len(got.segments) == len(vox.segments)
                assert all(s['count'] == t['count'] and np.array_equal(bits(s['median']), bits(t['median'])) for s, t in zip(got.segments, vox.segments))
            if mv == 'all':
                assert (want['pan'] <= 0).all() and want['floaters'] == int((rv['pan'] > 0).sum()) and want['relabelled'] == 0 and want_segments == []
            out[conn, mv] = (ref, want)
    return case, out


@pytest.mark.parametrize('size', ['mid', 'one', 'alone'])
@pytest.mark.parametrize('which', ['none', 'half', 'all'])
@pytest.mark.parametrize('name', ['two_view', 'mixed'])
def test_small_scenes(name, which, size):
    case, out = check_scene(name, which, size)
    rv = case['ref_vox']
    Mv = len(rv['pan'])
    if which == 'none':
        assert Mv == 0 and all(len(ref['size']) == 0 for ref, _ in out.values())
        return
    ref, want = out[26, 4]
    print('%s / %s / %s: %d voxels, %d components at 26 (%d singletons), min_voxels 4: %d relabelled, %d floaters'
          % (name, which, size, Mv, len(ref['size']), int((ref['size'] == 1).sum()), want['relabelled'], want['floaters']))
    if size == 'one':
        assert Mv == 1 and ref['size'].tolist() == [1] and want['pan'].tolist() == [0]           # alone and small: a floater
    elif size == 'alone':
        # every point its own voxel at a size far below the point spacing: no two voxels touch, every component has size 1
        assert Mv == len(case['ref_cloud']['index']) and all((r['size'] == 1).all() for r, _ in out.values())
    else:
        # the content of the comparison: a component of more than one voxel, a small one that is relabelled, a floater
        assert ref['size'].max() > 1 and want['relabelled'] > 0 and out[6, 4][1]['floaters'] > 0 and (which != 'half' or want['floaters'] > 0)
        assert len(out[6, 4][0]['size']) > len(out[18, 4][0]['size']) >= len(ref['size'])        # more connectivity, fewer components
    if (name, which, size) == ('two_view', 'half', 'mid'):
        assert (Mv, len(ref['size']), int((ref['size'] == 1).sum())) == (485, 94, 75)           # as measured when the stage was proposed


def test_void_voxels_belong_to_no_component_and_are_never_relabelled():
    case, out = check_scene('two_view_void', 'all', 'mid', min_voxels_list=(1, 4))
    rv = case['ref_vox']
    ref, want = out[26, 4]
    void = rv['pan'] <= 0
    assert void.any() and (~void).any() and (ref['root'][void] == -1).all() and (ref['component'][void] == -1).all()
    assert (want['pan'][void] == rv['pan'][void]).all() and want['relabelled'] > 0
    assert ref['size'].sum() == int((~void).sum())


# ---------------------------------------------------------------- adversarial grids, uploaded as voxel clouds built by hand
def grid_cloud(cells, pan, count=None):
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
    n = len(cells)
    count = np.ones(n, dtype=np.int32) if count is None else np.asarray(count, dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pts = cells.astype(F)
    rgb = np.full((n, 3), 0.25, dtype=F)
    return VoxelCloud(t(pts), t(rgb), t(np.asarray(pan, dtype=np.int32)), t(rgb), t(count), t(count), t(np.arange(n, dtype=np.int64)),
                      t(np.arange(n, dtype=np.int32)), [], None, [0, n], 1.0, 0, opacity=0.5, cells=t(cells))


def serpentine(n=100000, width=316):
    """one line of n cells that snakes through the plane z = 0: full rows at even y joined at alternating ends by one cell at odd y"""
    cells, y = [], 0
    while len(cells) < n:
        xs = range(width) if (y // 2) % 2 == 0 else range(width - 1, -1, -1)
        cells += [(x, y, 0) for x in xs]
        cells.append((cells[-1][0], y + 1, 0))
        y += 2
    return np.array(cells[:n])


def grids():
    g = np.random.Generator(np.random.PCG64(9))
    out = {}
    line = serpentine()
    out['serpentine'] = (line[g.permutation(len(line))], np.full(len(line), 5), 50)                 # shuffled rows: the deep-tree case of find
    a = np.arange(64)
    out['solid'] = (np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3), np.full(64 ** 3, 2), 64 ** 3 + 1)
    a = np.arange(32)
    board = np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3)
    out['checkerboard'] = (board, 1 + board.sum(axis=1) % 2, 4)
    a = np.arange(-6, 6)
    cube = np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3)
    keep = g.uniform(0, 1, len(cube)) < 0.6
    cube = cube[keep][g.permutation(int(keep.sum()))]
    out['straddle'] = (cube, g.integers(0, 4, len(cube)), 4)                                         # ids 0 .. 3 around cell 0 on every axis, void among them
    e = (1 << 20) - 1
    a = np.array([0, 1, 2])
    block = np.stack(np.meshgrid(a, a, a, indexing='ij'), axis=-1).reshape(-1, 3)
    ends = np.concatenate([np.array(s) * (e - block) for s in [(1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (1, 1, -1)]])
    ends = np.concatenate([ends, [(e, 0, 0), (-e, 1, 0), (-e, 0, 0), (0, e, -e)]])
    out['ends'] = (ends, g.integers(1, 3, len(ends)), 3)
    return out


GRIDS = None


@pytest.mark.parametrize('name', ['serpentine', 'solid', 'checkerboard', 'straddle', 'ends'])
def test_adversarial_grids(name):
    global GRIDS
    GRIDS = GRIDS or grids()
    cells, pan, min_voxels = GRIDS[name]
    count = 1 + (np.arange(len(cells)) % 7)
    vox = grid_cloud(cells, pan, count)
    old = hip.VCC_MERGE
    try:
        for conn in (6, 26) if name == 'solid' else CONNECTIVITIES:           # (the restatement of 64^3 at 26 takes seconds)
            ref = R.components(cells, pan, count, conn)
            want_pan, moved, gone = R.clean_pan(cells, pan, count, min_voxels, conn, comp=ref)
            n = len(ref['size'])
            if name == 'serpentine':
                assert n == 1 and ref['size'][0] == 100000 and ref['roots'][0] == 0
            elif name == 'solid':
                assert n == 1 and ref['size'][0] == 64 ** 3 and ref['cell_hi'].tolist() == [[63, 63, 63]] and gone == 64 ** 3
            elif name == 'checkerboard':
                assert n == (32 ** 3 if conn == 6 else 2)
                assert gone == (32 ** 3 if conn == 6 else 0)
            else:
                assert n > 1 and ref['size'].max() > 1 and (moved > 0 or name == 'ends')
            results = []
            for merge in (old, 1 - old, old):                                  # two calls with one setting and one with the other: identical bytes
                hip.VCC_MERGE = merge
                comps = vox.components(conn)                                   # (a status word that is not 0 raises)
                assert_components(comps, ref, 1.0, conn)
                cleaned = vox.clean_labels(min_voxels, conn)
                assert np.array_equal(cleaned.pan.cpu().numpy(), want_pan) and (cleaned.relabelled, cleaned.floaters) == (moved, gone)
                results.append((comps, cleaned))
            for comps, cleaned in results[1:]:
                for k in VoxelComponents.FIELDS:
                    assert np.array_equal(bits(getattr(comps, k)), bits(getattr(results[0][0], k))), k
                assert_equal_clouds(cleaned, results[0][1])
    finally:
        hip.VCC_MERGE = old


# ---------------------------------------------------------------- behaviour
def test_despeckling_cleans_the_maps_further_than_the_vote():
    """the behavioural claim: on the 8-view scene with a fifth of every view's pixels relabelled at random, the share of kept pixels that carry the clean
    label is higher by more than 0.05 after clean_labels(4) than after the vote alone (measured when the stage was proposed: 0.9117 -> 0.9893).  Shown
    on the restatement, which the device equals exactly.  Scene-scope PQ of the input, the voted and the cleaned maps against the clean ones is printed;
    the cleaned maps must not score below the voted ones."""
    SCENES['eight_view'] = dict(shapes=[(96, 128)] * 8, seed=7, opacity=0.5, mid=0.1)
    case, out = check_scene('eight_view', 'half', 'mid', min_voxels_list=(4,))
    x, im, pan, info, cams, clean = case['scene']
    rc, rv = case['ref_cloud'], case['ref_vox']
    ref, want = out[26, 4]
    kept = np.zeros(sum(p.size for p in pan), dtype=bool)
    kept[rc['index']] = True
    flat = lambda ms: np.concatenate([np.asarray(m).reshape(-1) for m in ms])
    voted, cleaned = V.consistent_maps(rv, rc, pan), V.consistent_maps(want, rc, pan)
    share = lambda ms: float(np.mean(flat(ms)[kept] == flat(clean)[kept]))
    s_in, s_vote, s_clean = share(pan), share(voted), share(cleaned)
    print('%d voxels, %d components (%d singletons), %d relabelled, %d floaters' % (len(rv['pan']), len(ref['size']), int((ref['size'] == 1).sum()),
                                                                                   want['relabelled'], want['floaters']))
    print('share of kept pixels with the clean label: %.4f in the input maps, %.4f after the vote, %.4f after clean_labels(4)' % (s_in, s_vote, s_clean))
    pq = [eval_ref.panoptic_quality(m, info, clean, info, scope='scene')['pq'] for m in (pan, voted, cleaned)]
    print('scene-scope PQ against the clean maps: %.4f input, %.4f voted, %.4f cleaned' % tuple(pq))
    assert s_clean > s_vote + 0.05
    assert pq[2] >= pq[1]
    assert np.array_equal(flat(cleaned)[~kept], flat(pan)[~kept])              # a pixel below the threshold keeps its 2-D id


def test_reconstruct_with_min_component_voxels_equals_reconstruct_then_clean_labels():
    Vn, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(Vn, H, W)]
    ts = torch.tensor([[H, W]] * Vn)
    kw = dict(min_conf_thr=1.5, opacity=0.4, postprocess_kwargs=dict(cls_threshold=0.0, mask_threshold=0.0, overlap_threshold=0.0), num_keyframes=K, amp='fp16')
    cloud = h.reconstruct(imgs, ts, tiny.NAMES, **kw)[0]
    pts = cloud.points.float().cpu().numpy()
    s = float(np.abs(pts[np.isfinite(pts).all(axis=1)]).max()) / 40 if len(cloud) else 1.0
    plain = h.reconstruct(imgs, ts, tiny.NAMES, voxel_size=s, **kw)
    out = h.reconstruct(imgs, ts, tiny.NAMES, voxel_size=s, min_component_voxels=3, **kw)
    assert len(out) == 4 and len(plain[3]) > 0
    want = plain[3].clean_labels(3)
    assert_equal_clouds(out[3], want)
    print('reconstruct: %d voxels, %d relabelled, %d floaters' % (len(want), want.relabelled, want.floaters))
    # ... and against the restatement, on what the model produced
    vox = plain[3]
    rv = {k: getattr(vox, k).cpu().numpy() for k in FIELDS}
    cells = vox.cells.cpu().numpy()
    colors = default_colors(max([x['id'] for x in out[2][0]['segments_info']] + [1]) + 1)
    ref, ref_segments = R.clean(rv, cells, cloud.segments, colors, 3, 26, 0.4)
    assert_clean(want, ref, ref_segments, vox)
    with pytest.raises(ValueError, match='only together with voxel_size'):
        h.reconstruct(imgs, ts, tiny.NAMES, min_component_voxels=3, **kw)


def test_refusals_and_the_identity():
    case = scene_case('two_view', 'half', 'mid')
    vox = case['vox']
    same = vox.clean_labels(1)
    for k in FIELDS + ('cells',):                                              # min_voxels = 1: the input, byte for byte, in tensors of its own
        assert np.array_equal(bits(getattr(same, k)), bits(getattr(vox, k))), k
    assert same.pan.data_ptr() != vox.pan.data_ptr() and (same.relabelled, same.floaters) == (0, 0)
    before = vox.pan.clone()
    cleaned = clean_voxel_labels(vox, 4)
    assert torch.equal(vox.pan, before) and not torch.equal(cleaned.pan, before)                    # the input is untouched
    assert len(voxel_components(vox, 6)) >= len(voxel_components(vox))
    r = cleaned.render(case['scene'][4][:1], 17.6, (24, 32))                                         # render works on the result unchanged
    hit = (r.index >= 0).cpu().numpy()
    assert hit.any() and np.array_equal(r.pan.cpu().numpy()[hit], cleaned.pan.cpu().numpy()[r.index.cpu().numpy()[hit]])
    for bad in (0, 7, 27, None):
        with pytest.raises(ValueError, match='connectivity'):
            vox.components(bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match='min_voxels'):
            vox.clean_labels(bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vox.cpu().components()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vox.cpu().clean_labels(2)
    by_hand = VoxelCloud(vox.points, vox.rgb, vox.pan, vox.colors, vox.count, vox.votes, vox.first_index, vox.point_voxel, vox.segments, vox.cameras,
                         vox.view_offsets, vox.voxel_size, vox.dropped)
    with pytest.raises(RuntimeError, match='does not hold the cells'):
        by_hand.components()
    # two voxels in one cell are not a voxel cloud: the device reports it, the host raises
    twice = grid_cloud([(0, 0, 0), (1, 0, 0), (0, 0, 0)], [1, 1, 1])
    with pytest.raises(RuntimeError, match='share one cell'):
        twice.components()
    with pytest.raises(RuntimeError, match='outside'):
        grid_cloud([(0, 0, 0), (1 << 20, 0, 0)], [1, 1]).components()
