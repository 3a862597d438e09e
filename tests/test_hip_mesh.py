"""The rasterisation of a labelled mesh on the GPU (csrc/mesh.hip, panst3r_amd/engine/mesh.py) against the numpy restatement of tests/mesh_ref.py: every
field of `MeshRender`, and the maps, counts and segments of `ground_truth_maps`, BIT FOR BIT - fixed-point coverage, a depth rounded once from fp64 and
a minimum of integers leave no tolerance to choose.

Conditions, not measurements: before the GPU is compared, `check_conditions` asserts ON THE RESTATEMENT that the scene exercises what it was built for
- empty pixels, pixels with several candidate faces, a duplicated face that loses to its original, faces on both sides of hip.MESH_LANE_PIXELS (one
with exactly that many pixels in its box, one with one more), a nearest-corner tie, the deliberately bad faces left out, and for the area filter one
listed id removed, one kept and one unlisted id voided.  (tests/test_mesh_host.py runs the same check without a GPU.)"""
import functools
import types

import numpy as np
import pytest
import torch

import mesh_ref as M
import render_ref as R
import eval_ref as E
from panst3r_amd import hip
from panst3r_amd.engine import render_mesh, ground_truth_maps, panoptic_quality, render_cloud, MeshRender
from panst3r_amd.engine import mesh as mesh_mod

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(24, 32), (37, 51), (48, 64)]
FIELDS = ('depth', 'face', 'pan')
MIN_AREA = 50                                                                  # the reference's MIN_INST_AREA


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def scene():
    return M.scene()


@functools.lru_cache(maxsize=None)
def reference(shape, ids='vertex'):
    """the restatement's render of the five cameras at one shape (computed once per shape and labelling, shared, never written to)"""
    s = scene()
    kw = {'vertex': dict(vertex_ids=s['vertex_ids']), 'face': dict(face_ids=s['face_ids']), 'none': {}}[ids]
    return M.render(s['vertices'], s['faces'], s['cams'], M.focal_of(shape), shape, **kw)


@functools.lru_cache(maxsize=None)
def reference_gt(aniso=1.0):
    """the restatement's ground truth of the five cameras, shapes mixed (two of them share one)"""
    s = scene()
    cameras = M.camera_dicts(s['cams'], [(48, 64), (37, 51), (48, 64), (24, 32), (37, 51)], aniso)
    return cameras, M.ground_truth(s['vertices'], s['faces'], s['vertex_ids'], s['segments'], cameras, min_area=MIN_AREA)


def check_conditions(want):
    """on the restatement alone, at 48 x 64: the comparison decides what it is meant to decide"""
    s, sp, L = scene(), scene()['special'], hip.MESH_LANE_PIXELS
    face, cand, box = want['face'], want['candidates'], want['box']
    assert (face == -1).any() and (face >= 0).any() and (cand >= 2).any()
    assert (face[4] == -1).all() and (face[3] == -1).any() and (face[3] >= 0).any()       # looking away: empty; outside: the room and empty pixels around it
    assert (want['usable'][0] == 0).sum() > 100                                # camera 0: the faces behind it
    dup = face == sp['original']
    assert dup.any() and (cand[dup] >= 2).all() and not (face == sp['duplicate']).any()   # equal depths: the smaller index
    live = box[box > 0]
    assert (live < L).any() and (live > L + 1).any() and box[0, sp['box64']] == L and box[0, sp['box65']] == L + 1
    assert (face[0] == sp['box64']).any() and (face[0] == sp['box65']).any() and (face == s['special']['tie']).any()
    assert want['ties'].any() and want['ties'][0][face[0] == sp['tie']].any()  # a nearest-corner tie, on the face placed for it
    for name in ('degenerate', 'nan', 'index_high', 'index_negative'):
        assert (box[:, sp[name]] == 0).all() and not (face == sp[name]).any(), name
    assert not want['usable'][0, sp['near']] and not (face[0] == sp['near']).any()        # it straddles camera 0's near plane: left out whole there
    ids = [g['id'] for g in s['segments']]
    out, counts = M.area_filter(want['pan'], ids, MIN_AREA)
    assert ((counts > 0) & (counts < MIN_AREA)).any() and (counts >= MIN_AREA).any()      # a listed id removed, one kept
    assert (want['pan'] == M.UNLISTED).any() and not (out == M.UNLISTED).any()            # an unlisted id voided
    assert (out != want['pan']).any() and (out > 0).any()


@functools.lru_cache(maxsize=None)
def device_mesh():
    s = scene()
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(s[k])).to(device=DEV, dtype=dt)
    return t('vertices', torch.float32), t('faces', torch.int64), t('vertex_ids', torch.int32), t('face_ids', torch.int32)


def assert_same(got, want):
    assert isinstance(got, MeshRender)
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        assert tuple(g.shape) == w.shape and g.cpu().numpy().dtype == w.dtype, (k, tuple(g.shape), w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (k, int((bits(g) != bits(w)).sum()))
    assert np.array_equal(got.hit.cpu().numpy(), want['face'] >= 0)


def assert_equal_renders(a, b):
    for k in FIELDS:
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def render(shape, ids='vertex', **kw):
    v, f, vid, fid = device_mesh()
    lab = {'vertex': dict(vertex_ids=vid), 'face': dict(face_ids=fid), 'none': {}}[ids]
    return render_mesh(v, f, scene()['cams'], M.focal_of(shape), shape, **lab, **kw)


@pytest.mark.parametrize('ids', ['vertex', 'face', 'none'])
@pytest.mark.parametrize('shape', SHAPES)
def test_every_field_equals_the_restatement(shape, ids):
    want = reference(shape, ids)
    if shape == (48, 64):
        check_conditions(reference(shape))
    assert (want['face'] >= 0).any() and (want['candidates'] >= 2).any() and ((want['pan'] == 0).all() if ids == 'none' else (want['pan'] > 0).any())
    got = render(shape, ids)
    assert_same(got, want)
    if ids != 'none':
        assert not np.array_equal(reference(shape, 'vertex')['pan'], reference(shape, 'face')['pan'])       # the two labellings differ somewhere


def test_int32_faces_anisotropic_focals_and_principal_points():
    s, shape = scene(), (37, 51)
    v, f, vid, _ = device_mesh()
    fs, pps = [[25.0, 27.5], [30.0, 22.0], [18.0, 18.0], [26.0, 24.0], [25.0, 25.0]], [(25.5, 18.5), (20.0, 10.0), (30.0, 25.0), (25.0, 18.0), (0.0, 0.0)]
    want = M.render(s['vertices'], s['faces'], s['cams'], fs, shape, vertex_ids=s['vertex_ids'], pp=pps, near=0.3, far=9.0)
    assert (want['face'] >= 0).any() and (want['depth'].max() <= 9.0) and want['depth'][want['face'] >= 0].min() >= np.float32(0.3)
    f32 = torch.where((f < 0) | (f >= len(v)), torch.full_like(f, -7), f).to(torch.int32)
    got = render_mesh(v.double(), f32, torch.from_numpy(np.stack(s['cams'])).to(DEV), torch.tensor(fs), shape, vertex_ids=vid.long(), pp=pps, near=0.3, far=9.0)
    assert_same(got, want)


def test_calls_repeat_and_options_do_not_change_the_result(monkeypatch):
    shape = (48, 64)
    want = reference(shape)
    a, b = render(shape), render(shape)
    assert_same(a, want)
    assert_equal_renders(a, b)                                                 # two calls: identical bytes
    monkeypatch.setattr(hip, 'MESH_PRECHECK', 1 - hip.MESH_PRECHECK)           # with and without the pre-check
    assert_equal_renders(a, render(shape))
    monkeypatch.setattr(mesh_mod, 'ZBUF_BYTES', 2 * 8 * shape[0] * shape[1])   # two cameras per launch: three chunks
    assert_equal_renders(a, render(shape))
    monkeypatch.setattr(hip, 'MESH_BIG_CAPACITY', 3)                           # a list that runs full: the faces beyond it stay with their lanes
    assert (want['box'][:2] > hip.MESH_LANE_PIXELS).sum() > 3                  # ... in the first chunk of two cameras
    assert_equal_renders(a, render(shape))
    monkeypatch.setattr(hip, 'MESH_BIG_CAPACITY', 0)                           # no list at all
    assert_equal_renders(a, render(shape))
    h = a.cpu()
    assert h.face.device.type == 'cpu' and np.array_equal(bits(h.depth), bits(a.depth)) and np.array_equal(bits(a[2].pan), bits(a.pan[2:3]))


def test_a_camera_looking_away_renders_nothing():
    s, shape = scene(), (24, 32)
    v, f, vid, _ = device_mesh()
    want = M.render(s['vertices'], s['faces'], s['cams'][4:], M.focal_of(shape), shape, vertex_ids=s['vertex_ids'])
    assert (want['face'] == -1).all() and (want['depth'] == 0).all() and (want['pan'] == 0).all()
    got = render_mesh(v, f, s['cams'][4:], M.focal_of(shape), shape, vertex_ids=vid)
    assert_same(got, want)


@pytest.mark.parametrize('aniso', [1.0, 1.08])
def test_ground_truth_maps_equal_the_restatement(aniso):
    cameras, (maps, segs, depths, counts) = reference_gt(aniso)
    s = scene()
    assert len({(c['height'], c['width']) for c in cameras}) < len(cameras)    # some cameras share a shape
    ids = [g['id'] for g in s['segments']]
    assert 0 < len(segs) < len(ids) and any(0 < n < MIN_AREA for c in counts for n in c)
    v, f, vid, _ = device_mesh()
    g_maps, g_segs, g_depths = ground_truth_maps(v, f, vid, s['segments'], [dict(c, cam2world=torch.from_numpy(c['cam2world'])) for c in cameras], min_area=MIN_AREA)
    assert g_segs == segs
    for k in range(len(cameras)):
        assert g_maps[k].dtype == torch.int32 and g_maps[k].is_cuda and tuple(g_maps[k].shape) == maps[k].shape
        assert np.array_equal(g_maps[k].cpu().numpy(), maps[k]) and np.array_equal(bits(g_depths[k]), bits(depths[k])), k
    # the counts, through the kernels themselves; and min_area = 0 only removes the unlisted id
    shape = (48, 64)
    r = render(shape)
    want_out, want_counts = M.area_filter(reference(shape)['pan'], ids, MIN_AREA)
    tab = np.full(max(ids) + 1, -1, dtype=np.int32)
    tab[ids] = np.arange(len(ids))
    id2row = torch.from_numpy(tab).to(DEV)
    cnt, out = torch.zeros(5, len(ids), dtype=torch.int32, device=DEV), torch.empty_like(r.pan)
    hip.mesh_area_count(r.pan, id2row, cnt)
    hip.mesh_area_apply(r.pan, id2row, cnt, MIN_AREA, out)
    assert np.array_equal(cnt.cpu().numpy(), want_counts) and np.array_equal(out.cpu().numpy(), want_out)
    hip.mesh_area_apply(r.pan, id2row, cnt, 0, out)
    assert np.array_equal(out.cpu().numpy(), M.area_filter(reference(shape)['pan'], ids, 0)[0])


def test_reconstruct_style_cameras_and_an_empty_segment_list():
    s = scene()
    v, f, vid, _ = device_mesh()
    shapes = [(24, 32), (48, 64)]
    cameras = [{'cam2world': torch.from_numpy(c), 'focal': M.focal_of(sh), 'height': sh[0], 'width': sh[1]} for c, sh in zip(s['cams'][:2], shapes)]
    want = M.ground_truth(s['vertices'], s['faces'], s['vertex_ids'], s['segments'], M.camera_dicts(s['cams'][:2], shapes), min_area=10)
    maps, segs, depths = ground_truth_maps(v, f, s['vertex_ids'], s['segments'], cameras, min_area=10)       # (vertex_ids as a numpy array)
    assert segs == want[1] and all(np.array_equal(m.cpu().numpy(), w) for m, w in zip(maps, want[0]))
    maps, segs, depths = ground_truth_maps(v, f, vid, [], cameras)
    assert segs == [] and all(not m.any() for m in maps) and all(np.array_equal(bits(d), bits(w)) for d, w in zip(depths, want[2]))


def test_the_ground_truth_scores_itself_with_pq_one():
    cameras, (maps, segs, depths, counts) = reference_gt(1.0)
    s = scene()
    v, f, vid, _ = device_mesh()
    gt, gt_segs, _ = ground_truth_maps(v, f, vid, s['segments'], cameras, min_area=MIN_AREA)
    for scope in ('scene', 'view'):
        r = panoptic_quality(gt, gt_segs, gt, gt_segs, scope=scope)
        assert r['pq'] == 1.0 and r['sq'] == 1.0 and r['rq'] == 1.0 and r['miou'] == 1.0 and r['pixel_acc'] == 1.0
        assert r['void_pixels'] == sum(int((m == 0).sum()) for m in maps) > 0


def test_a_splat_of_the_labelled_vertices_scores_against_the_ground_truth():
    """composition with the point renderer: the mesh's own vertices, labelled by vertex_ids, splatted from the same cameras and scored"""
    s, shape = scene(), (48, 64)
    v, f, vid, _ = device_mesh()
    cameras = M.camera_dicts(s['cams'][:3], [shape] * 3)
    gt, gt_segs, _ = ground_truth_maps(v, f, vid, s['segments'], cameras, min_area=MIN_AREA)
    ok = torch.isfinite(v).all(dim=1)
    zeros = torch.zeros(int(ok.sum()), 3, device=DEV)
    cloud = types.SimpleNamespace(points=v[ok], rgb=zeros, colors=zeros, pan=vid[ok])
    pred = render_cloud(cloud, s['cams'][:3], M.focal_of(shape), shape, radius=2)
    r = panoptic_quality(pred.pan, splat_segments(), gt, gt_segs)
    want = splat_reference()
    print('pq %.3f sq %.3f rq %.3f miou %.3f' % (r['pq'], r['sq'], r['rq'], r['miou']))
    assert 0 < r['pq'] <= 1 and 0 < r['miou'] <= 1
    assert r['pq'] == want['pq'] and r['miou'] == want['miou'] and E.totals(r) == E.totals(want)


def splat_segments():
    return [{'id': g['id'], 'category_id': g['category_id'] if 'category_id' in g else g['class_id']} for g in scene()['segments']]


@functools.lru_cache(maxsize=None)
def splat_reference():
    """the same on the restatements alone: render_ref's splat scored by eval_ref against mesh_ref's ground truth"""
    s, shape = scene(), (48, 64)
    maps, segs, _, _ = M.ground_truth(s['vertices'], s['faces'], s['vertex_ids'], s['segments'], M.camera_dicts(s['cams'][:3], [shape] * 3), min_area=MIN_AREA)
    keep = np.isfinite(s['vertices']).all(axis=1)
    z = np.zeros((int(keep.sum()), 3), dtype=np.float32)
    pred = R.render(s['vertices'][keep], z, z, s['vertex_ids'][keep], s['cams'][:3], M.focal_of(shape), shape, radius=2)
    return E.panoptic_quality(list(pred['pan']), splat_segments(), maps, segs)
