"""The cross-view depth consistency on the GPU (csrc/consistency.hip, panst3r_amd/engine/consistency.py) against the numpy restatement of
tests/consistency_ref.py: agree, violate, same_label and the bits of depth, BIT FOR BIT - the stage is compares, integer counts and separately
rounded fp32 operations, so there is no tolerance to choose.  The shapes are those at which the code can go wrong, not the workload's: pixel counts
that are no multiple of 4 or of the 1024-pixel workgroup, more than one workgroup per view, planes that start off a 16-byte boundary."""
import numpy as np
import pytest
import torch

import cloud_ref
import consistency_ref as R
import tiny
from panst3r_amd import hip
from panst3r_amd.engine import panoptic_point_cloud, view_consistency

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
MIXED = [(5, 7), (8, 12), (33, 40)]


def off16(a):
    """the array on the device, its first element 4 bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=DEV)
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def to_dev(x, pan=None, misalign=False):
    put = off16 if misalign else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return [{k: put(v) for k, v in d.items()} for d in x], None if pan is None else [put(p) for p in pan]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_same(vc, ref):
    for k in ('depth', 'agree', 'violate', 'same_label'):
        got, want = getattr(vc, k), ref[k]
        if want is None:
            assert got is None, k
            continue
        assert tuple(got.shape) == want.shape and got.cpu().numpy().dtype == want.dtype, k
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert len(bad) == 0, '%s: %d of %d differ, first at %d: got %r, want %r' % (k, len(bad), len(want), bad[0], got.cpu().numpy()[bad[0]], want[bad[0]])


def run(x, cams, focals, pan=None, misalign=False, **kw):
    ref = R.consistency(x, cams, focals, pan=pan, **kw)
    xd, pd = to_dev(x, pan, misalign)
    vc = view_consistency(xd, [torch.from_numpy(np.asarray(c)) for c in cams], focals, pan=pd, **kw)
    assert_same(vc, ref)
    return vc, ref


def median_conf(x):
    return float(np.sort(np.concatenate([v['conf'].reshape(-1) for v in x]))[sum(v['conf'].size for v in x) // 2])


@pytest.fixture(scope='module')
def mixed():
    return R.rotated_scene(MIXED, seed=3)


@pytest.mark.parametrize('local_pointmaps', [False, True])
@pytest.mark.parametrize('labels', [False, True])
def test_mixed_shapes_rotated_cameras(mixed, local_pointmaps, labels):
    """35, 96 and 1320 pixels: no multiple of 4 or 1024, two workgroups for the last view, every plane 4 bytes off a 16-byte boundary"""
    x, cams, focals, pan = mixed
    _, ref = run(x, cams, focals, pan if labels else None, misalign=True, min_conf_thr=median_conf(x), rel_tol=0.1, local_pointmaps=local_pointmaps)
    N = sum(h * w for h, w in MIXED)
    live = ref['depth'] != 0
    assert 0.3 * N <= live.sum() <= 0.7 * N                                   # "about half" measured something
    assert ref['agree'].max() >= 2 and ref['violate'].max() >= 1 and (ref['agree'][live] == 0).any() and not ref['agree'][~live].any()
    if labels:                                                                # void ids, equal and unequal labels all occur among the agreeing pairs
        s = ref['same_label']
        assert (s > 0).any() and (s < ref['agree']).any() and (np.concatenate([p.reshape(-1) for p in pan]) == 0).any()


def test_everything_kept_and_rel_tol_zero(mixed):
    x, cams, focals, pan = mixed
    lowest = float(min(v['conf'].min() for v in x))
    _, ref = run(x, cams, focals, pan, min_conf_thr=lowest, rel_tol=0.25)
    assert (ref['depth'] != 0).all()
    _, ref0 = run(x, cams, focals, pan, min_conf_thr=lowest, rel_tol=0.0)     # only exact equality agrees: everything seen is nearer or farther
    assert ref0['agree'].sum() <= ref['agree'].sum() and ref0['violate'].sum() > ref['violate'].sum()


def test_single_view_sees_nothing():
    x, cams, focals, pan = R.rotated_scene([(33, 40)], seed=5)
    vc, ref = run(x, cams, focals, pan, min_conf_thr=1.5, rel_tol=0.1)
    assert not ref['agree'].any() and not ref['violate'].any() and not ref['same_label'].any() and (ref['depth'] != 0).any()
    assert [tuple(m.shape) for m in vc.maps('depth')] == [(33, 40)]


def test_targets_behind_and_points_nearer_than_near():
    """a camera that looks the other way (every point behind it), one pushed forward past the wall, and a near plane inside the depth range"""
    x, cams, focals, pan = R.rotated_scene([(20, 31), (17, 23), (20, 31), (9, 14)], seed=7)
    back = np.diag([-1.0, 1.0, -1.0, 1.0])                                    # half a turn about y
    cams[1] = cams[1] @ back
    x[1]['pts3d'] = cloud_ref.geotrf(cams[1].astype(F)[:3, :4], x[1]['pts3d_local'].reshape(-1, 3)).reshape(17, 23, 3)
    cams[3][2, 3] = 3.5                                                       # beyond the wall (z <= 2.7): the other views' points are behind it
    x[3]['pts3d'] = cloud_ref.geotrf(cams[3].astype(F)[:3, :4], x[3]['pts3d_local'].reshape(-1, 3)).reshape(9, 14, 3)
    for near in (1e-3, 1.9):
        for local in (False, True):
            _, ref = run(x, cams, focals, pan, min_conf_thr=1.2, rel_tol=0.1, local_pointmaps=local, near=near)
            d = ref['depth']
            assert (d[(d != 0)] >= F(near)).all() and (d != 0).any()
    assert (d == 0).sum() > 0.2 * len(d)                                      # near = 1.9 cuts into the wall


def test_non_finite_points_and_confidences(mixed):
    x, cams, focals, pan = mixed
    x = [{k: v.copy() for k, v in d.items()} for d in x]
    rng = np.random.default_rng(11)
    for d in x:
        H, W = d['conf'].shape
        for val in (np.nan, np.inf, -np.inf, 3e38):
            for key in ('pts3d', 'pts3d_local'):
                k = rng.integers(0, H * W, 3)
                d[key].reshape(-1, 3)[k, rng.integers(0, 3, 3)] = val
        d['conf'].reshape(-1)[rng.integers(0, H * W, 4)] = np.nan
        d['conf'].reshape(-1)[rng.integers(0, H * W, 2)] = np.inf
    for local in (False, True):
        _, ref = run(x, cams, focals, pan, min_conf_thr=1.3, rel_tol=0.1, local_pointmaps=local)
        assert np.isfinite(ref['depth']).all()
        conf = np.concatenate([d['conf'].reshape(-1) for d in x])
        assert not ref['depth'][np.isnan(conf)].any()


def test_projections_onto_the_image_border():
    x, cams, focals, idx, inside = R.border_scene()
    vc, ref = run(x, cams, focals, min_conf_thr=3.0, rel_tol=0.0, pp=(4.0, 3.0))
    assert vc.agree.cpu().numpy()[idx].tolist() == [int(s) for s in inside]
    assert vc.same_label is None


def test_tolerance_edges_on_the_device():
    zs = np.array([2.5, np.nextafter(F(2.5), F(np.inf)), 1.5, np.nextafter(F(1.5), F(-np.inf))], dtype=F)
    x, cams, focals = R.edge_scene(zs)
    vc, _ = run(x, cams, focals, min_conf_thr=3.0, rel_tol=0.25, pp=(2.0, 1.0))
    assert vc.agree.cpu().numpy()[:4].tolist() == [1, 0, 1, 0] and vc.violate.cpu().numpy()[:4].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize('floaters', [False, True])
@pytest.mark.parametrize('local_pointmaps', [False, True])
def test_plane_scenes_against_their_closed_forms(floaters, local_pointmaps):
    x, cams, focals, pan = R.plane_scene(floaters)
    agree, violate = R.plane_closed_form(floaters)
    vc, _ = run(x, cams, focals, pan, min_conf_thr=3.0, rel_tol=0.01, local_pointmaps=local_pointmaps, pp=R.PLANE_PP)
    assert np.array_equal(vc.agree.cpu().numpy(), agree) and np.array_equal(vc.violate.cpu().numpy(), violate)
    assert np.array_equal(vc.same_label.cpu().numpy(), agree)
    assert vc.keep().cpu().numpy().tolist() == ((agree >= 1) & (violate == 0)).tolist()


def test_two_calls_return_equal_bytes(mixed):
    x, cams, focals, pan = mixed
    xd, pd = to_dev(x, pan)
    a = view_consistency(xd, cams, focals, pan=pd, min_conf_thr=1.5, rel_tol=0.1)
    b = view_consistency(xd, cams, focals, pan=pd, min_conf_thr=1.5, rel_tol=0.1)
    for k in ('depth', 'agree', 'violate', 'same_label'):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k


def test_launchers_refuse_bad_arguments_and_launch_nothing(mixed):
    from panst3r_amd.engine.consistency import own_camera_table
    x, cams, focals, pan = mixed
    xd, pd = to_dev(x, pan)
    views = [(d['conf'], d['pts3d'], d['pts3d_local'], p) for d, p in zip(xd, pd)]
    c34 = [np.asarray(c, dtype=F)[:3, :4] for c in cams]
    table, camd, dims, nwg, N = hip.consist_view_table(views, c34, own_camera_table(cams, focals, MIXED), MIXED, DEV)
    V = len(MIXED)
    assert nwg == 4 and N == 35 + 96 + 1320
    depth = torch.full((N,), -7.0, dtype=torch.float32, device=DEV)
    out = [torch.full((N,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    p = lambda t: t.data_ptr()
    good_d = [p(table), p(camd), V, nwg, N, 1.5, 0, p(depth)]
    good_c = [p(table), p(camd), p(dims), V, nwg, N, 0.1, 0, p(depth), p(out[0]), p(out[1]), p(out[2])]

    def refused(what, good, at, value, match):
        a = list(good)
        a[at] = value
        with pytest.raises(RuntimeError, match=match):
            hip._call(what, *a)
    for at, value in ((2, 0), (2, 65536), (4, 0), (4, 2 ** 31), (3, 0), (3, N + 1)):
        refused('pst_consist_depth', good_d, at, value, 'bad shape')
    for at in (0, 1, 7):
        refused('pst_consist_depth', good_d, at, None, 'null operand')
    for at, value in ((3, 0), (3, 65536), (5, 0), (5, 2 ** 31), (4, 0), (4, N + 1)):
        refused('pst_consist_count', good_c, at, value, 'bad shape')
    for value in (float('nan'), float('inf'), 1.0, -0.01, -float('inf')):
        refused('pst_consist_count', good_c, 6, value, 'rel_tol')
    for at in (0, 1, 2, 8, 9, 10):
        refused('pst_consist_count', good_c, at, None, 'null operand')
    torch.cuda.synchronize()
    assert (depth == -7.0).all() and all((t == -7).all() for t in out)        # nothing was launched
    hip._call('pst_consist_depth', *good_d)                                   # ... and the same arguments, unspoilt, are accepted
    hip._call('pst_consist_count', *good_c)
    ref = R.consistency(x, cams, focals, pan=pan, min_conf_thr=1.5, rel_tol=0.1)
    assert np.array_equal(bits(depth), bits(ref['depth'])) and np.array_equal(out[0].cpu().numpy(), ref['agree'])
    assert np.array_equal(out[1].cpu().numpy(), ref['violate']) and np.array_equal(out[2].cpu().numpy(), ref['same_label'])


# ---------------------------------------------------------------- the filter on a cloud
def floater_cloud_inputs():
    x, cams, focals, pan = R.plane_scene(floaters=True)
    rng = np.random.default_rng(2)
    for d in x:
        d['conf'] = rng.uniform(3.5, 6.0, d['conf'].shape).astype(F)          # all above the threshold 3 of the closed form, spread for rethreshold
    imgs = [rng.uniform(-1, 1, (3,) + R.PLANE_SHAPE).astype(F) for _ in x]
    ids = sorted(set(np.concatenate([p.reshape(-1) for p in pan]).tolist()))
    info = [{'id': int(i), 'query_id': k, 'category_id': int(i) % 3} for k, i in enumerate(ids)]
    return x, imgs, pan, info, cams, focals


def ref_filtered_cloud(x, imgs, pan, info, cams, keep, thr, colors):
    """tests/cloud_ref.py's cloud of the scene whose rejected pixels have no confidence"""
    masked, a = [], 0
    for d in x:
        n = d['conf'].size
        masked.append(dict(d, conf=np.where(keep[a:a + n].reshape(d['conf'].shape), d['conf'], F(np.nan)).astype(F)))
        a += n
    with np.errstate(invalid='ignore'):
        return cloud_ref.cloud(masked, imgs, pan, info, cams, min_conf_thr=thr, opacity=0.5, colors=colors)


def assert_cloud(cloud, ref):
    assert len(cloud) == len(ref['index'])
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        assert np.array_equal(bits(getattr(cloud, k)), bits(ref[k])), k
    assert [(s['id'], s['count']) for s in cloud.segments] == [(s['id'], s['count']) for s in ref['segments']]
    for a, b in zip(cloud.segments, ref['segments']):
        assert np.array_equal(bits(a['median']), bits(b['median'].astype(F))), a['id']


def test_filter_consistent_on_the_floater_scene():
    from panst3r_amd.engine import default_colors
    x, imgs, pan, info, cams, focals = floater_cloud_inputs()
    colors = default_colors(max(s['id'] for s in info) + 1)
    xd, pd = to_dev(x, pan)
    imd = [torch.from_numpy(i).to(DEV) for i in imgs]
    camd = [torch.from_numpy(c) for c in cams]
    cloud = panoptic_point_cloud(xd, imd, None, pd, info, camd, focals, min_conf_thr=3.0, colors=colors)
    N = 4 * 24 * 32
    assert len(cloud) == N
    res = R.consistency(x, cams, focals, min_conf_thr=3.0, rel_tol=0.01)      # pp defaults to the centre (16, 12)
    agree, violate = R.plane_closed_form(floaters=True)
    assert np.array_equal(res['agree'], agree) and np.array_equal(res['violate'], violate)
    keep = R.keep(res, 1, 0)
    assert 0 < keep.sum() < N
    vc = cloud.consistency(rel_tol=0.01)
    assert np.array_equal(vc.agree.cpu().numpy(), agree) and np.array_equal(vc.violate.cpu().numpy(), violate) and vc.same_label is not None
    before = [d['conf'].clone() for d in xd]
    filt = cloud.filter_consistent(rel_tol=0.01)
    index = cloud.index.cpu().numpy()
    assert np.array_equal(filt.index.cpu().numpy(), index[keep[index]])      # the unfiltered rows minus exactly the rejected ones
    assert_cloud(filt, ref_filtered_cloud(x, imgs, pan, info, cams, keep, 3.0, colors))
    assert all(torch.equal(a.view(torch.int32), d['conf'].view(torch.int32)) for a, d in zip(before, xd))      # the caller's planes are untouched
    patch = np.zeros((4, 24, 32), dtype=bool)
    patch[0][R.PATCH] = True
    gone = np.setdiff1d(index, filt.index.cpu().numpy())
    assert np.isin(np.nonzero(patch.reshape(-1) & (violate > 0))[0], gone).all()
    for thr in (4.5, 1.0):                                                    # stricter and laxer: it stays filtered
        again = filt.rethreshold(thr)
        assert_cloud(again, ref_filtered_cloud(x, imgs, pan, info, cams, keep, thr, colors))
    assert len(filt.rethreshold(1.0)) == keep.sum() and len(cloud.rethreshold(1.0)) == N
    loose = cloud.filter_consistent(min_views=0, max_violations=1, rel_tol=0.01)
    assert np.array_equal(loose.index.cpu().numpy(), index[R.keep(res, 0, 1)[index]])
    mesh = filt.mesh()
    faces = mesh.faces.cpu().numpy()
    assert len(faces) > 0 and faces.min() >= 0 and faces.max() < len(filt)
    vox = filt.voxelize(0.05)
    assert 0 < len(vox) <= len(filt) and int(vox.count.sum()) + vox.dropped == len(filt)
    r = filt.render(camd[:1], focals[0], R.PLANE_SHAPE)
    assert r.hit.any()
    # the opt-in of panoptic_point_cloud is the same filter
    opt = panoptic_point_cloud(xd, imd, None, pd, info, camd, focals, min_conf_thr=3.0, colors=colors, consistency={'rel_tol': 0.01})
    assert_cloud(opt, ref_filtered_cloud(x, imgs, pan, info, cams, keep, 3.0, colors))
    with pytest.raises(ValueError, match='focals'):
        panoptic_point_cloud(xd, imd, None, pd, info, camd, min_conf_thr=3.0, colors=colors, consistency=True)
    with pytest.raises(ValueError, match='focals'):
        panoptic_point_cloud(xd, imd, None, pd, info, camd, min_conf_thr=3.0, colors=colors).consistency(rel_tol=0.01)
    with pytest.raises(ValueError, match='min_views'):
        cloud.filter_consistent(min_views=-1, rel_tol=0.01)
    with pytest.raises(ValueError, match='rel_tol'):
        cloud.filter_consistent(rel_tol=1.0)
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        cloud.cpu().filter_consistent(rel_tol=0.01)


def equal_clouds(a, b):
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert [(s['id'], s['count']) for s in a.segments] == [(s['id'], s['count']) for s in b.segments]
    for s, t in zip(a.segments, b.segments):
        assert np.array_equal(bits(s['median']), bits(t['median']))


def test_default_off_changes_nothing():
    x, imgs, pan, info, cams, focals = floater_cloud_inputs()
    xd, pd = to_dev(x, pan)
    imd = [torch.from_numpy(i).to(DEV) for i in imgs]
    camd = [torch.from_numpy(c) for c in cams]
    a = panoptic_point_cloud(xd, imd, None, pd, info, camd, focals, min_conf_thr=4.0)
    b = panoptic_point_cloud(xd, imd, None, pd, info, camd, focals, min_conf_thr=4.0, consistency=None)
    equal_clouds(a, b)
    assert len(a) < 4 * 24 * 32


def test_reconstruct_default_off():
    """(the opt-in itself is `panoptic_point_cloud`'s, tested above: the tiny model's seeded random weights give focals of 0, with which nothing projects)"""
    V, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    kw = dict(min_conf_thr=1.5, opacity=0.4, postprocess_kwargs=dict(cls_threshold=0.0, mask_threshold=0.0, overlap_threshold=0.0), num_keyframes=K, amp='fp16')
    plain = h.reconstruct(imgs, ts, tiny.NAMES, **kw)
    off = h.reconstruct(imgs, ts, tiny.NAMES, consistency=None, **kw)
    assert len(plain) == len(off) == 3
    equal_clouds(plain[0], off[0])
    for p, q in zip(plain[2][0]['pan'], off[2][0]['pan']):
        assert torch.equal(p, q)
    with pytest.raises(ValueError, match='consistency'):
        h.reconstruct(imgs, ts, tiny.NAMES, consistency='yes', **kw)
