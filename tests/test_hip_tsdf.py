"""The fused TSDF surface on the GPU (csrc/tsdf.hip, panst3r_amd/engine/tsdf.py) against the numpy restatement of tests/tsdf_ref.py, BIT FOR BIT:
nodes, sdf, weight, vertices, vertex ids, colours, faces, face ids, edge keys and the stats - the stage is compares, integer ranks, separately rounded
fp32 operations and fp64 crossings in a stated order, so there is no tolerance to choose.  (tests/test_tsdf_host.py holds the restatement to closed
forms.)  The shapes are those at which the loops can go wrong, not the workload's."""
import functools

import numpy as np
import pytest
import torch

import consistency_ref as R
import surface_ref
import tiny
import tsdf_ref as T
from panst3r_amd import hip
from panst3r_amd.engine import FusedMesh, PanopticMesh, VoxelCloud, default_colors, fuse_surface, load_ply_mesh, panoptic_point_cloud, score_reconstruction

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
COLORS = np.asarray(default_colors(5), dtype=F)
INFO = [{'id': i, 'query_id': i - 1, 'category_id': i} for i in (1, 2, 3)]
SAME, MIXED = [(5, 7)] * 3, [(5, 7), (6, 4), (9, 3)]
THR, VS = 1.2, 0.2


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, dtype, what):
    want = np.ascontiguousarray(np.asarray(want).astype(dtype, copy=False))
    assert tuple(got.shape) == want.shape and got.cpu().numpy().dtype == want.dtype, (what, tuple(got.shape), want.shape)
    bad = np.nonzero((bits(got) != bits(want)).reshape(len(want), -1).any(axis=1))[0] if want.size else []
    assert len(bad) == 0, '%s: %d of %d rows differ, first at %d: got %r, want %r' % (what, len(bad), len(want), bad[0], got.cpu().numpy()[bad[0]], want[bad[0]])


def assert_fused(mesh, ref):
    assert isinstance(mesh, FusedMesh) and isinstance(mesh, PanopticMesh)
    assert mesh.tsdf_stats == ref['stats'], (mesh.tsdf_stats, ref['stats'])
    for got, key, dtype in ((mesh.nodes, 'nodes', np.int32), (mesh.sdf, 'sdf', F), (mesh.weight, 'weight', np.int32), (mesh.vertices, 'vertices', F),
                            (mesh.vertex_ids, 'vertex_ids', np.int32), (mesh.colors, 'colors', F), (mesh.faces, 'faces', np.int32),
                            (mesh.face_ids, 'face_ids', np.int32), (mesh.quad, 'edge', np.int64)):
        same_bits(got, ref[key], dtype, key)


def rotated(shapes, seed=3):
    x, cams, focals, pan = R.rotated_scene(shapes, seed=seed, spread=0.1)
    return x, [np.zeros((3,) + s, dtype=F) for s in shapes], pan, INFO, cams, focals


def device_cloud(sc, thr=THR, local_pointmaps=False, colors=COLORS):
    x, imgs, pan, info, cams, focals = sc[:6]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return panoptic_point_cloud([{k: put(v) for k, v in d.items()} for d in x], [put(i) for i in imgs], None, [put(p) for p in pan], info,
                                [torch.from_numpy(np.asarray(c)) for c in cams], focals, min_conf_thr=thr, colors=colors, local_pointmaps=local_pointmaps)


def reference(sc, vs, thr=THR, **kw):
    return T.fuse_scene(*sc[:6], vs, COLORS, min_conf_thr=thr, **kw)


@functools.lru_cache(maxsize=None)
def sphere():
    sc = T.sphere_scene()
    return sc, reference(sc, 0.1, 3.0, band=2)[0]


# ---------------------------------------------------------------- small and mixed shapes
@pytest.mark.parametrize('band', [1, 2])
@pytest.mark.parametrize('shapes', [SAME, MIXED], ids=['5x7', 'mixed'])
def test_small_views_equal_the_restatement(shapes, band):
    sc = rotated(shapes)
    ref = reference(sc, VS, band=band)[0]
    assert len(ref['faces']) > 50 and {0, 1, 2, 3} == set(ref['face_ids'].tolist()) and (ref['weight'] == 0).any() and (ref['weight'] == 3).any()
    assert_fused(device_cloud(sc).fused_mesh(VS, band=band), ref)


def test_local_pointmaps_and_min_weight():
    sc = rotated(MIXED)
    ref = reference(sc, VS, band=2, min_weight=2, local_pointmaps=True)[0]
    assert len(ref['faces']) > 20 and 0 < ref['stats']['valid_nodes'] < int((ref['weight'] >= 1).sum())
    cloud = device_cloud(sc, local_pointmaps=True)
    assert_fused(cloud.fused_mesh(VS, band=2, min_weight=2), ref)
    assert_fused(fuse_surface(cloud, VS, band=2, min_weight=2, vox=cloud.voxelize(VS)), ref)        # with the voxels given


def test_principal_point_and_near_plane():
    sc = rotated(SAME, seed=4)
    kw = dict(band=1, pp=(3.0, 2.0), near=1.9)
    ref = reference(sc, VS, **kw)[0]
    assert ref['stats']['valid_nodes'] > 0
    assert_fused(device_cloud(sc).fused_mesh(VS, **kw), ref)


# ---------------------------------------------------------------- the scan's workgroup edges, the table at its smallest capacity
def strip_voxels(n_cells, vs):
    """a VoxelCloud built by hand: n_cells cells in a row along x through the plane's node layer (z index 8 at vs = 0.25), with counts and ids of
    their own; at band 1 they have 4 (n_cells + 1) nodes"""
    cells = np.stack([np.arange(n_cells) - n_cells // 2, np.zeros(n_cells, dtype=np.int64), np.full(n_cells, 8)], axis=1)
    count = (1 + np.arange(n_cells) % 3).astype(np.int32)
    pan = (1 + np.arange(n_cells) % 4).astype(np.int32)
    colors = (np.arange(3 * n_cells).reshape(n_cells, 3) / F(3 * n_cells)).astype(F)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    z3 = torch.zeros(n_cells, 3, device=DEV)
    vox = VoxelCloud(z3, z3, put(pan), put(colors), put(count), put(count), torch.zeros(n_cells, dtype=torch.int64, device=DEV),
                     torch.zeros(0, dtype=torch.int32, device=DEV), [], None, [0], vs, 0, cells=put(cells.astype(np.int32)))
    return vox, cells, count, pan, colors


@pytest.mark.parametrize('n_cells', [254, 255, 256])
def test_nodes_around_one_scan_workgroup(n_cells):
    """1020, 1024 and 1028 active nodes: just under, exactly and just over the 1024 nodes of one workgroup of the scans; at 256 cells the table
    has its smallest legal capacity, twice the 2048 pairs, so that probes wrap"""
    sc = T.plane_scene(2.0)
    x, imgs, pan, info, cams, focals = sc
    vox, cells, count, vpan, vcol = strip_voxels(n_cells, 0.25)
    ref = T.fuse(cells, count, vpan, vcol, x, cams, focals, 0.25, band=1)
    assert ref['stats']['active_nodes'] == 4 * (n_cells + 1) and len(ref['vertices']) > 2          # (one row of cells: vertices, no faces)
    if n_cells == 256:
        assert hip.tsdf_capacity(n_cells, 1) == 2 * hip.tsdf_pairs(n_cells, 1) == 4096
    mesh = fuse_surface(device_cloud(sc, 3.0), 0.25, band=1, vox=vox)
    assert_fused(mesh, ref)
    assert (mesh.vertices[:, 2] == 2.0).all() and (mesh.sdf == 0).any()        # D == 0 exactly at a node, the crossing exactly on the plane


def test_more_than_one_workgroup_of_nodes_vertices_and_faces():
    sc, ref = sphere()
    assert ref['stats']['active_nodes'] > 4096 and len(ref['vertices']) > 1024 and len(ref['faces']) > 2048
    assert T.topology(ref['faces'], len(ref['vertices'])) == (True, 1, 2)
    mesh = device_cloud(sc, 3.0).fused_mesh(0.1)                               # band 2 is the default
    assert_fused(mesh, ref)
    again = device_cloud(sc, 3.0).fused_mesh(0.1)                              # two calls return equal bytes
    for k in ('nodes', 'sdf', 'weight', 'vertices', 'vertex_ids', 'colors', 'faces', 'face_ids', 'quad'):
        assert np.array_equal(bits(getattr(mesh, k)), bits(getattr(again, k))), k


# ---------------------------------------------------------------- views that see nothing, non-finite inputs, a filtered cloud
def test_blind_views_and_non_finite_inputs():
    shapes = [(5, 7), (6, 4), (9, 3), (5, 7), (4, 6)]
    x, imgs, pan, info, cams, focals = rotated(shapes, seed=6)
    x = [{k: v.copy() for k, v in d.items()} for d in x]
    x[3]['conf'][:] = 1.0                                                      # a view with no measured pixel
    cams[4] = cams[4] @ np.diag([-1.0, 1.0, -1.0, 1.0])                        # a view that looks the other way: every node is behind it
    rng = np.random.default_rng(5)
    for d in x[:3]:
        H, W = d['conf'].shape
        for val in (np.nan, np.inf, -np.inf, 3e38):
            for key in ('pts3d', 'pts3d_local'):
                d[key].reshape(-1, 3)[rng.integers(0, H * W, 2), rng.integers(0, 3, 2)] = val
        d['conf'].reshape(-1)[rng.integers(0, H * W, 2)] = np.nan
    sc = (x, imgs, pan, info, cams, focals)
    for local in (False, True):
        ref = reference(sc, VS, band=2, local_pointmaps=local)[0]
        assert len(ref['faces']) > 20 and np.isfinite(ref['sdf']).all() and ref['weight'].max() <= 4
        assert_fused(device_cloud(sc, local_pointmaps=local).fused_mesh(VS), ref)


def test_a_filtered_cloud_with_nan_confidences():
    sc = rotated(MIXED)
    x, imgs, pan, info, cams, focals = sc
    keep = R.keep(R.consistency(x, cams, focals, min_conf_thr=THR, rel_tol=0.1), 1, 1)
    assert 0 < keep.sum() < len(keep)
    masked, a = [], 0
    for d in x:
        n = d['conf'].size
        masked.append(dict(d, conf=np.where(keep[a:a + n].reshape(d['conf'].shape), d['conf'], F(np.nan)).astype(F)))
        a += n
    ref = reference((masked,) + tuple(sc[1:]), VS, band=1)[0]
    assert len(ref['faces']) > 0
    assert_fused(device_cloud(sc).filter_consistent(1, 1, rel_tol=0.1).fused_mesh(VS, band=1), ref)


# ---------------------------------------------------------------- the empty results, the range, refusals
def test_empty_results_and_errors():
    sc = rotated(SAME)
    cloud = device_cloud(sc)
    nothing = device_cloud(sc, thr=1e9).fused_mesh(VS)                        # an empty cloud
    assert isinstance(nothing, FusedMesh) and len(nothing) == 0 and nothing.tsdf_stats == {'active_nodes': 0, 'valid_nodes': 0, 'surface_cells': 0}
    assert nothing.vertices.shape == (0, 3) and nothing.nodes.shape == (0, 3) and nothing.render([np.eye(4)], 8.0, (4, 5)).depth.shape == (1, 4, 5)
    flat = cloud.fused_mesh(VS, band=1, min_weight=4)                          # three views: no node is valid, no surface cell
    ref = reference(sc, VS, band=1, min_weight=4)[0]
    assert len(flat) == 0 and flat.tsdf_stats['valid_nodes'] == 0 and flat.tsdf_stats['active_nodes'] > 0
    assert_fused(flat, ref)
    assert len(flat.drop_small(2)) == 0
    vox = cloud.voxelize(VS)
    vox.cells = vox.cells.clone()
    vox.cells[1, 2] = 2 ** 20 - 1                                              # its upper nodes lie at 2^20
    with pytest.raises(RuntimeError, match='outside'):
        fuse_surface(cloud, VS, band=1, vox=vox)
    vox.cells = None
    with pytest.raises(RuntimeError, match='cells'):
        fuse_surface(cloud, VS, vox=vox)
    with pytest.raises(ValueError, match='voxel_size'):
        fuse_surface(cloud, VS, vox=cloud.voxelize(0.3))
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        cloud.cpu().fused_mesh(VS)
    x, imgs, pan, info, cams, focals = sc
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    no_focals = panoptic_point_cloud([{k: put(v) for k, v in d.items()} for d in x], [put(i) for i in imgs], None, [put(p) for p in pan], info,
                                     [torch.from_numpy(np.asarray(c)) for c in cams], min_conf_thr=THR, colors=COLORS)
    with pytest.raises(ValueError, match='focals'):
        no_focals.fused_mesh(VS)


def test_launchers_refuse_bad_arguments():
    cells = torch.zeros(4, 3, dtype=torch.int32, device=DEV)
    ws = hip.tsdf_workspace(4, 1, DEV)
    p = lambda t: t.data_ptr()
    good = [p(cells), 4, 1, p(ws['keys']), ws['cap'], p(ws['first']), p(ws['point_slot']), p(ws['status'])]

    def refused(at, value, match):
        a = list(good)
        a[at] = value
        with pytest.raises(RuntimeError, match=match):
            hip._call('pst_tsdf_insert', *a)
    for at, value in ((1, 0), (2, 0), (2, 5), (1, 2 ** 28), (4, 32), (4, 96)):
        refused(at, value, 'bad shape')
    for at in (0, 3, 5, 6, 7):
        refused(at, None, 'null operand')
    nodes = torch.zeros(8, 3, dtype=torch.int32, device=DEV)
    f8, i8 = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='min_weight'):
        hip._call('pst_tsdf_cells', p(nodes), 8, p(ws['keys']), ws['cap'], p(ws['slot_rank']), p(f8), p(i8), 0, p(i8), p(i8), p(ws['status']))
    with pytest.raises(RuntimeError, match='bad shape'):
        hip._call('pst_tsdf_cells', p(nodes), 8, p(ws['keys']), 8, p(ws['slot_rank']), p(f8), p(i8), 1, p(i8), p(i8), p(ws['status']))
    with pytest.raises(RuntimeError, match='null operand'):
        hip._call('pst_tsdf_integrate', p(nodes), 8, 0.1, 1, None, p(f8), p(i8), 1, p(f8), p(f8), p(i8))
    with pytest.raises(RuntimeError, match='voxel size'):
        hip._call('pst_tsdf_integrate', p(nodes), 8, float('nan'), 1, p(f8), p(f8), p(i8), 1, p(f8), p(f8), p(i8))
    torch.cuda.synchronize()
    assert int(ws['status'].abs().sum()) == 0 and int((ws['keys'] != -1).sum()) == 0      # nothing was launched


# ---------------------------------------------------------------- through the existing consumers
def test_render_ply_islands_and_score_take_the_fused_mesh(tmp_path):
    sc, ref = sphere()
    mesh = device_cloud(sc, 3.0).fused_mesh(0.1)
    # render: the mesh rasteriser on the restated mesh
    cam, f, shape = sc[4][1], 30.0, (24, 32)
    want = surface_ref.render(ref['vertices'], ref, [cam], f, shape)
    assert (want['face'] >= 0).sum() > 50
    got = mesh.render([cam], f, shape)
    for k in ('depth', 'face', 'pan'):
        assert np.array_equal(bits(getattr(got, k)), bits(want[k])), k
    # write_ply -> load_ply_mesh
    v, fc = load_ply_mesh(mesh.write_ply(str(tmp_path / 'fused.ply')))
    assert np.array_equal(bits(v), bits(ref['vertices'])) and np.array_equal(fc.numpy(), ref['faces'].astype(np.int64))
    # islands: the sphere is one component; a filter keeps the class and the volume
    comp = mesh.face_component()
    assert np.array_equal(comp.cpu().numpy(), surface_ref.face_component(ref['faces'], len(ref['vertices'])))
    kept = mesh.drop_small(2)
    want_kept = surface_ref.drop_small({'faces': ref['faces'], 'face_ids': ref['face_ids'], 'quad': ref['edge']}, len(ref['vertices']), 2)
    assert type(kept) is FusedMesh and kept.tsdf_stats == mesh.tsdf_stats and len(kept) == len(want_kept['faces']) > 0
    assert np.array_equal(kept.faces.cpu().numpy(), want_kept['faces']) and np.array_equal(kept.quad.cpu().numpy(), want_kept['quad'])
    assert len(mesh.drop_small(10 ** 6)) == 0 and type(mesh.cpu()) is FusedMesh
    # score_reconstruction: the same call on a PanopticMesh of the same arrays
    plain = PanopticMesh(mesh.vertices, mesh.faces, mesh.face_ids, mesh.vertex_ids, mesh.colors, mesh.quad, list(mesh.view_offsets), mesh.segments, mesh.cameras)
    gv, gf = mesh.vertices * 1.01, mesh.faces.long()
    kw = dict(thresholds=(0.02, 0.05), spacing=0.05, metric='surface')
    a, b = score_reconstruction(mesh, gv, gf, **kw), score_reconstruction(plain, gv, gf, **kw)
    assert a['fscore'] == b['fscore'] and a['accuracy_mean'] == b['accuracy_mean'] and a['completeness_mean'] == b['completeness_mean'] and a['fscore'][-1] > 0.9


def test_reconstruct_opt_in_is_the_direct_call_and_off_by_default():
    """(the tiny model's seeded random weights give focals of 0, with which nothing projects - tests/test_hip_consistency.py meets the same: the
    opt-in reaches `fuse_surface` with the cloud's own cameras and is refused there exactly as the direct call is; the fusion itself is tested above)"""
    V, K, H, W = 5, 3, 64, 96
    h = tiny.build(tiny.hip_ns(), 'v2').to(DEV)
    imgs = [i.to(DEV) for i in tiny.images(V, H, W)]
    ts = torch.tensor([[H, W]] * V)
    kw = dict(min_conf_thr=1.5, opacity=0.4, postprocess_kwargs=dict(cls_threshold=0.0, mask_threshold=0.0, overlap_threshold=0.0), num_keyframes=K, amp='fp16')
    for bad in ('yes', True, {'band': 2}, -1.0, {'voxel_size': 0.1, 'band': 7}, {'voxel_size': 0.1, 'min_weight': 0}):
        with pytest.raises(ValueError, match='fused_mesh|voxel_size|band|min_weight'):
            h.reconstruct(imgs, ts, tiny.NAMES, fused_mesh=bad, **kw)          # before the forward pass
    plain = h.reconstruct(imgs, ts, tiny.NAMES, **kw)
    off = h.reconstruct(imgs, ts, tiny.NAMES, fused_mesh=None, voxel_size=0.5, **kw)
    assert len(plain) == 3 and len(off) == 4 and isinstance(off[3], VoxelCloud)                       # None: what it always returned
    for k in ('points', 'points_local', 'rgb', 'pan', 'colors', 'index'):
        assert np.array_equal(bits(getattr(plain[0], k)), bits(getattr(off[0], k))), k
    assert any(float(c['focal']) == 0 for c in plain[1])
    with pytest.raises(ValueError, match='focals must be one positive finite number') as direct:
        plain[0].fused_mesh(0.5, band=1)
    with pytest.raises(ValueError, match='focals must be one positive finite number') as opted:
        h.reconstruct(imgs, ts, tiny.NAMES, fused_mesh={'voxel_size': 0.5, 'band': 1}, **kw)
    assert str(direct.value) == str(opted.value)
