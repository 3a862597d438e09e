"""The fused TSDF surface without a GPU: the numpy restatement tests/tsdf_ref.py - the yardstick of tests/test_hip_tsdf.py - held to closed forms, so
that it is not its own judge, and the argument checks of the host API, which need no device."""
import numpy as np
import pytest

import tsdf_ref as T
from panst3r_amd.engine import default_colors

F = np.float32
COLORS = np.asarray(default_colors(4), dtype=F)


def fused(scene, vs, **kw):
    return T.fuse_scene(*scene[:6], vs, COLORS, **kw)


@pytest.fixture(scope='module')
def sphere():
    sc = T.sphere_scene()
    return sc, {band: fused(sc, 0.125, band=band)[0] for band in (1, 2)}


# ---------------------------------------------------------------- the fronto-parallel plane
@pytest.mark.parametrize('band', [1, 2])
@pytest.mark.parametrize('z_plane', [2.0, 2.125])
def test_plane_is_recovered_exactly(z_plane, band):
    """Two cameras on the z axis, at z = 0 and z = -1, see the plane: each measures one constant depth, so S is linear along z and the crossing is
    exact - on a node layer (z = 2: a node with D == 0, which is outside) and between two (z = 2.125)."""
    sc = T.plane_scene(z_plane)
    r, vox, cells = fused(sc, 0.25, band=band)
    assert r['stats']['surface_cells'] == len(r['vertices']) > 0 and len(r['faces']) > 0
    assert (r['vertices'][:, 2] == F(z_plane)).all()
    assert (T.face_normals(r['vertices'], r['faces'])[:, 2] < 0).all()         # towards the cameras
    # within the band every camera whose image contains the node measures it: weight counts images, sdf is the distance to the plane
    want = T.views_containing(r['nodes'], 0.25, sc[4], sc[5], [T.PLANE_SHAPE] * 2, T.PLANE_PP)
    assert np.array_equal(r['weight'], want) and (want == 0).any() and (want == 2).any()
    seen = r['weight'] > 0
    assert np.array_equal(r['sdf'][seen], (F(z_plane) - r['nodes'][seen, 2].astype(F) * F(0.25)).astype(F))
    assert not r['sdf'][~seen].any()
    if z_plane == 2.0:
        assert (r['sdf'][seen] == 0).any()                                     # D == 0 exactly at a node
    assert (r['vertex_ids'] == 1).all() and (r['face_ids'] == 1).all()
    assert T.topology(r['faces'], len(r['vertices'])) == (True, 1, 2)


# ---------------------------------------------------------------- topology
@pytest.mark.parametrize('band', [1, 2])
def test_sphere_is_one_oriented_sheet(sphere, band):
    """naive surface nets does not promise a manifold for arbitrary input: these scenes meet it, which is what the GPU test relies on"""
    r = sphere[1][band]
    Nv = len(r['vertices'])
    assert len(r['faces']) > 200 and T.topology(r['faces'], Nv) == (True, 1, 2)
    n, centre = T.face_normals(r['vertices'], r['faces']), r['vertices'][r['faces']].mean(axis=1)
    assert ((n * centre).sum(axis=1) > 0).all()                                # outwards: from inside to outside, towards the cameras
    radius = np.linalg.norm(r['vertices'], axis=1)
    assert 0.95 < radius.min() and radius.max() < 1.06                         # the sphere of radius 1, within half a cell of 0.125


# ---------------------------------------------------------------- carving
def test_views_that_see_through_a_patch_carve_it_away():
    one = T.carving_scene(False)
    r1 = fused(one, 0.125, band=1)[0]
    near1 = r1['vertices'][:, 2] < 3
    z1 = r1['vertices'][near1, 2]                                              # alone, view 0's patch at z = 2 is a surface: four cells, whose crossings
    assert near1.sum() == 4 and (z1 >= F(2.0)).all() and (z1 <= F(2.125)).all()      # lie in the node layer's cells [2, 2.125] (the rim sees the wall too)
    assert (r1['vertex_ids'][near1] == 2).all()
    three = T.carving_scene(True)
    r3 = fused(three, 0.125, band=1)[0]
    assert not (r3['vertices'][:, 2] < 3).any() and (r3['vertices'][:, 2] == F(4.0)).all() and len(r3['faces']) > 0
    # every node within the band of the patch is in the two other views' images and measured: weight 3, and behind the patch (-s + tau + tau) / 3 > 0
    p = r3['nodes'].astype(np.float64) * 0.125
    # (band 1 around the patch's cells: the node layers z = 2 and z = 2.125, 3 x 3 nodes each)
    at_patch = (np.abs(p[:, 2] - 2.0) <= 0.125) & (np.abs(p[:, 0]) <= 0.25) & (np.abs(p[:, 1]) <= 0.25)
    assert at_patch.sum() == 18 and (r3['weight'][at_patch] == 3).all() and (r3['sdf'][at_patch] > 0).all()
    behind = at_patch & (p[:, 2] == 2.125) & np.isin(p[:, 0], (-0.125, 0.0)) & np.isin(p[:, 1], (-0.125, 0.0))      # on the rays of the patch's pixels 6 .. 9
    assert behind.sum() == 4 and (r3['sdf'][behind] == F((F(-0.125) + F(0.125) + F(0.125)) / F(3))).all()


# ---------------------------------------------------------------- the rules
def test_min_weight_removes_what_one_view_alone_saw():
    sc = T.carving_scene(False)
    assert len(fused(sc, 0.125, band=1, min_weight=1)[0]['faces']) > 0
    r = fused(sc, 0.125, band=1, min_weight=2)[0]
    assert r['stats'] == dict(r['stats'], valid_nodes=0, surface_cells=0) and len(r['faces']) == 0 and len(r['vertices']) == 0
    # two views of the plane: the nodes only one of them holds in its image go, the rest stays
    pl = T.plane_scene(2.0)
    a, b = fused(pl, 0.25, band=1, min_weight=1)[0], fused(pl, 0.25, band=1, min_weight=2)[0]
    assert 0 < b['stats']['valid_nodes'] < a['stats']['valid_nodes'] and b['stats']['valid_nodes'] == int((a['weight'] >= 2).sum())
    assert 0 < len(b['vertices']) <= len(a['vertices'])


def test_canonical_order_of_nodes_vertices_and_faces():
    sc = T.plane_scene(2.125)
    r, vox, cells = fused(sc, 0.25, band=2)
    seen, nodes = {}, []
    for row, c in enumerate(cells.tolist()):                                   # pair order: row, then the offset x fastest
        for oz in range(4):
            for oy in range(4):
                for ox in range(4):
                    n = (c[0] + ox - 1, c[1] + oy - 1, c[2] + oz - 1)
                    if n not in seen:
                        seen[n] = len(nodes)
                        nodes.append(n)
    assert r['nodes'].tolist() == [list(n) for n in nodes]
    assert [seen[tuple(c)] for c in cells.tolist()] == np.nonzero(r['voxel_row'] >= 0)[0][np.argsort(r['voxel_row'][r['voxel_row'] >= 0])].tolist()
    cv = r['cell_vertex'][r['cell_vertex'] >= 0]
    assert cv.tolist() == list(range(len(r['vertices'])))                      # vertices in the rank order of their cells' nodes
    e = r['edge']
    assert (np.diff(e) >= 0).all() and (e[0::2] == e[1::2]).all() and len(np.unique(e)) * 2 == len(e)
    assert (r['faces'][0::2, 0] == r['faces'][1::2, 0]).all()                  # both triangles of an edge start at q0


def test_label_falls_back_to_the_fullest_neighbour():
    sc = T.plane_scene(2.125)
    x, imgs, pan, info, cams, focals = sc
    _, vox, cells = fused(sc, 0.25, band=2)
    Mv = len(cells)
    keep = np.ones(Mv, dtype=bool)
    keep[[2, 5, 6]] = False                                                    # cells that stay surface cells through their neighbours' nodes
    cells2 = cells[keep]
    M2 = len(cells2)
    count = np.array([3 + (k * 7) % 4 for k in range(M2)], dtype=np.int32)     # many ties
    ids = np.arange(1, M2 + 1, dtype=np.int32)
    cols = np.stack([ids, ids, ids], axis=1).astype(F) / F(64)
    r = T.fuse(cells2, count, ids, cols, x, cams, focals, 0.25, band=2)
    row_of = {tuple(c): k for k, c in enumerate(cells2.tolist())}
    fell_back = none = 0
    rows = np.nonzero(r['cell_vertex'] >= 0)[0]
    assert len(rows) == len(r['vertices']) > 0
    for v, node in enumerate(r['nodes'][rows].tolist()):
        w = row_of.get(tuple(node), -1)
        if w < 0:
            cand = [row_of[n] for n in ((node[0] + dx, node[1] + dy, node[2] + dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
                    if n in row_of]
            w = min(cand, key=lambda k: (-int(count[k]), k)) if cand else -1
            fell_back += w >= 0
            none += w < 0
        assert r['vertex_ids'][v] == (ids[w] if w >= 0 else 0)
        assert np.array_equal(r['colors'][v], cols[w] if w >= 0 else np.zeros(3, dtype=F))
    assert fell_back >= 3
    # no voxel at or next to a cell: id 0 and colour 0
    far = T.fuse(cells2[:1], count[:1], ids[:1], cols[:1], x, cams, focals, 0.25, band=4)
    lone = [v for v, node in enumerate(far['nodes'][far['cell_vertex'] >= 0].tolist()) if max(abs(a - b) for a, b in zip(node, cells2[0].tolist())) > 1]
    assert lone and (far['vertex_ids'][lone] == 0).all() and not far['colors'][lone].any()


def test_face_id_is_the_id_two_corners_share():
    a, b, c = np.array([1, 1, 2, 3, 0, 5]), np.array([1, 2, 1, 4, 0, 0]), np.array([2, 1, 1, 5, 7, 5])
    assert T.face_id(a, b, c).tolist() == [1, 1, 1, 0, 0, 5]
    r = fused(T.carving_scene(False), 0.125, band=2)[0]                        # two ids meet where the patch's band touches the wall's
    ids = r['vertex_ids'][r['faces']]
    want = [x if x in (y, z) else (y if y == z else 0) for x, y, z in ids.tolist()]
    assert r['face_ids'].tolist() == want and set(want) >= {1, 2}


def test_a_node_beyond_the_range_raises():
    x, imgs, pan, info, cams, focals = T.plane_scene(2.0)
    with pytest.raises(RuntimeError, match='outside'):
        T.fuse(np.array([[0, 0, 2 ** 20 - 1]]), [1], [1], COLORS[:1], x, cams, focals, 0.25, band=1)
    T.fuse(np.array([[0, 0, 2 ** 20 - 2]]), [1], [1], COLORS[:1], x, cams, focals, 0.25, band=1)


# ---------------------------------------------------------------- the host API's argument checks (no device)
def test_argument_errors_need_no_device():
    import torch
    from panst3r_amd.engine import FusedMesh, PanopticCloud, PanopticMesh, fuse_surface
    from panst3r_amd.engine.tsdf import check_fuse_arguments, fused_mesh_keywords
    assert check_fuse_arguments(0.25) == (0.25, 2, 1)                          # the defaults
    for bad in (0, -1.0, float('nan'), float('inf'), 1e-46, 1e39):
        with pytest.raises(ValueError, match='voxel_size'):
            fuse_surface(None, bad)
    for bad in (0, 5, 1.5, True, None):
        with pytest.raises(ValueError, match='band'):
            fuse_surface(None, 0.1, band=bad)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match='min_weight'):
            fuse_surface(None, 0.1, min_weight=bad)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    cloud = PanopticCloud(z(4, 3), z(4, 3), z(4, 3), z(4, dtype=torch.int32), z(4, 3), z(4, dtype=torch.int64), [0, 4], [])
    with pytest.raises(RuntimeError, match='does not hold its device inputs'):
        cloud.fused_mesh(0.1)
    assert fused_mesh_keywords(None) is None and fused_mesh_keywords(0.05) == {'voxel_size': 0.05}
    assert fused_mesh_keywords({'voxel_size': 0.05, 'band': 1}) == {'voxel_size': 0.05, 'band': 1}
    for bad in ('yes', True, {'band': 2}, {'voxel_size': 0.1, 'bands': 2}, {'voxel_size': 0.1, 'band': 9}, -0.5):
        with pytest.raises(ValueError):
            fused_mesh_keywords(bad)
    # a FusedMesh is a PanopticMesh and keeps its class and its volume through cpu() and a face filter
    e = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype)
    m = FusedMesh(z(2, 3), e(1, 3), e(1), e(2), z(2, 3), e(1, dtype=torch.int64), [0, 4], [], nodes=e(5, 3), sdf=z(5), weight=e(5),
                  tsdf_stats={'active_nodes': 5, 'valid_nodes': 0, 'surface_cells': 2}, voxel_size=0.1, band=2, min_weight=1)
    assert isinstance(m, PanopticMesh) and len(m) == 1
    for other in (m.cpu(), m._with_faces(m.faces[:0], m.face_ids[:0], m.quad[:0])):
        assert type(other) is FusedMesh and other.tsdf_stats == m.tsdf_stats and other.nodes.shape == (5, 3) and (other.band, other.min_weight) == (2, 1)
    assert len(m._with_faces(m.faces[:0], m.face_ids[:0], m.quad[:0])) == 0
