"""numpy restatement of the fused TSDF surface (panst3r_amd/engine/tsdf.py, csrc/tsdf.hip), the yardstick the kernels are held to bit for bit, and
the closed-form scenes that hold the restatement itself (tests/test_tsdf_host.py).

Own design (the reference has no such stage).  The five steps of the contract in include/panst3r_hip.h:
  1 nodes      node n in Z^3 at p = float32(n) * vs, vs = float32(voxel_size).  Per occupied cell c the (2 band)^3 nodes c - band + 1 <= n <= c + band
               are active; pair = row (2 band)^3 + offset, offset x fastest; a node's rank is the order of its smallest pair.  voxel_row: the voxel
               whose cell is the node.  A node outside +-2^20 is an error.
  2 integrate  views in ascending order; consistency_ref.project (finite, zc >= near, |u|, |v| <= 2^20, nearest pixel centre, in the image);
               d = depth_j there, 0 = unseen; s = d - zc; tau = float32(band) * vs; s < -tau: occluded; else S += min(s, tau), W += 1;
               sdf = S / float32(W) (0 where W = 0); valid iff W >= min_weight; inside iff sdf < 0.
  3 cells      surface cell: eight corners active, valid, mixed sides.  Vertex = the mean of the edge crossings in float64, edges in the order axis x,
               y, z and (b, c) offsets 00, 10, 01, 11; t = Da / (Da - Db) in float64; vertex = float32((c + mean) * float64(vs)).
  4 labels     the voxel of the cell, else the fullest voxel among the 26 neighbouring cells (ties to the smaller row), else id 0 and colour 0.
  5 faces      per lattice edge (node, axis) between valid nodes of different sides whose four cells are surface cells: two triangles, normals from
               inside to outside; face id = the id two corners share, else 0; key 3 rank + axis; order rank, axis, first before second.
Elementwise float32 numpy rounds every operation on its own, which is what the kernels promise; the float64 sums are taken in the stated order.
`fuse` = NodeTable -> `integrate` -> `extract`; `integrate_planes` (step 2 on depth planes and dims as given) and `extract` (steps 3 - 5 on a field as
given) are the stages on their own, which tests/tsdf_stage_cases.py feeds by hand."""
import numpy as np

import cloud_ref
import consistency_ref
import voxel_ref

F = np.float32
LIM = 1 << 20


def keys_of(n):
    n = np.asarray(n, dtype=np.int64) + LIM
    return n[..., 0] | (n[..., 1] << 21) | (n[..., 2] << 42)


class NodeTable:
    """the active nodes in canonical order, and the rank of any node (-1: not active)"""

    def __init__(self, cells, band):
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
        side = 2 * band
        o = np.arange(side ** 3)
        offs = np.stack([o % side, (o // side) % side, o // (side * side)], axis=1) - band + 1              # offset x fastest
        pairs = (cells[:, None, :] + offs[None]).reshape(-1, 3)                                              # pair = row (2 band)^3 + offset
        if len(pairs) and (np.abs(pairs) >= LIM).any():
            raise RuntimeError('a lattice node lies outside +-2^20')
        k = keys_of(pairs)
        self.sorted_keys, first = np.unique(k, return_index=True)
        order = np.argsort(first, kind='stable')
        self.rank_of_sorted = np.empty(len(first), dtype=np.int64)
        self.rank_of_sorted[order] = np.arange(len(first))
        self.nodes = pairs[first[order]]
        self.voxel_row = np.full(len(self.nodes), -1, dtype=np.int64)
        r = self.rank(cells)
        assert (r >= 0).all() and len(np.unique(r)) == len(r), 'cells must be unique per voxel'
        self.voxel_row[r] = np.arange(len(cells))

    def __len__(self):
        return len(self.nodes)

    def rank(self, n):
        n = np.asarray(n, dtype=np.int64)
        ok = (np.abs(n) < LIM).all(axis=-1)
        k = keys_of(np.where(ok[..., None], n, 0))
        if len(self.sorted_keys) == 0:
            return np.full(k.shape, -1, dtype=np.int64)
        i = np.minimum(np.searchsorted(self.sorted_keys, k), len(self.sorted_keys) - 1)
        return np.where(ok & (self.sorted_keys[i] == k), self.rank_of_sorted[i], -1)


def integrate_planes(nodes, cam_table, depths, dims, npix, voxel_size, band):
    """step 2 on depth planes as they are given: cam_table float32 [V, 16], depths = one float32 plane per view (its first H W values are the image),
    dims int [V, 2] = (H, W), npix int [V] = the length of each plane.  A view with H W > npix or a dim < 1 takes no part.
    -> (sdf float32 [Nn], weight int32 [Nn])"""
    vs = F(voxel_size)
    tau = F(F(band) * vs)
    p = (np.asarray(nodes).reshape(-1, 3).astype(F) * vs).astype(F)
    S, W = np.zeros(len(p), dtype=F), np.zeros(len(p), dtype=np.int32)
    for j in range(len(dims)):
        H, Wd = int(dims[j][0]), int(dims[j][1])
        if H < 1 or Wd < 1 or H * Wd > int(npix[j]):
            continue
        depth = np.asarray(depths[j], dtype=F).reshape(-1)
        inside, cell, zc = consistency_ref.project(p, cam_table[j], H, Wd)
        with np.errstate(over='ignore', invalid='ignore'):
            d = np.where(inside, depth[cell], F(0)).astype(F)
            s = (d - zc).astype(F)
            use = inside & (d != 0) & ~(s < -tau)
            S = np.where(use, (S + np.minimum(s, tau)).astype(F), S)
        W += use
    with np.errstate(divide='ignore', invalid='ignore'):
        sdf = np.where(W > 0, (S / W.astype(F)).astype(F), F(0)).astype(F)
    return sdf, W


def integrate(nodes, x_out, cams2world, focals, voxel_size, min_conf_thr, band, local_pointmaps=False, pp=None, near=1e-3):
    """-> (sdf float32 [Nn], weight int32 [Nn])"""
    shapes = [tuple(x['conf'].shape) for x in x_out]
    tab = consistency_ref.camera_tables(cams2world, focals, shapes, pp, near)
    world = consistency_ref.world_points(x_out, cams2world, local_pointmaps)
    depths = [consistency_ref.own_depth(world[j], x_out[j]['conf'], tab[j], min_conf_thr) for j in range(len(shapes))]
    return integrate_planes(nodes, tab, depths, shapes, [H * Wd for H, Wd in shapes], voxel_size, band)


CORNERS = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)])                                      # x fastest
EDGE_CELLS = [(0, 0), (-1, 0), (-1, -1), (0, -1)]                                                           # q0 .. q3 in (b, c)


def surface_cells(tab, sdf, weight, min_weight):
    """-> (is a surface cell bool [Nn], corner ranks int64 [Nn, 8])"""
    q = np.stack([tab.rank(tab.nodes + c) for c in CORNERS], axis=1) if len(tab) else np.zeros((0, 8), dtype=np.int64)
    ok = (q >= 0).all(axis=1)
    qq = np.maximum(q, 0)
    ok &= (weight[qq] >= min_weight).all(axis=1)
    inside = (sdf[qq] < 0).sum(axis=1)
    return ok & (inside > 0) & (inside < 8), q


def cell_vertices(cells_c, D, voxel_size):
    """cells_c int [n, 3], D float32 [n, 8] (corner k = x + 2 y + 4 z) -> float32 [n, 3]"""
    n = len(cells_c)
    total, num = np.zeros((n, 3), dtype=np.float64), np.zeros(n, dtype=np.int64)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for e in range(4):
            ob, oc = e & 1, e >> 1
            lo = (ob << b) | (oc << c)
            hi = lo | (1 << a)
            Da, Db = D[:, lo].astype(np.float64), D[:, hi].astype(np.float64)
            cross = (D[:, lo] < 0) != (D[:, hi] < 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                t = Da / (Da - Db)
            pos = np.zeros((n, 3), dtype=np.float64)
            pos[:, a], pos[:, b], pos[:, c] = t, float(ob), float(oc)
            total = np.where(cross[:, None], total + pos, total)
            num += cross
    mean = total / np.maximum(num, 1).astype(np.float64)[:, None]
    return ((np.asarray(cells_c, dtype=np.float64) + mean) * np.float64(F(voxel_size))).astype(F)


def vertex_voxels(tab, cell_rows, count):
    """the voxel row of every surface cell (cell_rows: the ranks of their nodes), -1 for none"""
    own = tab.voxel_row[cell_rows]
    best, best_n = np.full(len(cell_rows), -1, dtype=np.int64), np.zeros(len(cell_rows), dtype=np.int64)
    for d in range(27):
        if d == 13:
            continue
        g = tab.rank(tab.nodes[cell_rows] + np.array([d % 3 - 1, (d // 3) % 3 - 1, d // 9 - 1]))
        w = np.where(g >= 0, tab.voxel_row[np.maximum(g, 0)], -1)
        n = np.where(w >= 0, np.asarray(count, dtype=np.int64)[np.maximum(w, 0)], 0)
        take = (w >= 0) & ((best < 0) | (n > best_n) | ((n == best_n) & (w < best)))
        best, best_n = np.where(take, w, best), np.where(take, n, best_n)
    return np.where(own >= 0, own, best)


def face_id(a, b, c):
    return np.where((a == b) | (a == c), a, np.where(b == c, b, 0)).astype(np.int32)


def build_faces(tab, sdf, weight, min_weight, cell_vertex, vertex_ids):
    """-> (faces int32 [F, 3], face_ids int32 [F], edge int64 [F])"""
    Nn = len(tab)
    valid, inside = weight >= min_weight, sdf < 0
    rows, tris = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = np.zeros(3, dtype=np.int64)
        e[a] = 1
        g = tab.rank(tab.nodes + e) if Nn else np.zeros(0, dtype=np.int64)
        gg = np.maximum(g, 0)
        emit = valid & (g >= 0) & valid[gg] & (inside != inside[gg])
        v = []
        for ob, oc in EDGE_CELLS:
            o = np.zeros(3, dtype=np.int64)
            o[b], o[c] = ob, oc
            h = tab.rank(tab.nodes + o) if Nn else np.zeros(0, dtype=np.int64)
            cv = np.where(h >= 0, cell_vertex[np.maximum(h, 0)], -1)
            emit &= cv >= 0
            v.append(cv)
        r = np.nonzero(emit)[0]
        v = [x[r] for x in v]
        ins = inside[r]
        first = np.stack([v[0], np.where(ins, v[1], v[2]), np.where(ins, v[2], v[1])], axis=1)
        second = np.stack([v[0], np.where(ins, v[2], v[3]), np.where(ins, v[3], v[2])], axis=1)
        rows.append(np.repeat(3 * r + a, 2))
        tris.append(np.stack([first, second], axis=1).reshape(-1, 3))
    edge = np.concatenate(rows).astype(np.int64)
    faces = np.concatenate(tris).astype(np.int32)
    order = np.argsort(edge, kind='stable')                                                                  # rank, axis; first before second
    edge, faces = edge[order], faces[order]
    ids = np.asarray(vertex_ids, dtype=np.int32)
    fid = face_id(ids[faces[:, 0]], ids[faces[:, 1]], ids[faces[:, 2]]) if len(faces) else np.zeros(0, dtype=np.int32)
    return faces.reshape(-1, 3), fid, edge


def fuse(cells, count, pan, colors, x_out, cams2world, focals, voxel_size, min_conf_thr=3.0, band=2, min_weight=1, local_pointmaps=False, pp=None, near=1e-3):
    """cells int [Mv, 3], count, pan int [Mv], colors float32 [Mv, 3] of the voxels; the views as consistency_ref.consistency takes them.
    -> dict(nodes int32 [Nn, 3], sdf, weight, voxel_row, vertices, vertex_ids, colors, faces, face_ids, edge, cell_vertex, stats)"""
    tab = NodeTable(cells, band)
    sdf, weight = integrate(tab.nodes, x_out, cams2world, focals, voxel_size, min_conf_thr, band, local_pointmaps, pp, near)
    return extract(tab, sdf, weight, min_weight, count, pan, colors, voxel_size)


WG_NODES = 1024                                                                                              # nodes per workgroup of the count / emit kernels


def extract(tab, sdf, weight, min_weight, count, pan, colors, voxel_size):
    """steps 3 - 5 on a field as it is given: sdf float32 [Nn], weight int [Nn] on the nodes of `tab`; count, pan int [Mv], colors float32 [Mv, 3] of
    the voxels.  -> the dict of `fuse`, and with it what the kernels hand from stage to stage: is_cell bool [Nn], cell_counts and face_counts int64
    [ceil(Nn / 1024)] (the surface cells and the faces per 1024 nodes in rank order), face_mask int32 [Nn] (bit a: the edge from the node along
    axis a emits its two triangles)"""
    Nn = len(tab)
    sdf, weight = np.asarray(sdf, dtype=F), np.asarray(weight)
    is_cell, q = surface_cells(tab, sdf, weight, min_weight)
    rows = np.nonzero(is_cell)[0]
    cell_vertex = np.full(Nn, -1, dtype=np.int64)
    cell_vertex[rows] = np.arange(len(rows))
    vertices = cell_vertices(tab.nodes[rows], sdf[q[rows]].reshape(-1, 8), voxel_size)
    w = vertex_voxels(tab, rows, count)
    pan, colors = np.asarray(pan, dtype=np.int32), np.asarray(colors, dtype=F).reshape(-1, 3)
    vertex_ids = np.where(w >= 0, pan[np.maximum(w, 0)] if len(pan) else 0, 0).astype(np.int32)
    vcol = np.where((w >= 0)[:, None], colors[np.maximum(w, 0)] if len(pan) else F(0), F(0)).astype(F).reshape(-1, 3)
    faces, face_ids, edge = build_faces(tab, sdf, weight, min_weight, cell_vertex, vertex_ids)
    stats = {'active_nodes': Nn, 'valid_nodes': int((weight >= min_weight).sum()), 'surface_cells': len(rows)}
    nwg = (Nn + WG_NODES - 1) // WG_NODES
    face_mask = np.zeros(Nn, dtype=np.int32)
    np.bitwise_or.at(face_mask, edge // 3, (1 << (edge % 3)).astype(np.int32))
    return {'nodes': tab.nodes.astype(np.int32), 'sdf': sdf, 'weight': weight.astype(np.int32), 'voxel_row': tab.voxel_row, 'vertices': vertices,
            'vertex_ids': vertex_ids, 'colors': vcol, 'faces': faces, 'face_ids': face_ids, 'edge': edge, 'cell_vertex': cell_vertex, 'stats': stats,
            'is_cell': is_cell, 'cell_counts': np.bincount(rows // WG_NODES, minlength=nwg), 'face_counts': np.bincount(edge // 3 // WG_NODES, minlength=nwg),
            'face_mask': face_mask}


def voxel_cells(points, voxel_size, point_voxel, Mv):
    """int64 [Mv, 3]: the cell of every voxel of voxel_ref.voxelize (the cell of its points)"""
    _, c, keep = voxel_ref.cells(points, voxel_size)
    out = np.zeros((Mv, 3), dtype=np.int64)
    pv = np.asarray(point_voxel)
    out[pv[keep]] = c[keep].astype(np.int64)
    return out


def fuse_scene(x_out, imgs, pan, info, cams2world, focals, voxel_size, colors, min_conf_thr=3.0, opacity=0.5, local_pointmaps=False, **kw):
    """cloud_ref.cloud -> voxel_ref.voxelize -> fuse: what `cloud.fused_mesh(voxel_size, **kw)` computes.  -> (fused dict, voxel dict, cells)"""
    with np.errstate(invalid='ignore'):
        cl = cloud_ref.cloud(x_out, imgs, pan, info, cams2world, min_conf_thr=min_conf_thr, opacity=opacity, colors=colors, local_pointmaps=local_pointmaps)
        vox = voxel_ref.voxelize(cl['points'], cl['rgb'], cl['pan'], cl['index'], [s['id'] for s in info], voxel_size, colors, opacity)
    cells = voxel_cells(cl['points'], voxel_size, vox['point_voxel'], len(vox['pan']))
    return fuse(cells, vox['count'], vox['pan'], vox['colors'], x_out, cams2world, focals, voxel_size, min_conf_thr, local_pointmaps=local_pointmaps, **kw), vox, cells


# ---------------------------------------------------------------- checks on a mesh
def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def topology(faces, Nv):
    """(every index < Nv and no face repeats a vertex, the largest number of times a directed edge occurs, ... an undirected edge occurs)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return True, 0, 0
    sane = bool((f >= 0).all() and (f < Nv).all() and (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all())
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = np.unique(d[:, 0] * Nv + d[:, 1], return_counts=True)[1].max()
    u = np.sort(d, axis=1)
    undirected = np.unique(u[:, 0] * Nv + u[:, 1], return_counts=True)[1].max()
    return sane, int(directed), int(undirected)


# ---------------------------------------------------------------- closed-form scenes: everything exact in float32
def ray_view(H, W, f, pp, z, t=(0.0, 0.0, 0.0), conf=5.0):
    """a view with identity rotation at position t whose pixel (y, x) sees the camera-frame depth z[y, x] along its own ray -> (x_out entry, cam2world)"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (H, W))
    loc = np.stack([(xs - pp[0]) * z / f, (ys - pp[1]) * z / f, z], axis=-1)
    c = np.eye(4)
    c[:3, 3] = t
    pts = loc + np.asarray(t, dtype=np.float64)
    return {'pts3d': pts.astype(F), 'pts3d_local': loc.astype(F), 'conf': np.full((H, W), conf, dtype=F)}, c


PLANE_F, PLANE_SHAPE, PLANE_PP = 64.0, (24, 32), (16.0, 12.0)


def plane_scene(z_plane=2.0, cam_z=(0.0, -1.0)):
    """cameras on the z axis at cam_z, identity rotation, looking at the plane z = z_plane: the measured depth of camera j is z_plane - cam_z[j]
    everywhere, exactly.  One segment, id 1.  -> (x_out, imgs, pan, info, cams2world, focals)"""
    H, W = PLANE_SHAPE
    x_out, cams = [], []
    for cz in cam_z:
        x, c = ray_view(H, W, PLANE_F, PLANE_PP, z_plane - cz, (0.0, 0.0, cz))
        x_out.append(x); cams.append(c)
    imgs = [np.zeros((3, H, W), dtype=F) for _ in cam_z]
    pan = [np.ones((H, W), dtype=np.int32) for _ in cam_z]
    return x_out, imgs, pan, [{'id': 1, 'query_id': 0, 'category_id': 1}], cams, [PLANE_F] * len(cam_z)


def views_containing(nodes, voxel_size, cams2world, focals, shapes, pp):
    """int [Nn]: the number of cameras (identity rotation) in front of the node whose image contains its nearest pixel centre, in float64"""
    p = np.asarray(nodes, dtype=np.float64) * float(F(voxel_size))
    n = np.zeros(len(p), dtype=np.int64)
    for c, f, (H, W) in zip(cams2world, focals, shapes):
        q = p - np.asarray(c)[:3, 3]
        with np.errstate(divide='ignore', invalid='ignore'):
            u, v = f * q[:, 0] / q[:, 2] + pp[0], f * q[:, 1] / q[:, 2] + pp[1]
            px, py = np.floor(u + 0.5), np.floor(v + 0.5)
        n += (q[:, 2] > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    return n


def carving_scene(extra_views):
    """View 0 (16 x 16, f = 32, at the origin) sees a wall at z = 4 and, in its middle 4 x 4 pixels, a patch at z = 2 in front of it.  With
    `extra_views`, two more views from x = -+1 at the same height whose every pixel measures the wall at z = 4: they look past where the patch
    would be, see the wall through it, and their images (64 x 64, f = 32, pp at the centre) hold every node near the patch.
    -> (x_out, imgs, pan, info, cams2world, focals, shapes, the patch's depth)"""
    H = W = 16
    z = np.full((H, W), 4.0)
    z[6:10, 6:10] = 2.0
    x0, c0 = ray_view(H, W, 32.0, (8.0, 8.0), z)
    x_out, cams, shapes, focals = [x0], [c0], [(H, W)], [32.0]
    if extra_views:
        for tx in (-1.0, 1.0):
            x, c = ray_view(64, 64, 32.0, (32.0, 32.0), 4.0, (tx, 0.0, 0.0))
            x_out.append(x); cams.append(c); shapes.append((64, 64)); focals.append(32.0)
    imgs = [np.zeros((3,) + s, dtype=F) for s in shapes]
    pan = [np.ones(s, dtype=np.int32) for s in shapes]
    pan[0][6:10, 6:10] = 2
    info = [{'id': 1, 'query_id': 0, 'category_id': 1}, {'id': 2, 'query_id': 1, 'category_id': 2}]
    return x_out, imgs, pan, info, cams, focals, shapes, 2.0


def sphere_scene(V=6, shape=(40, 48), radius=1.0, distance=3.0):
    """V cameras on a circle of radius `distance` around a sphere at the origin, looking at its centre (voxel_ref's look-at, z up): a pixel whose ray
    meets the sphere measures it exactly (in float64, rounded once), any other has confidence 1 (below the threshold 3) and a point far behind.
    One segment, id 1.  -> (x_out, imgs, pan, info, cams2world, focals)"""
    H, W = shape
    f = 1.1 * max(H, W)
    x_out, cams = [], []
    for v in range(V):
        ang = 2 * np.pi * v / V + 0.2
        eye = np.array([distance * np.cos(ang), distance * np.sin(ang), 0.3])
        c2w = voxel_ref._look_at(eye, np.zeros(3))
        ys, xs = np.mgrid[0:H, 0:W]
        dc = np.stack([(xs - W / 2) / f, (ys - H / 2) / f, np.ones((H, W))], axis=-1).reshape(-1, 3)          # pixel x sits at u = x
        dw = dc @ c2w[:3, :3].T
        a, b, c = (dw * dw).sum(1), 2 * dw @ eye, eye @ eye - radius ** 2
        disc = b * b - 4 * a * c
        hit = disc > 0
        s = np.where(hit, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 10.0)
        loc = (dc * s[:, None]).astype(F)
        c32 = c2w.astype(F)
        x_out.append({'pts3d': cloud_ref.geotrf(c32[:3, :4], loc).reshape(H, W, 3), 'pts3d_local': loc.reshape(H, W, 3),
                      'conf': np.where(hit, F(5), F(1)).astype(F).reshape(H, W)})
        cams.append(c32.astype(np.float64))
    imgs = [np.zeros((3, H, W), dtype=F) for _ in range(V)]
    pan = [np.ones((H, W), dtype=np.int32) for _ in range(V)]
    return x_out, imgs, pan, [{'id': 1, 'query_id': 0, 'category_id': 1}], cams, [float(f)] * V
