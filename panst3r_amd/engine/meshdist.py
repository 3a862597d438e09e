"""The exact distance from points to a triangle mesh within a radius (stage f12): for every query the nearest point of the mesh's SURFACE - its squared
distance, its face and the point itself - where `nearest_points` measures to samples of the surface.  `score_reconstruction(metric='surface')` is
built on it; `closest` is what an ICP against the surface will need.

    d2, face, closest = mesh_distance(points, gt_vertices, gt_faces, 0.05)

No counterpart in the reference: *restated, unpinned*.  Four kernels (csrc/meshdist.hip; the contract is the meshdist section of
include/panst3r_hip.h, restated in tests/meshdist_ref.py and held bit for bit):
  count / insert / scatter   every kept face is listed in the cells of its bounding box, dilated by one cell of edge `radius`: one lane per (face,
                             cell) pair, the voxel stages' hash table, integer atomics only.
  query                      the list of the query's own cell, every candidate's closest point in fp64 (Ericson's region sequence, a fixed order of
                             operations), the minimum of (distance bits, face): the nearest face within the radius, ties to the smaller face.
The search is exact against the triangles; no BVH, no pruning of cells against a triangle's plane, no signed distance, no normals."""
import math

import torch

from .. import hip
from .score3d import _build_lists, _check_mesh, _check_points, _check_radius, _gpu_only, _int32_faces, _is_int, _search_status


def _check_limits(max_cell_faces, max_pairs):
    if not _is_int(max_cell_faces) or not 1 <= max_cell_faces <= 2 ** 31 - 1:
        raise ValueError('max_cell_faces must be an integer >= 1, got %r' % (max_cell_faces,))
    if not _is_int(max_pairs) or not 1 <= max_pairs <= hip.MESHDIST_MAX:
        raise ValueError('max_pairs must be an integer in 1 .. 2^30, got %r' % (max_pairs,))
    return int(max_cell_faces), int(max_pairs)


class MeshIndex:
    """The search structure of `mesh_distance` over one mesh (internal: the build and the query as two steps, with the counts the public call does not
    return): `dropped_faces` were left out (an index outside the vertices, a non-finite corner, zero area, or a cell beyond +-2^20), `pairs` is the
    number of (face, cell) entries, `max_occupancy` the longest list of a cell.  int32 and int64 faces.  `query(points)` -> (d2, face, closest), or
    (d2, face, None) with `closest=False`; `check()` reads the status words after the queries and raises if a kernel gave up."""

    def __init__(self, vertices, faces, radius, *, max_cell_faces=4096, max_pairs=2 ** 27):
        Nv, self.F = _check_mesh(vertices, faces, 'search', hip.MESHDIST_MAX)
        self.radius, self.inv, self.r2 = _check_radius(radius)
        self.max_cell_faces, self.max_pairs = _check_limits(max_cell_faces, max_pairs)
        _gpu_only('mesh_distance', vertices=vertices, faces=faces)
        dev = self.device = vertices.device
        self.dropped_faces, self.pairs, self.max_occupancy, self.bad_queries, self.ws = self.F, 0, 0, 0, None
        if self.F == 0 or Nv == 0:
            return
        i32 = dict(dtype=torch.int32, device=dev)
        self.vertices, self.faces = vertices.float().contiguous(), _int32_faces(faces, Nv)
        self.counts, total, self.status = torch.empty(self.F, **i32), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(4, **i32)
        hip.meshdist_count(self.vertices, self.faces, self.inv, self.counts, total, self.status)
        self.pairs, _, self.dropped_faces, _, _ = torch.cat([total, self.status.to(torch.int64)]).tolist()      # the host sync of the pair total
        if self.pairs > self.max_pairs:                                           # before anything is allocated for them
            raise ValueError('mesh_distance: the radius %g is too small for these faces: their cell boxes hold %s%d (face, cell) pairs, above max_pairs = %d '
                             '(a larger radius makes fewer pairs)' % (self.radius, 'at least ' if self.pairs >= hip.MESHDIST_FACE_CAP else '', self.pairs,
                                                                      self.max_pairs))
        if self.pairs == 0:
            return
        self.prefix = torch.empty(self.F + 1, **i32)
        hip.cloud_scan(self.counts, self.prefix)
        ws = self.ws = hip.meshdist_workspace(self.pairs, dev)
        hip.meshdist_insert(self.vertices, self.faces, self.inv, self.prefix, ws, self.status)
        _, self.max_occupancy = _build_lists(
            'mesh_distance', ws, lambda: hip.meshdist_scatter(self.prefix, ws, self.status), self.status, 'the radius %g is too large for this mesh: one cell '
            'of that edge lists %d of the %d faces, above max_cell_faces = %d (every query in it would visit them all; a smaller radius makes shorter lists)',
            self.radius, self.F, self.max_cell_faces)

    @torch.no_grad()
    def query(self, points, closest=True):
        Nq = _check_points(points, 'points')
        _gpu_only('mesh_distance', points=points)
        q = points.float().contiguous()
        d2 = torch.full((Nq,), math.inf, dtype=torch.float32, device=self.device)
        face = torch.full((Nq,), -1, dtype=torch.int32, device=self.device)
        near = q.clone() if closest else None                                     # without a hit: the query itself
        if Nq and self.ws is not None:
            hip.meshdist_query(q, self.vertices, self.faces, self.inv, self.r2, self.ws, self.max_cell_faces, d2, face, near, self.status)
        return d2, face, near

    def check(self):
        """after the queries (a host sync): the status bits, and the number of non-finite queries so far"""
        if self.ws is not None:
            self.bad_queries = _search_status('mesh_distance', self.status)
        return self.bad_queries


@torch.no_grad()
def mesh_distance(points, vertices, faces, radius, *, max_cell_faces=4096, max_pairs=2 ** 27):
    """For every point [Nq,3] the nearest point of the triangle mesh (vertices [Nv,3] float, faces [Nf,3] int32 / int64, device tensors) within `radius`
    -> (d2 fp32 [Nq], face int32 [Nq], closest fp32 [Nq,3]): the squared distance to the surface, computed in fp64 and cast once, the face it lies on
    (ties to the smaller face) and the nearest point itself; d2 = +inf, face -1 and closest = the point where no face lies within
    d2 <= float32(radius)^2, and for a point with a non-finite coordinate.  The search is exact against the triangles.  A face with an index outside
    the vertices, a non-finite corner or zero area, or beyond +-2^20 radius, is left out.  A hash grid of cell edge `radius`: every face is listed in the
    cells of its bounding box dilated by one cell, and a point reads the list of its own cell.  A radius far below the faces' size makes many (face,
    cell) pairs: more than `max_pairs` raise ValueError before anything is allocated for them (a larger radius makes fewer pairs).  A radius far above
    it makes long lists: if one cell lists more than `max_cell_faces` faces the call raises ValueError after the build and launches no query (a smaller
    radius makes shorter lists).  Empty points or an empty mesh are legal (nothing is launched, nothing is built).  Two calls return identical bytes.
    Three host syncs: the pair total, the build's status with the longest list, and the query's status, which raises RuntimeError if a kernel gave
    up.  GPU only: CPU tensors raise."""
    Nq = _check_points(points, 'points')
    _, Nf = _check_mesh(vertices, faces, 'search', hip.MESHDIST_MAX)
    _check_radius(radius)
    _check_limits(max_cell_faces, max_pairs)
    _gpu_only('mesh_distance', points=points, vertices=vertices, faces=faces)
    if Nq == 0 or Nf == 0 or vertices.shape[0] == 0:                              # nothing to search: no build, no launch
        dev = points.device
        return (torch.full((Nq,), math.inf, dtype=torch.float32, device=dev), torch.full((Nq,), -1, dtype=torch.int32, device=dev),
                points.float().contiguous().clone())
    index = MeshIndex(vertices, faces, radius, max_cell_faces=max_cell_faces, max_pairs=max_pairs)
    out = index.query(points)
    index.check()
    return out
