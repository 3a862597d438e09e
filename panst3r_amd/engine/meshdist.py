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
The search is exact against the triangles; no BVH, no pruning of cells against a triangle's plane, no signed distance.

`icp_to_mesh` (stage f13) aligns points to the mesh by POINT-TO-PLANE ICP on the same lists: one more kernel, icp_plane_step (the icp-plane section
of the header, restated in tests/icp_plane_ref.py and held bit for bit) - the sources moved by the current transform, the query's list walk, the
winner's unnormalised face normal and the fp64 normal equations of the linearised plane distances in f11's fixed order - and the 7 x 7 host solve
`pointmaps.plane_step_from_moments`.  The normals are the ground truth's faces'; the sources need none.

    a = icp_to_mesh(points, gt_vertices, gt_faces, max_dist=0.3)       # or refine_alignment(..., target='surface')"""
import math

import numpy as np
import torch

from .. import hip
from .pointmaps import plane_step_from_moments
from .score3d import (Alignment, _build_lists, _check_icp, _check_mesh, _check_points, _check_radius, _corner_shift, _gpu_only, _icp_radius, _int32_faces,
                      _is_int, _search_status)


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


@torch.no_grad()
def icp_to_mesh(source, vertices, faces, *, max_dist, init=None, with_scale=True, iters=50, min_dist=None, shrink=0.8, tol=1e-4, every=1,
                max_cell_faces=4096, max_pairs=2 ** 27):
    """Point-to-plane ICP against the triangles: the similarity (`with_scale=False`: rigid) transform that carries `source` [N, 3] onto the surface of
    the mesh (vertices [Nv, 3] float, faces [Nf, 3] int32 / int64, device tensors), started from `init` ([4, 4], default the identity) ->
    `Alignment`.  One `MeshIndex` of cell edge `max_dist` is built once.  Step k moves the sources by float32(T), matches each to its nearest face
    within r_k (the schedule of `icp`: float32(max(min_dist, max_dist shrink^k)), `min_dist=None`: max_dist throughout; the radius shrinks without a
    rebuild), and sums the normal equations of the squared distances to the PLANES of the matched faces, linearised in a small rotation, shift and
    scale about c0 - all of it ONE fused launch, `hip.icp_plane_step` - and after ONE host sync (the 40 doubles and the status)
    `pointmaps.plane_step_from_moments` solves the 7 x 7 (rigid: 6 x 6) system for an INCREMENT, T <- increment @ T in float64: increments
    compose here, where `icp` solves for the total transform at every step - the plane objective is not a Procrustes problem and has no closed
    form for the total; each increment is a similarity by construction (Rodrigues' formula), so the product is one.  c0 = float32 of T applied to
    the centre of the sources' bounding box; the columns of the system are scaled by half the box's diagonal times cbrt(|det T[:3, :3]|).  A point on
    a wall may slide along it at no cost, which is the point: `icp` pins every source to its nearest sample and creeps (docs/experiments.md 6r).
    `every=k` uses the source rows 0, k, 2k, ...  Stops: 'converged' - the radius has reached its floor and the eight corners of the sources' box
    moved by at most `tol` r_k in this step; 'iters'; 'degenerate' - fewer matched sources than unknowns (7, rigid 6), or the matched planes do not
    fix the motion (`plane_step_from_moments` returns None: a single plane, parallel planes, a corridor) - the transform of the step before is
    returned, at step 0 that is `init`.  A first step without a single match raises ValueError, as does a non-finite source.  `history` holds per
    step `radius`, `matched`, `rmse` (to the triangles) and `plane_rmse` (to the planes of the matched faces), before that step's solve.
    `max_cell_faces` and `max_pairs` guard the index as in `mesh_distance`.  The moments are summed in a fixed order: two calls return identical
    bytes.  No source normals, no robust weights.  GPU only: CPU tensors raise."""
    _check_points(source, 'source')
    _check_mesh(vertices, faces, 'search', hip.MESHDIST_MAX)
    max_dist, T, min_dist, shrink, tol = _check_icp(max_dist, init, with_scale, iters, min_dist, shrink, tol, every)
    _check_limits(max_cell_faces, max_pairs)
    _gpu_only('icp_to_mesh', 'a %(device)s %(name)s', source=source, vertices=vertices, faces=faces)
    src = source.float()[::every].contiguous()
    unknowns = 7 if with_scale else 6
    if src.shape[0] < unknowns:
        raise ValueError('icp_to_mesh needs at least %d source points, got %d (every=%d)' % (unknowns, src.shape[0], every))
    lo, hi = (v.double().cpu().numpy() for v in torch.aminmax(src, dim=0))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError('icp_to_mesh: a source point is not finite')
    box = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    centre, half = 0.5 * (lo + hi), 0.5 * float(np.sqrt(((hi - lo) ** 2).sum()))
    index = MeshIndex(vertices, faces, max_dist, max_cell_faces=max_cell_faces, max_pairs=max_pairs)
    iws = hip.icp_plane_workspace(src.shape[0], src.device)
    history, reason = [], 'iters'
    for k in range(int(iters)):
        r, r2, floor = _icp_radius(k, max_dist, min_dist, shrink)
        c0 = (T[:3, :3] @ centre + T[:3, 3]).astype(np.float32)
        length = half * float(np.cbrt(abs(np.linalg.det(T[:3, :3]))))
        if index.ws is None:                                                      # no face was kept: nothing can match
            mom, bits = np.zeros(hip.ICP_PLANE_MOMENTS), 0
        else:
            iws['status'].zero_()
            out = hip.icp_plane_step(src, T[:3].astype(np.float32), c0, index.vertices, index.faces, index.inv, index.r2, float(r2), index.ws,
                                     index.max_cell_faces, iws)
            got = torch.cat([out, iws['status'].double()]).cpu().numpy()         # the one host sync of the step
            mom, bits = got[:hip.ICP_PLANE_MOMENTS], int(got[hip.ICP_PLANE_MOMENTS])
        if bits:
            raise RuntimeError('icp_to_mesh: the search did not finish (status %d)' % bits)
        n = int(mom[0])
        history.append({'radius': float(r), 'matched': n, 'rmse': float(np.sqrt(mom[37] / mom[0])) if n else math.nan,
                        'plane_rmse': float(np.sqrt(mom[36] / mom[0])) if n else math.nan})
        if n == 0 and k == 0:
            raise ValueError('icp_to_mesh: nothing within max_dist of the initial alignment (none of %d sources matched within %g)' % (src.shape[0], max_dist))
        inc = plane_step_from_moments(mom, c0.astype(np.float64), length, with_scale) if n >= unknowns else None
        if inc is None:
            reason = 'degenerate'
            break
        new = inc @ T
        shift, T = _corner_shift(box, T, new), new
        if floor and shift <= tol * float(r):
            reason = 'converged'
            break
    return Alignment(torch.from_numpy(T), len(history), reason == 'converged', reason, history)
