"""A reconstruction scored against a ground-truth mesh in 3-D (stage f10): how close the predicted geometry lies to the true surface (precision, recall
and F-score at distance thresholds, accuracy / completeness / chamfer) and how good the fused labels are on that surface (a panoptic quality whose
unit is a piece of ground-truth surface instead of a pixel).  It scores what the other stages leave on the device - a `PanopticCloud`, a `VoxelCloud`,
a `PanopticMesh` or plain points - against the mesh that `load_ply_mesh` / `panoptic_vertex_ids` give.

    T = similarity_from_cameras([c['cam2world'] for c in cameras], gt_cams2world)
    s = score_reconstruction(cloud, gt_vertices, gt_faces, thresholds=(0.05, 0.1), spacing=0.02, transform=T, gt_vertex_ids=ids, gt_segments=segs,
                             refine=True)                  # T refined on the geometry by ICP before anything is scored (stage f11)

TWO METRICS.  `metric='points'` (the default): the ground-truth surface is replaced by a deterministic lattice of samples about `spacing` apart and
every distance is one between two points; a distance is therefore off by up to about spacing / sqrt(3) against the true surface: choose `spacing`
well below the smallest threshold.  `metric='surface'` (stage f12): the distance from a predicted point is the exact one to the ground truth's
triangles (`mesh_distance`, engine/meshdist.py), so precision and accuracy no longer depend on `spacing`; the other direction is exact too when the
prediction is a surface, and stays point to point when it is a cloud.  No BVH.  No counterpart in the reference: *restated, unpinned*.  Two kernels (csrc/nearest.hip; the contract
is the score3d section of include/panst3r_hip.h, restated in tests/nearest_ref.py and held bit for bit):
  sample_mesh      face f gets n_f^2 samples, the centroids of the n_f^2 congruent sub-triangles of its uniform subdivision, n_f the smallest whole
                   number with n_f spacing >= the face's longest edge (clamped to max_subdiv).  The density differs between faces by what rounding
                   n_f up implies (a face just over a multiple of `spacing` is sampled up to (n + 1)^2 / n^2 denser): a CHOICE - a lattice per face
                   is deterministic and needs no random numbers; an area-weighted draw would be uniform in expectation only.
  nearest_points   a hash grid of cell = radius over the targets, the 27 cells around a query, the minimum of (distance bits, row): the nearest target
                   within the radius, ties to the smaller row.
  icp_step         (stage f11) the sources moved by the current transform, each one's nearest target through the same search, and the float64
                   moments of the matched pairs in a fixed order, in one pass: the hot path of `icp` / `refine_alignment`, which refine the alignment
                   that `similarity_from_cameras` can only take from the camera centres.  Restated in tests/icp_ref.py, held bit for bit.
Everything else composes: the counts are integer compares of the squared distances against float32(tau)^2, the means are float64 reductions of
sqrt(d2) through torch, the labels go through `panoptic_quality` as one [1, S] map."""
import math

import numpy as np
import torch

from .. import hip
from .pointmaps import procrustes_from_moments

PLANE_RANK_TOL = 1e-6      # similarity_from_cameras: the centres span a plane iff their second singular value exceeds this share of the first


class MeshSamples:
    """points [S,3] fp32, face [S] int32 (the face of every sample), ids [S] int32 (the face's id, the id of the nearest corner, or 0), in face order;
    dropped_faces (an index outside the vertices, a non-finite corner or zero area), clamped_faces (more than max_subdiv subdivisions wanted)."""

    def __init__(self, points, face, ids, dropped_faces, clamped_faces):
        self.points, self.face, self.ids, self.dropped_faces, self.clamped_faces = points, face, ids, int(dropped_faces), int(clamped_faces)

    def __len__(self):
        return int(self.face.shape[0])

    def cpu(self):
        return MeshSamples(self.points.cpu(), self.face.cpu(), self.ids.cpu(), self.dropped_faces, self.clamped_faces)


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _check_length(value, name):
    """a positive finite length that is still positive and finite as float32 -> that float32 as a Python float"""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(float(value)) or float(value) <= 0:
        raise ValueError('%s must be a positive finite number, got %r' % (name, value))
    with np.errstate(over='ignore', under='ignore'):
        v = np.float32(float(value))
    if not (np.isfinite(v) and v > 0):
        raise ValueError('%s %r is not a positive finite float32' % (name, value))
    return float(v)


def _check_radius(radius, name='radius'):
    """-> (radius, inv, r2) as float32 values: inv = float32(1 / radius), r2 = float32(radius radius), all positive and finite"""
    r = np.float32(_check_length(radius, name))
    with np.errstate(over='ignore', under='ignore'):
        inv, r2 = np.float32(1.0) / r, r * r
    if not (np.isfinite(inv) and inv > 0 and np.isfinite(r2) and r2 > 0):
        raise ValueError('%s %r has no positive finite float32 inverse and square' % (name, radius))
    return float(r), float(inv), float(r2)


def _check_points(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or not t.dtype.is_floating_point:
        raise ValueError('%s must be a floating-point [N, 3] tensor, got %s' % (name, '%s %s' % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.shape[0] > hip.NN_MAX_POINTS:
        raise ValueError('%s holds %d points; one search takes 2^30 at the most' % (name, t.shape[0]))
    return int(t.shape[0])


def _gpu_only(who, what='%(device)s %(name)s', **tensors):
    """`who` has no CPU path: a given tensor that is not on the GPU raises; `what` = how the caller's message names it"""
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError('%s got %s: it runs on the GPU only (no CPU fallback)' % (who, what % dict(device=t.device, name=name)))


def _check_mesh(vertices, faces, use, max_faces, **ids):
    """the mesh of `sample_mesh` (use = 'sample') and of `mesh_distance` ('search'), of at most max_faces = 2^30 faces -> (Nv, Nf); `ids`: further
    tensors or None"""
    for name, t in dict(vertices=vertices, faces=faces, **ids).items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise ValueError('%s must be a torch tensor, got %s' % (name, type(t).__name__))
    if vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.dtype.is_floating_point:
        raise ValueError('vertices must be a floating-point [Nv, 3] tensor, got %s %s' % (vertices.dtype, tuple(vertices.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('faces must be an int32 / int64 [Nf, 3] tensor, got %s %s' % (faces.dtype, tuple(faces.shape)))
    Nv, Nf = int(vertices.shape[0]), int(faces.shape[0])
    if not (Nv <= 2 ** 31 - 1 and Nf <= max_faces):
        raise ValueError('a mesh to %s has at most 2^31 - 1 vertices and 2^30 faces, got %d and %d' % (use, Nv, Nf))
    return Nv, Nf


def _int32_faces(faces, Nv):
    """contiguous int32 faces; an int64 index that does not fit int32 is outside the vertices: -1 keeps it so"""
    if faces.dtype == torch.int64:
        faces = torch.where((faces < 0) | (faces >= Nv), torch.full_like(faces, -1), faces)
    return faces.to(torch.int32).contiguous()


def _build_lists(who, ws, scatter, status, too_long, radius, n, limit):
    """The tail of a hash-grid build, after the insert has counted the cells: the offsets of the per-cell lists, the scatter (`scatter()` launches
    it), the host sync of the build and its two refusals -> (status[1], the longest list).  `too_long` is the text after '`who`: ', formatted with
    (radius, the longest list, n, limit)."""
    csum = torch.cumsum(ws['cell_count'], 0, dtype=torch.int32)               # plumbing: the offsets of the per-cell lists
    ws['start'] = csum - ws['cell_count']
    scatter()
    bits, left_out, longest, _ = status.tolist()                              # the host sync of the build
    if bits:
        raise RuntimeError('%s: the build did not finish (status %d): the cell table ran full or its lists are inconsistent' % (who, bits))
    if longest > limit:
        raise ValueError('%s: ' % who + too_long % (radius, longest, n, limit))
    return left_out, longest


def _search_status(who, status):
    """after the queries (a host sync): raises if a kernel gave up -> the number of non-finite queries so far"""
    bits, _, _, bad = status.tolist()
    if bits:
        raise RuntimeError('%s: the search did not finish (status %d)' % (who, bits))
    return bad


def _check_sample_mesh(vertices, faces, vertex_ids, face_ids, max_subdiv):
    Nv, Nf = _check_mesh(vertices, faces, 'sample', hip.NN_MAX_POINTS, vertex_ids=vertex_ids, face_ids=face_ids)
    if vertex_ids is not None and face_ids is not None:
        raise ValueError('give vertex_ids or face_ids, not both')
    for name, t, n in (('vertex_ids', vertex_ids, Nv), ('face_ids', face_ids, Nf)):
        if t is not None and (t.dim() != 1 or t.shape[0] != n or t.dtype.is_floating_point or t.dtype == torch.bool):
            raise ValueError('%s must be an integer [%d] tensor, got %s %s' % (name, n, t.dtype, tuple(t.shape)))
    if not _is_int(max_subdiv) or not 1 <= max_subdiv <= hip.MESH_SAMPLE_MAX_SUBDIV:
        raise ValueError('max_subdiv must be an integer in 1 .. %d, got %r' % (hip.MESH_SAMPLE_MAX_SUBDIV, max_subdiv))
    return Nv, Nf


@torch.no_grad()
def sample_mesh(vertices, faces, spacing, *, vertex_ids=None, face_ids=None, max_subdiv=1024, capacity=None):
    """The surface of a device mesh (vertices [Nv,3] float, faces [Nf,3] int) as points about `spacing` apart -> `MeshSamples`.  Face f gets n^2 samples,
    the centroids of the n^2 congruent sub-triangles of its uniform subdivision, n = the smallest whole number with n spacing >= its longest edge,
    clamped to `max_subdiv` (clamped faces are counted: they are sampled more coarsely than asked).  `face_ids` [Nf] gives a sample its face's id,
    `vertex_ids` [Nv] the id of its nearest corner (the largest barycentric weight, ties to the lower corner; never a blend); with neither ids are 0.
    A face with an index outside the vertices, a non-finite corner or zero area has no samples and is counted in `dropped_faces`.  Samples come in
    face order; two calls return identical bytes.  `capacity`: the most samples to make, default 2^31 - 256; more raise ValueError and nothing is
    written.  Two host syncs (the number of samples; the status after the emit).  GPU only: CPU tensors raise."""
    Nv, Nf = _check_sample_mesh(vertices, faces, vertex_ids, face_ids, max_subdiv)
    spacing = _check_length(spacing, 'spacing')
    if capacity is None:
        capacity = hip.MESH_SAMPLE_MAX_TOTAL
    if not _is_int(capacity) or not 0 <= capacity <= hip.MESH_SAMPLE_MAX_TOTAL:
        raise ValueError('capacity must be an integer in 0 .. 2^31 - 256, got %r' % (capacity,))
    _gpu_only('sample_mesh', 'a %(device)s tensor', vertices=vertices, faces=faces, vertex_ids=vertex_ids, face_ids=face_ids)
    dev = vertices.device
    i32 = dict(dtype=torch.int32, device=dev)

    def result(S, dropped, clamped, points=None, face=None, ids=None):
        if S == 0:
            points, face, ids = torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, **i32), torch.empty(0, **i32)
        return MeshSamples(points, face, ids, dropped, clamped)
    if Nf == 0 or Nv == 0:
        return result(0, Nf, 0)
    verts, faces = vertices.float().contiguous(), _int32_faces(faces, Nv)
    vid = None if vertex_ids is None else vertex_ids.to(torch.int32).contiguous()
    fid = None if face_ids is None else face_ids.to(torch.int32).contiguous()
    counts, prefix = torch.empty(Nf, **i32), torch.empty(Nf + 1, **i32)
    total, status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(4, **i32)
    hip.mesh_sample_count(verts, faces, spacing, max_subdiv, counts, total, status)
    hip.cloud_scan(counts, prefix)
    S, _, dropped, clamped, _ = torch.cat([total, status.to(torch.int64)]).tolist()      # the host sync
    if S > capacity:
        raise ValueError('sample_mesh: spacing %g gives %d samples, above the capacity of %d: a larger spacing or a smaller max_subdiv gives fewer'
                         % (spacing, S, capacity))
    if S == 0:
        return result(0, dropped, clamped)
    points, face, ids = torch.empty(S, 3, dtype=torch.float32, device=dev), torch.empty(S, **i32), torch.empty(S, **i32)
    hip.mesh_sample_emit(verts, faces, prefix, S, vid, fid, points, face, ids, status)
    if int(status[0]):                                                        # the second host sync: the emit refused (never: the prefix is this call's)
        raise RuntimeError('sample_mesh: the emit pass refused its prefix (status %d); no result' % int(status[0]))
    return result(S, dropped, clamped, points, face, ids)


class NearestIndex:
    """The search structure of `nearest_points` over one set of targets (internal: the build and the query as two steps, with the counts the public call
    does not return): `dropped` targets were left out (a non-finite coordinate or a cell beyond +-2^20), `max_occupancy` is the fullest cell.
    `query(queries)` -> (d2, row); `check()` reads the status words after the queries and raises if a kernel gave up."""

    def __init__(self, targets, radius, *, max_cell_points=4096):
        self.M = _check_points(targets, 'targets')
        self.radius, self.inv, self.r2 = _check_radius(radius)
        if not _is_int(max_cell_points) or not 1 <= max_cell_points <= 2 ** 31 - 1:
            raise ValueError('max_cell_points must be an integer >= 1, got %r' % (max_cell_points,))
        self.max_cell_points = int(max_cell_points)
        _gpu_only('nearest_points', targets=targets)
        self.device, self.dropped, self.max_occupancy, self.bad_queries = targets.device, 0, 0, 0
        if self.M == 0:
            return
        self.targets = targets.float().contiguous()
        ws = self.ws = hip.nn_workspace(self.M, self.device)
        hip.nn_insert(self.targets, self.inv, ws)
        self.dropped, self.max_occupancy = _build_lists(
            'nearest_points', ws, lambda: hip.nn_scatter(ws), ws['status'], 'the radius %g is too large for this density: one cell of that edge holds %d '
            'of the %d targets, above max_cell_points = %d (every query next to it would visit them all)', self.radius, self.M, self.max_cell_points)

    @torch.no_grad()
    def query(self, queries):
        Nq = _check_points(queries, 'queries')
        _gpu_only('nearest_points', queries=queries)
        d2 = torch.full((Nq,), math.inf, dtype=torch.float32, device=self.device)
        row = torch.full((Nq,), -1, dtype=torch.int32, device=self.device)
        if Nq and self.M:
            hip.nn_query(queries.float().contiguous(), self.targets, self.inv, self.r2, self.ws, self.max_cell_points, d2, row)
        return d2, row

    def check(self):
        """after the queries (a host sync): the status bits, and the number of non-finite queries so far"""
        if self.M:
            self.bad_queries = _search_status('nearest_points', self.ws['status'])
        return self.bad_queries


@torch.no_grad()
def nearest_points(queries, targets, radius, *, max_cell_points=4096):
    """For every query [Nq,3] the nearest of the targets [M,3] (device float tensors) within `radius` -> (d2 fp32 [Nq], row int32 [Nq]): the squared
    distance (dx dx + dy dy) + dz dz in fp32 and the target's row, ties to the smaller row; row -1 and d2 = +inf where no target lies within
    d2 <= float32(radius)^2, and for a query with a non-finite coordinate.  Targets with a non-finite coordinate or beyond +-2^20 radius are left out.
    A hash grid of cell edge `radius`; a query visits the 27 cells around its own, so a radius far above the point spacing makes it slow: if one cell
    holds more than `max_cell_points` targets the call raises ValueError after the build and launches no query.  Empty queries or targets are legal
    (nothing is launched, nothing is built).  Two calls return identical bytes.  Two host syncs: the build's status with the fullest cell, and the
    query's status, which raises RuntimeError if a kernel gave up.  GPU only: CPU tensors raise."""
    Nq = _check_points(queries, 'queries')
    _check_points(targets, 'targets')
    _check_radius(radius)
    if not _is_int(max_cell_points) or not 1 <= max_cell_points <= 2 ** 31 - 1:
        raise ValueError('max_cell_points must be an integer >= 1, got %r' % (max_cell_points,))
    _gpu_only('nearest_points', queries=queries, targets=targets)
    if Nq == 0 or targets.shape[0] == 0:                                      # nothing to search: no build, no launch
        dev = queries.device
        return torch.full((Nq,), math.inf, dtype=torch.float32, device=dev), torch.full((Nq,), -1, dtype=torch.int32, device=dev)
    index = NearestIndex(targets, radius, max_cell_points=max_cell_points)
    out = index.query(queries)
    index.check()
    return out


def _centres(cams, name):
    c = np.stack([np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64) for m in cams]) if len(cams) else np.zeros((0, 4, 4))
    if c.ndim != 3 or c.shape[1] < 3 or c.shape[2] != 4:
        raise ValueError('%s must be V camera-to-world matrices [4, 4] (or [3, 4]), got %s' % (name, c.shape))
    if not np.isfinite(c).all():
        raise ValueError('%s holds a non-finite entry' % name)
    return c[:, :3, 3]


def _spans_plane(x):
    s = np.linalg.svd(x - x.mean(0), compute_uv=False)
    return s[0] > 0 and s[1] > PLANE_RANK_TOL * s[0]


def similarity_from_cameras(pred_cams2world, gt_cams2world):
    """The similarity transform that carries the predicted frame into the ground truth's, from V >= 3 corresponding cameras: the scaled Kabsch
    registration of their centres (`pointmaps.rigid_points_registration(..., compute_scaling=True)`'s host step on the centres' float64 moments -
    camera poses are host values here) -> a [4, 4] float64 tensor [[s R, t], [0, 1]] with gt_centre ~ s R pred_centre + t: the scale is folded in.
    Raises ValueError for fewer than 3 cameras, and for centres that do not span a plane - collinear or coincident centres leave the rotation about
    their line free.  The test is a CHOICE: with s1 >= s2 the singular values of the centred centres, s2 > 1e-6 s1 (`PLANE_RANK_TOL`), for both sets;
    it rejects the degenerate case, it does not promise a well-conditioned one.  The orientations of the cameras are not used.  The residual of
    the camera centres is all it minimises: `refine_alignment` (or `score_reconstruction(refine=True)`) refines the result on the geometry."""
    x, y = _centres(pred_cams2world, 'pred_cams2world'), _centres(gt_cams2world, 'gt_cams2world')
    if len(x) != len(y):
        raise ValueError('similarity_from_cameras needs as many ground-truth cameras as predicted ones, got %d and %d' % (len(y), len(x)))
    if len(x) < 3:
        raise ValueError('similarity_from_cameras needs at least 3 cameras, got %d' % len(x))
    if not (_spans_plane(x) and _spans_plane(y)):
        raise ValueError('similarity_from_cameras: the camera centres do not span a plane (collinear or coincident): the rotation is not determined')
    R, t, s = procrustes_from_moments(float(len(x)), x.sum(0), y.sum(0), y.T @ x, float((x * x).sum()))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, t
    return torch.from_numpy(T)


def _moved(points, T, what):
    """fp32 points on the device, carried by the [4, 4] matrix T (or as they are)"""
    _gpu_only('score_reconstruction', **{what: points})
    points = points.float()
    if T is not None:
        A = torch.from_numpy(T).to(device=points.device, dtype=torch.float32)
        points = points @ A[:3, :3].T + A[:3, 3]
    return points.contiguous()


def _pred_points(pred, spacing, max_subdiv, T):
    """-> (points [N,3] in the ground truth's frame, ids [N] or None, segments or None) of what is scored.  A mesh is moved BEFORE it is sampled, so
    that `spacing` is a length of the ground truth's frame for both surfaces whatever scale T holds."""
    from .cloud import PanopticCloud
    from .surface import PanopticMesh
    from .voxels import VoxelCloud
    if isinstance(pred, PanopticMesh):
        s = sample_mesh(_moved(pred.vertices, T, 'vertices'), pred.faces, spacing, face_ids=pred.face_ids, max_subdiv=max_subdiv)
        return s.points, s.ids, pred.segments
    if isinstance(pred, (PanopticCloud, VoxelCloud)):
        return _moved(pred.points, T, 'points'), pred.pan, pred.segments
    if isinstance(pred, torch.Tensor):
        _check_points(pred, 'pred')
        return _moved(pred, T, 'points'), None, None
    raise ValueError('pred must be a PanopticCloud, a VoxelCloud, a PanopticMesh or an [N, 3] tensor, got %s' % type(pred).__name__)


def _check_transform(transform):
    T = np.asarray(transform.detach().cpu().numpy() if isinstance(transform, torch.Tensor) else transform, dtype=np.float64)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError('transform must be a finite [4, 4] matrix, got shape %s' % (T.shape,))
    return T


class Alignment:
    """The result of `icp` / `refine_alignment`: `transform` [4, 4] float64 tensor [[s R, t], [0, 1]] with the scale folded in (as
    `similarity_from_cameras` gives it), `iterations` (steps run), `converged`, `reason` ('converged', 'iters' or 'degenerate') and `history`, per
    step a dict of `radius`, `matched` (pairs within it) and `rmse` = sqrt(sum d2 / matched) BEFORE that step's solve (nan without a match)."""

    def __init__(self, transform, iterations, converged, reason, history):
        self.transform, self.iterations, self.converged, self.reason, self.history = transform, int(iterations), bool(converged), reason, history

    def __repr__(self):
        last = self.history[-1] if self.history else {}
        return 'Alignment(%s after %d iterations, %s matched, rmse %s)' % (self.reason, self.iterations, last.get('matched'), last.get('rmse'))


def _icp_radius(k, max_dist, min_dist, shrink):
    """(r_k as float32, its fp32 square, whether the schedule has reached its floor)"""
    r = np.float32(max_dist if min_dist is None else max(min_dist, max_dist * shrink ** k))
    return r, r * r, min_dist is None or max_dist * shrink ** k <= min_dist


def _corner_shift(box, T0, T1):
    """the farthest that one of the eight corners moves between two transforms"""
    a, b = box @ T0[:3, :3].T + T0[:3, 3], box @ T1[:3, :3].T + T1[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1)).max())


def _check_icp(max_dist, init=None, with_scale=True, iters=50, min_dist=None, shrink=0.8, tol=1e-4, every=1, max_cell_points=4096):
    """the keywords of `icp`, checked -> (max_dist and min_dist as their float32 values, the start as a [4, 4] float64 array, shrink, tol)"""
    max_dist = _check_length(max_dist, 'max_dist')
    _check_radius(max_dist, 'max_dist')
    if min_dist is not None:
        min_dist = _check_length(min_dist, 'min_dist')
        if min_dist > max_dist:
            raise ValueError('min_dist %g lies beyond max_dist %g' % (min_dist, max_dist))
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating)) or not 0 < float(shrink) < 1:
        raise ValueError('shrink must be a number in (0, 1), got %r' % (shrink,))
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (math.isfinite(float(tol)) and float(tol) >= 0):
        raise ValueError('tol must be a finite number >= 0, got %r' % (tol,))
    for name, v in (('iters', iters), ('every', every), ('max_cell_points', max_cell_points)):
        if not _is_int(v) or not 1 <= v <= 2 ** 31 - 1:
            raise ValueError('%s must be an integer >= 1, got %r' % (name, v))
    T = np.eye(4) if init is None else _check_transform(init).copy()
    return max_dist, T, min_dist, float(shrink), float(tol)


@torch.no_grad()
def icp(source, target, *, max_dist, init=None, with_scale=True, iters=50, min_dist=None, shrink=0.8, tol=1e-4, every=1, max_cell_points=4096):
    """Point-to-point ICP: the similarity (`with_scale=False`: rigid) transform that carries `source` [N, 3] onto `target` [M, 3] (device float
    tensors), started from `init` ([4, 4], default the identity) -> `Alignment`.  One `NearestIndex` of cell edge `max_dist` over the targets is
    built once.  Step k moves the sources by float32(T), matches each to its nearest target within r_k = float32(max(min_dist, max_dist shrink^k))
    (`min_dist=None`: r_k = max_dist throughout; the radius shrinks without a rebuild, the cells stay `max_dist` wide), sums the moments of the
    matched pairs - all of it ONE fused launch, `hip.icp_step` - and after ONE host sync (the 20 doubles and the status) solves
    `pointmaps.procrustes_from_moments` for the TOTAL transform from the original sources to their matches, never an increment, so nothing drifts.
    `every=k` uses the source rows 0, k, 2k, ...  Stops: 'converged' - the radius has reached its floor and the eight corners of the sources' bounding
    box (one device min / max before the loop; a non-finite source keeps this from ever holding) moved by at most `tol` r_k between two successive
    T; 'iters' - `iters` steps were run; 'degenerate' - fewer than 3 pairs remain, or with s1 >= s2 the singular values of the centred moment matrix
    sum (y - ym)(x - xm)^T, s2 <= PLANE_RANK_TOL s1: the matched sources lie on a line, the same CHOICE as in `similarity_from_cameras`; the transform
    of the step before is returned.  A first step with fewer than 3 pairs raises ValueError.  The schedule, the defaults and the stop rule are
    CHOICES: a geometric radius schedule sheds outliers as the fit tightens, and a test on the box corners is a length, comparable with the radius,
    where a test on matrix entries is not.  The moments are summed in a fixed order: two calls return identical bytes.  GPU only: CPU tensors raise."""
    _check_points(source, 'source')
    _check_points(target, 'target')
    max_dist, T, min_dist, shrink, tol = _check_icp(max_dist, init, with_scale, iters, min_dist, shrink, tol, every, max_cell_points)
    _gpu_only('icp', 'a %(device)s %(name)s', source=source, target=target)
    src = source.float()[::every].contiguous()
    if src.shape[0] < 3 or target.shape[0] < 3:
        raise ValueError('icp needs at least 3 source points and 3 targets, got %d (every=%d) and %d' % (src.shape[0], every, target.shape[0]))
    index = NearestIndex(target, max_dist, max_cell_points=max_cell_points)
    iws = hip.icp_workspace(src.shape[0], src.device)
    lo, hi = (v.double().cpu().numpy() for v in torch.aminmax(src, dim=0))
    box = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    history, reason = [], 'iters'
    for k in range(int(iters)):
        r, r2, floor = _icp_radius(k, max_dist, min_dist, shrink)
        iws['status'].zero_()
        out = hip.icp_step(src, T[:3].astype(np.float32), index.targets, index.inv, index.r2, float(r2), index.ws, index.max_cell_points, iws)
        got = torch.cat([out, iws['status'].double()]).cpu().numpy()         # the one host sync of the step
        mom, bits = got[:20], int(got[20])
        if bits:
            raise RuntimeError('icp: the search did not finish (status %d)' % bits)
        n = int(mom[0])
        history.append({'radius': float(r), 'matched': n, 'rmse': float(np.sqrt(mom[17] / mom[0])) if n else math.nan})
        if n < 3:
            if k == 0:
                raise ValueError('icp: nothing within max_dist of the initial alignment (%d of %d sources matched within %g)' % (n, src.shape[0], max_dist))
            reason = 'degenerate'
            break
        xm, ym = mom[1:4] / mom[0], mom[4:7] / mom[0]
        sv = np.linalg.svd(mom[7:16].reshape(3, 3) - mom[0] * np.outer(ym, xm), compute_uv=False)
        if sv[1] <= PLANE_RANK_TOL * sv[0]:
            reason = 'degenerate'
            break
        new = np.eye(4)
        if with_scale:
            R, t, s = procrustes_from_moments(mom[0], mom[1:4], mom[4:7], mom[7:16].reshape(3, 3), mom[16])
            new[:3, :3], new[:3, 3] = s * R, t
        else:
            new[:3, :3], new[:3, 3] = procrustes_from_moments(mom[0], mom[1:4], mom[4:7], mom[7:16].reshape(3, 3))
        shift, T = _corner_shift(box, T, new), new
        if floor and shift <= tol * float(r):
            reason = 'converged'
            break
    return Alignment(torch.from_numpy(T), len(history), reason == 'converged', reason, history)


@torch.no_grad()
def refine_alignment(pred, gt_vertices, gt_faces, *, spacing, max_dist, init=None, max_subdiv=1024, target='samples', **icp_kwargs):
    """Refine the alignment of a prediction - a `PanopticCloud`, a `VoxelCloud`, a `PanopticMesh` or an [N, 3] device tensor - to the ground-truth mesh
    on the geometry -> `Alignment` whose `transform` is T_icp @ init, ready for `score_reconstruction(transform=)`.  The prediction is carried by
    `init` ([4, 4], e.g. `similarity_from_cameras`; default the identity) as `score_reconstruction` carries it - a mesh is moved BEFORE it is
    sampled at `spacing` - the ground truth is `sample_mesh` at `spacing`, and `icp` runs from the identity on the moved points with
    `max_dist` and `icp_kwargs`.  The direction is prediction -> ground truth, a CHOICE: a prediction covers part of the scene and the mesh all of
    it, so the reverse direction would pull the fit towards surface the prediction never saw.  `target='samples'` (the default, what it always
    was): point-to-point `icp` against the samples.  `target='surface'` (stage f13): point-to-plane `icp_to_mesh` (engine/meshdist.py) of the same
    points against the ground truth's TRIANGLES - `gt_vertices` / `gt_faces` as they are; `spacing` then only samples a `PanopticMesh` prediction,
    and `icp_kwargs` are `icp_to_mesh`'s (`max_cell_faces`, `max_pairs` instead of `max_cell_points`).  On scenes made of large planes the
    point-to-point fit resists sliding along every wall and creeps; the plane fit does not (docs/experiments.md 6r).  GPU only."""
    spacing = _check_length(spacing, 'spacing')
    T0 = None if init is None else _check_transform(init)
    if not _is_int(max_subdiv) or not 1 <= max_subdiv <= hip.MESH_SAMPLE_MAX_SUBDIV:
        raise ValueError('max_subdiv must be an integer in 1 .. %d, got %r' % (hip.MESH_SAMPLE_MAX_SUBDIV, max_subdiv))
    if target not in ('samples', 'surface'):
        raise ValueError("target must be 'samples' or 'surface', got %r" % (target,))
    if target == 'surface':
        from .meshdist import _check_limits, icp_to_mesh
        kw = dict(icp_kwargs)
        _check_limits(kw.pop('max_cell_faces', 4096), kw.pop('max_pairs', 2 ** 27))      # before the GPU is touched, as below
        if 'max_cell_points' in kw:
            raise ValueError("refine_alignment(target='surface') takes max_cell_faces and max_pairs, not max_cell_points")
        _check_icp(max_dist, **kw)
        _check_mesh(gt_vertices, gt_faces, 'search', hip.MESHDIST_MAX)
        points, _, _ = _pred_points(pred, spacing, max_subdiv, T0)
        a = icp_to_mesh(points, gt_vertices, gt_faces, max_dist=max_dist, **icp_kwargs)
        if T0 is not None:
            a.transform = torch.from_numpy(a.transform.numpy() @ T0)
        return a
    _check_icp(max_dist, **icp_kwargs)                                        # before the GPU is touched (`init` is this call's own: icp starts from the identity)
    points, _, _ = _pred_points(pred, spacing, max_subdiv, T0)
    gt = sample_mesh(gt_vertices, gt_faces, spacing, max_subdiv=max_subdiv)
    a = icp(points, gt.points, max_dist=max_dist, **icp_kwargs)
    if T0 is not None:
        a.transform = torch.from_numpy(a.transform.numpy() @ T0)
    return a


def _direction(d2, row):
    """matched share, mean and median distance (float64 through torch) of one direction; the median is the lower middle element"""
    n = int(d2.numel())
    d = torch.sqrt(d2[row >= 0].double())
    m = int(d.numel())
    if m == 0:
        return 0.0, math.nan, math.nan, 0
    return m / n, float(d.sum() / m), float(torch.sort(d).values[(m - 1) // 2]), m


def _surface_distances(pred, points, ids, gt, gt_vertices, gt_faces, radius, T, max_cell_points, max_cell_faces, max_pairs):
    """the two directions of `metric='surface'` -> ((d2, row) predicted -> ground truth, (d2, row) ground truth -> predicted, the ids that `row` of the
    second indexes, the extra entries of the dict).  `row` is a face where the target is a surface and a point where it is a cloud."""
    from .meshdist import MeshIndex
    from .surface import PanopticMesh
    kw = dict(max_cell_faces=max_cell_faces, max_pairs=max_pairs)
    to_gt = MeshIndex(gt_vertices, gt_faces, radius, **kw)
    acc = to_gt.query(points, closest=False)[:2]
    to_gt.check()
    if isinstance(pred, PanopticMesh):                                        # a surface: the ground-truth samples against its triangles
        to_pred = MeshIndex(_moved(pred.vertices, T, 'vertices'), pred.faces, radius, **kw)
        comp, ids = to_pred.query(gt.points, closest=False)[:2], pred.face_ids
    else:                                                                     # no surface there: point to point, as under 'points'
        to_pred = NearestIndex(points, radius, max_cell_points=max_cell_points)
        comp = to_pred.query(gt.points)
    to_pred.check()
    return acc, comp, ids, {'gt_pairs': to_gt.pairs, 'gt_max_cell_faces': to_gt.max_occupancy}


@torch.no_grad()
def score_reconstruction(pred, gt_vertices, gt_faces, *, thresholds, spacing, max_dist=None, transform=None, gt_vertex_ids=None, gt_segments=None,
                         things=None, max_subdiv=1024, max_cell_points=4096, refine=None, metric='points', max_cell_faces=4096, max_pairs=2 ** 27):
    """Score `pred` - a `PanopticCloud`, a `VoxelCloud` (their `points`), a `PanopticMesh` (sampled with the same `spacing` and its `face_ids`) or an
    [N, 3] device tensor - against the ground-truth mesh (gt_vertices [Nv,3], gt_faces [Nf,3] on the device), sampled by `sample_mesh` at `spacing`.
    `transform`: a [4, 4] matrix applied to the predicted points first (`similarity_from_cameras`), in fp32 on the device; a mesh's vertices are moved
    before the mesh is sampled, so `spacing` is a length of the ground truth's frame for both surfaces.  `max_dist`, default
    max(thresholds), is the search radius: a point without a counterpart within it is unmatched.  Returns a dict: per threshold tau `precision` (the
    share of predicted points with a ground-truth sample within tau; unmatched points are misses), `recall` (the same from the ground-truth samples
    to the prediction), `fscore` (their harmonic mean, 0 when both are 0), `pred_within`, `gt_within` (the counts: d2 <= float32(tau)^2, exact);
    per direction `accuracy_matched` / `_mean` / `_median` (predicted -> ground truth) and `completeness_*` (ground truth -> predicted): the share of
    points matched within max_dist, and the mean and median distance over those (float64; the median is the lower middle element; nan without a
    match); `chamfer` = accuracy_mean + completeness_mean; n_pred, n_gt, dropped_faces, clamped_faces, thresholds, max_dist, spacing.
    With `gt_vertex_ids` [Nv], `gt_segments` and a labelled `pred`, also `pq3d`: every ground-truth sample takes the panoptic id of its nearest
    predicted point (0 without one within max_dist), and that [1, S] map is scored against the samples' own ids by `panoptic_quality` (`things=`) - PQ
    / SQ / RQ / mIoU over pieces of ground-truth surface; None otherwise.  `refine`: True, or a dict of `refine_alignment` keywords - the alignment
    is refined by ICP on the geometry, starting from `transform`, before anything is scored; its `max_dist` defaults to 4 times the search radius
    (a CHOICE: wide enough for the error a camera fit leaves, narrow enough for the cells to stay small), its `max_cell_points` to this call's.  The
    scores are then those of the refined transform and `alignment` holds the `Alignment`.  Without `refine` the dict has no such key and is what it
    always was.  `metric`: 'points' - every distance above is one to the nearest SAMPLE or predicted point (`nearest_points`), as it always was - or
    'surface': predicted -> ground truth is `mesh_distance` to the ground truth's triangles within max_dist (`max_cell_faces`, `max_pairs` are its
    guards), so `precision`, `pred_within` and `accuracy_*` do not depend on `spacing`; ground truth -> predicted takes the ground-truth samples to
    the triangles of a `PanopticMesh` (moved by `transform` first; `pq3d` takes the `face_ids` of the nearest face), and for a cloud, a voxel cloud or
    a tensor - no surface there - it stays `nearest_points`.  The dict holds `metric`, and under 'surface' also `gt_pairs` and `gt_max_cell_faces`
    (the (face, cell) pairs and the longest cell list of the ground truth's index).  `refine=True` is point-to-point ICP against the samples under
    both metrics, as it always was; `refine={'target': 'surface'}` opts into the point-to-plane ICP against the ground truth's triangles
    (`icp_to_mesh`, stage f13; its `max_cell_faces` and `max_pairs` default to this call's), so that `metric='surface'` measures under an alignment
    fitted to the same triangles.  GPU only."""
    if metric not in ('points', 'surface'):
        raise ValueError("metric must be 'points' or 'surface', got %r" % (metric,))
    if metric == 'surface':
        from .meshdist import _check_limits
        _check_limits(max_cell_faces, max_pairs)                                  # before the GPU is touched
    taus = [_check_length(t, 'a threshold') for t in (thresholds if isinstance(thresholds, (list, tuple, np.ndarray)) else [thresholds])]
    if not taus:
        raise ValueError('score_reconstruction needs at least one threshold')
    spacing = _check_length(spacing, 'spacing')
    radius = max(taus) if max_dist is None else _check_length(max_dist, 'max_dist')
    radius, _, r2 = _check_radius(radius, 'max_dist')
    if max(taus) > radius:
        raise ValueError('threshold %g lies beyond the search radius max_dist = %g' % (max(taus), radius))
    T = None if transform is None else _check_transform(transform)
    if (gt_vertex_ids is None) != (gt_segments is None):
        raise ValueError('gt_vertex_ids and gt_segments go together')
    if refine is not None and refine is not True and refine is not False and not isinstance(refine, dict):
        raise ValueError('refine must be True or a dict of refine_alignment keywords, got %r' % (refine,))
    alignment = None
    if refine is True or isinstance(refine, dict):
        kw = {} if refine is True else dict(refine)
        kw.setdefault('max_dist', 4 * radius)
        if kw.get('target', 'samples') == 'surface':                          # the opt-in of f13: point to plane against the triangles
            kw.setdefault('max_cell_faces', max_cell_faces)
            kw.setdefault('max_pairs', max_pairs)
        else:
            kw.setdefault('max_cell_points', max_cell_points)
        alignment = refine_alignment(pred, gt_vertices, gt_faces, spacing=spacing, init=T, max_subdiv=max_subdiv, **kw)
        T = alignment.transform.numpy()
    points, ids, segments = _pred_points(pred, spacing, max_subdiv, T)
    gt = sample_mesh(gt_vertices, gt_faces, spacing, vertex_ids=gt_vertex_ids, max_subdiv=max_subdiv)
    dev = points.device
    surface = {}
    if metric == 'surface':
        acc, comp, ids, surface = _surface_distances(pred, points, ids, gt, gt_vertices, gt_faces, radius, T, max_cell_points, max_cell_faces, max_pairs)
    else:
        to_gt, to_pred = NearestIndex(gt.points, radius, max_cell_points=max_cell_points), NearestIndex(points, radius, max_cell_points=max_cell_points)
        acc, comp = to_gt.query(points), to_pred.query(gt.points)
        to_gt.check(); to_pred.check()
    n_pred, n_gt = int(points.shape[0]), len(gt)
    out = {'thresholds': taus, 'max_dist': radius, 'spacing': spacing, 'n_pred': n_pred, 'n_gt': n_gt, 'dropped_faces': gt.dropped_faces,
           'clamped_faces': gt.clamped_faces, 'precision': [], 'recall': [], 'fscore': [], 'pred_within': [], 'gt_within': [], 'metric': metric}
    out.update(surface)
    t2 = torch.tensor([float(np.float32(t) * np.float32(t)) for t in taus], dtype=torch.float32, device=dev)
    within = torch.stack([(acc[0][None, :] <= t2[:, None]).sum(1), (comp[0][None, :] <= t2[:, None]).sum(1)]).tolist()
    for a, c in zip(*within):
        p, r = (a / n_pred if n_pred else 0.0), (c / n_gt if n_gt else 0.0)
        out['pred_within'].append(a); out['gt_within'].append(c)
        out['precision'].append(p); out['recall'].append(r); out['fscore'].append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    for name, (d2, row) in (('accuracy', acc), ('completeness', comp)):
        out[name + '_matched'], out[name + '_mean'], out[name + '_median'], _ = _direction(d2, row)
    out['chamfer'] = out['accuracy_mean'] + out['completeness_mean']
    out['pq3d'] = None
    if gt_vertex_ids is not None and ids is not None and segments is not None and n_gt:
        from .evaluate import panoptic_quality
        taken = torch.zeros(n_gt, dtype=torch.int32, device=dev)
        if ids.numel():
            row = comp[1].long()
            taken = torch.where(row >= 0, ids.to(torch.int32)[row.clamp(min=0)], taken)
        out['pq3d'] = panoptic_quality(taken[None, None, :], segments, gt.ids[None, None, :], gt_segments, things=things)
    if alignment is not None:
        out['alignment'] = alignment
    return out
