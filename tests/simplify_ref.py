"""numpy restatement of the mesh simplification by vertex clustering (panst3r_amd/engine/simplify.py, csrc/simplify.hip), the yardstick the kernels
are held to bit for bit, and the hand-built scene of tests/test_hip_simplify.py with the check that it holds every case it was built for.

Own design (the reference has no such stage).  The five steps of the contract in include/panst3r_hip.h:
  1 used     a vertex takes part iff a face names it; a face with a corner outside [0, M) is an error (ValueError here).
  2 cluster  voxel_ref.voxelize (steps 1-5 of the voxel section) of the used vertices in increasing row order with voxel_size = cell_size and palette
             weight 0: one new vertex per occupied cell - mean position, mean colour, voted id - in the order of the cells' smallest member rows;
             cluster[v] = the new row of vertex v, -1 for an unused vertex or one left out.
  3 remap    face f -> cluster[face f]; left out if a corner is -1, else degenerate if two corners are equal; both dropped, counted separately.
  4 dedupe   of the remaining faces with one unordered corner set the one with the smallest f survives, whatever its winding; needs at most 2^21 - 2
             new vertices (ValueError above).
  5 emit     the survivors in the order of the originals, the new corners in the original corner order, the original's quad, src_face = f, face id =
             the id at least two corners' new vertex ids share, else 0.
A mesh without faces, or one whose every face is dropped, is a mesh of zero faces AND zero vertices (cluster all -1, vertices_out 0)."""
import numpy as np

import voxel_ref as V

F = np.float32
MAX_KEYED = 2 ** 21 - 2
STAT_KEYS = ('vertices_in', 'vertices_used', 'vertices_left_out', 'vertices_out', 'faces_in', 'faces_left_out', 'faces_degenerate', 'faces_duplicate',
             'faces_out')


def face_id(ids):
    """[n, 3] int -> the id two corners share, else 0"""
    a, b, c = ids[:, 0], ids[:, 1], ids[:, 2]
    return np.where((a == b) | (a == c), a, np.where(b == c, b, 0)).astype(np.int32)


def _empty(M, stats):
    stats = dict(stats, vertices_out=0, faces_out=0)
    return {'vertices': np.zeros((0, 3), F), 'colors': np.zeros((0, 3), F), 'vertex_ids': np.zeros(0, np.int32), 'faces': np.zeros((0, 3), np.int32),
            'face_ids': np.zeros(0, np.int32), 'quad': np.zeros(0, np.int64), 'src_face': np.zeros(0, np.int32), 'cluster': np.full(M, -1, np.int32),
            'stats': stats}


def simplify(vertices, colors, vertex_ids, faces, quad, segment_ids, cell_size, dedupe=True, detail=False):
    """vertices, colors [M, 3] float32, vertex_ids [M] int, faces [F, 3] int, quad [F] int64, segment_ids: the listed ids.  Returns dict(vertices, colors,
    vertex_ids, faces, face_ids, quad, src_face, cluster, stats); detail=True adds what `scene_conditions` looks at."""
    vertices, colors = np.asarray(vertices, dtype=F).reshape(-1, 3), np.asarray(colors, dtype=F).reshape(-1, 3)
    vertex_ids, faces, quad = np.asarray(vertex_ids).astype(np.int32).reshape(-1), np.asarray(faces).astype(np.int64).reshape(-1, 3), np.asarray(quad).astype(np.int64)
    M, Fn = len(vertices), len(faces)
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats.update(vertices_in=M, faces_in=Fn)
    if Fn == 0:
        return _empty(M, stats)
    if ((faces < 0) | (faces >= M)).any():
        raise ValueError('a face names a vertex outside the vertex rows')
    used = np.zeros(M, dtype=bool)                                                                    # step 1
    used[faces.reshape(-1)] = True
    rows = np.nonzero(used)[0]
    vox = V.voxelize(vertices[rows], colors[rows], vertex_ids[rows], rows, segment_ids, cell_size, np.zeros((1, 3), F), opacity=0.0)      # step 2
    cluster = np.full(M, -1, dtype=np.int32)
    cluster[rows] = vox['point_voxel']
    Mv = len(vox['pan'])
    stats.update(vertices_used=len(rows), vertices_left_out=vox['dropped'], vertices_out=Mv)
    n = cluster[faces]                                                                                # step 3
    left = (n < 0).any(axis=1)
    deg = ~left & ((n[:, 0] == n[:, 1]) | (n[:, 0] == n[:, 2]) | (n[:, 1] == n[:, 2]))
    cand = np.nonzero(~left & ~deg)[0]
    stats.update(faces_left_out=int(left.sum()), faces_degenerate=int(deg.sum()))
    keep = cand
    if dedupe:                                                                                        # step 4
        if Mv > MAX_KEYED:
            raise ValueError('%d new vertices exceed the 2^21 - 2 of dedupe' % Mv)
        if len(cand):
            s = np.sort(n[cand].astype(np.int64), axis=1)
            key = (s[:, 0] + 1) | ((s[:, 1] + 1) << 21) | ((s[:, 2] + 1) << 42)
            _, first = np.unique(key, return_index=True)                                              # the first occurrence: cand ascends, so the smallest f
            keep = np.sort(cand[first])
    stats.update(faces_duplicate=len(cand) - len(keep), faces_out=len(keep))
    if len(keep) == 0:
        return _empty(M, stats)
    nf = n[keep].astype(np.int32)                                                                     # step 5
    out = {'vertices': vox['points'], 'colors': vox['rgb'], 'vertex_ids': vox['pan'], 'faces': nf, 'face_ids': face_id(vox['pan'][nf]), 'quad': quad[keep],
           'src_face': keep.astype(np.int32), 'cluster': cluster, 'stats': stats}
    if detail:
        out.update(used=used, new=n, left=left, degenerate=deg, candidates=cand, count=vox['count'])
    return out


# ---------------------------------------------------------------- the scene of the GPU test
CELL = 0.25                        # inv = 4 exactly: a coordinate that is a multiple of 0.25 lies ON a cell wall
SEGMENT_IDS = tuple(range(1, 9))   # listed; 99 is carried by vertices but is in no list
N_SHEET = 36


def scene(seed=0):
    """-> dict(vertices, colors, vertex_ids, faces, quad, marks): two coincident 36 x 36 sheets on disjoint vertex rows (the second with seeded noise
    and relabelled vertices) around the origin, so cells with negative coordinates, and hand-written pieces far from them; unused rows in between."""
    g = np.random.Generator(np.random.PCG64(seed))
    verts, ids, faces, marks = [], [], [], {}

    def add(p, i):
        verts.append(np.asarray(p, dtype=np.float64))
        ids.append(int(i))
        return len(verts) - 1

    def pad_to_lane(lane, filler):
        while len(faces) % 64 != lane:
            faces.append(filler)

    def sheet(noise, relabel):
        base = len(verts)
        for j in range(N_SHEET):
            for i in range(N_SHEET):
                p = np.array([-1.8 + 0.1 * i + 0.013, -1.7 + 0.1 * j + 0.021, 0.1 + 0.02 * np.sin(0.7 * i + 0.3 * j)])
                lab = 1 + i // 9 + 4 * (j // 18)
                if relabel:
                    u = g.uniform()
                    lab = int(g.integers(1, 9)) if u < 0.25 else 0 if u < 0.30 else 99 if u < 0.35 else lab
                    p = p + g.standard_normal(3) * noise
                add(p, lab)
        out = []
        for j in range(N_SHEET - 1):
            for i in range(N_SHEET - 1):
                a = base + j * N_SHEET + i
                out += [(a, a + N_SHEET, a + N_SHEET + 1), (a, a + N_SHEET + 1, a + 1)]
        return out

    for k in range(3):
        add((0.3 * k, 5.0, 5.0), 1)                                              # rows that no face names
    faces_a = sheet(0.0, False)
    for k in range(4):
        add((0.05, 0.05, 0.1 + 0.01 * k), 7)                                     # unused, inside a cell of the sheets: they must not vote there
    # hand-written pieces, every one in cells of its own
    t1 = [add((10.25, 10.5, 10.0), 1), add((11.1, 10.1, 10.1), 2), add((10.1, 11.1, 10.1), 3)]      # one member per cell, ON cell walls; three ids
    t2 = [add((12.1, 10.1, 10.1), 4), add((13.1, 10.1, 10.1), 4), add((12.1, 11.1, 10.1), 5)]       # two corners share an id
    t3 = [add((14.1, 10.1, 10.1), 6), add((15.1, 10.1, 10.1), 6), add((14.1, 11.1, 10.1), 6)]       # three do
    tie = [add((16.10, 10.1, 10.1), 5), add((16.12, 10.1, 10.1), 3)]                                  # a tie: the smaller id, 3
    void = [add((17.10, 10.1, 10.1), 0), add((17.12, 10.1, 10.1), 99), add((17.14, 10.1, 10.1), -1)]  # void votes only: id 0
    weak = [add((18.10, 10.1, 10.1), 0), add((18.12, 10.1, 10.1), 0), add((18.14, 10.1, 10.1), 8)]    # void wins only alone: 8
    nan = add((np.nan, 10.1, 10.1), 1)
    far = add((3.0e5, 10.1, 10.1), 1)                                            # cell 1.2e6 >= 2^20
    marks.update(t1=t1, t2=t2, t3=t3, tie=tie, void=void, weak=weak, nan=nan, far=far)
    faces_b = sheet(1e-3, True)
    fan0 = len(verts)
    for k in range(100):                                                         # 100 consecutive rows in one cell: a run across a wave's edge
        add(20.1 + g.uniform(0, 0.05, 3), 2)
    add((0.0, 6.0, 5.0), 2)                                                      # the last row: unused
    fan = [(fan0 + k, fan0 + k + 1, fan0 + k + 2) for k in range(98)]            # three equal new corners
    filler = fan[0]
    faces += faces_a
    faces += [(nan, t1[0], t1[1]), (far, t2[0], t2[1]), (t3[0], t3[0], t3[1])]   # left out twice; degenerate in the input
    faces += [tuple(reversed(t3)), (t2[1], t2[2], t2[0])]                        # t3 reversed and t2 rotated come BEFORE their plain copies
    pad_to_lane(63, filler)
    marks['t1_first'] = len(faces)
    faces += [tuple(t1), tuple(t1), tuple(t1)]                                   # a triple copy: the winner in a wave's last lane, a run of two in the next wave
    faces += faces_b
    faces += fan
    faces += [tuple(t2), tuple(t3), tuple(t1)]
    faces += [(tie[0], void[0], weak[0]), (tie[1], void[1], weak[1]), (tie[0], void[2], weak[2])]     # three input faces, one new face
    vertices = np.stack(verts).astype(F)
    colors = g.uniform(-0.1, 1.1, vertices.shape).astype(F)
    colors[5, 1] = np.nan
    faces = np.asarray(faces, dtype=np.int32)
    quad = (np.arange(len(faces), dtype=np.int64) * 7 + 3) % 100003
    return {'vertices': vertices, 'colors': colors, 'vertex_ids': np.asarray(ids, dtype=np.int32), 'faces': faces, 'quad': quad, 'marks': marks}


def of_scene(sc, dedupe=True, detail=False, cell=CELL):
    return simplify(sc['vertices'], sc['colors'], sc['vertex_ids'], sc['faces'], sc['quad'], SEGMENT_IDS, cell, dedupe, detail)


def scene_conditions(sc):
    """asserts ON THE RESTATEMENT that the scene holds every case the kernels can get wrong; returns (with dedupe, without)"""
    r, r0 = of_scene(sc, True, True), of_scene(sc, False, True)
    v, ids, faces, marks, st = sc['vertices'], sc['vertex_ids'], sc['faces'].astype(np.int64), sc['marks'], r['stats']
    M, Fn = len(v), len(faces)
    assert 2 * 1024 < M < 3 * 1024 and 19 * 256 < Fn < 22 * 256                 # more than two workgroups of the voxel stage, a scan with a carry; of the face kernels
    used, cluster, n = r['used'], r['cluster'], r['new']
    assert (~used).sum() == 8 and not used[0] and not used[M - 1] and (cluster[~used] == -1).all()
    assert used[marks['nan']] and used[marks['far']] and cluster[marks['nan']] == -1 and cluster[marks['far']] == -1
    assert st['vertices_left_out'] == 2 and st['vertices_used'] == M - 8 and st['faces_left_out'] == 2
    t, c, keep = V.cells(v, CELL)
    ok = used & keep
    assert (c[ok] < 0).any() and (c[ok] > 0).any() and ((t[ok] == c[ok]).any(axis=1) & (t[ok] != 0).all(axis=1)).any()       # negative cells; ON a wall
    assert np.array_equal(np.nonzero(ok)[0], np.nonzero(cluster >= 0)[0])
    count = r['count']
    assert (count == 1).any() and (count > 64).any() and count.sum() == ok.sum()
    # the unused rows inside an occupied cell did not join it
    key = lambda cc: (cc[:, 0].astype(np.int64) * 4096 + cc[:, 1].astype(np.int64)) * 4096 + cc[:, 2].astype(np.int64)
    assert np.isin(key(c[np.nonzero(~used)[0][3:7]]), key(c[ok])).all()
    # votes: per new vertex the listed ids of its members
    listed = np.isin(ids, SEGMENT_IDS) & (ids > 0)
    tie_seen = void_seen = False
    for row in range(st['vertices_out']):
        mem = np.nonzero(cluster == row)[0]
        votes = np.bincount(ids[mem][listed[mem]], minlength=10)
        if votes.sum() == 0:
            void_seen = True
            assert r['vertex_ids'][row] == 0
            continue
        top = np.sort(votes)[::-1]
        if top[0] == top[1]:
            tie_seen = True
        assert r['vertex_ids'][row] == int(np.argmax(votes))                     # argmax: the first, so the smallest, of the ids with the most votes
    assert tie_seen and void_seen
    assert r['vertex_ids'][cluster[marks['tie'][0]]] == 3 and r['vertex_ids'][cluster[marks['void'][0]]] == 0 and r['vertex_ids'][cluster[marks['weak'][0]]] == 8
    # faces
    eq = (n[:, 0] == n[:, 1]).astype(int) + (n[:, 0] == n[:, 2]) + (n[:, 1] == n[:, 2])
    live = ~r['left']
    assert (live & (eq == 1)).any() and (live & (eq == 3)).any() and st['faces_degenerate'] == int((live & (eq > 0)).sum())
    raw_deg = (faces[:, 0] == faces[:, 1]) | (faces[:, 0] == faces[:, 2]) | (faces[:, 1] == faces[:, 2])
    assert raw_deg.any() and r['degenerate'][raw_deg].all()
    cand = r['candidates']
    s = np.sort(n[cand], axis=1)
    _, inverse, sizes = np.unique(s, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    rotation = reverse = triple = split = False
    for grp in np.nonzero(sizes > 1)[0]:
        mem = cand[inverse == grp]                                               # ascending: mem[0] wins
        w = n[mem[0]]
        for f in mem[1:]:
            x = n[f]
            rolls = [np.array_equal(np.roll(x, k), w) for k in range(3)]
            rotation |= any(rolls[1:])
            reverse |= not any(rolls)
            split |= f // 256 != mem[0] // 256
        triple |= len(mem) >= 3 and all(np.array_equal(faces[f], faces[mem[0]]) for f in mem[:3])
        assert np.isin(mem[0], r['src_face']) and not np.isin(mem[1:], r['src_face']).any()
    assert rotation and reverse and triple and split
    f0 = marks['t1_first']
    assert f0 % 64 == 63 and [tuple(faces[f0 + k]) for k in range(3)] == [tuple(marks['t1'])] * 3 and f0 in r['src_face']     # the winner in a wave's last lane, a run of two in the next
    rev = np.nonzero((faces == np.array(marks['t3'][::-1])).all(axis=1))[0][0]
    assert rev in r['src_face'] and np.array_equal(r['faces'][r['src_face'] == rev][0], cluster[marks['t3'][::-1]])              # the reversed copy came first: its winding stays
    new_ids = r['vertex_ids'][r['faces']]
    same = (new_ids[:, 0] == new_ids[:, 1]).astype(int) + (new_ids[:, 0] == new_ids[:, 2]) + (new_ids[:, 1] == new_ids[:, 2])
    assert (same == 0).any() and (same == 1).any() and (same == 3).any() and (r['face_ids'][same == 0] == 0).all() and (r['face_ids'][same == 1] > 0).any()
    assert (np.diff(r['src_face']) > 0).all() and np.array_equal(r['quad'], sc['quad'][r['src_face']])
    # dedupe=False: every candidate, nothing else differs
    assert st['faces_duplicate'] > 100 and r0['stats']['faces_duplicate'] == 0 and r0['stats']['faces_out'] == st['faces_out'] + st['faces_duplicate'] == len(cand)
    assert st['faces_in'] == Fn == st['faces_left_out'] + st['faces_degenerate'] + st['faces_duplicate'] + st['faces_out']
    assert np.array_equal(r0['src_face'], cand) and np.array_equal(r0['vertices'], r['vertices'], equal_nan=True)
    assert 100 < st['vertices_out'] < st['vertices_used'] // 4 and 200 < st['faces_out'] < Fn // 4
    return r, r0


def random_mesh(M, Fn, seed, box=2.0):
    """M vertices in a box, Fn faces of random corners (some repeated): the sizes of the workgroup-edge cases"""
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.uniform(-box, box, (M, 3)).astype(F)
    faces = g.integers(0, M, (Fn, 3)).astype(np.int32)
    return {'vertices': v, 'colors': g.uniform(0, 1, (M, 3)).astype(F), 'vertex_ids': g.integers(0, 9, M).astype(np.int32), 'faces': faces,
            'quad': np.arange(Fn, dtype=np.int64), 'marks': {}}


# ---------------------------------------------------------------- closed forms (tests/test_simplify_host.py)
def grid_plane(k, s, z=0.3):
    """a (2k+1) x (2k+1) vertex grid with spacing s whose lattice is offset by s / 2 from the walls of cells of edge 2 s: vertex (i, j) at
    ((i + 0.5) s, (j + 0.5) s, z); two triangles per grid square -> (vertices float32, faces int32)"""
    n = 2 * k + 1
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = np.stack([(i + 0.5) * s, (j + 0.5) * s, np.full((n, n), z)], axis=-1).reshape(-1, 3).astype(F)
    a = (j[:-1, :-1] * n + i[:-1, :-1]).reshape(-1)
    faces = np.stack([np.stack([a, a + n, a + n + 1], axis=1), np.stack([a, a + n + 1, a + 1], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    return v, faces
