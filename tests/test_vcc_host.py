"""Host side of the connected components of the voxel cloud and of the label despeckling (panst3r_amd/engine/voxels.py, csrc/components.hip): known
answers of the numpy restatement the GPU tests compare against (tests/vcc_ref.py), and the product's side without a GPU - the C ABI, the refusals,
the handling of the device status word.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import vcc_ref as R

LIM = 1 << 20
VCC_SYMBOLS = ['pst_vcc_apply', 'pst_vcc_build', 'pst_vcc_cells', 'pst_vcc_count', 'pst_vcc_flatten', 'pst_vcc_link', 'pst_vcc_rank', 'pst_vcc_votes']


def comp(cells, pan, connectivity=26, count=None):
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 3)
    return R.components(cells, pan, np.ones(len(cells), dtype=np.int32) if count is None else count, connectivity)


def cube_pair(shift):
    """two unit cubes (one cell each would touch by definition: 2 x 2 x 2 cells each), the second moved by `shift` cells"""
    a = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    return np.concatenate([a, a + np.array(shift)])


@pytest.mark.parametrize('shift, want', [((2, 0, 0), (1, 1, 1)), ((2, 2, 0), (2, 1, 1)), ((2, 2, 2), (2, 2, 1))])
def test_contacts_by_face_edge_and_corner(shift, want):
    cells = cube_pair(shift)
    got = tuple(len(comp(cells, [3] * 16, c)['size']) for c in (6, 18, 26))
    assert got == want
    # single cells instead of cubes: the same answers
    one = np.array([(0, 0, 0), tuple(s // 2 for s in shift)])
    assert tuple(len(comp(one, [3, 3], c)['size']) for c in (6, 18, 26)) == want
    assert [len(R.offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]


def test_two_ids_stay_separate_and_void_gets_minus_one():
    cells = cube_pair((2, 0, 0))
    pan = [3] * 8 + [4] * 8
    c = comp(cells, pan)
    assert c['size'].tolist() == [8, 8] and c['pan'].tolist() == [3, 4] and c['roots'].tolist() == [0, 8]
    pan = [3, 3, 0, 3, -2, 3, 3, 3] + [3] * 8                                  # void voxels in the middle of a block
    c = comp(cells, pan)
    assert c['root'].tolist() == [0, 0, -1, 0, -1] + [0] * 11 and c['component'].tolist() == [0, 0, -1, 0, -1] + [0] * 11
    assert c['size'].tolist() == [14] and c['points'].tolist() == [14]
    # void does not connect: a line 5 - 0 - 5 is two components
    c = comp([(0, 0, 0), (1, 0, 0), (2, 0, 0)], [5, 0, 5])
    assert c['root'].tolist() == [0, -1, 2] and c['component'].tolist() == [0, -1, 1]
    # no voxel at all, and only void ones
    assert len(comp(np.zeros((0, 3)), [])['size']) == 0 and comp([(1, 1, 1)], [0])['root'].tolist() == [-1]


def test_root_is_the_smallest_row_under_a_shuffled_order():
    g = np.random.Generator(np.random.PCG64(3))
    line = np.array([(i, 0, 0) for i in range(40)] + [(i, 5, 0) for i in range(25)] + [(0, 9, i) for i in range(7)])
    pan = np.array([1] * 40 + [1] * 25 + [2] * 7)
    perm = g.permutation(len(line))
    cells, p = line[perm], pan[perm]
    c = comp(cells, p, 6)
    group = np.array([0] * 40 + [1] * 25 + [2] * 7)[perm]
    want_root = np.array([np.nonzero(group == k)[0].min() for k in range(3)])
    assert np.array_equal(c['root'], want_root[group])
    assert np.array_equal(c['roots'], np.sort(want_root))                      # components in the order of their roots
    assert np.array_equal(c['component'], np.argsort(np.argsort(want_root))[group])
    assert sorted(c['size'].tolist()) == [7, 25, 40]


def test_table_of_an_l_shaped_component():
    cells = [(2, -1, 7), (3, -1, 7), (4, -1, 7), (4, 0, 7), (4, 1, 7), (10, 10, 10)]
    c = comp(cells, [6, 6, 6, 6, 6, 6], 6, count=[5, 1, 2, 70000, 3, 9])
    assert c['size'].tolist() == [5, 1] and c['points'].tolist() == [70011, 9] and c['points'].dtype == np.int64
    assert c['cell_lo'].tolist() == [[2, -1, 7], [10, 10, 10]] and c['cell_hi'].tolist() == [[4, 1, 7], [10, 10, 10]]
    lo, hi = R.boxes(c, 0.25)
    assert lo.dtype == np.float64 and lo.tolist() == [[0.5, -0.25, 1.75], [2.5, 2.5, 2.5]] and hi.tolist() == [[1.25, 0.5, 2.0], [2.75, 2.75, 2.75]]
    # a count beyond 32 bits in total
    c = comp([(0, 0, 0), (1, 0, 0), (2, 0, 0)], [1, 1, 1], count=[2 ** 30, 2 ** 30, 2 ** 30])
    assert c['points'].tolist() == [3 * 2 ** 30]


def test_cells_at_the_ends_of_the_range_have_no_neighbour_beyond_it():
    e = LIM - 1
    # the neighbours of (e, 0, 0) at x + 1 and of (-e, ., .) at x - 1 do not exist: no key is formed for them (the x field would carry into y)
    cells = [(e, 0, 0), (-e, 1, 0), (e, e, e), (-e, -e, -e), (e - 1, 0, 0), (-e, 0, 0), (-3, -4, -5), (-2, -4, -5), (0, 0, 0), (-1, -1, -1)]
    c = comp(cells, [1] * len(cells))
    v, n = R.pairs(np.array(cells), 26)
    got = sorted((int(a), int(b)) for a, b in zip(v, n))
    assert got == [(0, 4), (1, 5), (4, 0), (5, 1), (6, 7), (7, 6), (8, 9), (9, 8)]
    assert c['root'].tolist() == [0, 1, 2, 3, 0, 1, 6, 6, 8, 8]
    assert comp(cells, [1] * len(cells), 6)['root'].tolist() == [0, 1, 2, 3, 0, 1, 6, 6, 8, 9]
    with pytest.raises(AssertionError):
        R.pairs(np.array([(LIM, 0, 0)]), 26)


def slab(n=5):
    return [(x, y, 0) for y in range(n) for x in range(n)]


def test_a_single_wrong_voxel_inside_a_slab_takes_the_slabs_id():
    cells = slab()
    pan = [2] * 25
    pan[12] = 7
    out, moved, gone = R.clean_pan(cells, pan, np.ones(25), 2, 26)
    assert out.tolist() == [2] * 25 and (moved, gone) == (1, 0)
    out, moved, gone = R.clean_pan(cells, pan, np.ones(25), 1, 26)             # min_voxels = 1: nothing is small
    assert out.tolist() == pan and (moved, gone) == (0, 0)


def test_ties_go_to_the_smallest_id_and_void_does_not_vote():
    # the middle voxel sees one 5, one 3 (a tie) and two void voxels
    cells = [(0, 0, 0), (-1, 0, 0), (-2, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, -1, 0)]
    pan = [9, 5, 5, 3, 3, 0, -4]
    out, moved, gone = R.clean_pan(cells, pan, np.ones(7), 2, 6)
    assert out.tolist() == [3, 5, 5, 3, 3, 0, -4] and (moved, gone) == (1, 0)
    # void neighbours alone: a floater
    out, moved, gone = R.clean_pan([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [9, 0, 0], np.ones(3), 2, 6)
    assert out.tolist() == [0, 0, 0] and (moved, gone) == (0, 1)


def test_a_small_component_whose_only_neighbours_are_small_becomes_void():
    cells = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (10, 0, 0), (11, 0, 0), (12, 0, 0)]
    pan = [1, 2, 1, 2, 4, 4, 4]
    out, moved, gone = R.clean_pan(cells, pan, np.ones(7), 3, 26)
    assert out.tolist() == [0, 0, 0, 0, 4, 4, 4] and (moved, gone) == (0, 4)
    # everything is small: everything becomes void
    out, moved, gone = R.clean_pan(cells, pan, np.ones(7), 4, 26)
    assert out.tolist() == [0] * 7 and gone == 7


def test_votes_count_pairs_not_distinct_neighbours():
    """the small component {a, b} of id 9; ONE voxel of id 5 touches both a and b (two pairs), ONE voxel of id 3 touches b only (one pair).  Counting
    pairs, 5 wins 2 : 1; counting distinct neighbours it would be a 1 : 1 tie, which goes to 3."""
    cells = [(0, 0, 0), (1, 0, 0),               # a, b
             (0, 1, 0), (0, 2, 0), (0, 3, 0),   # id 5: only (0, 1, 0) touches, a and b
             (2, 0, 0), (3, 0, 0), (4, 0, 0)]   # id 3: only (2, 0, 0) touches, b
    pan = [9, 9, 5, 5, 5, 3, 3, 3]
    out, moved, gone = R.clean_pan(cells, pan, np.ones(8), 3, 26)
    assert out.tolist() == [5, 5, 5, 5, 5, 3, 3, 3] and (moved, gone) == (2, 0)
    # a second voxel of id 3 that touches b: 2 : 2 pairs, the tie goes to 3
    cells, pan = cells + [(2, -1, 0)], pan + [3]
    out, moved, gone = R.clean_pan(cells, pan, np.ones(9), 3, 26)
    assert out.tolist() == [3, 3, 5, 5, 5, 3, 3, 3, 3]
    # at connectivity 6 (0, 1, 0) touches a only and (2, -1, 0) nothing: 1 : 1, to 3 again; a and b vote as ONE component
    out, moved, gone = R.clean_pan(cells, pan, np.ones(9), 3, 6)
    assert out[:2].tolist() == [3, 3]


def test_clean_reblends_the_colours_and_rebuilds_the_segments():
    colors = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    cells = slab(3)
    pan = np.array([1] * 9, dtype=np.int32)
    pan[4] = 3
    vox = {'pan': pan, 'count': np.ones(9, dtype=np.int32), 'rgb': np.full((9, 3), 0.5, dtype=np.float32),
           'points': np.array(cells, dtype=np.float32), 'colors': np.zeros((9, 3), dtype=np.float32)}
    info = [{'id': 1}, {'id': 3}]
    out, segs = R.clean(vox, cells, info, colors, 2, 26, opacity=0.5)
    assert out['pan'].tolist() == [1] * 9 and out['relabelled'] == 1 and out['floaters'] == 0
    assert out['colors'].tolist() == [[0.75, 0.25, 0.25]] * 9 and vox['pan'][4] == 3          # the input is untouched
    assert [s['id'] for s in segs] == [1] and segs[0]['count'] == 9
    same, segs1 = R.clean(vox, cells, info, colors, 1, 26, opacity=0.5)
    assert np.array_equal(same['pan'], pan) and [s['count'] for s in segs1] == [8, 1]


# ---------------------------------------------------------------- the product, without a GPU
def test_header_signatures_and_library_agree_on_the_vcc_symbols():
    from panst3r_amd import hip
    from panst3r_amd.build import build
    declared = sorted(p[0] for p in abi_header.prototypes() if p[0].startswith('pst_vcc_'))
    assert declared == VCC_SYMBOLS == sorted(s for s in hip.SIGNATURES if s.startswith('pst_vcc_'))
    lib = ctypes.CDLL(build(verbose=False))
    for s in declared:
        assert hasattr(lib, s), s
    assert hip.ABI_VERSION == 20 == abi_header.defines()['PST_ABI_VERSION']    # additive entry points: the version stays
    d = abi_header.defines()
    assert (d['PST_VCC_FULL'], d['PST_VCC_DUPLICATE'], d['PST_VCC_RANGE'], d['PST_VCC_LOOP']) == (hip.VCC_FULL, hip.VCC_DUPLICATE, hip.VCC_RANGE, hip.VCC_LOOP)
    import panst3r_amd.ops as O
    for s in declared:
        assert s[4:] in O.registered_ops() and hasattr(torch.ops.panst3r_hip, s[4:]) and hasattr(hip, s[4:])
    assert hip.VCC_MERGE in (0, 1)
    assert [hip.vcc_pair_capacity(m, n) for m, n in ((1, 1), (100, 3), (100, 26), (100, 500), (2 ** 30, 26))] == [2, 1024, 8192, 8192, 2 ** 31]


def hand_voxels(cells=True, n=4):
    from panst3r_amd.engine import VoxelCloud
    pts = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    ones = torch.ones(n, dtype=torch.int32)
    return VoxelCloud(pts, pts, ones, pts, ones, ones, torch.arange(n), torch.arange(n, dtype=torch.int32), [], None, [0, n], 1.0, 0,
                      cells=pts.to(torch.int32) if cells else None)


def test_the_constructor_keeps_cells_and_cpu_carries_them():
    v = hand_voxels()
    assert v.cells.dtype == torch.int32 and tuple(v.cells.shape) == (4, 3) and torch.equal(v.cpu().cells, v.cells)
    assert hand_voxels(cells=False).cells is None and hand_voxels(cells=False).cpu().cells is None
    assert v.relabelled is None and v.floaters is None


def test_refusals_without_a_gpu():
    from panst3r_amd.engine import voxel_components, clean_voxel_labels
    v = hand_voxels()
    for bad in (0, 4, 8, 27, '26', None, 6.5):
        with pytest.raises(ValueError, match='connectivity'):
            v.components(bad)
        with pytest.raises(ValueError, match='connectivity'):
            v.clean_labels(2, bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='min_voxels'):
            v.clean_labels(bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):                 # a CPU cloud
        voxel_components(v)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clean_voxel_labels(v, 2)
    with pytest.raises(RuntimeError, match='does not hold the cells'):         # built by hand without cells
        hand_voxels(cells=False).components()
    with pytest.raises(RuntimeError, match='does not hold the cells'):
        hand_voxels(cells=False).clean_labels(2)


def test_reconstruct_refuses_min_component_voxels_before_the_forward_pass():
    from panst3r_amd.panst3r import PanSt3R

    class Never:
        def forward_inference_multi_ar(self, *a, **k):
            raise AssertionError('the forward pass ran')
    with pytest.raises(ValueError, match='only together with voxel_size'):
        PanSt3R.reconstruct(Never(), [], None, [], min_component_voxels=4)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='min_voxels'):
            PanSt3R.reconstruct(Never(), [], None, [], voxel_size=0.1, min_component_voxels=bad)


def test_a_status_word_reported_by_the_device_raises():
    from panst3r_amd import hip
    from panst3r_amd.engine.voxels import check_vcc_status
    check_vcc_status(np.int32(0))
    for bit, text in ((hip.VCC_FULL, 'ran full'), (hip.VCC_DUPLICATE, 'share one cell'), (hip.VCC_RANGE, 'outside'), (hip.VCC_LOOP, 'reached its bound')):
        with pytest.raises(RuntimeError, match=text):
            check_vcc_status(np.int32(bit))
