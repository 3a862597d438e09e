"""The numpy restatement of the cross-view depth consistency (tests/consistency_ref.py) against closed forms, so that it is not its own judge, and the
host side of panst3r_amd/engine/consistency.py: the keep rule, the masked confidence planes, the camera tables and the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

import abi_header
import consistency_ref as R
from panst3r_amd import hip
from panst3r_amd.engine import consistency as E
from panst3r_amd.engine import view_consistency, ViewConsistency
from panst3r_amd.engine.cloud import consistency_keywords

F = np.float32


def test_plane_scene_matches_its_closed_form():
    """pixel x of view i lands on pixel x + 32 (t_i - t_j) of view j: agree = the number of j for which that is inside [0, 32), violate = 0"""
    x, cams, focals, pan = R.plane_scene()
    agree, violate = R.plane_closed_form()
    for local in (False, True):
        res = R.consistency(x, cams, focals, min_conf_thr=3.0, rel_tol=0.01, pan=pan, local_pointmaps=local, pp=R.PLANE_PP)
        assert np.array_equal(res['agree'], agree) and np.array_equal(res['violate'], violate) and not violate.any()
        assert np.array_equal(res['same_label'], agree)                       # ids follow the world column: every agreeing pair carries equal ids
        assert np.array_equal(res['depth'], np.full(len(agree), 2.0, dtype=F))
    H, W = R.PLANE_SHAPE
    a = agree.reshape(4, H, W)
    assert a.min() == 0 and a.max() == 2 and (a == a[:, :1]).all()            # the closed form itself: rows are equal, some pixels are seen by nobody
    assert a[0, 0].tolist() == [sum(0 <= xx + 32 * (0.0 - t) < W for t in R.PLANE_TX[1:]) for xx in range(W)]


def test_floaters_violate_and_hide_what_is_behind_them():
    """view 0's patch at half depth shifts by 64 (t_0 - t_j), agrees with nobody and violates every view it lands inside"""
    x, cams, focals, pan = R.plane_scene(floaters=True)
    agree, violate = R.plane_closed_form(floaters=True)
    res = R.consistency(x, cams, focals, min_conf_thr=3.0, rel_tol=0.01, pan=pan, pp=R.PLANE_PP)
    assert np.array_equal(res['agree'], agree) and np.array_equal(res['violate'], violate)
    H, W = R.PLANE_SHAPE
    patch = np.zeros((4, H, W), dtype=bool)
    patch[0][R.PATCH] = True
    patch = patch.reshape(-1)
    assert (agree[patch] == 0).all() and violate[patch].max() >= 1 and (violate[~patch] == 0).all()
    inside = [sum(0 <= xx + 64 * (0.0 - t) < W for t in R.PLANE_TX[1:]) for xx in range(W)]
    assert violate.reshape(4, H, W)[0][R.PATCH][0].tolist() == inside[R.PATCH[1]]
    clean = R.plane_closed_form()[0]
    assert (agree <= clean).all() and (agree < clean).any()                   # the plane behind a floater is occluded in view 0: one agreeing view fewer
    kept = R.keep(res, 1, 0)
    assert not kept[patch & (violate > 0)].any()


def test_tolerance_edges():
    """|zc - d| == rel_tol d agrees (a tie), one ulp beyond does not: farther is occluded, nearer violates"""
    d, tol = F(2.0), F(0.25)
    up, dn = np.nextafter(F(2.5), F(np.inf)), np.nextafter(F(1.5), F(-np.inf))
    zc = np.array([2.5, up, 1.5, dn, 2.0], dtype=F)
    ag, vi = R.compare(zc, np.full(5, d), tol)
    assert ag.tolist() == [True, False, True, False, True] and vi.tolist() == [False, False, False, True, False]
    ag, vi = R.compare(zc, np.full(5, d), 0.0)                                # rel_tol = 0: only equality agrees
    assert ag.tolist() == [False, False, False, False, True] and vi.tolist() == [False, False, True, True, False]
    ag, vi = R.compare(np.array([np.nan, 2.0], dtype=F), np.array([2.0, np.nan], dtype=F), tol)
    assert not ag.any() and not vi.any()                                      # a NaN fails every test
    # the same through the whole restatement: two views at one pose, view 1 at depth 2, view 0's pixels on their rays at the edge depths
    x, cams, focals = R.edge_scene(zc[:4])
    res = R.consistency(x, cams, focals, min_conf_thr=3.0, rel_tol=0.25, pp=(2.0, 1.0))
    assert res['agree'][:4].tolist() == [1, 0, 1, 0] and res['violate'][:4].tolist() == [0, 0, 0, 1]


def test_projections_round_to_the_nearest_pixel_centre():
    """u + 0.5 = W is column W (out), just below it column W - 1 (in); u + 0.5 = 0 is column 0 (in), just below it column -1 (out); rows likewise"""
    x, cams, focals, idx, inside = R.border_scene()
    assert inside == [False, True, True, False, False, True, True, False]
    res = R.consistency(x, cams, focals, min_conf_thr=3.0, rel_tol=0.0, pp=(4.0, 3.0))
    assert res['agree'][idx].tolist() == [int(s) for s in inside] and not res['violate'].any()
    rest = np.setdiff1d(np.arange(2 * 48), idx)
    assert (res['agree'][rest] == 1).all()                                    # every other pixel lands on itself in the other view, exactly


def test_keep_and_masked_conf():
    agree = torch.tensor([0, 1, 2, 3, 1, 0], dtype=torch.int32)
    violate = torch.tensor([0, 0, 1, 2, 1, 3], dtype=torch.int32)
    assert E.keep_mask(agree, violate).tolist() == [False, True, False, False, False, False]
    assert E.keep_mask(agree, violate, 0, 0).tolist() == [True, True, False, False, False, False]
    assert E.keep_mask(agree, violate, 2, 1).tolist() == [False, False, True, False, False, False]
    vc = ViewConsistency(agree, violate, None, torch.ones(6), [0, 6], [(2, 3)])
    assert vc.keep(1, 1).tolist() == [False, True, True, False, True, False] and len(vc) == 6
    assert [tuple(m.shape) for m in vc.maps('agree')] == [(2, 3)] and vc.maps('violate')[0][1, 2] == 3
    with pytest.raises(ValueError):
        vc.maps('same_label')
    with pytest.raises(ValueError):
        vc.maps('conf')
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            E.keep_mask(agree, violate, min_views=bad)
        with pytest.raises(ValueError):
            E.keep_mask(agree, violate, max_violations=bad)
    conf = torch.tensor([[5.0, 1.5, float('inf')], [3.0, float('nan'), 0.0]])
    before = conf.clone()
    keep = torch.tensor([True, False, False, True, True, False])
    m = E.masked_conf(conf, keep)
    assert torch.equal(conf.view(torch.int32), before.view(torch.int32)) and m.data_ptr() != conf.data_ptr()      # a copy
    k2 = keep.reshape(2, 3)
    assert torch.equal(m.view(torch.int32)[k2], conf.view(torch.int32)[k2]) and torch.isnan(m[~k2]).all()
    for thr in (float('-inf'), -1.0, 0.0, 3.0):                               # whatever the threshold, a dropped pixel stays dropped
        assert not (m >= thr)[~k2].any()
        assert torch.equal((m >= thr)[k2], (conf >= thr)[k2])


def test_camera_tables_are_render_camera_table_per_view():
    x, cams, focals, _ = R.rotated_scene([(5, 7), (8, 12), (33, 40)], seed=1)
    shapes = [(5, 7), (8, 12), (33, 40)]
    for pp in (None, (3.5, 2.25), [(3.0, 2.0), (6.0, 4.0), (20.0, 16.5)]):
        got = E.own_camera_table(cams, focals, shapes, pp, 0.01)
        want = R.camera_tables(cams, focals, shapes, pp, 0.01)
        assert got.dtype == F and got.shape == (3, 16) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert E.own_camera_table(cams, focals, shapes)[:, 13:15].tolist() == [[3.5, 2.5], [6.0, 4.0], [20.0, 16.5]]
    assert np.array_equal(E.own_camera_table(cams, 7.0, shapes)[:, 12], np.full(3, 7.0, dtype=F))


def test_argument_errors():
    x, cams, focals, pan = R.plane_scene()
    xt = [{k: torch.from_numpy(v) for k, v in d.items()} for d in x]
    with pytest.raises(ValueError, match='focals'):
        view_consistency(xt, cams, None, rel_tol=0.03)
    for bad in (-0.01, 1.0, 2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='rel_tol'):
            view_consistency(xt, cams, focals, rel_tol=bad)
    with pytest.raises(ValueError):
        view_consistency(xt, cams[:3], focals, rel_tol=0.03)
    with pytest.raises(ValueError):
        view_consistency([], [], [], rel_tol=0.03)
    with pytest.raises(RuntimeError, match='no CPU fallback'):               # GPU only, like its neighbours
        view_consistency(xt, cams, focals, rel_tol=0.03)
    with pytest.raises(ValueError):
        E.own_camera_table(cams, focals[:2], [R.PLANE_SHAPE] * 4)
    with pytest.raises(ValueError):
        E.own_camera_table(cams, focals, [R.PLANE_SHAPE] * 4, pp=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError):
        E.own_camera_table(cams, focals, [R.PLANE_SHAPE] * 4, near=0.0)
    assert consistency_keywords(None) is None and consistency_keywords(True) == {} and consistency_keywords({'rel_tol': 0.1}) == {'rel_tol': 0.1}
    for bad in ('yes', 1, {'tolerance': 0.1}, ['rel_tol']):
        with pytest.raises(ValueError):
            consistency_keywords(bad)


def test_reconstruct_refuses_a_bad_consistency_argument_before_the_forward_pass():
    from panst3r_amd.panst3r import PanSt3R

    class Never:
        def forward_inference_multi_ar(self, *a, **k):
            raise AssertionError('the forward pass ran')
    for bad in ('yes', 3, {'tolerance': 0.1}):
        with pytest.raises(ValueError, match='consistency must be'):
            PanSt3R.reconstruct(Never(), [], None, [], consistency=bad)
    for fine in (None, True, {'rel_tol': 0.05, 'min_views': 2}):              # these reach the forward pass
        with pytest.raises(AssertionError, match='the forward pass ran'):
            PanSt3R.reconstruct(Never(), [], None, [], consistency=fine)


def test_binding_declares_the_two_entry_points():
    protos = {p[0]: p for p in abi_header.prototypes()}
    assert protos['pst_consist_depth'][2] == ['pst_cloud_view*', 'float*', 'int', 'int', 'int64_t', 'float', 'int', 'float*', 'void*']
    assert len(protos['pst_consist_count'][2]) == 13 and protos['pst_consist_count'][2][:3] == ['pst_cloud_view*', 'float*', 'int32_t*']
    assert hip.SIGNATURES['pst_consist_depth'] == 'i:ppiilfipp' and hip.SIGNATURES['pst_consist_count'] == 'i:pppiilfippppp'
    assert hip.ABI_VERSION == abi_header.defines()['PST_ABI_VERSION']
    assert set(abi_header.structs()) == {'pst_gemm_params', 'pst_attn_params', 'pst_cloud_view'}      # pst_cloud_view keeps its layout; no new struct
