"""`engine.camera_quality` (host float64, no kernel) on poses whose errors are known.  No GPU."""
import numpy as np
import pytest

from panst3r_amd.engine import camera_quality


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def pose(R, c):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c
    return T


def ring(V=6, seed=0):
    r = np.random.Generator(np.random.PCG64(seed))
    return [pose(rot(r.normal(size=3), r.uniform(0, 120)), r.uniform(-2, 2, 3)) for _ in range(V)]


def test_identical_poses_score_zero():
    gt = ring()
    out = camera_quality(gt, gt, pred_focals=[500.0] * 6, gt_focals=[500.0] * 6)
    assert out['n_pairs'] == 15 and out['n_no_baseline'] == 0 and out['pairs'][:2] == [(0, 1), (0, 2)]
    assert max(out['rot_err_deg']) < 1e-9 and max(out['trans_err_deg']) < 1e-9
    assert out['rra'] == {5: 1.0, 15: 1.0, 30: 1.0} and out['rta'] == {5: 1.0, 15: 1.0, 30: 1.0} and out['maa_30'] == 1.0
    assert out['ate_rmse'] < 1e-12 and out['ate_reason'] is None and out['focal_rel_err'] == 0.0


def test_a_known_yaw():
    gt = [pose(np.eye(3), [0, 0, 0]), pose(np.eye(3), [1, 0, 0])]
    pred = [gt[0], pose(rot([0, 1, 0], 10.0), [1, 0, 0])]
    out = camera_quality(pred, gt, taus=(5, 10, 15))
    assert out['rot_err_deg'] == [pytest.approx(10.0, abs=1e-9)] and out['trans_err_deg'] == [pytest.approx(0.0, abs=1e-9)]
    assert out['rra'] == {5: 0.0, 10: 0.0 if out['rot_err_deg'][0] >= 10 else 1.0, 15: 1.0}
    assert out['maa_30'] == pytest.approx(20 / 30, abs=1 / 30 + 1e-12)            # tau = 11 .. 30 pass; tau = 10 is on the edge
    assert out['ate_rmse'] is None and 'at least 3 cameras' in out['ate_reason']
    # a rotation of 180 degrees, where acos of the trace loses half its digits
    out = camera_quality([gt[0], pose(rot([0, 0, 1], 180.0), [1, 0, 0])], gt)
    assert out['rot_err_deg'][0] == pytest.approx(180.0, abs=1e-9)
    # the baseline turned by 30 degrees about z
    out = camera_quality([gt[0], pose(np.eye(3), rot([0, 0, 1], 30.0) @ [1, 0, 0])], gt)
    assert out['trans_err_deg'][0] == pytest.approx(30.0, abs=1e-9) and out['rta'] == {5: 0.0, 15: 0.0, 30: 0.0 if out['trans_err_deg'][0] >= 30 else 1.0}


def test_a_global_similarity_changes_nothing():
    gt = ring(V=7, seed=1)
    R, s, t = rot([1, 2, 3], 77.0), 3.7, np.array([5.0, -2.0, 9.0])
    pred = [pose(R @ T[:3, :3], s * R @ T[:3, 3] + t) for T in gt]
    out = camera_quality(pred, gt)
    assert max(out['rot_err_deg']) < 1e-9 and max(out['trans_err_deg']) < 1e-9 and out['maa_30'] == 1.0
    extent = np.linalg.norm(np.ptp(np.stack([T[:3, 3] for T in gt]), axis=0))
    assert out['ate_rmse'] < 1e-12 * extent


def test_the_translation_angle_is_tight_away_from_zero():
    """atan2(|a x b|, a . b) near 0 degrees is limited by the cross product's rounding; held to 1e-9 on a pair that is not parallel to an axis"""
    gt = ring(V=5, seed=2)
    R, s, t = rot([3, -1, 2], 41.0), 0.25, np.array([1.0, 2.0, 3.0])
    pred = [pose(R @ T[:3, :3], s * R @ T[:3, 3] + t) for T in gt]
    out = camera_quality(pred, gt)
    assert max(out['trans_err_deg']) < 1e-9 and max(out['rot_err_deg']) < 1e-9


def test_a_zero_baseline_pair_is_counted_and_left_out():
    gt = ring(V=4, seed=3)
    gt[2] = pose(gt[2][:3, :3], gt[0][:3, 3])                                    # cameras 0 and 2 share a centre: a pure rotation
    out = camera_quality(gt, gt)
    k = out['pairs'].index((0, 2))
    assert out['n_no_baseline'] == 1 and out['trans_err_deg'][k] is None and out['rot_err_deg'][k] < 1e-9
    assert sum(t is not None for t in out['trans_err_deg']) == 5 and out['rta'][5] == 1.0 and out['maa_30'] == 1.0
    two = camera_quality(gt[0:3:2], gt[0:3:2])
    assert two['n_no_baseline'] == 1 and two['maa_30'] is None and two['rta'] == {5: None, 15: None, 30: None} and two['rra'][5] == 1.0


def test_the_flip_ambiguity():
    gt = [pose(np.eye(3), [0, 0, 0]), pose(np.eye(3), [1, 0, 0]), pose(np.eye(3), [0, 2, 0])]
    pred = [gt[0], pose(np.eye(3), [-1, 0, 0]), gt[2]]                           # the first baseline reversed
    on, off = camera_quality(pred, gt), camera_quality(pred, gt, ambiguity=False)
    assert on['trans_err_deg'][0] == pytest.approx(0.0, abs=1e-9) and off['trans_err_deg'][0] == pytest.approx(180.0, abs=1e-9)
    assert on['rta'][30] == 2 / 3 and off['rta'][30] == 1 / 3                    # the pair (1, 2) is 53 degrees off either way


def test_focals_and_refusals():
    gt = ring(V=3, seed=4)
    out = camera_quality(gt, gt, pred_focals=[550.0, 500.0, 450.0], gt_focals=[500.0] * 3)
    assert out['focal_rel_err'] == pytest.approx(0.2 / 3)
    with pytest.raises(ValueError):
        camera_quality(gt, gt[:2])
    with pytest.raises(ValueError):
        camera_quality(gt[:1], gt[:1])
    with pytest.raises(ValueError):
        camera_quality(gt, gt, pred_focals=[1.0] * 3)
