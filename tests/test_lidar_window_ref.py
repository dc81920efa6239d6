"""CPU checks of tests/lidar_window_ref.py, the declared semantics of LiDAR plane factors in the window solve: the factor against the
oracle's Jet autodiff of the reference functor, the tangent Jacobian against central differences, the loop against oracle/lm.h, and the
scene that shows what the planes are for."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import lidar_window_cases as lc
from tests import lidar_window_ref as lw
from tests.test_oracle_lm_numpy import quat_plus


def _blocks(seed, n=60, n_kf=3):
    rng = np.random.default_rng(seed)
    poses = syn.drive_poses(n_kf, rng)
    poses[:, :4] *= rng.uniform(0.8, 1.25, (n_kf, 1))          # un-normalised quaternions: the ambient Jacobian carries the projector
    p, pa, pb, pc = (rng.normal(0, 5.0, (n, 3)) for _ in range(4))
    pa[7], pb[7], pc[7] = (1.0, 2.0, 3.0), (2.0, 4.0, 6.0), (3.0, 6.0, 9.0)      # a collinear triple, exactly: a null block
    return poses, lw.make_lidar(p, pa, pb, pc, rng.integers(0, n_kf, n)), pb, pc


def test_plane_rows_equal_the_oracle(oracle):
    poses, lid, pb, pc = _blocks(1)
    assert np.abs(lid["nrm"] - oracle.plane_normals(lid["pa"], pb, pc)).max() <= 1e-15
    assert not lid["nrm"][7].any()
    r, J = lw.plane_rows(lid, poses)
    for k in range(len(poses)):
        m = lid["kf"] == k
        r0, J0 = oracle.lidar_plane_se3(lid["p"][m], lid["pa"][m], lid["nrm"][m], poses[k])
        assert np.abs(r[m] - r0).max() <= 1e-12 * max(1.0, np.abs(r0).max())
        assert np.abs(J[m] - J0).max() <= 1e-12 * max(1.0, np.abs(J0).max())
    assert r[7] == 0.0 and not J[7].any()


def test_weight_scales_and_loss_is_the_corrector():
    poses, lid, _, _ = _blocks(2)
    r1, J1 = lw.plane_rows_local(lid, poses)
    lid2 = dict(lid); lid2["weight"] = np.full(len(r1), 0.01)
    r2, J2 = lw.plane_rows_local(lid2, poses)
    assert np.allclose(r2, 0.01 * r1, rtol=1e-15) and np.allclose(J2, 0.01 * J1, rtol=1e-15)
    a = float(np.median(np.abs(r1[r1 != 0])))
    lid3 = dict(lid); lid3["huber_a"] = np.full(len(r1), a)
    J, rr, cost, outside = lw.lidar_rows(lid3, poses, 15 * len(poses) + 4)
    assert outside.any() and (~outside).any()
    want = np.where(np.abs(r1) > a, 2 * a * np.abs(r1) - a * a, r1 * r1)
    assert abs(cost - 0.5 * want.sum()) <= 1e-12 * cost
    assert np.allclose(rr[outside], np.sqrt(a / np.abs(r1[outside])) * r1[outside], rtol=1e-14) and np.array_equal(rr[~outside], r1[~outside])
    assert not J[:, 15 * len(poses):].any() and not J[:, 6 * len(poses):15 * len(poses)].any()


def test_tangent_jacobian_agrees_with_central_differences():
    poses, lid, _, _ = _blocks(3)
    r, J6 = lw.plane_rows_local(lid, poses)
    h = 1e-6
    for c in range(6):
        d = np.zeros(6); d[c] = h
        plus, minus = poses.copy(), poses.copy()
        for k in range(len(poses)):
            plus[k, :4] = quat_plus(poses[k, :4], d[:3]); plus[k, 4:] += d[3:]
            minus[k, :4] = quat_plus(poses[k, :4], -d[:3]); minus[k, 4:] -= d[3:]
        fd = (lw.plane_rows(lid, plus)[0] - lw.plane_rows(lid, minus)[0]) / (2 * h)
        assert np.abs(fd - J6[:, c]).max() <= 1e-7 * max(1.0, np.abs(J6[:, c]).max())


def test_loop_with_no_lidar_block_is_the_oracle_loop(oracle):
    """decision for decision: every trial's accept / reject, the iteration counts, the reason the loop ended; costs and the state beside"""
    cfg = syn.config4_window(n_kf=5, n_lm=40, n_prewindow=20, seed=101, imu_samples=4)
    pre = lc.preint(oracle, cfg)
    for kw in (dict(max_num_iterations=8), dict(max_num_iterations=12, initial_trust_region_radius=1e16, function_tolerance=0.0)):
        win = oracle.Window(cfg, pre)
        ref = win.solve(**kw)
        s, state = lw.lm_solve(oracle, cfg, pre, lc.state_of_cfg(cfg), lw.empty_lidar(), **kw)
        assert (s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], s["why"], s["termination"]) == \
               (ref["num_iterations"], ref["num_successful_steps"], ref["num_unsuccessful_steps"], ref["why"], ref["termination"])
        assert len(s["trace"]) == len(ref["trace"]) and np.array_equal(s["trace"][:, 3], ref["trace"][:, 3]) and np.array_equal(s["trace"][:, 4], ref["trace"][:, 4])
        assert np.allclose(s["trace"][:, :3], ref["trace"][:, :3], rtol=1e-7)
        assert abs(s["final_cost"] - ref["final_cost"]) <= 1e-8 * ref["final_cost"] and abs(s["final_radius"] - ref["final_radius"]) <= 1e-6 * ref["final_radius"]
        for a, b in zip(state, (win.poses, win.vel, win.ba, win.bg, win.inv_depth)):
            assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())


def test_planes_fix_what_far_landmarks_cannot(oracle):
    """The scene that shows the point (lidar_window_cases.far_scene): with the planes of each keyframe's sweep in the problem, the newest
    keyframe's translation error after the solve is at least 5 times smaller than without them."""
    cfg, pre, lidar, pc = lc.far_scene()
    err = {}
    for name, lid in (("without", lw.empty_lidar()), ("with", lidar)):
        s, state = lw.lm_solve(oracle, cfg, pre, lc.state_of_cfg(cfg), lid, pose_const=pc)
        err[name] = float(np.linalg.norm(state[0][-1, 4:] - cfg["poses_true"][-1, 4:]))
        assert np.array_equal(state[0][0], cfg["poses"][0]), "the constant keyframe moved"
        print(f"far scene, {name} planes: {s['num_iterations']} iterations ({s['why']}), cost {s['initial_cost']:.4e} -> {s['final_cost']:.4e}, "
              f"newest keyframe's translation error {err[name]:.4f} m")
    assert err["with"] * 5.0 <= err["without"]
