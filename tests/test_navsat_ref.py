"""The CPU restatement of the GNSS (NavSat) alignment (tests/navsat_ref.py) checked on its own, without a GPU: its three functors against an
independent 50-digit mpmath statement (rotation matrices instead of the quaternion polynomials, finite-difference Jacobians), and its solves
on synthetic sections with known answers."""
import numpy as np
import pytest

from tests import navsat_ref as nr
from tests.helpers import RTOL, assert_parity

TRUST_YAW, TRUST_PITCH = 10.0, 30.0


def _blocks(n, seed):
    rng = np.random.default_rng(seed)
    pose = np.concatenate([nr.quat_zyx(0.4, -0.1, 0.05) * 1.07, [3.0, -2.0, 0.5]])      # the functors normalise where they rotate
    return rng.normal(0, 20, (n, 3)), rng.normal(0, 20, (n, 3)), rng.uniform(0.01, 0.3, (n, 3)), pose


@pytest.mark.parametrize("x6", [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.3, -0.1, 0.05, 0.8, -0.5, 0.2), (-2.5, 0.4, -0.3, -30.0, 12.0, 4.0)])
def test_rx_functor_against_mpmath(x6):
    p0, p1, cov, pose = _blocks(4, 1)
    r, J = nr.navsat_rx(p0, p1, pose, cov, x6)
    for i in range(4):
        r0, J0 = nr.mp_fd(lambda x: nr.mp_navsat_rx(p0[i], p1[i], pose, cov[i], x), x6)
        assert_parity(r[i], r0, f"NavsatRXError r[{i}]"); assert_parity(J[i], J0, f"NavsatRXError J[{i}]")
        assert np.abs(r[i] - r0).max() <= RTOL * np.abs(r0).max()
    r2, none = nr.navsat_rx(p0, p1, pose, cov, x6, jac=False)
    assert none is None and np.array_equal(r2, r)


@pytest.mark.parametrize("x3", [(0.0, 0.0, 0.0), (0.7, 3.0, -2.0), (-3.0, -40.0, 15.0)])
def test_init_functor_against_mpmath(x3):
    p0, p1, cov, _ = _blocks(4, 2)
    r, J = nr.navsat_init(p0, p1, cov, x3)
    for i in range(4):
        r0, J0 = nr.mp_fd(lambda x: nr.mp_navsat_init(p0[i], p1[i], cov[i], x), x3)
        assert_parity(r[i], r0, f"NavsatInitError r[{i}]"); assert_parity(J[i], J0, f"NavsatInitError J[{i}]")


@pytest.mark.parametrize("roll", [0.0, 0.2, -1.3])
def test_r_functor_against_mpmath(roll):
    _, _, _, pose = _blocks(1, 3)
    y = np.array([0.4, 11.5, -0.8])
    r, J = nr.navsat_r(y, pose, roll)
    r0, J0 = nr.mp_fd(lambda x: nr.mp_navsat_r(y, pose, x[0]), [roll])
    assert_parity(r[0], r0, "NavsatRError r"); assert_parity(J[0], J0, "NavsatRError J")


def test_cov2sqrt_info_is_the_inverse_square_root():
    assert np.allclose(nr.cov2sqrt_info([0.04, 0.09, 0.25]), [5.0, 1.0 / 0.3, 2.0], rtol=1e-15)


def test_optimize_bc_recovers_a_planted_offset(oracle):
    planted = np.array([0.05, -0.02, 0.0, 0.8, -0.5, 0.3])      # yaw, pitch, x, y, z (roll held: mode 0b000100)
    poses, has, fix, cov = nr.planted_section(oracle, 60, 3, planted, noise=0.0, missing=0.2, n_update=4)
    out = nr.optimize_bc(oracle, poses, 60, has, fix, cov, 0b000100, 100.0, TRUST_YAW, TRUST_PITCH, -100.0, 100.0)
    assert not out["skipped"] and out["main"]["termination"] == 0 and out["main"]["contractions"] == 0
    assert np.abs(out["para"] - planted).max() < 1e-4
    true = nr.drive(64, 3)
    assert np.abs(out["poses"][:, 4:] - true[:, 4:]).max() < 2e-3           # every pose, the update-only ones included, is back on the road
    assert np.array_equal(poses, nr.planted_section(oracle, 60, 3, planted, noise=0.0, missing=0.2, n_update=4)[0])      # the input is not touched


def test_optimize_bc_early_return_and_constant_pitch(oracle):
    planted = np.array([0.05, -0.02, 0.0, 0.8, -0.5, 0.3])
    poses, has, fix, cov = nr.planted_section(oracle, 30, 4, planted, noise=0.02)
    out = nr.optimize_bc(oracle, poses, 30, has, fix, cov, 0, 5.0, TRUST_YAW, TRUST_PITCH, -100.0, 100.0)
    assert out["skipped"] and np.array_equal(out["poses"], poses) and out["main"] is None
    out = nr.optimize_bc(oracle, poses, 30, has, fix, cov, 0, 20.0, TRUST_YAW, TRUST_PITCH, -100.0, 100.0)      # between: roll pre-solved, pitch held
    assert not out["skipped"] and out["roll"] is not None and out["para"][1] == 0.0 and out["para"][0] != 0.0
    out = nr.optimize_bc(oracle, poses, 30, has, fix, cov, 0b110111, 5.0, TRUST_YAW, TRUST_PITCH, -100.0, 100.0)      # translation only: no early return
    assert not out["skipped"] and out["roll"] is None and np.count_nonzero(out["para"]) == 1 and out["para"][3] != 0.0


def test_optimize_bc_without_fixes_still_applies_the_products(oracle):
    poses, has, fix, cov = nr.planted_section(oracle, 12, 5, np.zeros(6), n_update=3)
    out = nr.optimize_bc(oracle, poses, 12, np.zeros(12, np.int32), fix, cov, 0b000100, 100.0, TRUST_YAW, TRUST_PITCH, -1.0, 1.0)
    assert np.array_equal(out["para"], np.zeros(6)) and out["main"]["num_iterations"] == 0
    assert np.abs(out["poses"] - poses).max() < 1e-13 and np.abs(out["transform"] - [0, 0, 0, 1, 0, 0, 0]).max() < 1e-13


def test_optimize_bc_ends_on_an_active_z_bound(oracle):
    planted = np.array([0.3, 0.1, 0.0, 2.0, -1.0, 2.0])
    poses, has, fix, cov = nr.planted_section(oracle, 40, 3, planted, noise=0.02)
    free = nr.optimize_bc(oracle, poses, 40, has, fix, cov, 0b000100, 100.0, TRUST_YAW, TRUST_PITCH, -100.0, 100.0)
    assert free["para"][5] > 1.0                                            # the unconstrained optimum lies beyond the bound
    out = nr.optimize_bc(oracle, poses, 40, has, fix, cov, 0b000100, 100.0, TRUST_YAW, TRUST_PITCH, -0.05, 0.05)
    assert out["para"][5] == 0.05
    assert out["main"]["final_cost"] <= out["main"]["initial_cost"]         # initial_cost is the cost at the projected start
    assert out["main"]["contractions"] > 0                                  # the clipped first step is too long for the Armijo condition
    # a start point outside the box is projected before the first evaluation
    out = nr.optimize_bc(oracle, poses, 40, has, fix, cov, 0b000100, 100.0, TRUST_YAW, TRUST_PITCH, 0.5, 0.6)
    f, p1 = fix[has > 0], nr.sophus_transform_point(nr.sophus_inverse(poses[0]), poses[:40, 4:7])[has > 0]
    r, _ = nr.navsat_rx(f, p1, poses[0], cov[has > 0], [0, 0, 0, 0, 0, 0.5], jac=False)
    assert abs(out["main"]["initial_cost"] - 0.5 * nr.huber(0.1, (r * r).sum(axis=1))[0].sum()) <= 1e-12 * out["main"]["initial_cost"]
    assert 0.5 <= out["para"][5] <= 0.6 and out["main"]["final_cost"] <= out["main"]["initial_cost"]


def test_fix_chain_puts_every_keyframe_at_the_foot_of_its_fix(oracle):
    n = 40
    true, has, fix, cov = nr.chain_section(n, 7, noise=0.0, outlier_every=10 ** 6, missing=0.25, same_cov=True)      # noise-free fixes, one covariance for all axes
    poses = true.copy()
    poses[:, 4:] += np.cumsum(np.random.default_rng(70).normal(0.0, 0.08, (n, 3)), axis=0)                           # the estimate has drifted off the road
    out = nr.fix_chain(oracle, poses, has, fix, cov)
    # Tolerance: the first LM step at radius 1e4 is the Gauss-Newton step times 1 / (1 + 1e-4) (damping = H / radius) and the function-tolerance
    # test may end the solve right behind it, so x is within 2e-4 |x| of the foot; 1e-9 covers rounding.
    # Reconstruct what each step saw: step k moves pose k along ITS OWN x axis (the forward updates before it rotate nothing: only x is free).
    cur = poses.copy()
    for k in range(n - 1):
        ex = nr.quat_transform_vector(cur[k, :4], np.array([1.0, 0.0, 0.0]))
        if has[k]:
            along = float(np.dot(fix[k] - cur[k, 4:], ex))
            tol = 2e-4 * abs(along) + 1e-9
            assert np.abs(out["poses"][k, 4:] - (cur[k, 4:] + ex * along)).max() <= tol, k
            assert abs(out["x"][k] - along) <= tol and abs(along) > 1e-3
        else:
            assert out["x"][k] == 0.0 and out["iterations"][k] == 0
            assert np.abs(out["poses"][k] - cur[k]).max() < 1e-13
        shift = out["poses"][k, 4:] - cur[k, 4:]
        cur[k + 1:, 4:] += shift                                            # a pure translation is handed forward
        cur[k] = out["poses"][k]
    assert np.abs(out["poses"][n - 1] - cur[n - 1]).max() < 1e-10            # C is updated, not solved
    assert np.abs(out["poses"][:, :4] - poses[:, :4]).max() < 1e-13


def test_fix_chain_small_sizes(oracle):
    for n in (0, 1):
        poses, has, fix, cov = nr.chain_section(n, 1)
        out = nr.fix_chain(oracle, poses, has, fix, cov)
        assert np.array_equal(out["poses"], poses) and out["x"].size == 0


def test_initialize_recovers_a_planted_yaw_and_shift(oracle):
    rng = np.random.default_rng(5)
    para = np.array([0.7, 0.0, 0.0, 3.0, -2.0, 0.0])
    raw = rng.normal(0, 25, (30, 3))
    position = np.array([oracle.se3_apply(oracle.rpyxyz_to_se3(para), p) for p in raw])
    out, ext, s1, s2 = nr.initialize(oracle, position, raw, np.full((30, 3), 0.04))
    assert np.abs(out - para).max() < 1e-6 and s2["termination"] == 0
    assert s1["num_iterations"] > 0 and s2["final_cost"] <= s1["final_cost"] <= s1["initial_cost"]
    assert np.abs(ext - oracle.rpyxyz_to_se3(para)).max() < 1e-6
    out0, ext0, _, s2 = nr.initialize(oracle, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert np.array_equal(out0, np.zeros(6)) and s2["num_iterations"] == 0


def test_lm_dense_line_search_is_not_taken_without_bounds(oracle):
    planted = np.array([0.3, 0.1, 0.0, 2.0, -1.0, 2.0])
    poses, has, fix, cov = nr.planted_section(oracle, 40, 3, planted, noise=0.02)
    a = nr.optimize_bc(oracle, poses, 40, has, fix, cov, 0b100100, 100.0, TRUST_YAW, TRUST_PITCH, -0.05, 0.05)      # z constant: its bounds are never set
    assert a["main"]["contractions"] == 0 and a["para"][5] == 0.0
