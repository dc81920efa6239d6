"""CPU checks around the pose-chain solve: tests/pose_chain_ref.py (the declared semantics lvio_fusion_amd/csrc/pose_chain_kernels.hip follows)
is pinned to the oracle's loop and to dense linear algebra, the scenes of the GPU solve test are shown to be decidable (every comparison the
loop decides by has a relative margin of at least 1e-6, so iteration counts may be compared for equality), and the new entry points are
declared, typed and exported."""
import ctypes as C

import numpy as np
import pytest

from lvio_fusion_amd import _lib, synthetic as syn
from tests import pose_chain_ref as pc
from tests.helpers import assert_parity

NEW_SYMBOLS = ("lvf_pose_chain_capacity", "lvf_pose_chain_solve", "lvf_pose_chain_debug_step", "lvf_pose_chain_debug_system", "lvf_navsat_optimize_ab")


def test_ref_iterations_against_the_oracle_loop(oracle):
    """the pose-graph chain (PoseGraphError edges, RError unaries, no loss) through the ref's single iteration and through the oracle window's"""
    from tests.test_gpu_posegraph import chain
    n = 9
    P, before, pr = chain(oracle, n, 5)
    cfg = dict(n_kf=n, n_lm=0, poses=P, vel=np.zeros((n, 3)), ba=np.zeros((n, 3)), bg=np.zeros((n, 3)), inv_depth=np.zeros(0), w_kf=np.ones(n),
               cam0=syn.kitti_cameras()[0], cam1=syn.kitti_cameras()[1],
               tc=dict(left_ob=np.zeros((0, 2)), right_ob=np.zeros((0, 2)), lm_idx=np.zeros(0, np.int32), kf_idx=np.zeros(0, np.int32)),
               tf=dict(first_ob=np.zeros((0, 2)), ob=np.zeros((0, 2)), lm_idx=np.zeros(0, np.int32), kf1_idx=np.zeros(0, np.int32), kf2_idx=np.zeros(0, np.int32)),
               po=dict(ob=np.zeros((0, 2)), kf_idx=np.zeros(0, np.int32), pw_idx=np.zeros(0, np.int32), pw=np.zeros((1, 3))), imu=[])
    const = np.zeros(n, np.uint8); const[0] = const[-1] = 1
    win = oracle.Window(cfg, np.zeros((0, 467)), pose_const=const, use=(), priors=pr)
    pb = pc.from_priors(oracle, P, pr)
    X = pb["poses"].copy()
    assert abs(pc.linearize(oracle, pb, X, jac=False)["cost"] - win.cost()) <= 1e-9 * win.cost()
    radius, dec = 1e4, 2.0
    accepted = 0
    for it in range(5):
        ref = win.lm_iteration(radius, dec)
        X, got = pc.lm_iteration(oracle, pb, X, radius, dec)
        assert got["accepted"] == ref["accepted"]
        assert_parity(got["cost_after"], ref["cost_after"], f"cost it{it}")
        assert_parity(X, win.poses, f"poses it{it}")
        assert abs(got["radius"] - ref["radius"]) <= 1e-6 * ref["radius"]
        radius, dec = ref["radius"], ref["decrease_factor"]
        accepted += got["accepted"]
    assert accepted >= 1 and np.array_equal(X[0], P[0]) and np.array_equal(X[-1], P[-1])


@pytest.mark.parametrize("m", [1, 2, 3, 17])
def test_block_system_and_sweep_against_dense(oracle, m):
    """the ref's blocks against J^T J, J^T r of the stacked local Jacobians, and the block-Thomas sweep against a dense solve"""
    pb = pc.step_case(oracle, m, 20 + m)
    X, n = pb["poses"], pb["n"]
    lin = pc.linearize(oracle, pb, X)
    rows, res = [], []
    for k in range(n - 1):
        r, J1, J2 = oracle.pose_graph(pb["tg"][k], pb["ew"][k], pb["ev"][k], X[k], X[k + 1])
        J = np.zeros((6, 6 * n))
        J[:, 6 * k:6 * k + 6], J[:, 6 * k + 6:6 * k + 12] = oracle.pose_jac_to_local(X[k], J1), oracle.pose_jac_to_local(X[k + 1], J2)
        rows.append(J); res.append(r)
    zones = []
    for p in range(1, n - 1):
        r, J7 = oracle.t_error(pb["ut"][p, :3], pb["uw"][p], X[p])
        _, rho1 = pc.huber(pb["huber_a"], np.array([float(r @ r)]))
        sc = np.sqrt(rho1[0])
        zones.append(rho1[0] < 1.0)
        J = np.zeros((3, 6 * n))
        J[:, 6 * p:6 * p + 6] = sc * oracle.pose_jac_to_local(X[p], J7)
        rows.append(J); res.append(sc * r)
    J, r = np.concatenate(rows)[:, 6:6 * (n - 1)], np.concatenate(res)
    A = pc.dense(lin["D"], lin["O"])
    assert_parity(A, J.T @ J, "J^T J"); assert_parity(lin["g"], J.T @ r, "J^T r")
    assert np.array_equal(A, A.T)
    if m >= 3:
        assert any(zones) and not all(zones)               # both Huber zones in one linearisation
    h0 = np.einsum("fii->fi", lin["D"]).ravel().copy()
    for radius in (1e4, 1e-2):
        Dd = pc.damp(lin["D"], h0, radius)
        ok, x = pc.thomas(Dd, lin["O"], -lin["g"])
        okr, xr = pc.thomas(Dd, lin["O"], -lin["g"], reverse=True)
        xd = np.linalg.solve(pc.dense(Dd, lin["O"]), -lin["g"])
        assert ok and okr
        assert_parity(x, xd, f"Thomas vs dense, radius {radius}"); assert_parity(xr, xd, f"reversed Thomas vs dense, radius {radius}")
        xs = pc.refine(Dd, lin["O"], -lin["g"], x)
        assert pc.err(Dd, x, xs) < 1e-9 and pc.err(Dd, xs.astype(np.float64), xs) < 1e-15
        assert abs(pc.model_decrease(lin, x) + float(x @ (lin["g"] + 0.5 * (A @ x)))) <= 1e-12 * abs(float(x @ lin["g"]))
    bad = Dd.copy(); bad[m // 2, 3, 3] = -1.0
    assert pc.thomas(bad, lin["O"], -lin["g"])[0] is False
    bad[m // 2, 3, 3] = np.nan
    assert pc.thomas(bad, lin["O"], -lin["g"])[0] is False


def test_scene_conditions(oracle):
    """what makes the GPU solve test's equalities legitimate, shown on the ref alone"""
    rejected = 0
    for m, seed, kw, loss in pc.SOLVE_SCENES:
        poses, stamps, fix, relB = pc.ab_section(oracle, m, seed, **kw)
        X, s = pc.solve(oracle, pc.navsat_ab(oracle, poses, stamps, fix, relB, 0.1))
        assert s["termination"] == 0 and s["num_successful_steps"] >= 1 and s["final_cost"] < s["initial_cost"], (m, s["why"])
        assert pc.min_margin(s) >= 1e-6, (m, [mg for mg in s["margins"]])
        assert (s["huber_active"] > 0) == loss, (m, s["huber_active"])
        assert np.array_equal(X[0], poses[0]) and np.array_equal(X[-1], poses[-1])
        rejected += s["rejected"]
    assert rejected >= 1


def test_new_entry_points_are_declared_typed_and_exported():
    names = _lib.declared_symbols()
    _lib.build()
    so = C.CDLL(_lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in names and name in _lib._SIGS and hasattr(so, name), name
    so.lvf_pose_chain_capacity.restype = C.c_int
    assert so.lvf_pose_chain_capacity() >= 1022
