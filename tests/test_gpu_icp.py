"""GPU parity of the on-device scan-to-map solve (lvf_icp_solve) against the oracle's restatement of
ScanToMapWithGround / ScanToMapWithSegmented + the 4-iteration 3-DoF solve (mapping.cpp:154-178)."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    c = syn.config3_icp()
    sel = np.sort(np.random.default_rng(1).choice(c["query"].shape[0], 6000, replace=False))
    return c, c["query"][sel], c["query_ground"][sel]


@pytest.mark.parametrize("mode,prior", [(0, 0.0), (1, 0.0), (0, 500 * syn.W_VISUAL), (1, 500 * syn.W_VISUAL)])
def test_icp_solve_parity(ctx, oracle, scene, mode, prior):
    from lvio_fusion_amd import api
    c, q, qg = scene
    qq = q[qg] if mode == 0 else q[~qg]
    mm = c["map"][c["map_ground"]] if mode == 0 else c["map"][~c["map_ground"]]
    thr = c["thr_ground"] if mode == 0 else c["thr_surf"]
    w = syn.W_LIDAR_GROUND if mode == 0 else syn.W_LIDAR_SURF
    huber = 0.0 if mode == 0 else 0.1
    rel = oracle.se3_mul(oracle.se3_inv(c["map_pose"]), c["pose0"])
    rpyxyz0 = oracle.se3_to_rpyxyz(rel)
    ref_x, ref = oracle.icp_solve(mm, qq, c["map_pose"], c["pose0"], rpyxyz0, mode, thr, w, huber, prior_w=prior)
    mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
    x = rpyxyz0.copy()
    s = api.icp_solve(mp, sc, c["map_pose"], c["pose0"], x, mode, thr, w, huber, prior_weight=prior)
    assert s.num_residual_blocks == ref["num_residual_blocks"] and s.num_residual_blocks > 500
    assert s.num_iterations == ref["num_iterations"] and s.num_successful_steps == ref["num_successful_steps"]
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"])
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.allclose(x, ref_x, rtol=1e-6, atol=1e-9)
    assert s.final_cost <= s.initial_cost and (prior > 0 or s.final_cost < s.initial_cost)
    untouched = [0, 3, 4] if mode == 0 else [1, 2, 5]
    assert np.array_equal(x[untouched], rpyxyz0[untouched])      # only the three parameter blocks of the sub-problem move
    mp.close(); sc.close()


def test_icp_recovers_pose_like_mapping_optimize(ctx, oracle, scene):
    """Mapping::Optimize order: ground (pitch,roll,z) then surf (yaw,x,y); the composed pose moves toward the truth."""
    from lvio_fusion_amd import api
    c, q, qg = scene
    pose = c["pose0"].copy()
    rel = oracle.se3_mul(oracle.se3_inv(c["map_pose"]), pose)
    x = oracle.se3_to_rpyxyz(rel)
    e0 = np.abs(pose[4:] - c["pose_true"][4:]).max()
    for mode in (0, 1):
        qq = q[qg] if mode == 0 else q[~qg]
        mm = c["map"][c["map_ground"]] if mode == 0 else c["map"][~c["map_ground"]]
        thr = c["thr_ground"] if mode == 0 else c["thr_surf"]
        mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
        api.icp_solve(mp, sc, c["map_pose"], pose, x, mode, thr, syn.W_LIDAR_GROUND if mode == 0 else syn.W_LIDAR_SURF,
                      0.0 if mode == 0 else 0.1)
        pose = oracle.se3_mul(c["map_pose"], oracle.rpyxyz_to_se3(x))      # mapping.cpp:164
        mp.close(); sc.close()
    e1 = np.abs(pose[4:] - c["pose_true"][4:]).max()
    assert e1 < 0.5 * e0


def test_icp_no_correspondences(ctx):
    from lvio_fusion_amd import api
    m = np.zeros((10, 4), np.float32); m[:, 0] = 1000.0
    q = np.zeros((50, 4), np.float32)
    mp, sc = api.Map(ctx, m, 1.0), api.Scan(ctx, q)
    x = np.array([0.1, 0.0, 0.0, 1.0, 2.0, 3.0])
    s = api.icp_solve(mp, sc, [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 2, 3], x, 1, 1.0, 0.01, 0.1)
    assert s.num_residual_blocks == 0 and s.final_cost == 0.0
    assert np.array_equal(x, [0.1, 0.0, 0.0, 1.0, 2.0, 3.0])
    mp.close(); sc.close()


@pytest.mark.parametrize("mode,prior", [(0, 0.0), (1, 500 * syn.W_VISUAL)])
def test_lidar_solve_on_caller_built_batch(ctx, oracle, scene, mode, prior):
    """adapt::Solve-level drop-in: the caller keeps association.cpp's host loop (here: the device 3-NN result downloaded
    and turned into LidarPlaneError constructor arguments), hands the blocks over as one lidar batch, and
    lvf_lidar_solve must land exactly where the oracle's ScanToMap + solve lands."""
    from lvio_fusion_amd import api
    c, q, qg = scene
    qq = q[qg] if mode == 0 else q[~qg]
    mm = c["map"][c["map_ground"]] if mode == 0 else c["map"][~c["map_ground"]]
    thr = c["thr_ground"] if mode == 0 else c["thr_surf"]
    w = syn.W_LIDAR_GROUND if mode == 0 else syn.W_LIDAR_SURF
    huber = 0.0 if mode == 0 else 0.1
    rpyxyz0 = oracle.se3_to_rpyxyz(oracle.se3_mul(oracle.se3_inv(c["map_pose"]), c["pose0"]))
    ref_x, ref = oracle.icp_solve(mm, qq, c["map_pose"], c["pose0"], rpyxyz0, mode, thr, w, huber, prior_w=prior)
    mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
    api.knn3(mp, sc, c["pose0"], thr)
    idx, d2, valid = sc.download()
    v = valid > 0
    p = qq[v, :3].astype(np.float64)
    pa, pb, pc = (mm[idx[v, k], :3].astype(np.float64) for k in range(3))
    b = api.lidar_plane_batch(ctx, mode, p, pa, pb, pc, c["map_pose"], w)
    x = rpyxyz0.copy()
    s = api.lidar_solve(b, x, huber, prior_weight=prior)
    assert s.num_residual_blocks == ref["num_residual_blocks"]
    assert s.num_iterations == ref["num_iterations"] and s.num_successful_steps == ref["num_successful_steps"]
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"])
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.allclose(x, ref_x, rtol=1e-6, atol=1e-9)
    b.close(); mp.close(); sc.close()


@pytest.mark.parametrize("max_iters", [0, 1, 2, 3])
@pytest.mark.parametrize("far", [False, True])
def test_icp_iteration_caps_and_a_far_start(ctx, oracle, scene, max_iters, far):
    """The device loop runs ONE pass per LM iteration (the candidate pass carries the Jacobian; the last allowed iteration's pass only the
    cost): every cap, and a start far enough for the trust region to work (rejected / short steps), must end where ceres::Solve's
    restatement ends — same counts, same state."""
    from lvio_fusion_amd import api
    c, q, qg = scene
    mode = 1
    qq, mm = q[~qg], c["map"][~c["map_ground"]]
    thr, w, huber = c["thr_surf"], syn.W_LIDAR_SURF, 0.1
    pose0 = np.array(c["pose0"], float)
    if far:
        d = np.array([0.03, -0.02, 0.05, 1.0]); d /= np.linalg.norm(d)
        pose0 = oracle.se3_mul(np.concatenate([d, [0.6, -0.4, 0.1]]), pose0)
    rel = oracle.se3_mul(oracle.se3_inv(c["map_pose"]), pose0)
    rpyxyz0 = oracle.se3_to_rpyxyz(rel)
    ref_x, ref = oracle.icp_solve(mm, qq, c["map_pose"], pose0, rpyxyz0, mode, thr, w, huber, prior_w=0.0, max_iters=max_iters)
    mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
    x = rpyxyz0.copy()
    s = api.icp_solve(mp, sc, c["map_pose"], pose0, x, mode, thr, w, huber, prior_weight=0.0, max_num_iterations=max_iters)
    assert s.num_residual_blocks == ref["num_residual_blocks"]
    assert (s.num_iterations, s.num_successful_steps) == (ref["num_iterations"], ref["num_successful_steps"])
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"])
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"]) + 1e-12
    assert np.allclose(x, ref_x, rtol=1e-6, atol=1e-9)
    if max_iters == 0:
        assert np.array_equal(x, rpyxyz0) and s.num_iterations == 0
    mp.close(); sc.close()


# ----------------------------------------------------------------------------- rejected and invalid steps
# Far starts behind a wide association gate: the scan keeps its correspondences, the first Gauss-Newton-sized steps overshoot, and the
# trust region has to shrink before a step is taken.  Chosen on the CPU with the references alone (oracle.icp_solve; for the lines
# tests/edge_ref.py, whose plane-only solves agree with the oracle's on these inputs to 1e-14) so that they report more iterations than
# successful steps; scans of 250 points (one workgroup per pass) against 20000 map points of configs[2], six iterations allowed.
#   name: (mode, prior weight, start = (dq, dt) * pose0 with dq the vector part of a quaternion of scalar part 1, gate, line points)
REJECT_CASES = {
    "mode0": (0, 0.0, (0.647, -0.293, 0.117), (1.107, -0.332, -1.559), 25.0, 0),
    "mode1-prior": (1, 0.05, (-0.4, -1.186, -0.449), (-0.002, -0.014, -0.552), 100.0, 0),
    "edges": (1, 0.0, (0.133, -0.661, -0.278), (-0.798, -0.016, -1.496), 100.0, 12),
}
REJECT_ITERS = 6
_reject_cache = {}


def reject_inputs(case):
    """dict(map, scan, map_edge, scan_edge, map_pose, pose0, rpyxyz0, mode, prior, thr, weight, huber): the arrays of one REJECT_CASES entry"""
    from tests import edge_ref as er
    if "c" not in _reject_cache:
        _reject_cache["c"] = syn.config3_icp()
    c = _reject_cache["c"]
    mode, prior, dq, dt, thr, n_lines = case
    r = np.random.default_rng(7 + mode)
    qa = c["query"][c["query_ground"]] if mode == 0 else c["query"][~c["query_ground"]]
    ma = c["map"][c["map_ground"]] if mode == 0 else c["map"][~c["map_ground"]]
    qq = qa[np.sort(r.choice(qa.shape[0], 250, replace=False))]
    mm = ma[np.sort(r.choice(ma.shape[0], 20000, replace=False))]
    d = np.array(list(dq) + [1.0]); d /= np.linalg.norm(d)
    pose0 = er.se3_mul(np.concatenate([d, dt]), np.array(c["pose0"], float))
    out = dict(map=mm, scan=qq, map_edge=None, scan_edge=None, map_pose=np.array(c["map_pose"], float), pose0=pose0, mode=mode, prior=prior, thr=thr,
               rpyxyz0=er.se3_to_rpyxyz(er.se3_mul(er.se3_inv(c["map_pose"]), pose0)), weight=syn.W_LIDAR_GROUND if mode == 0 else syn.W_LIDAR_SURF,
               huber=0.0 if mode == 0 else 0.1)
    if n_lines:      # three poles around the true pose in the map, n_lines points of them in the scan
        pt = np.array(c["pose_true"], float)
        R, t = er.rotmat(pt[:4]), pt[4:]
        rng = np.random.default_rng(12)
        poles = [t[:2] + o for o in ([3.0, 2.0], [-3.0, 2.5], [4.0, -2.0])]
        out["map_edge"] = er._pad(np.concatenate([er._pole(rng, xy, 80, t[2] - 1.5, t[2] + 1.5) for xy in poles]))
        out["scan_edge"] = er._pad((np.concatenate([er._pole(rng, xy, n_lines // 3, t[2] - 1.2, t[2] + 1.2) for xy in poles]) - t) @ R)
    return out


def run_reject_case(ctx, case):
    """(rpyxyz, summary) of the device solve of one REJECT_CASES entry"""
    from lvio_fusion_amd import api
    i = reject_inputs(case)
    mp, sc = api.Map(ctx, i["map"], i["thr"]), api.Scan(ctx, i["scan"])
    x = i["rpyxyz0"].copy()
    if i["map_edge"] is None:
        s = api.icp_solve(mp, sc, i["map_pose"], i["pose0"], x, i["mode"], i["thr"], i["weight"], i["huber"], prior_weight=i["prior"], max_num_iterations=REJECT_ITERS)
    else:
        me, se = api.Map(ctx, i["map_edge"], i["thr"]), api.Scan(ctx, i["scan_edge"])
        s = api.icp_solve_edges(mp, sc, me, se, i["map_pose"], i["pose0"], x, i["thr"], i["weight"], i["huber"], api.edge_icp_options(0.2, thr=i["thr"]),
                                prior_weight=i["prior"], max_num_iterations=REJECT_ITERS)
        me.close(); se.close()
    mp.close(); sc.close()
    return x, s


@pytest.mark.parametrize("name", list(REJECT_CASES))
def test_icp_rejected_steps_parity(ctx, oracle, name):
    """The decision path of the device loop off its main line: steps that are rejected (the radius divided by a doubling factor) or invalid
    (the radius halved) before one is taken.  The CPU reference must report such steps by itself, then test_icp_solve_parity's tolerances."""
    from tests import edge_ref as er
    i = reject_inputs(REJECT_CASES[name])
    if i["map_edge"] is None:
        ref_x, ref = oracle.icp_solve(i["map"], i["scan"], i["map_pose"], i["pose0"], i["rpyxyz0"], i["mode"], i["thr"], i["weight"], i["huber"], prior_w=i["prior"],
                                      max_iters=REJECT_ITERS)
    else:
        ref_x, ref = er.icp_solve_edges(i["map"], i["scan"], i["map_edge"], i["scan_edge"], i["map_pose"], i["pose0"], i["rpyxyz0"], i["thr"], i["weight"], i["huber"],
                                        dict(er.edge_defaults(0.2), thr=i["thr"]), prior_w=i["prior"], max_iters=REJECT_ITERS)
        n_planes = er.plane_correspondences(i["map"], i["scan"], i["pose0"], i["thr"])[0].shape[0]
        assert ref["num_residual_blocks"] - n_planes >= 3                      # a few line blocks beside the planes
    assert ref["num_iterations"] > ref["num_successful_steps"] >= 1            # the reference alone: a rejected or invalid step, and an accepted one
    assert i["scan"].shape[0] <= 256 and ref["num_residual_blocks"] >= 100
    x, s = run_reject_case(ctx, REJECT_CASES[name])
    print(f"{name}: blocks {s.num_residual_blocks}, iterations {s.num_iterations} / {s.num_successful_steps} (reference {ref['num_iterations']} / "
          f"{ref['num_successful_steps']}), cost {s.initial_cost:.9e} -> {s.final_cost:.9e} (reference {ref['initial_cost']:.9e} -> {ref['final_cost']:.9e}), "
          f"|dx| {np.abs(x - ref_x).max():.2e}")
    assert s.num_residual_blocks == ref["num_residual_blocks"]
    assert s.num_iterations == ref["num_iterations"] and s.num_successful_steps == ref["num_successful_steps"]
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"])
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.allclose(x, ref_x, rtol=1e-6, atol=1e-9)
    untouched = [0, 3, 4] if i["mode"] == 0 else [1, 2, 5]
    assert np.array_equal(x[untouched], i["rpyxyz0"][untouched])
