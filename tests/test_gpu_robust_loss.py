"""GPU parity of every robust-loss call site with BOTH Huber branches inside one linearisation.

The rest of the suite enters the visual solvers all linear (huber_a = 1 under norms of 40 and more) and the LiDAR solves all quadratic
(huber_a = 0.1 over |r| <= 0.01).  Here the thresholds come from tests/robust_cases.py, whose census tests/test_robust_cases.py proves on
the CPU: about half of the blocks on either side at every linearisation.  Assertions and tolerances are those of the one-branch tests named
in each docstring."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import edge_ref as er
from tests import robust_cases as rc
from tests.helpers import assert_parity
from tests.test_gpu_solve_trajectory import check, close, make, okw, options
from tests.test_gpu_solver import build, state_of
from tests.test_oracle_lm_numpy import dense_system

pytestmark = pytest.mark.gpu

FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def device_window(api, ctx, oracle, name):
    """(st, prob, win, closer) of rc.window(name) on the device and in the oracle"""
    cfg, use = rc.window(name)
    n_kf, n_lm, seed, _, perm = rc.WINDOWS[name]
    if perm:
        w = make(api, ctx, oracle, 0, 0, seed, cfg=cfg)
        return w["st"], w["prob"], w["win"], lambda: close(w)
    cfg_b, st, b, prob, win = build(api, ctx, oracle, n_kf, max(n_lm, 1), seed, use=use)
    assert all(np.array_equal(cfg_b[k], cfg[k]) for k in ("poses", "inv_depth")) and np.array_equal(cfg_b["tf"]["ob"], cfg["tf"]["ob"])

    def closer():
        prob.close()
        for h in list(b.values()) + [st]:
            if h is not None:
                h.close()
    return st, prob, win, closer


def assert_state(api, st, win, what):
    s = state_of(api, st)
    for k in FIELDS:
        assert_parity(np.asarray(s[k]).reshape(np.asarray(getattr(win, k)).shape), getattr(win, k), f"{k} {what}")


def restore(api, w):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        w["st"].set(field, w["cfg"][key])


# ----------------------------------------------------------------------------- (a) the evaluate surface
def test_evaluate_local_cost_and_gradient_with_both_branches(ctx, oracle):
    """test_gpu_evaluate.test_local_jacobians_and_gradient at a threshold that splits every batch: robustified residuals and local Jacobians
    per batch against the rows of dense_system(huber_a = a), Problem.cost and Problem.gradient at that a; the imu batch ignores a."""
    from lvio_fusion_amd import api
    name = "kf8"
    n_kf, n_lm, seed, use, _ = rc.WINDOWS[name]
    cfg, st, b, prob, win = build(api, ctx, oracle, n_kf, n_lm, seed)
    a = rc.ladder(oracle, name)[0]["a"]
    pre = rc.preint(oracle, cfg)
    state = rc.state_of(cfg)
    J, r, cost = dense_system(oracle, cfg, pre, state, huber_a=a)
    J1, r1, cost1 = dense_system(oracle, cfg, pre, state)                     # the default threshold: a different system
    assert abs(cost1 - cost) > 1e-3 * cost
    g = J.T @ r
    opt = api.default_solver_options(); opt.huber_a = a
    gc, gl = prob.gradient(opt)
    assert_parity(gc, g[:15 * n_kf], "gradient (keyframe part)"); assert_parity(gl, g[15 * n_kf:], "gradient (inverse depths)")
    assert abs(prob.cost(opt) - cost) <= 1e-10 * cost
    tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
    row, seen = 0, {}
    rr, Jl = b["tc"].evaluate_local(st, a)
    raw, _ = b["tc"].evaluate_local(st, 0.0)
    seen["tc"] = np.abs(rr - raw).max(axis=1) > 0                              # blocks the loss scaled: the linear ones
    for i in range(b["tc"].n):
        assert_parity(rr[i], r[row:row + 2], "tc r"); assert_parity(Jl[i][:, 0], J[row:row + 2, 15 * n_kf + tc["lm_idx"][i]], "tc J"); row += 2
    rr, Jl = b["tf"].evaluate_local(st, a)
    raw, _ = b["tf"].evaluate_local(st, 0.0)
    seen["tf"] = np.abs(rr - raw).max(axis=1) > 0
    assert Jl.shape[2] == 13
    for i in range(b["tf"].n):
        k1, k2, l = tf["kf1_idx"][i], tf["kf2_idx"][i], tf["lm_idx"][i]
        ref = np.concatenate([J[row:row + 2, [15 * n_kf + l]], J[row:row + 2, 6 * k1:6 * k1 + 6], J[row:row + 2, 6 * k2:6 * k2 + 6]], axis=1)
        assert_parity(rr[i], r[row:row + 2], "tf r"); assert_parity(Jl[i], ref, "tf J"); row += 2
    rr, Jl = b["po"].evaluate_local(st, a)
    raw, _ = b["po"].evaluate_local(st, 0.0)
    seen["po"] = np.abs(rr - raw).max(axis=1) > 0
    for i in range(b["po"].n):
        k = po["kf_idx"][i]
        assert_parity(rr[i], r[row:row + 2], "po r"); assert_parity(Jl[i], J[row:row + 2, 6 * k:6 * k + 6], "po J"); row += 2
    rr, Jl = b["imu"].evaluate_local(st, a)
    r0, J0 = b["imu"].evaluate_local(st, 0.0)
    assert np.array_equal(rr, r0) and np.array_equal(Jl, J0), "the imu batch carries no loss: huber_a must not reach it"
    for f, fac in enumerate(cfg["imu"]):
        ki, kj = fac["kf_i"], fac["kf_j"]
        oi, oj = 6 * n_kf + 9 * ki, 6 * n_kf + 9 * kj
        ref = np.concatenate([J[row:row + 15, 6 * ki:6 * ki + 6], J[row:row + 15, oi:oi + 9], J[row:row + 15, 6 * kj:6 * kj + 6], J[row:row + 15, oj:oj + 9]], axis=1)
        assert_parity(rr[f], r[row:row + 15], "imu r"); assert_parity(Jl[f], ref, "imu J"); row += 15
    assert row == len(r)
    # the device took the branches the census counted
    want = rc.ladder(oracle, name)[0]["shares"]
    for k in rc.KINDS:
        assert float(seen[k].mean()) == want[k] and 0.0 < want[k] < 1.0, (k, float(seen[k].mean()), want[k])
    for h in list(b.values()) + [st]:
        h.close()
    prob.close()


# ----------------------------------------------------------------------------- (b) per-iteration parity over the ladder
@pytest.mark.parametrize("name", list(rc.WINDOWS))
def test_lm_iteration_parity_over_the_ladder(ctx, oracle, name):
    """test_gpu_solver.test_lm_iteration_parity's assertions with huber_a = a_k on both sides, a_k from the ladder: every linearisation, the
    cost pass of every candidate and the reduced system carry blocks of both branches"""
    from lvio_fusion_amd import api
    st, prob, win, closer = device_window(api, ctx, oracle, name)
    opt = api.default_solver_options()
    radius, dec = 1e4, 2.0
    for it, step in enumerate(rc.ladder(oracle, name)):
        a = step["a"]
        opt.huber_a = a
        if it == 0:
            c_gpu = prob.cost(opt)
            assert abs(c_gpu - win.cost(a)) <= 1e-9 * abs(c_gpu)
        ref = win.lm_iteration(radius, dec, huber_a=a)
        got = prob.lm_iteration(opt, radius, dec)
        print(f"{name} it{it}: a = {a:.4f}, cost {got['cost_before']:.9e} -> {got['cost_after']:.9e} (oracle {ref['cost_before']:.9e} -> {ref['cost_after']:.9e}), "
              f"accepted {got['accepted']} / {ref['accepted']}")
        assert abs(got["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"])
        S, rhs = prob.reduced_system()
        scale = np.abs(ref["S"]).max()
        assert np.abs(S - ref["S"]).max() <= 1e-7 * scale, f"iteration {it}: reduced system mismatch"
        assert_parity(rhs, ref["rhs"], f"rhs it{it}")
        assert got["accepted"] == ref["accepted"]
        assert abs(got["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"])
        assert abs(got["radius"] - ref["radius"]) <= 1e-5 * ref["radius"]
        assert_state(api, st, win, f"it{it}")
        assert abs(radius - step["radius"]) <= 1e-9 * radius                      # this chain IS the ladder's chain: its census holds here
        radius, dec = ref["radius"], ref["decrease_factor"]
    closer()


# ----------------------------------------------------------------------------- (c) all quadratic with a > 0
@pytest.mark.parametrize("name", ["kf8", "kf2"])
def test_all_quadratic_threshold_is_the_trivial_loss(ctx, oracle, name):
    """huber_a = 1e9 (every block quadratic THROUGH the loss) against huber_a = 0 (no loss) on the device: cost, reduced system and new state
    agree to 1e-12 relative; both agree with the oracle at 1e9.  The branch a well-tracked window lives in."""
    from lvio_fusion_amd import api
    out = []
    for a in (1e9, 0.0):
        st, prob, win, closer = device_window(api, ctx, oracle, name)
        opt = api.default_solver_options(); opt.huber_a = a
        got = prob.lm_iteration(opt, 1e4, 2.0)
        S, rhs = prob.reduced_system()
        out.append((got, np.tril(S), rhs, state_of(api, st)))
        if a > 0:
            ref = win.lm_iteration(1e4, 2.0, huber_a=a)
            assert abs(got["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"])
            assert np.abs(S - ref["S"]).max() <= 1e-7 * np.abs(ref["S"]).max()
            assert_parity(rhs, ref["rhs"], "rhs")
            assert got["accepted"] == ref["accepted"] and ref["accepted"]
            assert abs(got["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"])
            assert_state(api, st, win, "at 1e9")
            assert abs(win.cost(1.0) - ref["cost_after"]) > 1e-3 * ref["cost_after"]
        closer()
    (g1, S1, r1, s1), (g0, S0, r0, s0) = out
    rel = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max() / np.abs(np.asarray(y)).max())
    figs = dict(cost_before=rel(g1["cost_before"], g0["cost_before"]), cost_after=rel(g1["cost_after"], g0["cost_after"]), S=rel(S1, S0), rhs=rel(r1, r0),
                **{k: rel(s1[k], s0[k]) for k in FIELDS})
    print(f"{name}: 1e9 against 0, relative differences {figs}")
    assert g1["accepted"] == g0["accepted"]
    for k, v in figs.items():
        assert v <= 1e-12, (k, v)


# ----------------------------------------------------------------------------- (d) the device loop
@pytest.mark.parametrize("spec", rc.SOLVES, ids=lambda s: f"kf{s[0]}")
def test_device_loop_at_a_fixed_threshold(ctx, oracle, spec):
    """test_gpu_solve_trajectory.test_device_loop_equals_oracle_chain with huber_a = a_fix: the solve starts all linear and ends with every kind
    mixed, so blocks cross the threshold while the loop runs (the fused linearise-at-candidate kernel, or with LVF_FUSED_LIN=0 the classic
    cost + linearise pair, see below)"""
    from lvio_fusion_amd import api
    f = rc.a_fix(oracle, spec)
    w = make(api, ctx, oracle, *spec)
    assert np.array_equal(w["cfg"]["poses"], rc.solve_window(spec)["poses"])
    o = options(api, huber_a=f["a"])
    ref = w["win"].solve(**okw(o))
    assert (ref["num_iterations"], ref["why"]) == (f["ref"]["num_iterations"], f["ref"]["why"]) and ref["num_successful_steps"] >= 3      # the census' solve
    s = w["prob"].solve(o)
    print(f"{spec}: a_fix = {f['a']:.3f}, device {s.num_iterations} iterations ({s.num_successful_steps} ok), cost {s.initial_cost:.9e} -> {s.final_cost:.9e}; "
          f"oracle {ref['num_iterations']} ({ref['num_successful_steps']} ok), {ref['initial_cost']:.9e} -> {ref['final_cost']:.9e}")
    check(api, w, s, ref, f"{spec}, huber_a = {f['a']:.3f}")
    close(w)


def test_device_loop_at_a_fixed_threshold_classic_chain():
    """the same solve with LVF_FUSED_LIN=0: the cost kernel's three sites and the linearising kernels instead of the fused one (the switch is
    read once per process, hence the child process)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env["LVF_FUSED_LIN"] = "0"
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", os.path.join(root, "tests", "test_gpu_robust_loss.py"),
                        "-k", "test_device_loop_at_a_fixed_threshold and kf5"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "1 passed" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]


# ----------------------------------------------------------------------------- (e) the batch: tables rebuilt when huber_a changes
def test_batch_rebuilds_its_tables_for_another_threshold(ctx, oracle):
    """One ProblemBatch, solved with a_fix, with huber_a = 1 and with a_fix again from the same start: each solve against its oracle chains
    (test_batched_loop_equals_oracle_chains' check), the first and the third equal to 1e-12; then one batch.lm_iteration at a ladder-style
    threshold against the oracle."""
    from lvio_fusion_amd import api
    a_solve, a_step = rc.batch_thresholds(oracle)
    ws = [make(api, ctx, oracle, *spec) for spec in rc.SOLVES]
    batch = api.ProblemBatch(ctx, [w["prob"] for w in ws])
    runs = []
    for a in (a_solve, 1.0, a_solve):
        o = options(api, huber_a=a)
        assert batch.uses_tables(o) == 1
        for w in ws:
            restore(api, w)
            w["win"] = oracle.Window(w["cfg"], rc.preint(oracle, w["cfg"]))
        refs = [w["win"].solve(**okw(o)) for w in ws]
        out = batch.solve(o)
        for i, (w, s, ref) in enumerate(zip(ws, out, refs)):
            check(api, w, s, ref, f"batch member {i}, huber_a = {a:.3f}")
        runs.append(([(s.num_iterations, s.num_successful_steps, s.why) for s in out], [s.final_cost for s in out], [state_of(api, w["st"]) for w in ws]))
    assert runs[0][0] != runs[1][0] or abs(runs[0][1][0] - runs[1][1][0]) > 1e-3 * runs[0][1][0]      # huber_a = 1 is another problem
    assert runs[0][0] == runs[2][0]
    for i in range(len(ws)):
        d = {k: float(np.abs(runs[0][2][i][k] - runs[2][2][i][k]).max() / np.abs(runs[0][2][i][k]).max()) for k in FIELDS}
        d["final_cost"] = abs(runs[0][1][i] - runs[2][1][i]) / runs[0][1][i]
        print(f"batch member {i}: first against third solve, relative differences {d}")
        assert all(v <= 1e-12 for v in d.values()), d
    # one iteration through the per-call batch entry point
    o = options(api, huber_a=a_step)
    for w in ws:
        restore(api, w)
        w["win"] = oracle.Window(w["cfg"], rc.preint(oracle, w["cfg"]))
    got = batch.lm_iteration(o, [1e4] * len(ws), [2.0] * len(ws))
    for i, w in enumerate(ws):
        ref = w["win"].lm_iteration(1e4, 2.0, huber_a=a_step)
        g = got[i]
        assert abs(g["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"])
        S, rhs = w["prob"].reduced_system()
        assert np.abs(S - ref["S"]).max() <= 1e-7 * np.abs(ref["S"]).max()
        assert_parity(rhs, ref["rhs"], f"rhs, member {i}")
        assert g["accepted"] == ref["accepted"]
        assert abs(g["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"])
        assert abs(g["radius"] - ref["radius"]) <= 1e-5 * ref["radius"]
        assert_state(api, w["st"], w["win"], f"member {i} after the batch iteration")
    batch.close(); close(*ws)


# ----------------------------------------------------------------------------- (f) the LiDAR solves
def _icp_assert(s, ref, x, ref_x, rpyxyz0):
    """test_gpu_icp.test_icp_solve_parity's assertions"""
    print(f"blocks {s.num_residual_blocks}, iterations {s.num_iterations} / {s.num_successful_steps}, cost {s.initial_cost:.9e} -> {s.final_cost:.9e} "
          f"(oracle {ref['initial_cost']:.9e} -> {ref['final_cost']:.9e}), |dx| {np.abs(x - ref_x).max():.2e}")
    assert s.num_residual_blocks == ref["num_residual_blocks"] and s.num_residual_blocks > 500
    assert s.num_iterations == ref["num_iterations"] and s.num_successful_steps == ref["num_successful_steps"]
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"])
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.allclose(x, ref_x, rtol=1e-6, atol=1e-9)
    assert np.array_equal(x[[1, 2, 5]], rpyxyz0[[1, 2, 5]])


@pytest.mark.parametrize("which,prior", [("a_icp", 0.0), ("a_icp", 500 * syn.W_VISUAL), ("all_linear", 0.0)])
def test_icp_solve_with_both_branches(ctx, oracle, which, prior):
    """test_gpu_icp.test_icp_solve_parity (mode 1) with huber_a = a_icp, the median |r| (half of the planes linear), and with 1e-6: every
    plane linear with a scale of about 0.03"""
    from lvio_fusion_amd import api
    i = rc.icp_surf(oracle)
    c, mm, qq, thr, w, rp0 = i["c"], i["mm"], i["qq"], i["thr"], i["w"], i["rpyxyz0"]
    huber = i["a"] if which == "a_icp" else 1e-6
    ref_x, ref = oracle.icp_solve(mm, qq, c["map_pose"], c["pose0"], rp0, 1, thr, w, huber, prior_w=prior)
    _, ref01 = oracle.icp_solve(mm, qq, c["map_pose"], c["pose0"], rp0, 1, thr, w, 0.1, prior_w=prior)
    assert abs(ref01["initial_cost"] - ref["initial_cost"]) > 1e-3 * ref["initial_cost"]           # today's 0.1 is another problem
    mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
    x = rp0.copy()
    s = api.icp_solve(mp, sc, c["map_pose"], c["pose0"], x, 1, thr, w, huber, prior_weight=prior)
    _icp_assert(s, ref, x, ref_x, rp0)
    assert s.final_cost <= s.initial_cost and (prior > 0 or s.final_cost < s.initial_cost)
    mp.close(); sc.close()


def test_lidar_solve_with_both_branches(ctx, oracle):
    """test_gpu_icp.test_lidar_solve_on_caller_built_batch (mode 1, with the prior) at a_icp"""
    from lvio_fusion_amd import api
    i = rc.icp_surf(oracle)
    c, mm, qq, thr, w, rp0 = i["c"], i["mm"], i["qq"], i["thr"], i["w"], i["rpyxyz0"]
    prior = 500 * syn.W_VISUAL
    ref_x, ref = oracle.icp_solve(mm, qq, c["map_pose"], c["pose0"], rp0, 1, thr, w, i["a"], prior_w=prior)
    mp, sc = api.Map(ctx, mm, thr), api.Scan(ctx, qq)
    api.knn3(mp, sc, c["pose0"], thr)
    idx, d2, valid = sc.download()
    v = valid > 0
    p = qq[v, :3].astype(np.float64)
    pa, pb, pc = (mm[idx[v, k], :3].astype(np.float64) for k in range(3))
    b = api.lidar_plane_batch(ctx, 1, p, pa, pb, pc, c["map_pose"], w)
    x = rp0.copy()
    s = api.lidar_solve(b, x, i["a"], prior_weight=prior)
    _icp_assert(s, ref, x, ref_x, rp0)
    b.close(); mp.close(); sc.close()


@pytest.mark.parametrize("case,use_surf,use_edge", [("both", True, True), ("lines", False, True)])
def test_icp_solve_edges_with_both_branches(ctx, oracle, case, use_surf, use_edge):
    """test_gpu_edge.test_icp_solve_edges_parity's assertions on its largest scene with huber_a = a_icp for the planes and the median line
    norm for the lines"""
    from lvio_fusion_amd import api
    e = rc.edge_scene()
    s, a_plane, a_edge = e["s"], rc.icp_surf(oracle)["a"], e["a_edge"]
    edge = er.edge_defaults(rc.EDGE_RES); edge["huber_a"] = a_edge
    eo = api.edge_icp_options(rc.EDGE_RES, huber_a=a_edge)
    ms = api.Map(ctx, s["map_surf"], rc.EDGE_THR_SURF) if use_surf else None
    ss = api.Scan(ctx, s["scan_surf"]) if use_surf else None
    me, se = api.Map(ctx, s["map_edge"], edge["thr"]), api.Scan(ctx, s["scan_edge"])
    x = s["rpyxyz0"].copy()
    summ = api.icp_solve_edges(ms, ss, me, se, s["map_pose"], s["pose0"], x, rc.EDGE_THR_SURF, rc.EDGE_W_SURF, a_plane, eo)
    x_ref, ref = er.icp_solve_edges(s["map_surf"] if use_surf else None, s["scan_surf"], s["map_edge"], s["scan_edge"], s["map_pose"], s["pose0"], s["rpyxyz0"],
                                    rc.EDGE_THR_SURF, rc.EDGE_W_SURF, a_plane, edge)
    _, ref01 = er.icp_solve_edges(s["map_surf"] if use_surf else None, s["scan_surf"], s["map_edge"], s["scan_edge"], s["map_pose"], s["pose0"], s["rpyxyz0"],
                                  rc.EDGE_THR_SURF, rc.EDGE_W_SURF, 0.1, er.edge_defaults(rc.EDGE_RES))
    assert abs(ref01["initial_cost"] - ref["initial_cost"]) > 1e-3 * ref["initial_cost"]
    for h in (ms, ss, me, se):
        if h is not None:
            h.close()
    print(f"{case}: blocks {summ.num_residual_blocks}, iterations {summ.num_iterations} / {summ.num_successful_steps}, cost {summ.initial_cost:.9e} -> {summ.final_cost:.9e} "
          f"(reference {ref['initial_cost']:.9e} -> {ref['final_cost']:.9e}), |dx| {np.abs(x - x_ref).max():.2e}")
    assert summ.num_residual_blocks == ref["num_residual_blocks"] == (300 if use_surf else 0) + 257
    assert summ.num_iterations == ref["num_iterations"] and summ.num_successful_steps == ref["num_successful_steps"]
    assert abs(summ.initial_cost - ref["initial_cost"]) <= 1e-6 * abs(ref["initial_cost"])
    assert abs(summ.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.all(np.abs(x - x_ref) <= 1e-6 * np.abs(x_ref))
    assert np.array_equal(x[[1, 2, 5]], s["rpyxyz0"][[1, 2, 5]])
    assert summ.num_successful_steps >= 1 and summ.final_cost < summ.initial_cost
