"""The product form of the (v, ba, bg) back substitution (csrc/solver_chol.hip: back_product_ride; csrc/solver_back.hip: back_product_body,
chol_backsolve_body<false>): x_sparse = G [x_dense ; -1], with G formed by workgroups riding behind the block-step launches of the dense
Cholesky and multiplied by sibling workgroups of k_backsolve_tail, against the sequential sparse levels it replaces (LVF_BACK_PRODUCT=0).

Which branch a window takes is decided by its elimination plan: the product form needs one block-step launch per sparse level
(n_levels <= nb) and the merged back-substitution launch.  (n_levels, nb, lvf_problem_debug_back_product) of config4_window at 300
landmarks, as printed by test_plan_table_and_branches (MI355X):

    n_kf     5   8  10  16  20  24  32  50
    levels   1   3   1   3   2   3   3   5
    nb       1   1   2   2   3   3   4   5
    product  1   0   1   0   1   1   1   1

Kept windows (landmark counts small: the landmark pass is not what is tested):
    kf5   the smallest keyframe count where the path is on
    kf8   the smallest where it is off because n_levels > nb (both children run the sequential levels: the switch must change nothing)
    kf10  n_levels < nb: the riders are done before the last block step
    kf50  1 500 landmarks: five levels in five block steps and a (v, ba, bg) block left in the dense corner's padding
    kf20c a constant (v, ba, bg) keyframe in the middle of the chain; kf10p keyframe 0's pose constant

On against off runs in two child processes (the switch is read once per process), each running every window: one LM iteration from the
perturbed start at radius 1e4 (accepted), then a 6-iteration solve from the same start.  Tolerances: tests/test_gpu_handover.py's
same_state (1e-9 of the field's largest magnitude) and 1e-9 relative on the costs — the project's bound between alternative paths that
differ in summation order; run-to-run 1e-12 / 1e-11, as test_gpu_handover.py's repeatability checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAN_KFS = (5, 8, 10, 16, 20, 24, 32, 50)
# name: (n_kf, n_lm, seed, constant (v, ba, bg) keyframe or None, keyframe-0 pose constant, expected product path)
WINDOWS = {
    "kf5": (5, 300, 501, None, False, 1),
    "kf8": (8, 300, 502, None, False, 0),
    "kf10": (10, 400, 503, None, False, 1),
    "kf50": (50, 1500, 504, None, False, 1),
    "kf20c": (20, 600, 505, 9, False, 1),      # (the plan depends on n_kf and the IMU pairs only, not on constant flags: as 20 in the table)
    "kf10p": (10, 400, 506, None, True, 1),
}
FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")


def fixed(api, n):
    o = api.default_solver_options()
    o.max_num_iterations = n; o.function_tolerance = 0.0; o.parameter_tolerance = 0.0; o.gradient_tolerance = 0.0
    return o


def window(api, syn, ctx, n_kf, n_lm, seed, vbb_const=None, pose0_const=False):
    cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=max(100, n_lm // 5), seed=seed)
    pre = api.preintegrate_or_none(ctx, cfg)
    st = api.State(ctx, cfg["n_kf"], cfg["n_lm"])
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
        st.set(field, cfg[key])
    tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
    hs = [api.two_camera_batch(ctx, cfg["cam0"], cfg["cam1"], tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"]),
          api.two_frame_batch(ctx, cfg["cam0"], cfg["cam1"], tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"]),
          api.pose_only_batch(ctx, cfg["cam0"], po["ob"], po["kf_idx"], po["pw_idx"], po["pw"]),
          api.imu_batch(ctx, pre, [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]])]
    prob = api.Problem(ctx, st, *hs)
    if vbb_const is not None:
        prob.set_vbb_constant(int(vbb_const), True, True, True)
    if pose0_const:
        prob.set_pose_constant(0, True)
    return cfg, st, hs, prob


def reset(api, st, cfg):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        st.set(field, cfg[key])


def state(api, st):
    return {k: np.asarray(st.get(f), dtype=np.float64).ravel().tolist() for k, f in zip(FIELDS, (api.POSES, api.VEL, api.BA, api.BG, api.INV_DEPTH))}


def child():
    """Every window in this process: the plan table, one LM iteration and a 6-iteration solve per kept window; one JSON line."""
    from lvio_fusion_amd import api, synthetic as syn
    ctx = api.Context(0)
    out = {"plan": {}, "win": {}}
    for n_kf in PLAN_KFS:
        cfg, st, hs, prob = window(api, syn, ctx, n_kf, 300, 400 + n_kf)
        out["plan"][str(n_kf)] = prob.debug_back_product()
        prob.close()
        for h in hs + [st]:
            h.close()
    for name, (n_kf, n_lm, seed, vc, pc, _) in WINDOWS.items():
        cfg, st, hs, prob = window(api, syn, ctx, n_kf, n_lm, seed, vc, pc)
        r = {"product": prob.debug_back_product()}
        g = prob.lm_iteration(api.default_solver_options(), 1e4, 2.0)
        r["iteration"] = {k: float(g[k]) for k in ("cost_before", "cost_after", "radius")}
        r["iteration"]["accepted"] = bool(g["accepted"])
        r["iteration_state"] = state(api, st)
        reset(api, st, cfg)
        s = prob.solve(fixed(api, 6))
        r["solve"] = {"final_cost": s.final_cost, "initial_cost": s.initial_cost, "num_iterations": s.num_iterations,
                      "num_successful_steps": s.num_successful_steps, "num_unsuccessful_steps": s.num_unsuccessful_steps, "hand_over_retries": s.hand_over_retries}
        r["solve_state"] = state(api, st)
        out["win"][name] = r
        prob.close()
        for h in hs + [st]:
            h.close()
    ctx.close()
    print(json.dumps(out))


_runs = {}


def run(switch):
    """The child's results with LVF_BACK_PRODUCT unset (None) or "0"; its chain lines (LVF_CHAIN_INFO) carry n_levels and nb.  Run once, shared."""
    if switch not in _runs:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ)
        env.pop("LVF_BACK_PRODUCT", None)
        if switch is not None:
            env["LVF_BACK_PRODUCT"] = switch
        env["LVF_CHAIN_INFO"] = "1"
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        res = json.loads(p.stdout.strip().splitlines()[-1])
        chains = {}
        for line in p.stderr.splitlines():
            if line.startswith("chain: n_kf "):
                t = line.split()
                f = lambda key: int(t[t.index(key) + 1].strip("(),"))
                chains.setdefault(f("n_kf"), (f("levels"), f("(nb"), f("back_product")))      # the first chain built for a keyframe count: the plan table's
        res["chains"] = chains
        _runs[switch] = res
    return _runs[switch]


def test_plan_table_and_branches():
    """Both branches are covered and known: the table of the module docstring, and every kept window on the branch it was kept for."""
    on, off = run(None), run("0")
    print("n_kf: (n_levels, nb, product)")
    for n_kf in PLAN_KFS:
        lv, nb, bp = on["chains"][n_kf]
        print(f"  {n_kf}: ({lv}, {nb}, {on['plan'][str(n_kf)]})")
        assert on["plan"][str(n_kf)] == bp == (1 if 1 <= lv <= nb else 0)
        assert off["plan"][str(n_kf)] == 0
    c = on["chains"]
    assert c[5][2] == 1 and not any(c[k][2] for k in PLAN_KFS if k < 5), "kf5 is the smallest window on the product path"
    assert c[8][0] > c[8][1] and c[8][2] == 0 and all(c[k][2] for k in PLAN_KFS if k < 8), "kf8 is the smallest window that is off for n_levels > nb"
    assert c[10][0] < c[10][1] and c[10][2] == 1, "kf10: fewer levels than block steps"
    assert c[50][:2] == (5, 5) and c[50][2] == 1, "kf50: five levels in five block steps"
    for name, spec in WINDOWS.items():
        assert on["win"][name]["product"] == spec[5], name
        assert off["win"][name]["product"] == 0, name


@pytest.mark.parametrize("name", list(WINDOWS))
def test_on_against_off(name):
    """One accepted LM iteration and a 6-iteration solve: same accept / reject sequence and counts, states by same_state at 1e-9, costs to
    1e-9 relative.  kf20c (constant (v, ba, bg) block mid-chain) and kf10p (keyframe 0's pose constant) are the constant-block cases."""
    from tests.test_gpu_handover import same_state
    a, b = run(None)["win"][name], run("0")["win"][name]
    ia, ib = a["iteration"], b["iteration"]
    assert ia["accepted"] and ib["accepted"], "the radius must be large enough for the step to be taken"
    rel = lambda x, y: abs(x - y) / abs(y)
    print(name, "iteration cost_after rel", rel(ia["cost_after"], ib["cost_after"]), "solve final_cost rel", rel(a["solve"]["final_cost"], b["solve"]["final_cost"]))
    assert rel(ia["cost_before"], ib["cost_before"]) <= 1e-9 and rel(ia["cost_after"], ib["cost_after"]) <= 1e-9 and rel(ia["radius"], ib["radius"]) <= 1e-9
    same_state({k: np.array(v) for k, v in a["iteration_state"].items()}, {k: np.array(v) for k, v in b["iteration_state"].items()})
    sa, sb = a["solve"], b["solve"]
    assert sa["hand_over_retries"] == 0 and sb["hand_over_retries"] == 0
    for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps"):
        assert sa[k] == sb[k], k
    assert sa["num_successful_steps"] >= 1
    assert rel(sa["initial_cost"], sb["initial_cost"]) <= 1e-9 and rel(sa["final_cost"], sb["final_cost"]) <= 1e-9
    same_state({k: np.array(v) for k, v in a["solve_state"].items()}, {k: np.array(v) for k, v in b["solve_state"].items()})


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["kf5", "kf8", "kf10", "kf50", "kf10p"])
def test_against_the_oracle_chain(ctx, oracle, name):
    """The same windows through the oracle's chained LM loop, as tests/test_gpu_solve_trajectory.py compares (its helpers, its tolerances)."""
    from lvio_fusion_amd import api, synthetic as syn
    from tests.test_gpu_solve_trajectory import check, close, make, okw, options
    n_kf, n_lm, seed, _, pose0, want = WINDOWS[name]
    cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=max(100, n_lm // 5), seed=seed)
    pc = None
    if pose0:
        pc = np.zeros(n_kf, np.uint8); pc[0] = 1
    w = make(api, ctx, oracle, n_kf, n_lm, seed, cfg=cfg, pose_const=pc)
    if os.environ.get("LVF_BACK_PRODUCT", "1")[:1] != "0":
        assert w["prob"].debug_back_product() == want
    o = options(api, max_num_iterations=6)
    ref = w["win"].solve(**okw(o))
    s = w["prob"].solve(o)
    check(api, w, s, ref, f"{name}: {n_kf} KF / {n_lm} landmarks, K = 6")
    close(w)


def test_three_solves_agree(ctx):
    """Run-to-run: the same solve three times in one process on the product path (kf50: G of five levels, the block in the padding)."""
    from lvio_fusion_amd import api, synthetic as syn
    n_kf, n_lm, seed, _, _, _ = WINDOWS["kf50"]
    cfg, st, hs, prob = window(api, syn, ctx, n_kf, n_lm, seed)
    if os.environ.get("LVF_BACK_PRODUCT", "1")[:1] != "0":
        assert prob.debug_back_product() == 1
    runs = []
    for _ in range(3):
        reset(api, st, cfg)
        s = prob.solve(fixed(api, 6))
        runs.append((s.final_cost, s.num_iterations, s.num_successful_steps, {k: np.array(v) for k, v in state(api, st).items()}))
    for c, it, ok, x in runs[1:]:
        assert (it, ok) == runs[0][1:3]
        assert abs(c - runs[0][0]) <= 1e-12 * abs(runs[0][0])
        for k in FIELDS:
            scale = np.abs(runs[0][3][k]).max() + 1e-300
            assert np.abs(x[k] - runs[0][3][k]).max() <= 1e-11 * scale, k
    prob.close()
    for h in hs + [st]:
        h.close()


if __name__ == "__main__":
    child()
