"""The merged last launch (csrc/solver_back.hip, k_chol_backsolve_tail): block step nb - 1 of the dense Cholesky and the back substitution +
step tail as ONE launch.  The inverse workgroup of the block step publishes the solution's last block x_last = L_kk^-T y_last (csrc/solver_dev.hpp,
chol_step_body<.., XLAST>), the back-substitution workgroup forms T_{nb-2,nb-1} itself, waits (bounded) for x_last and runs the links; the G
rows of the last level are formed by riders of the same launch and handed to the G workgroups through an arrival counter.

The switch LVF_CHOL_BACK_MERGE is read once per process, so both positions run in child processes (as tests/test_gpu_back_blocks.py does);
a child says on stderr which window it builds next, and the LVF_CHAIN_INFO lines that follow say whether the merged launch is in use.

1. Parity, on against off: one lm_iteration at radius 1e4 and a 6-iteration solve of windows on both sides of the form's conditions — 20, 24,
   32 and 50 keyframes (on), 16 keyframes (sequential levels: off) and the LVF_FORCE_LEVELS=2 corner of tests/test_gpu_back_blocks.py (the
   right-hand-side row alone in the last block — ONE real column —: off).  States to tests/test_gpu_handover.same_state (1e-9), costs to 1e-9,
   iteration and step counts equal; the `on` child also compares its iteration with the oracle's (test_sparse_level_placements' bounds).
2. The solve itself: the systems of tests/reduced_cases.py through the override tap (the chain is not rebuilt for it: the form is the one the child reports),
   bound of tests/test_gpu_back_blocks.py, err <= M max(err64_bound, d 2^-53), M = 8.  The last block's real columns (the right-hand-side row
   included: CholArgs::last_cols = dr + 1, dr the row of the right-hand side) sit on both sides of a 16-pivot stage, where the stage skipping
   and the position of row dr can go wrong: 16 and 17 (21 / 30 keyframes under LVF_FORCE_LEVELS=3: dr = 15, 16), 18 (26 keyframes under
   LVF_FORCE_LEVELS=1: dr = 17) and 63 (12 keyframes: dr = 62); one real column is the corner of 1., where the form is off.  (The plans —
   nb, kept blocks — are asserted: a plan change that moves these sizes must fail here, not pass on other shapes.)
3. Failed factor: a pivot of the LAST block made negative / zero / NaN (tests/reduced_cases.poisoned on the last pose unknown): the step is
   rejected with the same fail code as with the switch off, below the hand-over codes, and a solve reports hand_over_retries == 0.
4. Time-out path: debug_force_handover_timeout(2) at 20 keyframes with the merged launch on (asserted through the stage table: nb - 1
   block-step launches): retried, same counts, cost and state as the undisturbed solve, and the same again on the next solve.
5. Repeatability: 25 two-iteration solves from one start at 20 keyframes / 4 000 landmarks agree to 1e-12 relative
   (tests/test_gpu_back_product.py's run-to-run bound)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import reduced_cases as rc

M = 8.0
RADIUS = 1e4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")
CASES = ("own", "shift3", "shift6", "dd")
# name: (n_kf, n_lm, seed, imu_drop)
PARITY = {"kf20": (20, 700, 301, ()), "kf24": (24, 600, 303, ()), "kf32": (32, 800, 305, ()), "kf50": (50, 700, 307, ()), "kf16": (16, 600, 309, ())}
CORNER = {"corner": (26, 300, 113, (5, 12, 18))}
MERGED = {"kf20": 1, "kf24": 1, "kf32": 1, "kf50": 1, "kf16": 0, "corner": 0}
# LVF_FORCE_LEVELS of the child ("" = unset): {name: window}, and per name (nb, dense unknowns): dr = ndense - 64 (nb - 1)
SOLVE = {"": {"kf12": (12, 200, 401, ())}, "3": {"kf21": (21, 300, 405, ()), "kf30": (30, 300, 403, ())}, "1": {"kf26": (26, 300, 407, ())}}
PLAN = {"kf12": (2, 126), "kf21": (3, 144), "kf30": (4, 207), "kf26": (5, 273)}
DR = {"kf12": 62, "kf21": 16, "kf30": 15, "kf26": 17}
SWITCH = {"on": {}, "off": {"LVF_CHOL_BACK_MERGE": "0"}}


def run_child(mode, switch, force="", arg=None):
    env = dict(os.environ)
    for k in ("LVF_CHOL_BACK_MERGE", "LVF_BACK_BLOCKS", "LVF_CHOL_SUBBLOCK", "LVF_BACK_TAIL_MERGE", "LVF_BACK_TAIL_WGS", "LVF_BACK_PRODUCT", "LVF_BACK_EARLY", "LVF_FORCE_LEVELS"):
        env.pop(k, None)
    env.update(SWITCH[switch])
    if force:
        env["LVF_FORCE_LEVELS"] = force
    env["LVF_CHAIN_INFO"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode, force or "-"] + ([arg] if arg else []), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    # the chain lines behind a window's marker: the form of the LAST chain built for it
    name = None
    for ln in p.stderr.splitlines():
        m = re.match(r"WINDOW (\w+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"chol_back_merged (\d)", ln)
        if m and name in out:
            out[name]["merged"] = int(m.group(1))
    return out


def mark(name):
    sys.stderr.write(f"WINDOW {name}\n"); sys.stderr.flush()


def state_lists(api, st):
    from tests.test_gpu_solver import state_of
    s = state_of(api, st)
    return {k: np.asarray(s[k], np.float64).ravel().tolist() for k in FIELDS}


def fixed(api, n):
    o = api.default_solver_options()
    o.max_num_iterations = n; o.function_tolerance = 0.0; o.parameter_tolerance = 0.0; o.gradient_tolerance = 0.0
    return o


def close_all(prob, b, st):
    prob.close()
    for h in list(b.values()) + [st]:
        if h is not None:
            h.close()


# ---------------------------------------------------------------------------------------------------------------- 1. parity
def child_parity(force):
    from lvio_fusion_amd import api
    from oracle import pyoracle
    from tests.helpers import assert_parity
    from tests.test_gpu_handover import reset
    from tests.test_gpu_solver import build, state_of
    pyoracle.build()
    ctx = api.Context(0)
    out = {}
    for name, (n_kf, n_lm, seed, drop) in (CORNER if force != "-" else PARITY).items():
        mark(name)
        cfg, st, b, prob, win = build(api, ctx, pyoracle, n_kf, n_lm, seed, imu_drop=drop)
        opt = api.default_solver_options()
        got = prob.lm_iteration(opt, RADIUS, 2.0)
        r = {"it": {k: float(got[k]) for k in ("cost_before", "cost_after", "radius")}, "accepted": bool(got["accepted"]), "it_state": state_lists(api, st)}
        if os.environ.get("LVF_CHOL_BACK_MERGE") != "0":
            ref = win.lm_iteration(RADIUS, 2.0)
            assert abs(got["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"]), name
            assert got["accepted"] == ref["accepted"], name
            assert abs(got["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"]), name
            s = state_of(api, st)
            assert_parity(s["poses"].reshape(-1, 7), win.poses, f"{name}: poses")
            assert_parity(s["vel"].reshape(-1, 3), win.vel, f"{name}: vel")
            assert_parity(s["bg"].reshape(-1, 3), win.bg, f"{name}: bg")
        reset(api, st, cfg)
        s = prob.solve(fixed(api, 6))
        r["solve"] = {"cost": float(s.final_cost), "iterations": int(s.num_iterations), "steps": int(s.num_successful_steps), "retries": int(s.hand_over_retries)}
        r["solve_state"] = state_lists(api, st)
        out[name] = r
        close_all(prob, b, st)
    ctx.close()
    print(json.dumps(out))


_runs = {}


def cached(mode, switch, force="", arg=None):
    key = (mode, switch, force)
    if key not in _runs:
        _runs[key] = run_child(mode, switch, force, arg)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY) + list(CORNER))
def test_on_and_off_agree(name):
    from tests.test_gpu_handover import same_state
    force = "2" if name in CORNER else ""
    on, off = cached("parity", "on", force)[name], cached("parity", "off", force)[name]
    assert on["merged"] == MERGED[name] and off["merged"] == 0, (name, on["merged"], off["merged"])
    assert on["accepted"] == off["accepted"]
    for k in ("cost_before", "cost_after", "radius"):
        print(f"{name} {k}: on {on['it'][k]!r} off {off['it'][k]!r}")
        assert abs(on["it"][k] - off["it"][k]) <= 1e-9 * abs(off["it"][k]), (name, k)
    same_state({k: np.array(v) for k, v in on["it_state"].items()}, {k: np.array(v) for k, v in off["it_state"].items()})
    print(f"{name} solve: on {on['solve']} off {off['solve']}")
    assert on["solve"]["iterations"] == off["solve"]["iterations"] == 6 and on["solve"]["steps"] == off["solve"]["steps"]
    assert on["solve"]["retries"] == 0 and off["solve"]["retries"] == 0
    assert abs(on["solve"]["cost"] - off["solve"]["cost"]) <= 1e-9 * abs(off["solve"]["cost"])
    same_state({k: np.array(v) for k, v in on["solve_state"].items()}, {k: np.array(v) for k, v in off["solve_state"].items()})


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. the solve, failed factors
def child_solve(force, path):
    """The steps of the SOLVE windows of this child's LVF_FORCE_LEVELS for the systems in `path`, and the fail codes of a poisoned last block."""
    from lvio_fusion_amd import api
    from oracle import pyoracle
    from tests.test_gpu_reduced_solve import Win, reset
    pyoracle.build()
    ctx = api.Context(0)
    sys_ = np.load(path)
    out = {}
    for name, w in SOLVE["" if force == "-" else force].items():
        mark(name)
        win = Win(api, ctx, pyoracle, w)
        r = {"nb": win.nb, "ndense": 6 * w[0] + 9 * int(np.sum(win.dense_kf)), "back_product": win.back_product, "blocks": win.prob.debug_back_blocks(), "x": {}, "fail": {}}
        for case in CASES:
            S, b = sys_[f"{name}_{case}_S"], sys_[f"{name}_{case}_b"]
            got, x, fail, _ = win.iterate(S, b)
            assert fail == 0 and got["solved"] and np.isfinite(x).all(), f"{name} {case}: fail flag {fail}"
            r["x"][case] = np.asarray(x, np.float64).tolist()
        j = 6 * w[0] - 1                    # the last pose unknown: the last real pivot of the last block
        for kind in ("neg", "zero", "nan"):
            got, x, fail, state = win.iterate(rc.poisoned(win.S0, j, kind), win.b0)
            assert got["solved"] is False and got["accepted"] is False, f"{name} {kind}"
            assert all(np.array_equal(state[k], win.start[k]) for k in FIELDS), f"{name} {kind}: the state moved"
            r["fail"][kind] = int(fail)
        reset(api, win.st, win.cfg)
        win.prob.debug_override_reduced(rc.poisoned(win.S0, j, "neg"), win.b0)
        try:
            s = win.prob.solve(fixed(api, 2))
        finally:
            win.prob.debug_clear_override()
        r["poisoned_solve"] = {"retries": int(s.hand_over_retries), "iterations": int(s.num_iterations), "steps": int(s.num_successful_steps)}
        got, x, fail, _ = win.iterate()     # nothing stale is left behind
        assert fail == 0 and got["solved"] and np.abs(x - win.x0).max() <= 1e-9 * np.abs(win.x0).max(), name
        out[name] = r
        win.close()
    ctx.close()
    print(json.dumps(out))


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """{name: {case: (S, b, x_star, floor)}} and the file the children read the systems from; computed once, never modified (the reduced
    system is written in the natural unknown order: it does not depend on the plan the child forces)"""
    from lvio_fusion_amd import api
    from tests.test_gpu_reduced_solve import Win
    ctx = api.Context(0)
    out, arrays = {}, {}
    for group in SOLVE.values():
        for name, w in group.items():
            win = Win(api, ctx, oracle, w)
            cs = rc.cases(win.S0, win.b0, w[2], CASES)
            out[name] = {}
            for case in CASES:
                S, b = cs[case]
                x_star, x64 = rc.ref_solve(S, b)
                floor = max(float(rc.err64_bound(S, b, x_star, w[2], x64)), win.d * 2.0 ** -53)
                for a in (S, b, x_star):
                    a.setflags(write=False)
                out[name][case] = (S, b, x_star, floor)
                arrays[f"{name}_{case}_S"], arrays[f"{name}_{case}_b"] = S, b
            win.close()
    ctx.close()
    path = str(tmp_path_factory.mktemp("chol_back_merge") / "systems.npz")
    np.savez(path, **arrays)
    return out, path


def force_of(name):
    return next(f for f, g in SOLVE.items() if name in g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for g in SOLVE.values() for n in g])
def test_the_step_is_as_accurate_as_a_float64_cholesky(refs, name):
    on, off = cached("solve", "on", force_of(name), refs[1])[name], cached("solve", "off", force_of(name), refs[1])[name]
    assert (on["nb"], on["ndense"]) == PLAN[name] and on["ndense"] - 64 * (on["nb"] - 1) == DR[name], (name, on["nb"], on["ndense"])
    assert on["back_product"] == 1 and on["blocks"] == 1 and on["merged"] == 1 and off["merged"] == 0, (name, on["merged"], off["merged"])
    for case in CASES:
        S, b, x_star, floor = refs[0][name][case]
        for sw, r in (("on", on), ("off", off)):
            e_dev = rc.err(S, np.array(r["x"][case]), x_star)
            print(f"ratio {name} dr={DR[name]} d={len(b)} {case} {sw}: err_dev {e_dev:.3e} floor {floor:.3e} ratio {e_dev / floor:.3f}")
            assert e_dev <= M * floor, f"{name} {case} {sw}: err {e_dev:.3e} > {M} x {floor:.3e} (ratio {e_dev / floor:.2f})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for g in SOLVE.values() for n in g])
def test_a_failed_factor_of_the_last_block_is_an_invalid_step(refs, name):
    from lvio_fusion_amd import api
    k_sparse, k_handover = api.fail_codes()
    on, off = cached("solve", "on", force_of(name), refs[1])[name], cached("solve", "off", force_of(name), refs[1])[name]
    assert on["merged"] == 1 and off["merged"] == 0
    for kind in ("neg", "zero", "nan"):
        print(f"{name} {kind}: fail on {on['fail'][kind]} off {off['fail'][kind]}")
        assert on["fail"][kind] == off["fail"][kind] == on["nb"], f"{name} {kind}: fail flags {on['fail'][kind]} / {off['fail'][kind]}, last block step {on['nb']}"
        assert on["fail"][kind] < k_sparse < k_handover
    assert on["poisoned_solve"] == off["poisoned_solve"] and on["poisoned_solve"]["retries"] == 0 and on["poisoned_solve"]["steps"] == 0, on["poisoned_solve"]


# ---------------------------------------------------------------------------------------------------------------- 4. / 5. in this process (switch unset)
@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def merged_in_use(prob, opt, nb):
    """the stage table of the current chain: the merged launch takes block step nb - 1 out of the Cholesky stage"""
    la = [n_launch for name, _, n_launch in prob.stage_times(opt, RADIUS, reps=2) if "chol" in name and "backsolve" not in name]
    return la == [nb - 1]


@pytest.mark.gpu
def test_forced_timeout_with_the_merged_launch(ctx, oracle):
    from lvio_fusion_amd import api
    from tests.test_gpu_handover import reset, same_state
    from tests.test_gpu_solver import build, state_of
    cfg, st, b, prob, win = build(api, ctx, oracle, 20, 4000, 78, n_pre=0)
    opt = fixed(api, 5)
    nb, _ = prob.debug_plan()
    assert merged_in_use(prob, api.default_solver_options(), nb), "the merged last launch is not in use at 20 keyframes"
    reset(api, st, cfg)
    ref = prob.solve(opt)
    x_ref = state_of(api, st)
    assert ref.hand_over_retries == 0
    reset(api, st, cfg)
    prob.debug_force_handover_timeout(2)
    got = prob.solve(opt)
    assert got.hand_over_retries >= 1 and got.num_iterations == ref.num_iterations and got.num_successful_steps == ref.num_successful_steps
    assert abs(got.final_cost - ref.final_cost) <= 1e-9 * abs(ref.final_cost)
    same_state(x_ref, state_of(api, st))
    reset(api, st, cfg)
    again = prob.solve(opt)
    assert again.num_iterations == ref.num_iterations and again.num_successful_steps == ref.num_successful_steps
    assert abs(again.final_cost - ref.final_cost) <= 1e-9 * abs(ref.final_cost)
    same_state(x_ref, state_of(api, st))
    close_all(prob, b, st)


@pytest.mark.gpu
def test_the_merged_launch_gives_the_same_answer_every_time(ctx, oracle):
    from lvio_fusion_amd import api
    from tests.test_gpu_handover import reset
    from tests.test_gpu_solver import build
    cfg, st, b, prob, win = build(api, ctx, oracle, 20, 4000, 79, n_pre=0)
    opt = fixed(api, 2)
    costs = []
    for _ in range(25):
        reset(api, st, cfg)
        s = prob.solve(opt)
        assert s.hand_over_retries == 0 and s.num_iterations == 2
        costs.append(s.final_cost)
    spread = (max(costs) - min(costs)) / abs(costs[0])
    print(f"relative spread of the final cost over 25 solves: {spread:.3e}")
    assert spread <= 1e-12, costs
    close_all(prob, b, st)


if __name__ == "__main__":
    if sys.argv[1] == "parity":
        child_parity(sys.argv[2])
    else:
        child_solve(sys.argv[2], sys.argv[3])
