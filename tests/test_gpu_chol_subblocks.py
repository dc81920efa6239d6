"""The dense Cholesky's 16-pivot sub-block sweep (csrc/solver_chol.hip, sub_pivots / chol_step_body<true>) at the corner sizes where
it can go wrong.  The corner has d = 6 n_kf unknowns plus the right-hand-side row, in blocks of 64 that are swept in stages of 16:

    n_kf   d + 1   exercises
      2      13    one block; the sweep ends inside the first stage
      3      19    one block; ends two pivots into stage 1, right after the first stage boundary
     10      61    one block; ends inside the last stage
     11      67    two blocks; the last block has 3 real columns; the panel and inverse workgroups run
     32     193    four blocks; the last block holds ONLY the right-hand-side row
     22     133    three blocks; trailing-tile workgroups beside the column workgroups

There is no stand-alone entry for the factor: it is driven as tests/test_gpu_solver.py::test_lm_iteration_parity drives it
(Problem.lm_iteration against the oracle's iteration, same helpers, same tolerances).  Also: a batch of two such windows against their
single solves (bench.py's batched_windows_vs_single tolerance) and the switch LVF_CHOL_SUBBLOCK at 0 and 1 in two child processes
(test_chained_levels_give_the_same_answer_every_time's relative spread)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

CASES = [(2, 60, 101), (3, 80, 103), (10, 200, 105), (11, 200, 107), (32, 300, 109), (22, 300, 111)]      # n_kf, n_lm, seed
N_IT = 4
_refs = {}


def reference(oracle, case):
    """The oracle's N_IT iterations of a case from its start state (computed once, shared, never modified): per iteration the oracle's
    result and the state it leaves."""
    if case not in _refs:
        from lvio_fusion_amd import synthetic as syn
        n_kf, n_lm, seed = case
        cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=40, seed=seed, imu_samples=5)
        pre = np.stack([oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
        win = oracle.Window(cfg, pre, use=("tc", "tf", "po", "imu"))
        its, radius, dec = [], 1e4, 2.0
        for _ in range(N_IT):
            ref = win.lm_iteration(radius, dec)
            its.append((ref, {k: np.array(getattr(win, k)) for k in ("poses", "inv_depth", "vel", "ba", "bg")}))
            radius, dec = ref["radius"], ref["decrease_factor"]
        _refs[case] = its
    return _refs[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"kf{c[0]}")
def test_the_oracle_accepts_the_first_step(oracle, case):
    """(CPU) cost_after is only a real comparison where the step is taken."""
    ref, _ = reference(oracle, case)[0]
    assert ref["accepted"] and ref["cost_after"] < ref["cost_before"]


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def close_all(prob, b, st):
    prob.close()
    for h in list(b.values()) + [st]:
        if h is not None:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"kf{c[0]}")
def test_lm_iteration_parity_at_the_stage_and_block_edges(ctx, oracle, case):
    from lvio_fusion_amd import api
    from tests.helpers import assert_parity
    from tests.test_gpu_solver import build, state_of
    n_kf, n_lm, seed = case
    cfg, st, b, prob, _ = build(api, ctx, oracle, n_kf, n_lm, seed)
    opt = api.default_solver_options()
    radius, dec = 1e4, 2.0
    for it, (ref, x) in enumerate(reference(oracle, case)):
        got = prob.lm_iteration(opt, radius, dec)
        assert abs(got["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"])
        S, rhs = prob.reduced_system()
        assert np.abs(S - ref["S"]).max() <= 1e-7 * np.abs(ref["S"]).max(), f"iteration {it}: reduced system mismatch"
        assert_parity(rhs, ref["rhs"], f"rhs it{it}")
        assert got["accepted"] == ref["accepted"]
        assert abs(got["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"])
        assert abs(got["radius"] - ref["radius"]) <= 1e-5 * ref["radius"]
        s = state_of(api, st)
        assert_parity(s["poses"].reshape(-1, 7), x["poses"], f"poses it{it}")
        assert_parity(s["inv_depth"], x["inv_depth"], f"inv_depth it{it}")
        assert_parity(s["vel"].reshape(-1, 3), x["vel"], f"vel it{it}")
        assert_parity(s["ba"].reshape(-1, 3), x["ba"], f"ba it{it}")
        assert_parity(s["bg"].reshape(-1, 3), x["bg"], f"bg it{it}")
        radius, dec = ref["radius"], ref["decrease_factor"]
    close_all(prob, b, st)


def fixed(api, n):
    o = api.default_solver_options()
    o.max_num_iterations = n; o.function_tolerance = 0.0; o.parameter_tolerance = 0.0; o.gradient_tolerance = 0.0
    return o


def reset(api, st, cfg):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        st.set(field, cfg[key])


@pytest.mark.gpu
def test_a_batch_of_two_corner_sizes_lands_where_the_single_solves_land(ctx, oracle):
    """Two and four blocks in one launch chain (the batched entry points share chol_step_body): each window against its own single solve."""
    from lvio_fusion_amd import api
    from tests.test_gpu_solver import build
    wins = [build(api, ctx, oracle, *c) for c in (CASES[3], CASES[4])]
    opt = fixed(api, 5)
    singles = []
    for cfg, st, b, prob, _ in wins:
        singles.append(prob.solve(opt))
        reset(api, st, cfg)
    batch = api.ProblemBatch(ctx, [w[3] for w in wins])
    ss = batch.solve(opt)
    for s1, s in zip(singles, ss):
        assert np.isfinite(s.final_cost)
        assert abs(s1.final_cost - s.final_cost) <= 1e-9 * abs(s1.final_cost) and s1.num_iterations == s.num_iterations
    batch.close()
    for cfg, st, b, prob, _ in wins:
        close_all(prob, b, st)


def child_solve():
    """One solve of the n_kf = 11 window in this process; prints its summary as one JSON line."""
    from lvio_fusion_amd import api
    from oracle import pyoracle
    from tests.test_gpu_solver import build
    pyoracle.build()
    ctx = api.Context(0)
    cfg, st, b, prob, _ = build(api, ctx, pyoracle, *CASES[3])
    s = prob.solve(fixed(api, 6))
    print(json.dumps({"final_cost": s.final_cost, "num_iterations": s.num_iterations, "num_successful_steps": s.num_successful_steps}))
    close_all(prob, b, st)
    ctx.close()


@pytest.mark.gpu
def test_both_sweeps_give_the_same_solve():
    """The pair-pivot sweep (LVF_CHOL_SUBBLOCK=0) and the sub-block sweep differ in summation order only.  The switch is read once per
    process, hence two fresh child processes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for v in ("0", "1"):
        env = dict(os.environ); env["LVF_CHOL_SUBBLOCK"] = v
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    old, new = out
    assert np.isfinite(new["final_cost"]) and new["num_successful_steps"] >= 1
    assert (old["num_iterations"], old["num_successful_steps"]) == (new["num_iterations"], new["num_successful_steps"])
    assert abs(old["final_cost"] - new["final_cost"]) <= 1e-9 * abs(old["final_cost"])


if __name__ == "__main__":
    child_solve()
