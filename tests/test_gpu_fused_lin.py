"""The fused LM chain (LVF_FUSED_LIN, default on: the candidate pass also linearises at x + dx, into the accumulator set that is not
active) against today's chain (LVF_FUSED_LIN=0), each in a child process of its own (the switch is read once per process).

Cases: configs[3] with K = 20 (bench.py's call), far starts whose steps are rejected (two in a row among them: an iteration that starts
from an already-reduced set), a 10-keyframe window, a window with constant pose / (v, ba, bg) blocks, solves that a candidate pass ends
early followed by further solves of the same problem, and a batch of 8 windows that were solved one by one first.  The counts and the
termination must be identical; the per-iteration costs (LVF_LM_HISTORY), the final costs and the states equal to 1e-12 relative — or no
further apart than two runs of today's chain are (its fp64 atomics add in no fixed order).  After a solve, gradient() and reduced_system()
must be those of a fresh linearisation at the returned state, and the next solve must start from the cost the last one ended with.  The
stage table of each run shows which chain ran."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")


def _cases(api, oracle, ctx):
    from lvio_fusion_amd import synthetic as syn
    from tests.test_gpu_solve_trajectory import make, close, options
    out = {}

    def history(name, w, s):
        # the decisions of the solve's passes: (cost_before, cost_new, accepted) per counted iteration
        h = np.zeros(512)
        L = ctx.L
        L.lvf_problem_debug_history.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.lvf_problem_debug_history.restype = C.c_int
        assert L.lvf_problem_debug_history(w["prob"].h, h.ctypes.data_as(C.POINTER(C.c_double))) == 0
        rows = h.reshape(64, 8)[:max(s.num_iterations, 0)]
        out[name + "/hist_costs"] = rows[:, 1:3].copy()
        out[name + "/hist_accepted"] = rows[:, 4].copy()

    def record(name, w, s, hist=True):
        if hist:
            history(name, w, s)
        out[name + "/counts"] = np.array([s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.termination], np.float64)
        out[name + "/why"] = np.array([str(s.why)])
        out[name + "/cost"] = np.array([s.initial_cost, s.final_cost])
        for f in FIELDS:
            out[name + "/" + f] = np.asarray(w["st"].get(getattr(api, {"poses": "POSES", "vel": "VEL", "ba": "BA", "bg": "BG", "inv_depth": "INV_DEPTH"}[f])), np.float64).ravel()

    w = make(api, ctx, oracle, 0, 0, syn.SEED_CFG4, cfg=syn.config4_window())
    record("cfg3", w, w["prob"].solve(options(api, max_num_iterations=20)))
    # the taps after a solve: a fresh linearisation at the returned state
    gc, gl = w["prob"].gradient(options(api))
    out["cfg3/gc"] = gc; out["cfg3/gl"] = gl
    # which chain the device loop runs on this problem: launches of k_lin_visual and of the candidate pass per timed iteration
    st = {n.split(" ")[0]: la for n, _, la in w["prob"].stage_times(options(api), reps=3)}
    out["cfg3/chain"] = np.array([st.get("k_lin_visual", 0), st.get("k_lin_cost_decide", 0)], np.float64)
    close(w)
    for i, (perturb, radius, seed) in enumerate([(20.0, 1e16, 5), (20.0, 1e4, 5), (30.0, 1e10, 9)]):
        w = make(api, ctx, oracle, 8, 300, seed, n_pre=60, perturb=perturb)
        record(f"reject{i}", w, w["prob"].solve(options(api, max_num_iterations=25, initial_trust_region_radius=radius)))
        close(w)
    w = make(api, ctx, oracle, 10, 300, 41, n_pre=60)
    record("kf10", w, w["prob"].solve(options(api, max_num_iterations=15)))
    w["prob"].lm_iteration(options(api), 1e4, 2.0)          # the per-iteration API after a fused solve: today's chain, set 0
    S, rhs = w["prob"].reduced_system()
    out["kf10/S"] = S; out["kf10/rhs"] = rhs
    close(w)
    pc = np.zeros(10, bool); pc[[0, 1]] = True
    w = make(api, ctx, oracle, 10, 300, 43, n_pre=60, pose_const=pc)
    for k in (0, 1):
        w["prob"].set_vbb_constant(k, True, True, True)
    record("const", w, w["prob"].solve(options(api, max_num_iterations=15)))
    close(w)
    # solves that a candidate pass ends (gradient / function tolerance at the first pass, the plain last iteration already enqueued), then
    # more solves of the same problem: each must start from the cost the previous one ended with
    w = make(api, ctx, oracle, 10, 300, 47, n_pre=60)
    chain = [options(api, max_num_iterations=30), options(api, max_num_iterations=2, gradient_tolerance=1e30),
             options(api, max_num_iterations=3, function_tolerance=1e30), options(api, max_num_iterations=2), options(api, max_num_iterations=4)]
    for k, o in enumerate(chain):
        record(f"resolve{k}", w, w["prob"].solve(o))
    close(w)
    # a batch of windows that were solved one by one first (the batched chain reads set 0: the single-window solves must leave it clean)
    ws = [make(api, ctx, oracle, 10, 300, 900 + i, n_pre=60, perturb=(1.0 if i % 4 else 12.0)) for i in range(8)]
    for i, w in enumerate(ws):
        record(f"single{i}", w, w["prob"].solve(options(api, max_num_iterations=3)))
    batch = api.ProblemBatch(ctx, [w["prob"] for w in ws])
    for i, (w, s) in enumerate(zip(ws, batch.solve(options(api, max_num_iterations=10)))):
        record(f"batch{i}", w, s, hist=False)
    batch.close(); close(*ws)
    return out


def _child(path):
    from lvio_fusion_amd import api
    from oracle import pyoracle
    pyoracle.build()
    ctx = api.Context(0)
    out = _cases(api, pyoracle, ctx)
    ctx.close()
    np.savez(path, **out)


def _run(tmp_path, tag, fused):
    env = dict(os.environ)
    env["LVF_FUSED_LIN"] = "1" if fused else "0"
    env["LVF_LM_HISTORY"] = "1"
    path = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_fused_lin", path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"{tag}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    return dict(np.load(path))


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


@pytest.mark.gpu
def test_fused_chain_equals_todays_chain(tmp_path):
    base = _run(tmp_path, "plain_a", False)
    again = _run(tmp_path, "plain_b", False)
    fused = _run(tmp_path, "fused", True)
    assert set(base) == set(fused)
    # the chain that ran: today's launches k_lin_visual every iteration, the fused one the candidate pass instead
    assert list(base["cfg3/chain"]) == [1, 0] and list(fused["cfg3/chain"]) == [0, 1], (base["cfg3/chain"], fused["cfg3/chain"])
    for run in (base, fused):
        # a solve ended by a candidate pass before the last iteration, and the solves after it start where it ended
        assert run["resolve1/why"][0] == "gradient_tolerance" and run["resolve2/why"][0] == "function_tolerance"
        assert run["resolve1/counts"][0] == 0 and run["resolve2/counts"][0] == 0
        for k in range(1, 5):
            prev_final, this_initial = run[f"resolve{k - 1}/cost"][1], run[f"resolve{k}/cost"][0]
            assert abs(this_initial - prev_final) <= 1e-12 * abs(prev_final), (k, this_initial, prev_final)
    report = {}
    for key in sorted(base):
        if key.endswith("/chain"):
            continue
        if key.endswith(("/counts", "/why", "/hist_accepted")):
            assert np.array_equal(base[key], fused[key]), (key, base[key], fused[key])
            continue
        d_fused, d_plain = _rel(fused[key], base[key]), _rel(again[key], base[key])
        report[key] = (d_fused, d_plain)
        # (the taps' gradient / right-hand side near the optimum is a difference of large terms: its relative noise between two runs of
        # today's chain is already ~1e-10, so it gets the 1e-8 floor)
        floor = 1e-8 if key.endswith(("/rhs", "/gc", "/gl")) else 1e-12
        assert d_fused <= max(floor, 4.0 * d_plain), (key, d_fused, d_plain)
    # the cases really exercise rejected steps, two in a row among them (an iteration that starts from an already-reduced set)
    def two_in_a_row(acc):
        return any(acc[i] == 0 and acc[i + 1] == 0 for i in range(len(acc) - 1))
    assert any(two_in_a_row(base[f"reject{i}/hist_accepted"]) for i in range(3))
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    _child(sys.argv[1])
