"""(CPU) tests/robust_cases.py: the thresholds it picks really put both Huber branches into every linearisation the GPU tests run
(conditions on the inputs, asserted with the oracle alone), and the oracle's own mixed-branch LM iteration is pinned to the dense numpy
restatement of tests/test_oracle_lm_numpy.py at those thresholds."""
import numpy as np
import pytest

from tests import robust_cases as rc
from tests.test_oracle_lm_numpy import cost_only, dense_system, quat_plus

MIN_KIND = 20          # a kind with fewer blocks than this is left out of the per-kind condition (its share moves in steps of > 5 %)


def fmt(sh):
    return " ".join(f"{k} {v:.3f}" for k, v in sh.items())


@pytest.mark.parametrize("name", list(rc.WINDOWS))
def test_ladder_census(oracle, name):
    """every step of every ladder: each visual kind with at least 20 blocks has at least 5 % of them in each branch, 30 - 70 % of all blocks
    are linear, and no norm lies within 1e-4 (relative) of the threshold"""
    lad = rc.ladder(oracle, name)
    assert len(lad) == rc.LADDER_STEPS
    for k, s in enumerate(lad):
        print(f"{name} step {k}: a_k = {s['a']:.4f}, margin {s['margin']:.2e}, linear share {fmt(s['shares'])}, blocks {s['counts']}")
        assert s["margin"] >= 1e-4
        assert 0.3 <= s["shares"]["all"] <= 0.7
        for kind, n in s["counts"].items():
            if n >= MIN_KIND:
                assert 0.05 <= s["shares"][kind] <= 0.95, (name, k, kind)
    assert any(n >= MIN_KIND for n in lad[0]["counts"].values())
    # the same window under the default threshold is all linear, under 1e9 all quadratic: what the rest of the suite sees, and (c)'s case
    cfg, use = rc.window(name)
    n0 = rc.norms(oracle, cfg, lad[0]["state"], use)
    assert rc.shares(n0, 1.0)["all"] == 1.0 and rc.shares(n0, 1e9)["all"] == 0.0 and rc.shares(n0, 0.0)["all"] == 0.0


def test_pick_a_and_shares():
    n = {"tc": np.array([1.0, 2.0, 3.5, 4.0]), "po": np.array([2.5, 10.0, 2.75, 0.5])}     # sorted: .5 1 [2 2.5 2.75 3.5] 4 10, band 0.4 - 0.6 = entries 2 .. 5
    a, m = rc.pick_a(n)
    assert a == 3.125 and m == pytest.approx(0.375 / 3.125)                            # the widest gap in the band is 2.75 .. 3.5 (1 .. 2 and 4 .. 10 lie outside it)
    assert rc.shares(n, a) == {"tc": 0.5, "po": 0.25, "all": 0.375}
    assert rc.shares(n, 0.0)["all"] == 0.0


@pytest.mark.parametrize("spec", rc.SOLVES, ids=lambda s: f"kf{s[0]}")
def test_fixed_threshold_census(oracle, spec):
    """a_fix: the solve starts (nearly) all linear and ends with at least 10 % of every kind in each branch"""
    f = rc.a_fix(oracle, spec)
    r = f["ref"]
    print(f"{spec}: a_fix = {f['a']:.3f}; linear share at the start {fmt(f['start'])}; at the end {fmt(f['end'])}; "
          f"{r['num_iterations']} iterations, {r['num_successful_steps']} successful, {r['why']}")
    assert f["start"]["all"] >= 0.9
    for kind in rc.KINDS:
        assert 0.1 <= f["end"][kind] <= 0.9, kind
    assert r["num_successful_steps"] >= 3 and r["termination"] == 0


def test_batch_threshold_census(oracle):
    """one huber_a for both windows of a batch: under SOLVES[0]'s thresholds SOLVES[1] is mixed too"""
    a_solve, a_step = rc.batch_thresholds(oracle)
    for spec in rc.SOLVES:
        c = rc.solve_census(oracle, spec, a_solve)
        cfg = rc.solve_window(spec)
        n0 = rc.norms(oracle, cfg, rc.state_of(cfg))
        s0 = rc.shares(n0, a_step)
        print(f"{spec}: a_solve = {a_solve:.3f}: linear share at the end {fmt(c['end'])}; a_step = {a_step:.3f}: at the start {fmt(s0)}")
        assert c["start"]["all"] >= 0.9 and all(0.1 <= c["end"][k] <= 0.9 for k in rc.KINDS)
        assert 0.3 <= s0["all"] <= 0.7 and all(0.05 <= s0[k] <= 0.95 for k in rc.KINDS)
        assert np.abs(np.concatenate(list(n0.values())) / a_step - 1).min() >= 1e-4
        assert rc.shares(n0, 1.0)["all"] == 1.0                  # the table rebuilt for huber_a = 1 is the all-linear one


@pytest.mark.parametrize("name", ["kf8", "kf2"])
def test_oracle_mixed_branch_iteration_matches_dense_numpy(oracle, name):
    """test_oracle_lm_numpy.test_lm_iteration_matches_dense_numpy_solve's check (its tolerances) along the ladder: dense_system(huber_a = a_k)
    against oracle.Window.lm_iteration(huber_a = a_k).  Each call is a one-iteration solve (Jacobi scaling from its own linearisation)."""
    cfg, use = rc.window(name)
    assert use == rc.ALL
    n_kf, n_lm = cfg["n_kf"], cfg["n_lm"]
    pre = rc.preint(oracle, cfg)
    win = oracle.Window(cfg, pre)
    state = rc.state_of(cfg)
    for it, step in enumerate(rc.ladder(oracle, name)):
        a, radius, dec = step["a"], step["radius"], step["dec"]
        for x, y in zip(state, step["state"]):
            assert np.abs(x - y).max() <= 1e-8 * max(1.0, np.abs(y).max())
        sh = rc.shares(rc.norms(oracle, cfg, state), a)
        assert sh == step["shares"] and 0.0 < sh["all"] < 1.0
        J, r, cost = dense_system(oracle, cfg, pre, state, huber_a=a)
        jac_scale = 1.0 / (1.0 + np.sqrt((J * J).sum(axis=0)))
        Js = J * jac_scale
        H, g = J.T @ J, J.T @ r
        Hs, gs = Js.T @ Js, Js.T @ r
        diag = np.minimum(np.maximum(np.diag(Hs), 1e-6), 1e32)
        y = np.linalg.solve(Hs + np.diag(diag / radius), -gs)
        dx = jac_scale * y
        model = -(Js @ y) @ (r + 0.5 * (Js @ y))
        D = diag / jac_scale ** 2 / radius
        new = [s.copy() for s in state]
        for k in range(n_kf):
            new[0][k, :4] = quat_plus(state[0][k, :4], dx[6 * k:6 * k + 3]); new[0][k, 4:] += dx[6 * k + 3:6 * k + 6]
            o = 6 * n_kf + 9 * k
            new[1][k] += dx[o:o + 3]; new[2][k] += dx[o + 3:o + 6]; new[3][k] += dx[o + 6:o + 9]
        new[4] = state[4] + dx[15 * n_kf:]
        cand = cost_only(oracle, cfg, pre, new, huber_a=a)
        rho = (cost - cand) / model
        ref = win.lm_iteration(radius, dec, huber_a=a)
        assert abs(ref["cost_before"] - cost) <= 1e-10 * cost
        assert abs(ref["model_cost_change"] - model) <= 1e-7 * abs(model)
        assert abs(ref["cost_after"] - cand) <= 1e-7 * cand
        assert abs(ref["rho"] - rho) <= 1e-6 * max(1.0, abs(rho))
        assert ref["accepted"] == (rho > 1e-3)
        d = 15 * n_kf
        A = H + np.diag(D)
        S = A[:d, :d] - A[:d, d:] @ np.diag(1.0 / np.diag(A[d:, d:])) @ A[d:, :d]
        assert np.abs(ref["S"] - S).max() <= 1e-9 * np.abs(S).max()
        rhs = -g[:d] + A[:d, d:] @ (g[d:] / np.diag(A[d:, d:]))
        assert np.abs(ref["rhs"] - rhs).max() <= 1e-9 * np.abs(rhs).max()
        if rho > 1e-3:
            t = 2 * rho - 1
            radius = min(radius / max(1 / 3, 1 - t ** 3), 1e16); dec = 2.0
            state = new
        else:
            radius /= dec; dec *= 2
        assert abs(ref["radius"] - radius) <= 1e-6 * radius and ref["decrease_factor"] == dec
        for x, y in zip(state, (win.poses, win.vel, win.ba, win.bg, win.inv_depth)):
            assert np.abs(x - y).max() <= 1e-8 * max(1.0, np.abs(y).max())
        # the default threshold is a different problem: the check above can tell a wrong branch
        assert abs(win.cost(1.0) - win.cost(a)) > 1e-3 * win.cost(a)
    assert it == rc.LADDER_STEPS - 1


def test_lidar_census(oracle):
    """The surf sub-problem of test_gpu_icp and the planes + lines scene of test_gpu_edge: under today's huber_a = 0.1 no residual is in the
    linear branch (|r| <= weight * gate = 0.01); under the median |r| half of them are."""
    i = rc.icp_surf(oracle)
    e = rc.edge_scene()
    lin = lambda r, a: float((r > a).mean())
    print(f"config3_icp surf: {len(i['r'])} planes, max |r| = {i['r'].max():.3e}, linear share at 0.1: {lin(i['r'], 0.1):.3f}; a_icp = {i['a']:.4e}, share {lin(i['r'], i['a']):.3f}")
    print(f"edge scene planes: {len(e['r_plane'])}, max |r| = {e['r_plane'].max():.3e}, linear share at 0.1: {lin(e['r_plane'], 0.1):.3f}; at a_icp: {lin(e['r_plane'], i['a']):.3f}")
    print(f"edge scene lines: {len(e['r_edge'])}, max |r| = {e['r_edge'].max():.3e}, linear share at 0.1: {lin(e['r_edge'], 0.1):.3f}; a_edge = {e['a_edge']:.4e}, "
          f"share {lin(e['r_edge'], e['a_edge']):.3f}")
    assert len(i["r"]) > 500 and len(e["r_plane"]) == 300 and len(e["r_edge"]) == 257
    for r in (i["r"], e["r_plane"], e["r_edge"]):
        assert r.max() <= 0.01 < 0.1 and lin(r, 0.1) == 0.0          # the claim: today's threshold never reaches the linear branch
        assert lin(r, 1e-6) >= 0.99                                  # ... and 1e-6 puts (nearly) everything into it
    assert 0.3 <= lin(i["r"], i["a"]) <= 0.7
    assert 0.3 <= lin(e["r_edge"], e["a_edge"]) <= 0.7
    assert 0.05 <= lin(e["r_plane"], i["a"]) <= 0.95                 # the planes of the edge scene under a_icp (what icp_solve_edges is run with)


@pytest.mark.parametrize("which", ["a_icp", "all_linear"])
def test_oracle_icp_solve_in_the_linear_branch_matches_numpy(oracle, which):
    """oracle.icp_solve is pinned by test_oracle_lm_numpy.test_icp_solve_matches_numpy_lm at huber_a = 0 and 0.1 only, i.e. never in the linear
    branch: the same check (its tolerances) at a_icp and at 1e-6 against tests/edge_ref.py's numpy loop on the oracle's correspondences"""
    from tests import edge_ref as er
    i = rc.icp_surf(oracle)
    c, huber = i["c"], (i["a"] if which == "a_icp" else 1e-6)
    x_ref, summ = oracle.icp_solve(i["mm"], i["qq"], c["map_pose"], c["pose0"], i["rpyxyz0"], 1, i["thr"], i["w"], huber)
    x, s = er.lm_solve(1, c["map_pose"], i["rpyxyz0"], dict(p=i["p"], a=i["pa"], n=i["n"], weight=i["w"], huber=huber))
    print(f"{which}: huber_a = {huber:.4e}, {summ['num_iterations']} iterations, cost {summ['initial_cost']:.6e} -> {summ['final_cost']:.6e}, |dx| {np.abs(x - x_ref).max():.2e}")
    assert summ["num_residual_blocks"] == s["num_residual_blocks"] == len(i["r"])
    assert (summ["num_iterations"], summ["num_successful_steps"]) == (s["num_iterations"], s["num_successful_steps"]) and s["num_successful_steps"] >= 1
    assert abs(summ["initial_cost"] - s["initial_cost"]) <= 1e-9 * s["initial_cost"]
    assert np.abs(x_ref - x).max() <= 1e-9
    assert abs(summ["final_cost"] - s["final_cost"]) <= 1e-8 * s["initial_cost"]
