"""The dense keyframe prior on the device (lvf_dense_prior_*, lvf_problem_set_dense_prior) and the marginalisation that produces one
(lvf_problem_marginal_prior) against the declared semantics of tests/dense_prior_ref.py.

Bounds.  The factor takes helpers.assert_parity (1e-6 relative, the bound of every factor here) and 1e-12 on the cost.  The with / without
comparison of the reduced system and the iterations and solves take what tests/test_gpu_lidar_window.py applies to the same comparisons:
S 1e-7 of its largest entry, rhs / states assert_parity, cost 1e-8 inside an iteration and 1e-6 at the candidate, radius 1e-5, equal
decisions.  lvf_problem_marginal_prior takes tests/test_gpu_marginal_window.py's construction on the matrix with the extra row: the
reference is the long-double elimination of the device's own reduced system, and the tolerance what the distance of two device assemblies
(block-count roundings plus one rounding of the diagonal) can do to it, plus M float64 floors (dense_prior_ref.propagated / err64_bound)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import dense_prior_ref as dp
from tests import lidar_window_cases as lc
from tests import lidar_window_ref as lw
from tests.helpers import assert_parity
from tests.test_gpu_lidar_window import Device, assert_state
from tests.test_gpu_marginal import M

pytestmark = pytest.mark.gpu
RADIUS_TRUTH = 1e16


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def kf_state(state, kfs):
    return np.array([np.concatenate([state[0][k], state[1][k], state[2][k], state[3][k]]) for k in kfs])


def make_prior(rng, x_at, n_sel, weight=30.0, rank=None, spread=0.02):
    """a prior near the states x_at [n_sel][16]: info = A^T A (rank rows; default m + 5: full rank), eta = A^T b, c0 = 1/2 |b|^2 + 0.1, x0 a
    few centimetres / hundredths of a radian off"""
    m = 15 * n_sel
    A = weight * rng.normal(size=(m + 5 if rank is None else rank, m))
    b = rng.normal(size=A.shape[0])
    x0 = dp.state_plus(x_at, spread * rng.normal(size=m))
    return dict(x0=x0, info=A.T @ A, eta=A.T @ b, c0=0.5 * float(b @ b) + 0.1)


# ------------------------------------------------------------------------------------------------ the factor
@pytest.mark.parametrize("n_sel", [1, 2, 8])
def test_factor_against_the_reference(ctx, n_sel):
    """lvf_dense_prior_evaluate on a 9-keyframe state: the prior's keyframes unordered; per case one keyframe 0.5 rad from x0 and, with more
    than one, one a hair short of pi/2 (d.w close to 0) and one at 2.2 rad (d.w < 0); un-normalised quaternions; a zero row / column of info
    (an absent unknown); at n_sel = 2 a rank-deficient info (7 rows for 30 unknowns); then one constant pose and one constant ba."""
    from lvio_fusion_amd import api
    rng = np.random.default_rng(40 + n_sel)
    n_kf = 9
    kfs = {1: [3], 2: [5, 1], 8: [8, 0, 2, 4, 6, 1, 3, 7]}[n_sel]
    poses = syn.drive_poses(n_kf, rng)
    poses[:, :4] *= rng.uniform(0.8, 1.3, (n_kf, 1))
    state = [poses, rng.normal(size=(n_kf, 3)), 0.1 * rng.normal(size=(n_kf, 3)), 0.01 * rng.normal(size=(n_kf, 3))]
    x = kf_state(state, kfs)
    angles = [0.5, np.pi / 2 - 1e-4, 2.2] + [1e-9, 0.0, 0.03, 0.2, 1.0]
    eps = 0.3 * rng.normal(size=15 * n_sel)
    for j in range(n_sel):
        d = rng.normal(size=3)
        eps[15 * j:15 * j + 3] = angles[j] * d / np.linalg.norm(d)
    x0 = dp.state_plus(x, -eps)
    x0[:, :4] *= rng.uniform(0.7, 1.2, (n_sel, 1))
    pr = make_prior(rng, x0, n_sel, rank=7 if n_sel == 2 else None, spread=0.0)
    pr["x0"] = x0
    pr["info"][4, :] = 0.0; pr["info"][:, 4] = 0.0; pr["eta"][4] = 0.0
    if n_sel == 2:
        assert np.linalg.matrix_rank(pr["info"]) <= 7
    e = dp.local(x, x0)
    assert abs(np.linalg.norm(e[:3]) - 0.5) <= 1e-9
    st = api.State(ctx, n_kf, 0)
    for f, v in ((api.POSES, state[0]), (api.VEL, state[1]), (api.BA, state[2]), (api.BG, state[3])):
        st.set(f, v)
    upper_junk = pr["info"] + np.triu(rng.normal(size=pr["info"].shape), 1)      # only the lower triangle is read
    prior = api.DensePrior(ctx, kfs, pr["x0"], upper_junk, pr["eta"], pr["c0"])
    try:
        for bits in (None, "const"):
            cb = None
            if bits:
                cb = np.zeros(n_kf, np.uint8)
                cb[kfs[0]] = 1                      # the pose of the first slot
                cb[kfs[-1]] |= 4                    # ba of the last slot (the same keyframe when n_sel = 1)
            c_ref, g_ref, H_ref = dp.evaluate(pr["x0"], pr["info"], pr["eta"], pr["c0"], x, None if cb is None else [cb[k] for k in kfs])
            c, g, H = prior.evaluate(st, cb)
            print(f"n_sel {n_sel} {bits}: cost dev {c:.15e} ref {c_ref:.15e}; max|H| {np.abs(H_ref).max():.3e} err {np.abs(H - H_ref).max():.3e}; max|g| {np.abs(g_ref).max():.3e} err {np.abs(g - g_ref).max():.3e}")
            assert abs(c - c_ref) <= 1e-12 * abs(c_ref)
            assert_parity(g, g_ref, "gradient"); assert_parity(H, H_ref, "matrix")
            assert np.array_equal(H, H.T) and not H[4].any() and g[4] == 0.0
            if cb is not None:
                assert not H[:6].any() and not g[:6].any() and not H[15 * (n_sel - 1) + 9:15 * (n_sel - 1) + 12].any()
        d = prior.download()
        assert np.array_equal(d["kfs"], kfs) and np.array_equal(d["x0"], pr["x0"]) and np.array_equal(d["eta"], pr["eta"]) and d["c0"] == pr["c0"]
    finally:
        prior.close(); st.close()


# ------------------------------------------------------------------------------------------------ the reduced system
def _window(oracle, n_kf, n_lm, seed=303):
    cfg = syn.config4_window(n_kf=n_kf, n_lm=max(n_lm, 8), n_prewindow=max(n_lm // 2, 4), seed=seed + n_kf, imu_samples=3)
    if n_lm == 0:
        cfg = lc.imu_only(cfg)
    return cfg, lc.preint(oracle, cfg)


def _reset(api, dev, cfg):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        if np.asarray(cfg[key]).size:
            dev.st.set(field, cfg[key])


@pytest.mark.parametrize("sel", ["first", "first_third", "newest"])
@pytest.mark.parametrize("n_lm", [0, 40])
@pytest.mark.parametrize("n_kf", [3, 7, 12])
def test_reduced_system_with_and_without_the_prior(ctx, oracle, n_kf, n_lm, sel):
    """n_kf = 3: level 0 only; 7: several sparse levels (early form with landmarks); 12: a dense corner past one 64-column block.  The
    reduced system of one iteration at radius 1e16 (the damping is below one rounding of the diagonal) with the prior equals the one
    without plus the scatter of T^T info T and T^T (info e + eta); the plan keeps the prior's keyframes dense and is back to what it was
    once the prior is removed; the step solves the system it was computed from."""
    from lvio_fusion_amd import api
    cfg, pre = _window(oracle, n_kf, n_lm)
    kfs = {"first": [0], "first_third": [2, 0], "newest": [n_kf - 1]}[sel]
    rng = np.random.default_rng(7 * n_kf + n_lm)
    state = lc.state_of_cfg(cfg)
    pr = make_prior(rng, kf_state(state, kfs), len(kfs), weight=1000.0)      # (entries of the order of the bias blocks', the system's largest)
    dev = Device(api, ctx, cfg, pre)
    prior = api.DensePrior(ctx, kfs, pr["x0"], pr["info"], pr["eta"], pr["c0"])
    try:
        opt = api.default_solver_options()
        d = ctx.L.lvf_problem_reduced_dim(dev.prob.h)
        assert d == 15 * n_kf
        dev.prob.lm_iteration(opt, RADIUS_TRUTH)
        S0, rhs0 = dev.prob.reduced_system()
        plan0 = dev.prob.debug_plan()
        _reset(api, dev, cfg)
        c0 = dev.prob.cost(opt)
        dev.prob.set_dense_prior(prior)
        c1 = dev.prob.cost(opt)
        c_ref, g_ref, H_ref = dp.evaluate(pr["x0"], pr["info"], pr["eta"], pr["c0"], kf_state(state, kfs))
        assert abs((c1 - c0) - c_ref) <= 1e-9 * abs(c1)
        got = dev.prob.lm_iteration(opt, RADIUS_TRUTH)
        S1, rhs1 = dev.prob.reduced_system()
        plan1 = dev.prob.debug_plan()
        x, fail = dev.prob.debug_step()
        gn, Hn = dp.scatter(n_kf, kfs, g_ref, H_ref)
        S_ref, rhs_ref = S0 + Hn, rhs0 - gn
        print(f"n_kf {n_kf} n_lm {n_lm} {sel}: nb {plan0[0]} -> {plan1[0]}, dense {plan0[1].sum()} -> {plan1[1].sum()}; S err {np.abs(S1 - S_ref).max() / np.abs(S_ref).max():.2e}; "
              f"max|Hn| / max|S0| {np.abs(Hn).max() / np.abs(S0).max():.2e}")
        assert np.abs(Hn).max() >= 1e-4 * np.abs(S0).max(), "the prior must show in the system"
        assert np.abs(S1 - S_ref).max() <= 1e-7 * np.abs(S_ref).max()
        assert_parity(rhs1, rhs_ref, "rhs")
        assert abs(got["cost_before"] - c1) <= 1e-8 * c1
        assert plan1[1][kfs].all(), "a keyframe of the prior was eliminated sparsely"
        assert ctx.L.lvf_problem_reduced_dim(dev.prob.h) == d
        # the step: backward error of the solve on the device's own system (a Cholesky factorisation's is of the order of d 2^-53;
        # 1e3 of that leaves room for the elimination's growth and says nothing about the condition)
        assert fail == 0 and dev.prob.debug_last_solved()
        Sf = np.tril(S1) + np.tril(S1, -1).T
        back = np.abs(Sf @ x - rhs1).max() / (np.abs(Sf).max() * np.abs(x).max() * d + np.abs(rhs1).max())
        print(f"    step backward error {back:.2e}")
        assert back <= 1e3 * d * 2.0 ** -53
        # removed: the plan and the system are what they were
        dev.prob.set_dense_prior(None)
        _reset(api, dev, cfg)
        dev.prob.lm_iteration(opt, RADIUS_TRUTH)
        S2, rhs2 = dev.prob.reduced_system()
        plan2 = dev.prob.debug_plan()
        assert plan2[0] == plan0[0] and np.array_equal(plan2[1], plan0[1]) and ctx.L.lvf_problem_reduced_dim(dev.prob.h) == d
        assert np.abs(S2 - S0).max() <= 1e-12 * np.abs(S0).max() and np.abs(rhs2 - rhs0).max() <= 1e-12 * np.abs(rhs0).max()
    finally:
        dev.close(); prior.close()


def test_reduced_system_with_poisoned_upper_triangle():
    """LVF_POISON_S=1 (every byte of S is NaN before the assembly; the switch is read once per process, hence the child): the with / without
    comparison and the step of the 7-keyframe cases must still hold"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env["LVF_POISON_S"] = "1"
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", os.path.join(root, "tests", "test_gpu_dense_prior.py"),
                        "-k", "with_and_without and 7-"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "6 passed" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ iterations and the solve
def _far_start(cfg, seed, rot_deg, trans, depth_noise=0.0):
    c, rng = dict(cfg), np.random.default_rng(seed)
    c["poses"] = syn.perturb_poses(cfg["poses"], rng, rot_deg, trans)
    c["inv_depth"] = cfg["inv_depth"] * (1 + rng.normal(0, depth_noise, cfg["inv_depth"].shape))
    return c


def test_iteration_and_solve_against_the_reference_loop(ctx, oracle):
    """7 keyframes, 40 landmarks, a prior on keyframes {2, 0} whose x0 is the state the scene was generated at: one lvf_problem_lm_iteration,
    then lvf_problem_solve, against lidar_window_ref's loop with the prior's rows in its dense system; keyframe 1's ba constant"""
    from lvio_fusion_amd import api
    base, pre = _window(oracle, 7, 40)
    kfs = [2, 0]
    rng = np.random.default_rng(77)
    pr = make_prior(rng, kf_state(lc.state_of_cfg(base), kfs), 2, weight=40.0)
    cfg = _far_start(base, 12, 3.0, 0.3)
    lid = lw.empty_lidar()
    with dp.in_dense_system(kfs, pr["x0"], pr["info"], pr["eta"], pr["c0"]):
        dev = Device(api, ctx, cfg, pre)
        prior = api.DensePrior(ctx, kfs, pr["x0"], pr["info"], pr["eta"], pr["c0"])
        try:
            dev.prob.set_dense_prior(prior)
            opt = api.default_solver_options()
            state = lc.state_of_cfg(cfg)
            t, state, r_next, d_next, acc = lw.lm_iteration(oracle, cfg, pre, state, lid, 1e4, 2.0, {})
            got = dev.prob.lm_iteration(opt, 1e4, 2.0)
            print(f"iteration: cost {t['cost_before']:.6e} -> {t['cost_after']:.6e} rho {t['rho']:.3f} accepted {acc} (device {got})")
            assert abs(got["cost_before"] - t["cost_before"]) <= 1e-8 * t["cost_before"]
            assert got["accepted"] == acc and abs(t["rho"] - 1e-3) > 0.1
            assert abs(got["cost_after"] - t["cost_after"]) <= 1e-6 * abs(t["cost_after"])
            assert abs(got["radius"] - r_next) <= 1e-5 * r_next and got["decrease_factor"] == d_next
            assert_state(dev.state(), state, "iteration")
        finally:
            dev.close()
        cfg = _far_start(base, 15, 40.0, 2.0, 0.3)
        dev = Device(api, ctx, cfg, pre)
        try:
            dev.prob.set_dense_prior(prior)
            opt = api.default_solver_options(); opt.max_num_iterations = 10
            ref, state = lw.lm_solve(oracle, cfg, pre, lc.state_of_cfg(cfg), lid, max_num_iterations=10)
            print("reference trace (cost_before, cost_after, radius, accepted, valid, rho):\n", ref["trace"])
            assert np.abs(ref["trace"][:, 5] - 1e-3).min() > 0.1, "no step quality near the threshold"
            s = dev.prob.solve(opt)
            print(f"solve: {s.num_iterations} iterations ({s.why}), {s.num_successful_steps} accepted; reference {ref['num_iterations']} ({ref['why']}), {ref['num_successful_steps']}")
            assert (s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.why) == \
                   (ref["num_iterations"], ref["num_successful_steps"], ref["num_unsuccessful_steps"], ref["why"])
            assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-8 * ref["initial_cost"] and abs(s.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
            assert_state(dev.state(), state, "solve")
        finally:
            dev.close(); prior.close()


# ------------------------------------------------------------------------------------------------ lvf_problem_marginal_prior
@pytest.mark.parametrize("case", ["one", "two", "gauge_free", "on_a_prior"])
def test_marginal_prior_against_the_long_double_reference(ctx, oracle, case):
    """5 keyframes.  one / two: the newest keyframe, keyframes {3, 1}, of the visual-inertial window; gauge_free: the same window without
    its PoseOnly blocks (no landmark with a frozen world point) — nothing anchors the position, so info is singular and that is no failure;
    on_a_prior: the IMU-only window (whose marginal on any keyframe is zero: every ImuError block has as many residuals as its end
    keyframe has unknowns) anchored by a dense prior on keyframe 0, which must enter the result.  Reference: the device's own reduced
    system, right-hand side and cost (a twin's iteration at radius 1e16), eliminated in long double.  The landmarks' share of the
    constant, 1/2 sum g_l^2 / H_ll, is formed from the device's landmark gradient and the numpy reference's H_ll, which stands for the
    device's to the parity bound of a cost (1e-9): an error delta of the corner is 2 delta D_last^2 / ||D A* D||_F <= delta / c0* in
    aug_err's norm, so the tolerance grows by 1e-9 c / c0* where there are landmarks."""
    from lvio_fusion_amd import api
    n_kf = 5
    if case == "gauge_free":
        cfg = syn.config4_window(n_kf=n_kf, n_lm=40, n_prewindow=0, seed=505, imu_samples=3)
        pre = lc.preint(oracle, cfg)
        assert len(cfg["po"]["kf_idx"]) == 0
    else:
        cfg, pre = _window(oracle, n_kf, 0 if case == "on_a_prior" else 40, seed=500)
    kfs = {"one": [4], "two": [3, 1], "gauge_free": [2], "on_a_prior": [4]}[case]
    dev, twin = (Device(api, ctx, cfg, pre) for _ in range(2))
    prior = None
    try:
        if case == "on_a_prior":
            pr = make_prior(np.random.default_rng(8), kf_state(lc.state_of_cfg(cfg), [0]), 1)
            prior = api.DensePrior(ctx, [0], pr["x0"], pr["info"], pr["eta"], pr["c0"])
            dev.prob.set_dense_prior(prior); twin.prob.set_dense_prior(prior)
        opt = api.default_solver_options()
        c_full = c = twin.prob.cost(opt)
        if cfg["n_lm"]:
            J = lw.dense_system(oracle, cfg, pre, lc.state_of_cfg(cfg), lw.empty_lidar())[0]
            gl = twin.prob.gradient(opt)[1]
            c = c_full - 0.5 * float((gl ** 2 / (J[:, 15 * n_kf:] ** 2).sum(axis=0)).sum())
        twin.prob.lm_iteration(opt, RADIUS_TRUTH)
        S, rhs = twin.prob.reduced_system()
        S = np.tril(S) + np.tril(S, -1).T
        sel = dp.natural_index(n_kf, kfs)
        ri, re, rc0 = dp.marginal_prior(S, -rhs, c, sel)
        A_star = dp.augmented(ri, re, rc0)
        n_blocks = len(cfg["tc"]["lm_idx"]) + len(cfg["tf"]["lm_idx"]) + n_kf + 1
        # (gauge_free: info* has exact zeros on its diagonal along the free directions, so the norm's scale comes from S's own diagonal)
        Dn = dp.system_scale(S, c, sel) if case == "gauge_free" else None
        tol = dp.propagated(S, -rhs, c, sel, A_star, n_blocks * 2.0 ** -53 + 2.0 ** -52, Dn)
        floor = M * max(dp.err64_bound(S, -rhs, c, sel, A_star, 11, Dn), (15 * n_kf + 1) * 2.0 ** -53)
        if cfg["n_lm"]:
            tol += 1e-9 * c_full / float(rc0)
        info, eta, c0, st = dev.prob.marginal_prior(opt, kfs)
        assert st["fail"] == 0 and st["n_present"] + st["n_absent"] == 15 * n_kf and 0.0 < st["min_pivot_ratio"] <= 1.0
        err = dp.aug_err(dp.augmented(info, eta, c0), A_star, Dn)
        w = np.linalg.eigvalsh(info)
        print(f"{case}: err {err:.3e} tol {tol:.3e} + floor {floor:.3e}; c {c:.6e} c0 {c0:.6e}; eig(info) {w.min():.3e} .. {w.max():.3e}; stats {st}")
        assert err <= tol + floor
        assert np.array_equal(info, info.T) and c0 >= 0.0 and c0 <= c_full * (1 + 1e-12)
        D = dp.system_scale(S, c, sel)[:len(sel)].astype(np.float64)
        w_ref = np.linalg.eigvalsh(D[:, None] * ri.astype(np.float64) * D[None, :])
        if case == "gauge_free":
            assert w_ref.min() <= 1e-9, "nothing anchors this window: the reference's info must be singular"
        else:
            assert w_ref.min() > 1e-9
        if case == "on_a_prior":
            dev.prob.set_dense_prior(None)
            i2, e2, c2, st2 = dev.prob.marginal_prior(opt, kfs)
            print(f"    without the prior: max|info| {np.abs(i2).max():.3e} (with: {np.abs(info).max():.3e}), c0 {c2:.3e}")
            assert st2["fail"] == 0 and np.abs(i2).max() <= 1e-6 * np.abs(info).max(), "an ImuError chain alone leaves nothing on its end"
        # the plain marginal of the same keyframes keeps its result beside it
        if case in ("one", "two"):
            info_m, _, st_m = dev.prob.marginal(opt, kfs)
            assert st_m["fail"] == 0 and np.abs(info_m - info).max() <= 1e-9 * np.abs(info).max()
    finally:
        dev.close(); twin.close()
        if prior is not None:
            prior.close()


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(ctx, oracle):
    from lvio_fusion_amd import api
    rng = np.random.default_rng(3)
    x0 = np.zeros((9, 16)); x0[:, 3] = 1.0
    info = np.eye(15 * 9)
    ok = lambda n: (list(range(n)), x0[:n], info[:15 * n, :15 * n])
    for n in (0, 9):
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            api.DensePrior(ctx, *ok(n))
    with pytest.raises(api.LvfError, match="lvf error 1:"):
        api.DensePrior(ctx, [1, 1], x0[:2], info[:30, :30])
    with pytest.raises(api.LvfError, match="lvf error 1:"):
        api.DensePrior(ctx, [-1], x0[:1], info[:15, :15])
    bad_info = info[:15, :15].copy(); bad_info[7, 2] = np.nan
    bad_x0 = x0[:1].copy(); bad_x0[0, 9] = np.inf
    bad_eta = np.zeros(15); bad_eta[3] = np.nan
    for args, kw in ((([0], x0[:1], bad_info), {}), (([0], bad_x0, info[:15, :15]), {}), (([0], x0[:1], info[:15, :15]), dict(eta=bad_eta)),
                     (([0], x0[:1], info[:15, :15]), dict(c0=np.inf))):
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            api.DensePrior(ctx, *args, **kw)
    upper = info[:15, :15].copy(); upper[2, 7] = np.nan          # not read
    api.DensePrior(ctx, [0], x0[:1], upper).close()
    # a keyframe that is not in the window
    cfg, pre = _window(oracle, 3, 0)
    dev = Device(api, ctx, cfg, pre)
    prior = api.DensePrior(ctx, [3], x0[:1], info[:15, :15])
    try:
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            dev.prob.set_dense_prior(prior)
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            prior.evaluate(dev.st)
        opt = api.default_solver_options()
        for kfs in ([], list(range(9)), [1, 1], [3]):
            with pytest.raises(api.LvfError, match="lvf error 1:"):
                dev.prob.marginal_prior(opt, kfs)
    finally:
        dev.close(); prior.close()
