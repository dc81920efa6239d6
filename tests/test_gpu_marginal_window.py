"""Marginal information and covariance of keyframes of a problem / a persistent window on device (lvf_problem_marginal, lvf_window_marginal)
against an independent truth, and the guarantee that the call disturbs nothing.

Truth: on a fresh window the CPU oracle's Window.lm_iteration(radius=1e16) returns the reduced system at the start point with a damping below
float64 resolution; marginal_ref on that S is the expectation for Problem.marginal at the same, untouched state.

Tolerance.  The device's assembled system agrees with the oracle's to 1e-7 of its largest entry (test_lm_iteration_parity).  That figure,
propagated through the case (marginal_ref.propagated: first-order, the condition entering through S^-1), is the tolerance this feature was
specified with — at 8 keyframes / 120 landmarks (cond 7.7e6) it is 34 (info) and 26 (cov) for the newest keyframe, i.e. it constrains nothing, and at
2 / 40, whose undamped system is singular to float64 (cond 2.9e18, smallest pivot ratio 1.6e-16), nothing can.  So beside it the test
measures how far a device assembly really is from the oracle's (a twin problem's lm_iteration at radius 1e16, the figure the parity test
bounds by 1e-7), allows the marginal's own assembly the same distance again plus one rounding of the diagonal (the damping the truth carries),
and propagates THAT: tol = propagated(2 delta + 2^-52) + M * max(err64, d 2^-53), M the margin of tests/test_gpu_marginal.py."""
import ctypes as C

import numpy as np
import pytest

from tests import marginal_ref as mr
from tests.test_gpu_marginal import M

pytestmark = pytest.mark.gpu
FULL = ("tc", "tf", "po", "imu")
RADIUS_TRUTH = 1e16


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def close(b, st, prob):
    prob.close()
    for h in list(b.values()) + [st]:
        if h is not None:
            h.close()


def sym(S):
    S = np.asarray(S, np.float64)
    return np.tril(S) + np.tril(S, -1).T


class Fresh:
    """a window on the device (untouched), a twin that takes one iteration at RADIUS_TRUTH, and the oracle's system at the start point"""

    def __init__(self, api, ctx, oracle, n_kf, n_lm, seed, use=FULL):
        from tests.test_gpu_solver import build, state_of
        self.api, self.n_kf = api, n_kf
        self.cfg, self.st, self.b, self.prob, win = build(api, ctx, oracle, n_kf, n_lm, seed, use=use)
        _, self.st2, self.b2, self.prob2, _ = build(api, ctx, oracle, n_kf, n_lm, seed, use=use)
        self.opt = api.default_solver_options()
        self.start = state_of(api, self.st)
        self.S = sym(win.lm_iteration(RADIUS_TRUTH, 2.0)["S"])
        self.prob2.lm_iteration(self.opt, RADIUS_TRUTH)
        S2 = sym(self.prob2.reduced_system()[0])
        self.delta = float(np.abs(S2 - self.S).max() / np.abs(self.S).max())
        assert self.delta <= 1e-7

    def tolerances(self, S, sel, ref, seed):
        keep = mr.layout(S, sel)[1][[int(s) for s in sel]]
        loose = mr.propagated(S, sel, ref, 1e-7)
        tight = mr.propagated(S, sel, ref, 2.0 * self.delta + 2.0 ** -52)
        e64 = mr.err64_bound(S, sel, ref, seed)
        floor = [max(e, S.shape[0] * 2.0 ** -53) for e in e64]
        return keep, loose, [t + M * f for t, f in zip(tight, floor)]

    def close(self):
        close(self.b, self.st, self.prob)
        close(self.b2, self.st2, self.prob2)


def test_truth_8kf(ctx, oracle):
    """the newest keyframe, and all eight in a scattered order, against the oracle's system; consistency of a keyframe's block across selections"""
    from lvio_fusion_amd import api
    from tests.test_gpu_solver import state_of
    w = Fresh(api, ctx, oracle, 8, 120, 3)
    try:
        covs = {}
        for kfs in ([7], [5, 0, 7, 2, 6, 1, 3, 4], [7, 2]):
            sel = mr.kf_selection(8, kfs)
            ref = mr.marginal(w.S, sel)
            assert ref["fail"] == 0
            keep, loose, tight = w.tolerances(w.S, sel, ref, 3)
            info, cov, st = w.prob.marginal(w.opt, kfs)
            assert st["fail"] == 0 and st["n_present"] == 120 and st["n_absent"] == 0
            e = mr.errors(info, cov, ref, keep)
            print(f"truth kf8 {kfs}: delta {w.delta:.3e} err info {e[0]:.3e} cov {e[1]:.3e} | tol(1e-7) info {loose[0]:.3e} cov {loose[1]:.3e} | tol(measured) info {tight[0]:.3e} cov {tight[1]:.3e}")
            assert e[0] <= loose[0] and e[1] <= loose[1]
            assert e[0] <= tight[0] and e[1] <= tight[1]
            assert np.array_equal(info, info.T) and np.array_equal(cov, cov.T)
            assert abs(st["min_pivot_ratio"] - ref["min_pivot_ratio"]) <= max(1e-6, max(tight)) * ref["min_pivot_ratio"]
            covs[tuple(kfs)] = (cov, max(tight))
            now = state_of(api, w.st)
            assert all(np.array_equal(now[k].view(np.uint8), w.start[k].view(np.uint8)) for k in now), "marginal moved the state"
        # consistency: cov({7}) is the block of keyframe 7 in cov({7, 2}) and in the cov of all eight
        c7, t7 = covs[(7,)]
        for kfs, at in (((7, 2), 0), ((5, 0, 7, 2, 6, 1, 3, 4), 2)):
            big, tb = covs[kfs]
            blk = big[15 * at:15 * at + 15, 15 * at:15 * at + 15]
            dsc = np.sqrt(np.diag(c7))
            rel = np.linalg.norm((blk - c7) / np.outer(dsc, dsc)) / np.linalg.norm(c7 / np.outer(dsc, dsc))
            print(f"consistency kf7 in {kfs}: {rel:.3e} (bound {t7 + tb:.3e})")
            assert rel <= t7 + tb
    finally:
        w.close()


def test_smallest_imu_window(ctx, oracle):
    """2 keyframes / 40 landmarks: the undamped system is singular to float64 (the reference's smallest pivot ratio is below 2^-52), so the
    call either flags a failure or reports a pivot ratio that says so — always LVF_OK, the state untouched"""
    from lvio_fusion_amd import api
    from tests.test_gpu_solver import state_of
    w = Fresh(api, ctx, oracle, 2, 40, 31)
    try:
        sel = mr.kf_selection(2, [1])
        ref = mr.marginal(w.S, sel)
        info, cov, st = w.prob.marginal(w.opt, [1])
        print(f"truth kf2: reference fail {ref['fail']} min_pivot_ratio {ref['min_pivot_ratio']}; device {st}")
        assert st["n_present"] + st["n_absent"] == 30
        if ref["fail"] == 0 and ref["min_pivot_ratio"] > 30 * 2.0 ** -53:
            keep, loose, tight = w.tolerances(w.S, sel, ref, 31)
            assert st["fail"] == 0
            e = mr.errors(info, cov, ref, keep)
            assert e[0] <= loose[0] and e[1] <= loose[1]
        else:
            bound = (ref["min_pivot_ratio"] or 0.0) + M * 30 * 2.0 ** -53
            assert st["fail"] != 0 or 0.0 < st["min_pivot_ratio"] <= bound
        now = state_of(api, w.st)
        assert all(np.array_equal(now[k].view(np.uint8), w.start[k].view(np.uint8)) for k in now)
    finally:
        w.close()


def test_window_without_imu(ctx, oracle):
    """every (v, ba, bg) unknown is absent; the pose blocks match the 6 n_kf-dimensional computation"""
    from lvio_fusion_amd import api
    n_kf = 6
    w = Fresh(api, ctx, oracle, n_kf, 80, 7, use=("tc", "tf", "po"))
    try:
        kfs = [5, 2]
        info, cov, st = w.prob.marginal(w.opt, kfs)
        assert st["fail"] == 0 and st["n_absent"] == 9 * n_kf and st["n_present"] == 6 * n_kf
        pose = np.concatenate([np.arange(15 * i, 15 * i + 6) for i in range(len(kfs))])
        vbb = np.setdiff1d(np.arange(15 * len(kfs)), pose)
        for X in (info, cov):
            assert not X[vbb, :].any() and not X[:, vbb].any()
        Sp = w.S[:6 * n_kf, :6 * n_kf]
        sel = np.concatenate([np.arange(6 * k, 6 * k + 6) for k in kfs]).astype(np.int32)
        ref = mr.marginal(Sp, sel)
        keep, loose, tight = w.tolerances(Sp, sel, ref, 7)
        e = mr.errors(info[np.ix_(pose, pose)], cov[np.ix_(pose, pose)], ref, keep)
        print(f"truth kf6 no IMU: delta {w.delta:.3e} err info {e[0]:.3e} cov {e[1]:.3e} | tol(1e-7) {loose[0]:.3e} {loose[1]:.3e} | tol(measured) {tight[0]:.3e} {tight[1]:.3e}")
        assert e[0] <= loose[0] and e[1] <= loose[1] and e[0] <= tight[0] and e[1] <= tight[1]
    finally:
        w.close()


def test_constant_pose(ctx, oracle):
    """set_pose_constant(0): keyframe 0's pose rows are zero, and fixing it cannot make the other keyframes less certain"""
    from lvio_fusion_amd import api
    w = Fresh(api, ctx, oracle, 8, 120, 3)
    try:
        kfs = [0, 7, 3]
        _, free, st0 = w.prob.marginal(w.opt, kfs)
        w.prob.set_pose_constant(0, True)
        info, cov, st = w.prob.marginal(w.opt, kfs)
        w.prob.set_pose_constant(0, False)
        assert st0["fail"] == 0 and st["fail"] == 0 and st["n_absent"] == 6 and st0["n_absent"] == 0
        for X in (info, cov):
            assert not X[:6, :].any() and not X[:, :6].any()
            assert X[6:, 6:].any()
        others = np.arange(15, 45)
        diff = free[np.ix_(others, others)] - cov[np.ix_(others, others)]
        dsc = np.sqrt(np.diag(free)[others])
        nd, nf = diff / np.outer(dsc, dsc), free[np.ix_(others, others)] / np.outer(dsc, dsc)
        sel = mr.kf_selection(8, kfs)
        _, _, tight = w.tolerances(w.S, sel, mr.marginal(w.S, sel), 3)
        lo = np.linalg.eigvalsh(0.5 * (nd + nd.T))[0]
        print(f"constant pose: smallest eigenvalue of the scaled difference {lo:.3e} (largest {np.linalg.eigvalsh(0.5 * (nd + nd.T))[-1]:.3e}), allowed {-2 * tight[1] * np.linalg.norm(nf):.3e}")
        assert lo >= -2.0 * tight[1] * np.linalg.norm(nf)
    finally:
        w.close()


def test_argument_errors(ctx, oracle):
    from lvio_fusion_amd import _lib, api
    w = Fresh(api, ctx, oracle, 2, 40, 31)
    try:
        buf, st = np.full((135, 135), -7.25), _lib.MarginalStats()

        def call(kfs, info=True, cov=True):
            k = np.ascontiguousarray(kfs, np.int32)
            return ctx.L.lvf_problem_marginal(w.prob.h, C.byref(w.opt), api._ip(k), len(kfs), api._dp(buf) if info else None, api._dp(buf) if cov else None, C.byref(st))
        assert call([0, 2]) == 1 and call([-1]) == 1          # out of range
        assert call([1, 1]) == 1                              # listed twice
        assert call([]) == 1 and call([0, 1, 0, 1, 0, 1, 0, 1, 0]) == 1
        assert call([0], info=False, cov=False) == 1
        assert (buf == -7.25).all()
    finally:
        w.close()


def test_non_interference(ctx, oracle):
    """A: two iterations.  B: one, marginal, the second.  The marginal call itself moves nothing (bit-equal state before and after), and B ends
    where A ends.  Bit for bit that cannot be asked of this solver: an identical re-run of A already differs from A in its last bits (the Schur
    complement, the elimination levels and the cost stripes are atomic adds in the scheduler's order; the test prints those differences).  What
    one more run may differ by is what the linear solve is good for: each run's reduced step is within 8 max(err64, d 2^-53) of the
    exact one in the norm ||Ds . ||, Ds = sqrt(diag S), so two runs differ by twice that per iteration, and over the two iterations an unknown j
    by at most 4 * 8 * floor * ||Ds x*|| / Ds_j — taken per state field at its smallest Ds_j (poses: the tangent entries; an inverse depth, which
    follows the camera step through the back substitution: the same relative figure of its own size)."""
    from lvio_fusion_amd import api
    from tests import reduced_cases as rc
    from tests.test_gpu_solver import build, state_of
    runs, system = [], None
    for with_marginal in (False, True, False):
        cfg, st, b, prob, _ = build(api, ctx, oracle, 11, 200, 107)
        opt = api.default_solver_options()
        r1 = prob.lm_iteration(opt, 1e4)
        if with_marginal:
            before = state_of(api, st)
            _, _, ms = prob.marginal(opt, [10, 4])
            assert ms["fail"] == 0
            after = state_of(api, st)
            assert all(np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)) for k in before)
        r2 = prob.lm_iteration(opt, r1["radius"], r1["decrease_factor"])
        runs.append((r1, r2, state_of(api, st)))
        if system is None:
            system = prob.reduced_system()
        close(b, st, prob)
    (a1, a2, sa), (b1, b2, sb), (_, _, sc) = runs
    S, rhs = system
    S = sym(S)
    x_star, x64 = rc.ref_solve(S, rhs)
    floor = max(rc.err64_bound(S, rhs, x_star, 107, x64), len(rhs) * 2.0 ** -53)
    ds = np.sqrt(np.diag(S))
    scale = float(np.linalg.norm(ds * x_star.astype(np.float64)))
    n_kf, dp = 11, 66
    part = {"poses": ds[:dp], "vel": np.concatenate([ds[dp + 9 * k:dp + 9 * k + 3] for k in range(n_kf)]),
            "ba": np.concatenate([ds[dp + 9 * k + 3:dp + 9 * k + 6] for k in range(n_kf)]), "bg": np.concatenate([ds[dp + 9 * k + 6:dp + 9 * k + 9] for k in range(n_kf)])}
    allowed = {k: 4.0 * 8.0 * floor * scale / float(v.min()) for k, v in part.items()}
    allowed["inv_depth"] = 4.0 * 8.0 * floor * float(np.abs(sa["inv_depth"]).max())
    diff = lambda x, y: {k: float(np.abs(x[k] - y[k]).max()) for k in x}
    got = diff(sa, sb)
    print(f"non-interference: |A - B| {got} ; an identical re-run |A - A'| {diff(sa, sc)} ; allowed {allowed} (floor {floor:.3e})")
    assert all(got[k] <= allowed[k] for k in sa)
    # (the costs are sums of striped atomic adds: decisions are compared exactly, radii and sums to rounding)
    for x, y in ((a1, b1), (a2, b2)):
        assert x["accepted"] == y["accepted"] and x["decrease_factor"] == y["decrease_factor"] and abs(x["radius"] - y["radius"]) <= 1e-9 * x["radius"]
        assert abs(x["cost_after"] - y["cost_after"]) <= 1e-12 * abs(x["cost_after"]) and abs(x["cost_before"] - y["cost_before"]) <= 1e-12 * abs(x["cost_before"])
    assert a1["accepted"] and a2["accepted"], "the comparison needs steps that move the state"


def test_launch_counts_unchanged(ctx, oracle):
    """the 50-keyframe window's iteration consists of the launches it consisted of, before and after a marginal call: k_tf_reduce, k_prepare, the
    Schur launch, four block steps on their own, the merged last launch (the fifth block step + back substitution + step tail) and the fused
    candidate pass — what the parent commit's library reports for this window"""
    from lvio_fusion_amd import api, synthetic as syn
    from tests.test_gpu_solve_trajectory import make, close as close_w, options
    w = make(api, ctx, oracle, 0, 0, syn.SEED_CFG4, cfg=syn.config4_window())
    try:
        opt = options(api)
        before = [(n, la) for n, _, la in w["prob"].stage_times(opt, 1e4, reps=2)]
        _, cov, st = w["prob"].marginal(opt, list(range(49, 41, -1)))
        assert st["fail"] == 0 and st["n_present"] == 750 and np.isfinite(cov).all()
        after = [(n, la) for n, _, la in w["prob"].stage_times(opt, 1e4, reps=2)]
        assert before == after
        assert [la for _, la in after if la] == [1, 1, 1, 4, 1, 1]
    finally:
        close_w(w)


def test_window_marginal(ctx, oracle):
    """After Window.solve, Window.marginal of the newest keyframe equals Problem.marginal on the equivalently built problem at the window's
    state.  Both linearise at bit-equal states; their block lists differ in order only, so an entry of S — a sum over at most n_blocks terms
    bounded by max|S| — differs by at most n_blocks * 2^-53 * max|S|: that figure is propagated through the system (a twin problem's iteration at
    radius 1e16 supplies it).  An unknown keyframe id is an argument error."""
    from lvio_fusion_amd import _lib, api, synthetic as syn
    n_kf = 6
    cfg = syn.config4_window(n_kf=n_kf, n_lm=150, n_prewindow=0, seed=606, imu_samples=4)
    cam0, cam1, tc, tf = cfg["cam0"], cfg["cam1"], cfg["tc"], cfg["tf"]
    pre = [oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]
    # (keyframe 0 has no ImuError block behind it and, under this threshold, counts as weakly seen: it gets the absolute prior that anchors the
    # window — without one the undamped system has the gauge freedom of the whole trajectory and no covariance)
    win = api.Window(ctx, cam0, cam1, baseline=syn.baseline(), weak_visual_threshold=10 ** 6)
    hs = []
    try:
        for t in range(n_kf):
            win.add_keyframe(100 + t, cfg["poses"][t], cfg["w_kf"][t])
            win.set_imu(100 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
            for i in np.nonzero(tc["kf_idx"] == t)[0]:
                win.add_landmark(5000 + int(tc["lm_idx"][i]), 100 + t, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][int(tc["lm_idx"][i])])
            for i in np.nonzero(tf["kf2_idx"] == t)[0]:
                win.add_observation(5000 + int(tf["lm_idx"][i]), 100 + t, tf["ob"][i])
        opt = api.default_solver_options()
        opt.max_num_iterations = 3
        win.solve(opt)
        cnt = win.counts()
        assert (cnt["kf"], cnt["tc"], cnt["tf"], cnt["po"], cnt["imu"], cnt["prior"]) == (n_kf, len(tc["lm_idx"]), len(tf["lm_idx"]), 0, n_kf - 1, 1)
        poses = np.array([win.pose(100 + t) for t in range(n_kf)])
        info, cov, st = win.marginal(opt, [100 + n_kf - 1])
        assert st["fail"] == 0 and st["n_present"] == 15 * n_kf
        assert all(np.array_equal(poses[t], win.pose(100 + t)) for t in range(n_kf)), "Window.marginal moved the window"
        again = win.marginal(opt, [100 + n_kf - 1])
        # the equivalently built problem (and a twin of it that gives the system itself), at the window's state
        imu = [win.imu(100 + t) for t in range(n_kf)]
        invd = np.array([win.inv_depth(5000 + l) if l in set(tc["lm_idx"].tolist()) else 1.0 for l in range(cfg["n_lm"])])
        btc = api.two_camera_batch(ctx, cam0, cam1, tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"])
        btc.set_block_weights((np.float32(5) * cfg["w_kf"][tc["kf_idx"]].astype(np.float32)).astype(np.float64))
        btf = api.two_frame_batch(ctx, cam0, cam1, tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"])
        bim = api.imu_batch(ctx, np.stack(pre), [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]])
        bpr = api.pose_prior_batch(ctx, [-1], [0], poses[:1], [100.0], [0.0])      # (the window's prior: keyframe 0 held at its current pose)
        hs += [btc, btf, bim, bpr]
        probs = []
        for _ in range(2):
            s = api.State(ctx, n_kf, cfg["n_lm"])
            for field, v in ((api.POSES, poses), (api.VEL, np.array([x[0] for x in imu])), (api.BA, np.array([x[1] for x in imu])),
                             (api.BG, np.array([x[2] for x in imu])), (api.INV_DEPTH, invd), (api.W_VISUAL, cfg["w_kf"])):
                s.set(field, v)
            probs.append(api.Problem(ctx, s, btc, btf, None, bim))
            probs[-1].set_pose_priors(bpr)
            hs += [s]
        info_p, cov_p, st_p = probs[0].marginal(opt, [n_kf - 1])
        assert st_p["fail"] == 0 and st_p["n_present"] == st["n_present"]
        probs[1].lm_iteration(opt, RADIUS_TRUTH)
        S = sym(probs[1].reduced_system()[0])
        sel = mr.kf_selection(n_kf, [n_kf - 1])
        ref = mr.marginal(S, sel)
        n_blocks = len(tc["lm_idx"]) + len(tf["lm_idx"]) + n_kf
        tol = mr.propagated(S, sel, ref, n_blocks * 2.0 ** -53 + 2.0 ** -52)
        floor = [M * max(e, 15 * n_kf * 2.0 ** -53) for e in mr.err64_bound(S, sel, ref, 606)]
        ref_p = dict(info=info_p.astype(np.longdouble), cov=cov_p.astype(np.longdouble))
        e = mr.errors(info, cov, ref_p, np.ones(15, bool))
        print(f"window against problem: err info {e[0]:.3e} cov {e[1]:.3e}, allowed {tol[0] + 2 * floor[0]:.3e} {tol[1] + 2 * floor[1]:.3e}")
        assert e[0] <= tol[0] + 2 * floor[0] and e[1] <= tol[1] + 2 * floor[1]
        e2 = mr.errors(again[0], again[1], dict(info=info.astype(np.longdouble), cov=cov.astype(np.longdouble)), np.ones(15, bool))      # (a second call: the same sums in another order)
        assert e2[0] <= tol[0] + 2 * floor[0] and e2[1] <= tol[1] + 2 * floor[1]
        for p in probs:
            p.close()
        buf, ms = np.full((15, 15), -7.25), _lib.MarginalStats()
        ids = np.array([987654321], np.int64)
        assert ctx.L.lvf_window_marginal(win.h, C.byref(opt), ids.ctypes.data_as(C.POINTER(C.c_int64)), 1, api._dp(buf), api._dp(buf), C.byref(ms)) == 1
        assert (buf == -7.25).all()
    finally:
        win.close()
        for h in hs:
            h.close()


