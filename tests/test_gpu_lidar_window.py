"""LiDAR plane factors on keyframe poses inside the window solve, on the device (lvf_lidar_pose_*, lvf_problem_set_lidar_planes,
lvf_window_set_lidar_*) against the declared semantics of tests/lidar_window_ref.py.

Bounds.  The factor (a) takes tests/test_gpu_factors.py's bound for the plane batches (helpers.assert_parity).  Cost, gradient, reduced
system, iterations and solves (b)-(d), (f) take what tests/test_gpu_priors.py, test_gpu_solver.py and test_gpu_window.py apply to a window
with pose priors, the nearest case on the same chain: cost 1e-9 (1e-8 inside an iteration, 1e-6 at the candidate), S 1e-7 of its largest
entry, rhs / gradient / states assert_parity, radius 1e-5, equal decisions.  The marginal (g) takes tests/test_gpu_marginal_window.py's
propagated tolerance."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import lidar_window_cases as lc
from tests import lidar_window_ref as lw
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu
FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


class Device:
    """a cfg (lidar_window_cases / synthetic.config4_window layout) as a device problem, with optional lidar blocks"""

    def __init__(self, api, ctx, cfg, pre, blocks=None, weight=None, huber_a=None):
        self.api, self.cfg = api, cfg
        n_kf, n_lm = cfg["n_kf"], cfg["n_lm"]
        self.st = api.State(ctx, n_kf, n_lm)
        for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
            if np.asarray(cfg[key]).size:
                self.st.set(field, cfg[key])
        tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
        self.h = []
        btc = api.two_camera_batch(ctx, cfg["cam0"], cfg["cam1"], tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"]) if len(tc["lm_idx"]) else None
        btf = api.two_frame_batch(ctx, cfg["cam0"], cfg["cam1"], tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"]) if len(tf["lm_idx"]) else None
        bpo = api.pose_only_batch(ctx, cfg["cam0"], po["ob"], po["kf_idx"], po["pw_idx"], po["pw"]) if len(po["kf_idx"]) else None
        bim = api.imu_batch(ctx, pre, [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]]) if cfg["imu"] else None
        self.prob = api.Problem(ctx, self.st, btc, btf, bpo, bim)
        self.lidar = None
        if blocks is not None:
            self.lidar = api.lidar_pose_batch(ctx, *blocks, weight=weight, huber_a=huber_a)
            self.prob.set_lidar_planes(self.lidar)
        self.h += [b for b in (btc, btf, bpo, bim, self.lidar) if b is not None]

    def state(self):
        api, n_kf = self.api, self.cfg["n_kf"]
        g = lambda f, w: np.asarray(self.st.get(f)).reshape(-1, w) if w else np.asarray(self.st.get(f)).reshape(-1)
        return [g(api.POSES, 7), g(api.VEL, 3), g(api.BA, 3), g(api.BG, 3), g(api.INV_DEPTH, 0)[:self.cfg["n_lm"]]]

    def close(self):
        self.prob.close()
        for b in self.h + [self.st]:
            b.close()


def assert_state(dev_state, ref_state, what):
    for name, a, b in zip(FIELDS, dev_state, ref_state):
        if np.asarray(b).size:
            assert_parity(a, b, f"{what}: {name}")


@pytest.fixture(scope="module")
def window5(oracle):
    """config4_window(n_kf=5, n_lm=40) plus 600 plane blocks, sorted by keyframe, whitened (weights of the order of 1 / the 1 cm range noise,
    so that they weigh against visual blocks of weight fx / 10 per pixel): half without a loss, half with a Huber threshold at the median
    of their residuals at the start, so that both branches of the loss are populated"""
    cfg = syn.config4_window(n_kf=5, n_lm=40, n_prewindow=20, seed=101, imu_samples=4)
    pre = lc.preint(oracle, cfg)
    rng = np.random.default_rng(5)
    blocks = lc.plane_blocks(cfg["poses_true"], 120, rng)
    n = len(blocks[4])
    weight = np.where(np.arange(n) % 2 == 0, 100.0, 200.0)
    raw = lw.plane_rows(lw.make_lidar(*blocks, weight=weight), cfg["poses"])[0]
    lossy = np.arange(n) % 2 == 1
    huber = np.where(lossy, float(np.median(np.abs(raw[lossy]))), 0.0)
    lid = lw.make_lidar(*blocks, weight=weight, huber_a=huber)
    outside = lw.lidar_rows(lid, cfg["poses"], 15 * 5 + 40)[3]
    assert outside[lossy].sum() >= 50 and (~outside[lossy]).sum() >= 50 and not outside[~lossy].any(), "both branches of the loss must be populated"
    return dict(cfg=cfg, pre=pre, blocks=blocks, weight=weight, huber=huber, lid=lid)


def _subset(w5, idx):
    blocks = tuple(a[idx] for a in w5["blocks"])
    return blocks, w5["weight"][idx], w5["huber"][idx], lw.take(w5["lid"], idx)


# ------------------------------------------------------------------------------------------------ (a) the factor
def test_factor_against_the_oracle(ctx, oracle):
    """130 blocks over 3 keyframes (two full waves and a ragged tail), a collinear triple and a zero weight among them"""
    from lvio_fusion_amd import api
    rng = np.random.default_rng(31)
    n, n_kf = 130, 3
    poses = syn.drive_poses(n_kf, rng)
    poses[:, :4] *= rng.uniform(0.85, 1.2, (n_kf, 1))          # un-normalised quaternions: the Jacobian carries the normalisation's projector
    p, pa, pb, pc = (rng.normal(0, 6.0, (n, 3)) for _ in range(4))
    pa[70], pb[70], pc[70] = (1.0, 2.0, 3.0), (2.0, 4.0, 6.0), (3.0, 6.0, 9.0)      # collinear, exactly: a zero normal, a null block
    kf = np.sort(rng.integers(0, n_kf, n)).astype(np.int32)
    w = rng.uniform(0.01, 3.0, n); w[11] = 0.0
    st = api.State(ctx, n_kf, 1)
    st.set(api.POSES, poses)
    b = api.lidar_pose_batch(ctx, p, pa, pb, pc, kf, weight=w, huber_a=np.full(n, 0.1))
    try:
        nrm = oracle.plane_normals(pa, pb, pc)
        got_n = b.normals()
        assert not got_n[70].any() and not nrm[70].any()
        assert_parity(got_n, nrm, "normals")
        assert b.num_valid() == n - 1
        b.evaluate(st)
        r, J = b.residuals()[:, 0], b.jacobian(0)[:, 0, :]
        for k in range(n_kf):
            m = kf == k
            r0, J0 = oracle.lidar_plane_se3(p[m], pa[m], nrm[m], poses[k])
            assert_parity(r[m], w[m] * r0, f"r, keyframe {k}"); assert_parity(J[m], w[m, None] * J0, f"J, keyframe {k}")
        assert r[70] == 0.0 and not J[70].any() and r[11] == 0.0 and not J[11].any()
        b.evaluate(st, jacobians=False)
        assert np.array_equal(b.residuals()[:, 0], r)
        with pytest.raises(api.LvfError):
            b.jacobian(0)
        # the Problem::Evaluate-shaped surface: each block's own loss applied, the pose block in its 6 tangent columns
        lid = lw.make_lidar(p, pa, pb, pc, kf, weight=w, huber_a=0.1)
        J_ref, r_ref, _, outside = lw.lidar_rows(lid, poses, 15 * n_kf)
        assert outside.any() and (~outside).any()
        assert ctx.L.lvf_batch_local_columns(b.h) == 6
        rl, Jl = b.evaluate_local(st, 1.0)
        assert rl.shape == (n, 1) and Jl.shape == (n, 1, 6)
        assert_parity(rl[:, 0], r_ref, "robustified residuals")
        assert_parity(Jl[:, 0, :], np.array([J_ref[i, 6 * kf[i]:6 * kf[i] + 6] for i in range(n)]), "local Jacobians")
        assert_parity(b.evaluate_local(st, 0.0, jacobians=False)[0][:, 0], r_ref, "robustified residuals alone")
        d = b.download()
        assert np.array_equal(d["p"], p) and np.array_equal(d["pa"], pa) and np.array_equal(d["kf_idx"], kf) and np.array_equal(d["weight"], w)
    finally:
        b.close(); st.close()
    bad_kf = kf.copy(); bad_kf[3] = -1
    bad_p = p.copy(); bad_p[5, 1] = np.nan
    bad_w = w.copy(); bad_w[9] = -1.0
    for args, kw in (((p, pa, pb, pc, bad_kf), {}), ((bad_p, pa, pb, pc, kf), {}), ((p, pa, pb, pc, kf), dict(weight=bad_w)),
                     ((p, pa, pb, pc, kf), dict(huber_a=np.full(n, np.inf)))):
        with pytest.raises(api.LvfError):
            api.lidar_pose_batch(ctx, *args, **kw)


# ------------------------------------------------------------------------------------------------ (b) the linearisation
@pytest.mark.parametrize("variant", ["sorted", "shuffled", "empty_keyframe", "constant_pose"])
def test_linearisation_against_the_dense_system(ctx, oracle, window5, variant):
    from lvio_fusion_amd import api
    w5 = window5
    cfg, pre = w5["cfg"], w5["pre"]
    n = len(w5["weight"])
    idx = np.arange(n)
    if variant == "shuffled":
        idx = np.random.default_rng(9).permutation(n)          # no wave shares one keyframe
    if variant == "empty_keyframe":
        idx = idx[w5["blocks"][4] != 2]
    blocks, weight, huber, lid = _subset(w5, idx)
    pc = np.zeros(5, bool); pc[1] = variant == "constant_pose"
    dev = Device(api, ctx, cfg, pre, blocks, weight, huber)
    try:
        if pc.any():
            dev.prob.set_pose_constant(1, True)
        opt = api.default_solver_options()
        state = lc.state_of_cfg(cfg)
        t = lw.trial_step(oracle, cfg, pre, state, lid, 1e4, {}, pose_const=pc if pc.any() else None)
        cost_without = lw.dense_system(oracle, cfg, pre, state, lw.empty_lidar())[2]
        assert t["cost_before"] > 1.01 * cost_without, "the planes must weigh in the cost"
        c = dev.prob.cost(opt)
        print(f"{variant}: cost dev {c:.12e} ref {t['cost_before']:.12e} rel {abs(c - t['cost_before']) / c:.2e}")
        assert abs(c - t["cost_before"]) <= 1e-9 * abs(c)
        gc, gl = dev.prob.gradient(opt)
        assert_parity(gc, t["g"][:75], "gradient (keyframe part)"); assert_parity(gl, t["g"][75:], "gradient (inverse depths)")
        got = dev.prob.lm_iteration(opt, 1e4, 2.0)
        S, rhs = dev.prob.reduced_system()
        S_ref, rhs_ref = lw.reduced(t["H"], t["g"], t["D"], 75)
        print(f"{variant}: S err {np.abs(S - S_ref).max() / np.abs(S_ref).max():.2e}")
        assert abs(got["cost_before"] - t["cost_before"]) <= 1e-8 * t["cost_before"]
        assert np.abs(S - S_ref).max() <= 1e-7 * np.abs(S_ref).max()
        assert_parity(rhs, rhs_ref, "rhs")
        assert got["accepted"] == (t["rho"] > 1e-3) and abs(got["cost_after"] - t["cost_after"]) <= 1e-6 * t["cost_after"]
        if pc.any():
            assert np.array_equal(dev.state()[0][1], cfg["poses"][1]), "the constant keyframe moved"
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (c) above kMaxStagedKf
def test_global_atomic_path_65_keyframes(ctx, oracle):
    """65 keyframes (kMaxStagedKf = 64: no LDS table, no staged poses), IMU and lidar blocks only, block order shuffled"""
    from lvio_fusion_amd import api
    n_kf = 65
    cfg = lc.imu_only(syn.config4_window(n_kf=n_kf, n_lm=8, n_prewindow=4, seed=77, imu_samples=3))
    pre = lc.preint(oracle, cfg)
    rng = np.random.default_rng(3)
    blocks = lc.plane_blocks(cfg["poses_true"], 12, rng)
    idx = rng.permutation(len(blocks[4]))
    idx[:128] = np.sort(idx[:128])                             # (two waves in keyframe order: uniform and mixed waves both occur)
    blocks = tuple(a[idx] for a in blocks)
    weight = np.full(len(idx), 30.0)
    lid = lw.make_lidar(*blocks, weight=weight, huber_a=0.5)
    dev = Device(api, ctx, cfg, pre, blocks, weight, np.full(len(idx), 0.5))
    try:
        opt = api.default_solver_options()
        J, r, cost = lw.dense_system(oracle, cfg, pre, lc.state_of_cfg(cfg), lid)
        g = J.T @ r
        gc, _ = dev.prob.gradient(opt)
        assert_parity(gc, g, "gradient")
        c = dev.prob.cost(opt)
        assert abs(c - cost) <= 1e-9 * cost
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (d) iterations and the solve
def _far_start(cfg, seed, rot_deg, trans, depth_noise=0.0):
    c, rng = dict(cfg), np.random.default_rng(seed)
    c["poses"] = syn.perturb_poses(cfg["poses"], rng, rot_deg, trans)
    c["inv_depth"] = cfg["inv_depth"] * (1 + rng.normal(0, depth_noise, cfg["inv_depth"].shape))
    return c


# the starts of the two solves: chosen on the reference alone, for rejected steps whose step quality is far from the threshold (rho of the
# ten trials, visual + IMU + lidar: 1.07 0.64 0.79 0.77 0.91 0.94 0.86 0.46 0.37 -0.50; IMU + lidar: -0.26 -0.12 0.37 -1.37 -0.65 0.60 0.92 1.03 1.41 1.64)
SOLVE_START = dict(visual_imu_lidar=(15, 90.0, 3.0, 0.4), imu_lidar=(13, 60.0, 3.0, 0.0))


@pytest.mark.parametrize("kind", ["visual_imu_lidar", "imu_lidar"])
def test_iterations_and_solve_against_the_reference_loop(ctx, oracle, window5, kind):
    """Five lvf_problem_lm_iteration calls chained through the radius and decrease factor each hands on, the third one a forced reject (a
    min_relative_decrease no step can reach, on both sides); then lvf_problem_solve from a far start whose reference loop rejects steps."""
    from lvio_fusion_amd import api
    w5 = window5
    pre, lid = w5["pre"], w5["lid"]
    trim = lc.imu_only if kind == "imu_lidar" else (lambda c: c)
    cfg = trim(_far_start(w5["cfg"], 12, 4.0, 0.4))
    dev = Device(api, ctx, cfg, pre, w5["blocks"], w5["weight"], w5["huber"])
    try:
        state, radius, dec, accepted = lc.state_of_cfg(cfg), 1e4, 2.0, []
        for it in range(5):
            opt = api.default_solver_options()
            mrd = 1e3 if it == 2 else 1e-3
            opt.min_relative_decrease = mrd
            # (lvf_problem_lm_iteration is a one-iteration solve: its Jacobi scaling is this linearisation's, hence the fresh {})
            t, state, r_next, d_next, acc = lw.lm_iteration(oracle, cfg, pre, state, lid, radius, dec, {}, min_relative_decrease=mrd)
            got = dev.prob.lm_iteration(opt, radius, dec)
            print(f"{kind} it {it}: radius {radius:.3e} cost {t['cost_before']:.6e} -> {t['cost_after']:.6e} rho {t['rho']:.3f} accepted {acc} (device {got['accepted']})")
            assert abs(got["cost_before"] - t["cost_before"]) <= 1e-8 * t["cost_before"]
            assert got["accepted"] == acc
            assert abs(got["cost_after"] - t["cost_after"]) <= 1e-6 * abs(t["cost_after"])
            assert abs(got["radius"] - r_next) <= 1e-5 * r_next and got["decrease_factor"] == d_next
            assert_state(dev.state(), state, f"it {it}")
            accepted.append(acc); radius, dec = r_next, d_next
        assert accepted == [True, True, False, True, True]
    finally:
        dev.close()
    seed, rot, trans, dn = SOLVE_START[kind]
    cfg = trim(_far_start(w5["cfg"], seed, rot, trans, dn))
    dev = Device(api, ctx, cfg, pre, w5["blocks"], w5["weight"], w5["huber"])
    try:
        opt = api.default_solver_options(); opt.max_num_iterations = 10
        ref, state = lw.lm_solve(oracle, cfg, pre, lc.state_of_cfg(cfg), lid, max_num_iterations=10)
        assert ref["num_unsuccessful_steps"] >= 1 and np.abs(ref["trace"][:, 5] - 1e-3).min() > 0.1, "the start is there for clear rejections"
        s = dev.prob.solve(opt)
        print(f"{kind} solve: {s.num_iterations} iterations ({s.why}), {s.num_successful_steps} accepted; reference {ref['num_iterations']} ({ref['why']}), {ref['num_successful_steps']}")
        assert (s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.why) == \
               (ref["num_iterations"], ref["num_successful_steps"], ref["num_unsuccessful_steps"], ref["why"])
        assert s.num_residual_blocks == len(cfg["tc"]["lm_idx"]) + len(cfg["tf"]["lm_idx"]) + len(cfg["po"]["kf_idx"]) + len(cfg["imu"]) + len(lid["kf"])
        assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-8 * ref["initial_cost"] and abs(s.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
        assert_state(dev.state(), state, "solve")
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ (e) the device-built batch
def _pair(rng, pose):
    """a small map on the three planes around `pose` and a scan of it taken from there (150 points in the body frame); every ninth scan
    point has no neighbour within the gate"""
    pts = []
    for n, d in lc.PLANES:
        a, b = lc._basis(n)
        foot = pose[4:] + (d - n @ pose[4:]) * n
        for _ in range(400):
            pts.append(foot + rng.uniform(-5, 5) * a + rng.uniform(-5, 5) * b)
    m = np.array(pts, np.float32)
    q_world = m[rng.choice(len(m), 150, replace=False)].astype(np.float64) + rng.normal(0, 0.03, (150, 3))
    q_world[::9] += 40.0                                       # far from every map point: these queries fail the gate
    q = syn.se3_apply(syn.se3_inv(pose), q_world).astype(np.float32)
    return m, q


def test_device_built_batch_equals_the_host_fed_one(ctx, oracle):
    from lvio_fusion_amd import api
    rng = np.random.default_rng(17)
    thr = 1.0
    hs, host = [], dict(p=[], pa=[], pb=[], pc=[], kf=[], w=[], a=[])
    kf_of, w_of, a_of = [1, 3], [1.0, 0.01], [0.0, 0.1]
    maps, scans = [], []
    try:
        for k in range(2):
            pose = np.array([0, 0, np.sin(0.05), np.cos(0.05), 0.3 + 0.1 * k, -0.2, 0.1])
            m, q = _pair(rng, pose)
            mp, sc = api.Map(ctx, m, thr), api.Scan(ctx, q)
            hs += [mp, sc]; maps.append(mp); scans.append(sc)
            if k == 0:
                with pytest.raises(api.LvfError):
                    api.lidar_pose_from_scans(ctx, [mp], [sc], [0])           # not searched yet
            api.knn3(mp, sc, pose, thr)
            idx, _, valid = sc.download()
            ok = valid > 0
            assert ok.sum() >= 100 and (~ok).sum() >= 10
            tri = [np.where(ok[:, None], m[np.where(ok, idx[:, j], 0), :3].astype(np.float64), 0.0) for j in range(3)]
            host["p"].append(q[:, :3].astype(np.float64)); host["pa"].append(tri[0]); host["pb"].append(tri[1]); host["pc"].append(tri[2])
            host["kf"].append(np.full(len(q), kf_of[k], np.int32)); host["w"].append(np.where(ok, w_of[k], 0.0)); host["a"].append(np.full(len(q), a_of[k]))
        dev = api.lidar_pose_from_scans(ctx, maps, scans, kf_of, weight=w_of, huber_a=a_of)
        cat = {k: np.concatenate(v) for k, v in host.items()}
        ref = api.lidar_pose_batch(ctx, cat["p"], cat["pa"], cat["pb"], cat["pc"], cat["kf"], weight=cat["w"], huber_a=cat["a"])
        hs += [dev, ref]
        assert dev.n == ref.n == 300
        a, b = dev.download(), ref.download()
        for key in ("p", "pa", "kf_idx", "weight", "huber_a"):
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
        assert np.array_equal(dev.normals().view(np.uint8), ref.normals().view(np.uint8)), "normals"
        assert dev.num_valid() == ref.num_valid() == int((cat["w"] > 0).sum())
        with pytest.raises(api.LvfError):
            api.lidar_pose_from_scans(ctx, maps, scans, [3, 1])                # not in keyframe order
        empty = api.Scan(ctx, np.zeros((0, 3), np.float32))                    # nothing to search: accepted, searched or not
        hs.append(empty)
        none = api.lidar_pose_from_scans(ctx, [maps[0]], [empty], [0])
        hs.append(none)
        assert none.n == 0 and none.num_valid() == 0
    finally:
        for h in hs:
            h.close()


# ------------------------------------------------------------------------------------------------ (f) the window
def test_window_with_lidar_scans_equals_the_hand_built_problem(ctx, oracle):
    """Window.set_lidar_scan on two keyframes, solve, slide past one of them, solve again: each solve equals a Problem built by hand from the
    same blocks (tests/test_gpu_window.py's bounds).  Landmarks are born from keyframe 1 on, so the slide past keyframe 0 converts no block."""
    from lvio_fusion_amd import api
    n_kf = 6
    cfg = syn.config4_window(n_kf=n_kf, n_lm=150, n_prewindow=0, seed=606, imu_samples=4)
    keep = cfg["tc"]["kf_idx"] >= 1
    remap = -np.ones(cfg["n_lm"], np.int64); remap[cfg["tc"]["lm_idx"][keep]] = np.arange(keep.sum())
    tc = {k: v[keep] for k, v in cfg["tc"].items()}; tc["lm_idx"] = remap[tc["lm_idx"]].astype(np.int32)
    keep_tf = remap[cfg["tf"]["lm_idx"]] >= 0
    tf = {k: v[keep_tf] for k, v in cfg["tf"].items()}; tf["lm_idx"] = remap[tf["lm_idx"]].astype(np.int32)
    n_lm = int(keep.sum())
    invd0 = cfg["inv_depth"][cfg["tc"]["lm_idx"][keep]]
    cam0, cam1 = cfg["cam0"], cfg["cam1"]
    pre = [oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]
    rng = np.random.default_rng(23)
    thr = 1.0
    win = api.Window(ctx, cam0, cam1, baseline=syn.baseline(), weak_visual_threshold=0)
    hs, scans = [], {}
    try:
        for t in range(n_kf):
            win.add_keyframe(100 + t, cfg["poses"][t], cfg["w_kf"][t])
            win.set_imu(100 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
            for i in np.nonzero(tc["kf_idx"] == t)[0]:
                win.add_landmark(5000 + int(tc["lm_idx"][i]), 100 + t, tc["left_ob"][i], tc["right_ob"][i], invd0[int(tc["lm_idx"][i])])
            for i in np.nonzero(tf["kf2_idx"] == t)[0]:
                win.add_observation(5000 + int(tf["lm_idx"][i]), 100 + t, tf["ob"][i])
        for k, (w, a) in ((0, (30.0, 0.0)), (4, (20.0, 0.5))):
            m, q = _pair(rng, cfg["poses_true"][k])
            mp, sc = api.Map(ctx, m, thr), api.Scan(ctx, q)
            api.knn3(mp, sc, cfg["poses"][k], thr)           # (associated at the estimate, as Mapping::Optimize does)
            hs += [mp, sc]; scans[k] = (mp, sc, w, a)
            win.set_lidar_scan(100 + k, mp, sc, w, a)
        assert win.lidar_count() == 300
        opt = api.default_solver_options(); opt.max_num_iterations = 4
        for first in (0, 1):
            if first:
                win.slide(100 + first)
                assert win.lidar_count() == 150
            act = list(range(first, n_kf))
            poses = np.array([win.pose(100 + t) for t in act]); imu = [win.imu(100 + t) for t in act]
            invd = np.array([win.inv_depth(5000 + l) for l in range(n_lm)])
            s_win = win.solve(opt)
            assert win.counts()["prior"] == 0 and win.counts()["po"] == 0 and win.counts()["imu"] == len(act) - 1
            st = api.State(ctx, len(act), n_lm)
            for field, v in ((api.POSES, poses), (api.VEL, np.array([x[0] for x in imu])), (api.BA, np.array([x[1] for x in imu])),
                             (api.BG, np.array([x[2] for x in imu])), (api.INV_DEPTH, invd), (api.W_VISUAL, cfg["w_kf"][act])):
                st.set(field, v)
            btc = api.two_camera_batch(ctx, cam0, cam1, tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"] - first)
            btc.set_block_weights((np.float32(5) * cfg["w_kf"][tc["kf_idx"]].astype(np.float32)).astype(np.float64))
            btf = api.two_frame_batch(ctx, cam0, cam1, tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"] - first, tf["kf2_idx"] - first)
            bim = api.imu_batch(ctx, np.stack(pre[first:]), [f["kf_i"] - first for f in cfg["imu"][first:]], [f["kf_j"] - first for f in cfg["imu"][first:]])
            sel = [k for k in sorted(scans) if k >= first]
            bl = api.lidar_pose_from_scans(ctx, [scans[k][0] for k in sel], [scans[k][1] for k in sel], [k - first for k in sel],
                                           weight=[scans[k][2] for k in sel], huber_a=[scans[k][3] for k in sel])
            prob = api.Problem(ctx, st, btc, btf, None, bim)
            prob.set_lidar_planes(bl)
            s_ref = prob.solve(opt)
            print(f"window from keyframe {first}: cost {s_win.initial_cost:.6e} -> {s_win.final_cost:.6e}; problem {s_ref.initial_cost:.6e} -> {s_ref.final_cost:.6e}")
            assert abs(s_win.initial_cost - s_ref.initial_cost) <= 1e-8 * abs(s_ref.initial_cost) + 1e-12
            assert abs(s_win.final_cost - s_ref.final_cost) <= 1e-6 * abs(s_ref.final_cost) + 1e-12
            assert s_win.num_successful_steps == s_ref.num_successful_steps and s_win.num_residual_blocks == s_ref.num_residual_blocks
            assert s_win.num_residual_blocks == len(tc["lm_idx"]) + len(tf["lm_idx"]) + len(act) - 1 + 150 * len(sel)
            P = st.get(api.POSES).reshape(-1, 7)
            for i, t in enumerate(act):
                assert_parity(win.pose(100 + t), P[i], f"from {first}: pose {t}")
            prob.close()
            for h in (btc, btf, bim, bl, st):
                h.close()
        win.set_lidar_planes(104, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
        assert win.lidar_count() == 0
        s = win.solve(opt)
        assert s.num_residual_blocks == len(tc["lm_idx"]) + len(tf["lm_idx"]) + n_kf - 2
    finally:
        win.close()
        for h in hs:
            h.close()


# ------------------------------------------------------------------------------------------------ (g) the marginal
def test_marginal_with_lidar_rows(ctx, oracle, window5):
    """lvf_problem_marginal of the newest keyframe with the batch attached against tests/marginal_ref.py on the numpy dense system with the
    lidar rows: the tolerance of tests/test_gpu_marginal_window.py (the measured distance of a device assembly from the reference system,
    twice, propagated through the case, plus M float64 floors)."""
    from lvio_fusion_amd import api
    from tests import marginal_ref as mr
    from tests.test_gpu_marginal import M
    from tests.test_gpu_marginal_window import RADIUS_TRUTH, sym
    w5 = window5
    cfg, pre = w5["cfg"], w5["pre"]
    def system(lid):
        t = lw.trial_step(oracle, cfg, pre, lc.state_of_cfg(cfg), lid, RADIUS_TRUTH, {})
        return sym(lw.reduced(t["H"], t["g"], t["D"], 75)[0])

    S, S_without = system(w5["lid"]), system(lw.empty_lidar())
    dev, twin = (Device(api, ctx, cfg, pre, w5["blocks"], w5["weight"], w5["huber"]) for _ in range(2))
    try:
        opt = api.default_solver_options()
        twin.prob.lm_iteration(opt, RADIUS_TRUTH)
        delta = float(np.abs(sym(twin.prob.reduced_system()[0]) - S).max() / np.abs(S).max())
        assert delta <= 1e-7
        sel = mr.kf_selection(5, [4])
        ref = mr.marginal(S, sel)
        assert ref["fail"] == 0
        keep = mr.layout(S, sel)[1][[int(s) for s in sel]]
        loose = mr.propagated(S, sel, ref, 1e-7)
        tight = [a + M * max(e, 75 * 2.0 ** -53) for a, e in zip(mr.propagated(S, sel, ref, 2.0 * delta + 2.0 ** -52), mr.err64_bound(S, sel, ref, 5))]
        info, cov, st = dev.prob.marginal(opt, [4])
        assert st["fail"] == 0
        e = mr.errors(info, cov, ref, keep)
        e_without = mr.errors(info, cov, mr.marginal(S_without, sel), keep)
        print(f"marginal with lidar rows: delta {delta:.3e} err info {e[0]:.3e} cov {e[1]:.3e} | tol(1e-7) {loose[0]:.3e} {loose[1]:.3e} | tol(measured) {tight[0]:.3e} {tight[1]:.3e}"
              f" | against the system without the rows {e_without[0]:.3e} {e_without[1]:.3e}")
        assert e[0] <= loose[0] and e[1] <= loose[1] and e[0] <= tight[0] and e[1] <= tight[1]
        assert e_without[0] > 100 * tight[0], "the lidar rows must show in the marginal"
    finally:
        dev.close(); twin.close()


# ------------------------------------------------------------------------------------------------ (h) nothing else moved
def test_attach_then_detach_leaves_the_problem_as_it_was(ctx, oracle, window5):
    """Attach a batch, detach it with NULL, solve: summary, state and launch counts equal those of a problem never touched, as closely as
    solves of untouched problems equal each other — bit for bit when those are; otherwise within 2 times the largest mutual difference of
    three untouched solves (the touched solve is a fourth draw of the same run-to-run noise, and the largest of three differences among three
    draws is itself a draw: a factor of 1 would fail a correct library about one time in four)."""
    from lvio_fusion_amd import api
    w5 = window5
    cfg, pre = w5["cfg"], w5["pre"]
    opt = api.default_solver_options(); opt.max_num_iterations = 6

    def run(touch):
        dev = Device(api, ctx, cfg, pre)
        try:
            if touch:
                b = api.lidar_pose_batch(ctx, *w5["blocks"], weight=w5["weight"], huber_a=w5["huber"])
                dev.prob.set_lidar_planes(b)
                assert dev.prob.cost(opt) > 0
                dev.prob.set_lidar_planes(None)
                b.close()
            s = dev.prob.solve(opt)
            state = np.concatenate([np.asarray(x).ravel() for x in dev.state()])
            for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
                dev.st.set(field, cfg[key])
            launches = [la for _, _, la in dev.prob.stage_times(opt, reps=2)]
            return (s.num_iterations, s.num_successful_steps, s.num_residual_blocks, s.why), np.array([s.initial_cost, s.final_cost]), state, launches
        finally:
            dev.close()

    plain = [run(False) for _ in range(3)]
    got = run(True)
    assert all(p[0] == got[0] for p in plain) and all(p[3] == got[3] for p in plain), "summary or launch counts changed"
    for q, name in ((1, "costs"), (2, "state")):
        spread = max(np.abs(a[q] - b[q]).max() for a in plain for b in plain)
        diff = max(np.abs(got[q] - a[q]).max() for a in plain)
        print(f"attach / detach, {name}: untouched solves differ by {spread:.3e}, the touched one by {diff:.3e}")
        assert diff == 0.0 if spread == 0.0 else diff <= 2.0 * spread
