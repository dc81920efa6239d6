"""The window's dense prior and the marginalising slide (lvf_window_set_dense_prior, lvf_window_get_dense_prior, lvf_window_slide_marginalize).

Exact composition is the property that defines the feature: with no block dropped by the rule (no landmarks, no weak-constraint prior), the
reduced system of the window after a marginalising slide IS the Schur complement of the window before it over the departed keyframes'
unknowns.  The reference is that Schur complement of the device's own 75-unknown system in long double; the bound is the one of
lvf_problem_marginal_prior (tests/test_gpu_dense_prior.py): what two device assemblies of a system may differ by, propagated through the
case, plus M float64 floors taken over elimination orders — no free tolerance.

With landmarks the rule drops blocks on purpose, so the reference is the rule itself: tests/window_ref.py's assembly of a mirror holding the
departing keyframes and the first kept one without its observations, as a hand-built problem."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import dense_prior_ref as dp
from tests import lidar_window_cases as lc
from tests.test_gpu_marginal import M

pytestmark = pytest.mark.gpu
RADIUS_TRUTH = 1e16
ID0 = 100


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _pre(oracle, cfg):
    return [oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]


def _fill(win, cfg, pre, with_landmarks):
    tc, tf = cfg["tc"], cfg["tf"]
    for t in range(cfg["n_kf"]):
        win.add_keyframe(ID0 + t, cfg["poses"][t], cfg["w_kf"][t])
        win.set_imu(ID0 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
        if not with_landmarks:
            continue
        for i in np.nonzero(tc["kf_idx"] == t)[0]:
            win.add_landmark(5000 + int(tc["lm_idx"][i]), ID0 + t, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][int(tc["lm_idx"][i])])
        for i in np.nonzero(tf["kf2_idx"] == t)[0]:
            win.add_observation(5000 + int(tf["lm_idx"][i]), ID0 + t, tf["ob"][i])


def _x_of(win, kf_id):
    v, a, g = win.imu(kf_id)
    return np.concatenate([win.pose(kf_id), v, a, g])


class Hand:
    """a problem built by hand over keyframes `ids` of a window at its current state: ImuError blocks between consecutive ones (pre[t - 1]
    ends at keyframe t), lidar plane blocks per keyframe, optional visual blocks, optional dense prior"""

    def __init__(self, api, ctx, win, ids, pre, planes, prior=None, visual=None, n_lm=0, inv_depth=None, w_kf=None, cams=None, win_imu=None):
        self.h = []
        n = len(ids)
        st = api.State(ctx, n, n_lm)
        x = np.array([_x_of(win, i) for i in ids])
        for f, v in ((api.POSES, x[:, :7]), (api.VEL, x[:, 7:10]), (api.BA, x[:, 10:13]), (api.BG, x[:, 13:16])):
            st.set(f, v)
        if w_kf is not None:
            st.set(api.W_VISUAL, w_kf)
        if n_lm:
            st.set(api.INV_DEPTH, inv_depth)
        pairs = [(k - 1, k) for k in range(1, n) if ids[k] - ids[k - 1] == 1]
        bim = api.imu_batch(ctx, np.stack([pre[ids[j] - ID0 - 1] for _, j in pairs]), [i for i, _ in pairs], [j for _, j in pairs]) if pairs else None
        btc = btf = bpo = None
        if visual:
            tc, tf, po = visual
            if len(tc["kf"]):
                btc = api.two_camera_batch(ctx, cams[0], cams[1], tc["left"], tc["right"], tc["lm"], tc["kf"])
                btc.set_block_weights(tc["w"])
            if len(tf["k2"]):
                btf = api.two_frame_batch(ctx, cams[0], cams[1], tf["first"], tf["ob"], tf["lm"], tf["k1"], tf["k2"])
            if len(po["kf"]):
                bpo = api.pose_only_batch(ctx, cams[0], po["ob"], po["kf"], np.arange(len(po["kf"]), dtype=np.int32), po["pw"])
        self.prob = api.Problem(ctx, st, btc, btf, bpo, bim)
        sel = [k for k in range(n) if ids[k] in planes]
        bl = None
        if sel:
            blocks = [np.concatenate([planes[ids[k]][0][q] for k in sel]) for q in range(4)]
            kf = np.concatenate([np.full(len(planes[ids[k]][0][0]), k, np.int32) for k in sel])
            bl = api.lidar_pose_batch(ctx, *blocks, kf, weight=np.concatenate([planes[ids[k]][1] for k in sel]), huber_a=np.concatenate([planes[ids[k]][2] for k in sel]))
            self.prob.set_lidar_planes(bl)
        self.dp = None
        if prior is not None:
            self.dp = api.DensePrior(ctx, [list(ids).index(int(i)) for i in prior["kf_ids"]], prior["x0"], prior["info"], prior["eta"], prior["c0"])
            self.prob.set_dense_prior(self.dp)
        self.st = st
        self.h = [b for b in (btc, btf, bpo, bim, bl, self.dp, st) if b is not None]
        # the same visual and ImuError blocks in the layout tests/lidar_window_ref.py's dense system reads (for the landmarks' H_ll)
        self.ref = None
        if visual and n_lm:
            tc, tf, po = visual
            e2, ei = np.zeros((0, 2)), np.zeros(0, np.int32)
            imu = []
            for i, j in pairs:
                f = dict(win_imu[ids[j] - ID0 - 1]); f["kf_i"], f["kf_j"] = i, j
                imu.append(f)
            cfg = dict(cam0=cams[0], cam1=cams[1], n_kf=n, n_lm=n_lm, w_kf=np.asarray(w_kf, np.float64), imu=imu,
                       tc=dict(left_ob=tc["left"], right_ob=tc["right"], lm_idx=tc["lm"], kf_idx=tc["kf"]),
                       tf=dict(first_ob=tf["first"], ob=tf["ob"], lm_idx=tf["lm"], kf1_idx=tf["k1"], kf2_idx=tf["k2"]),
                       po=dict(ob=po["ob"] if len(po["kf"]) else e2, kf_idx=po["kf"] if len(po["kf"]) else ei,
                               pw_idx=np.arange(len(po["kf"]), dtype=np.int32), pw=po["pw"] if len(po["kf"]) else np.zeros((1, 3))))
            self.ref = (cfg, np.stack([pre[ids[j] - ID0 - 1] for _, j in pairs]), [x[:, :7], x[:, 7:10], x[:, 10:13], x[:, 13:16], np.asarray(inv_depth, np.float64)])

    def system(self, api, oracle=None):
        """(S symmetric, g = -rhs, c) of the undamped reduced system (radius 1e16: below one rounding of the diagonal); c is the cost less
        the landmarks' share 1/2 sum g_l^2 / H_ll, formed as tests/test_gpu_dense_prior.py forms it: the device's landmark gradient, H_ll
        from the numpy reference's dense system of the same blocks (self.c_full keeps the cost itself)"""
        from tests import lidar_window_ref as lw
        opt = api.default_solver_options()
        c = self.c_full = self.prob.cost(opt)
        if self.st.n_lm:
            cfg, p, state = self.ref
            J = lw.dense_system(oracle, cfg, p, state, lw.empty_lidar())[0]
            gl = self.prob.gradient(opt)[1]
            c = c - 0.5 * float((gl ** 2 / (J[:, 15 * self.st.n_kf:] ** 2).sum(axis=0)).sum())
        keep = [self.st.get(f) for f in (api.POSES, api.VEL, api.BA, api.BG)]
        self.prob.lm_iteration(opt, RADIUS_TRUTH)
        S, rhs = self.prob.reduced_system()
        for f, v in zip((api.POSES, api.VEL, api.BA, api.BG), keep):      # (the iteration may have moved the state)
            self.st.set(f, v)
        return np.tril(S) + np.tril(S, -1).T, -rhs, c

    def close(self):
        self.prob.close()
        for b in self.h:
            b.close()


def _planes(cfg, rng, kfs, per_kf=40):
    """per keyframe id: ((p, pa, pb, pc), weight, huber): half the blocks beyond a Huber threshold near the median residual"""
    out = {}
    for k in kfs:
        p, pa, pb, pc, _ = lc.plane_blocks(cfg["poses_true"], per_kf, rng, kfs=[k])
        out[ID0 + k] = ((p, pa, pb, pc), np.where(np.arange(per_kf) % 2 == 0, 100.0, 200.0), np.where(np.arange(per_kf) % 2 == 1, 0.5, 0.0))
    return out


def _window(api, ctx, cfg, pre, planes, with_landmarks, thr=0):
    win = api.Window(ctx, cfg["cam0"], cfg["cam1"], baseline=syn.baseline(), weak_visual_threshold=thr)
    _fill(win, cfg, pre, with_landmarks)
    for kid, (blocks, w, a) in planes.items():
        win.set_lidar_planes(kid, *blocks, weight=w, huber_a=a)
    return win


def _blocks(win):
    return [tuple(x.copy() for x in win.debug_blocks(kind)) for kind in range(5)]


# ------------------------------------------------------------------------------------------------ exact composition
def test_slide_marginalize_is_the_schur_complement_of_the_window(ctx, oracle):
    """5 keyframes, ImuError and lidar plane blocks only (no landmarks; weak_visual_threshold = 0: no weak-constraint prior), an earlier
    dense prior on keyframe 0.  slide_marginalize to keyframe 2: system, right-hand side and cost constant of the new 3-keyframe window
    equal the Schur complement of the old 75-unknown system over the 30 unknowns of keyframes 0 and 1; the next solve's block lists equal
    those after a plain slide; the old prior is gone with its keyframe."""
    from lvio_fusion_amd import api
    n_kf = 5
    cfg = lc.imu_only(syn.config4_window(n_kf=n_kf, n_lm=8, n_prewindow=4, seed=909, imu_samples=4))
    pre = _pre(oracle, cfg)
    rng = np.random.default_rng(21)
    planes = _planes(cfg, rng, range(n_kf))
    ids = [ID0 + t for t in range(n_kf)]
    win, twin = (_window(api, ctx, cfg, pre, planes, False) for _ in range(2))
    hs = []
    try:
        A = 30.0 * rng.normal(size=(20, 15)); b = rng.normal(size=20)
        x0 = dp.state_plus(_x_of(win, ID0)[None, :], 0.02 * rng.normal(size=15))
        old = dict(kf_ids=np.array([ID0]), x0=x0, info=A.T @ A, eta=A.T @ b, c0=0.5 * float(b @ b) + 0.1)
        win.set_dense_prior(old["kf_ids"], old["x0"], old["info"], old["eta"], old["c0"])
        got = win.get_dense_prior()
        assert np.array_equal(got["kf_ids"], old["kf_ids"]) and np.array_equal(got["info"], old["info"]) and np.array_equal(got["x0"], old["x0"]) and got["c0"] == old["c0"]
        before = Hand(api, ctx, win, ids, pre, planes, prior=old); hs.append(before)
        S, g, c = before.system(api)
        kept = dp.natural_index(n_kf, [2, 3, 4])
        # natural order of the 3-keyframe window: [poses of 2, 3, 4 | (v, ba, bg) of 2, 3, 4]
        order = np.concatenate([[6 * k + t for k in (2, 3, 4) for t in range(6)], [6 * n_kf + 9 * k + t for k in (2, 3, 4) for t in range(9)]])
        ri, re, rc0 = dp.marginal_prior(S, g, c, order)
        A_star = dp.augmented(ri, re, rc0)
        opt = api.default_solver_options()
        st = win.slide_marginalize(ID0 + 2, opt)
        assert st["fail"] == 0 and st["n_present"] == 45 and win.counts()["kf"] == 3
        new = win.get_dense_prior()
        assert list(new["kf_ids"]) == [ID0 + 2] and np.array_equal(new["x0"][0], _x_of(win, ID0 + 2)) and new["c0"] >= 0.0
        after = Hand(api, ctx, win, ids[2:], pre, planes, prior=new); hs.append(after)
        S2, g2, c2 = after.system(api)
        n_blocks = 4 + sum(len(v[1]) for v in planes.values()) + 1
        tol = dp.propagated(S, g, c, order, A_star, n_blocks * 2.0 ** -53 + 2.0 ** -52)
        floor = M * max(dp.err64_bound(S, g, c, order, A_star, 5), 76 * 2.0 ** -53)
        err = dp.aug_err(dp.augmented(S2, g2, c2), A_star)
        plain = Hand(api, ctx, win, ids[2:], pre, planes); hs.append(plain)
        err_plain = dp.aug_err(dp.augmented(*plain.system(api)), A_star)
        print(f"composition: err {err:.3e} <= propagated {tol:.3e} + floor {floor:.3e}; a plain slide is {err_plain:.3e} away; c {c:.6e} -> c0 {new['c0']:.6e}, cost after {c2:.6e}")
        assert err <= tol + floor
        assert err_plain > 1e3 * (tol + floor), "the scene must tell a marginalising slide from a plain one"
        assert kept.size == 45
        # block lists of the next solve: those of a plain slide
        twin.slide(ID0 + 2)
        o0 = api.default_solver_options(); o0.max_num_iterations = 0
        s1, s2 = win.solve(o0), twin.solve(o0)
        for a, b2 in zip(_blocks(win), _blocks(twin)):
            assert np.array_equal(a[0], b2[0]) and np.array_equal(a[1], b2[1])
        assert s1.num_residual_blocks == s2.num_residual_blocks + 1 and abs(s1.initial_cost - c2) <= 1e-9 * c2
        # no departing keyframe: nothing happens; no kept keyframe: an error, the window untouched; a plain slide past the prior drops it
        assert win.slide_marginalize(ID0 + 2, opt)["n_present"] == 0 and win.counts()["kf"] == 3 and win.get_dense_prior() is not None
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            win.slide_marginalize(ID0 + 9, opt)
        assert win.counts()["kf"] == 3
        win.slide(ID0 + 3)
        assert win.get_dense_prior() is None
    finally:
        for h in hs:
            h.close()
        win.close(); twin.close()


# ------------------------------------------------------------------------------------------------ with landmarks
def _rule(win, cfg, ids_sub, drop):
    """The sub-problem's visual blocks from tests/window_ref.py's assembly (the numpy restatement of the window's tick) of a mirror that holds
    the departing keyframes and the first kept one, the latter WITHOUT its observations: the rule of lvf_window_slide_marginalize.  The mirror
    is made from the scene and from what the window says of its state (poses, inverse depths; a landmark whose birth keyframe has departed
    is frozen at that keyframe's last pose)."""
    from tests import window_ref as wr
    tc, tf = cfg["tc"], cfg["tf"]
    D = ids_sub[:drop]
    birth = np.zeros(cfg["n_lm"], np.int64); birth[tc["lm_idx"]] = ID0 + tc["kf_idx"]
    right = np.zeros((cfg["n_lm"], 2)); right[tc["lm_idx"]] = tc["right_ob"]
    okf, olm, oxy = [], [], []
    for k, kid in enumerate(D):
        for i in np.nonzero(tc["kf_idx"] == kid - ID0)[0]:
            okf.append(k); olm.append(int(tc["lm_idx"][i])); oxy.append(tc["left_ob"][i])
        for i in np.nonzero(tf["kf2_idx"] == kid - ID0)[0]:
            okf.append(k); olm.append(int(tf["lm_idx"][i])); oxy.append(tf["ob"][i])
    rows = sorted(set(olm))
    row_of = {l: r for r, l in enumerate(rows)}
    invd = np.array([win.inv_depth(5000 + l) for l in rows])
    fixed = np.array([birth[l] < ids_sub[0] for l in rows], bool)
    pw = np.zeros((len(rows), 3))
    for r, l in enumerate(rows):
        if fixed[r]:
            pw[r] = wr.to_world(cfg["cam1"], right[l], invd[r], win.pose(int(birth[l])))[0]
    n = len(ids_sub)
    kf = dict(id=ids_sub, pose=np.array([win.pose(i) for i in ids_sub]), w_visual=[cfg["w_kf"][i - ID0] for i in ids_sub], good_imu=[True] * n,
              has_pre=[False] + [True] * (n - 1))
    lm = dict(id=[5000 + l for l in rows], index=rows, birth=birth[rows], right_ob=right[rows], inv_depth=invd, fixed=fixed, pw=pw)
    out = wr.assemble(cfg["cam0"], cfg["cam1"], syn.baseline(), 0, kf, lm, dict(kf=okf, lm=[row_of[l] for l in olm], xy=np.array(oxy).reshape(-1, 2)))
    f = out["flat"]
    assert out["counts"]["imu"] == n - 1 and out["counts"]["prior"] == 0
    return (dict(lm=f["tc"]["lm"], kf=f["tc"]["kf"], left=f["tc"]["left_ob"], right=f["tc"]["right_ob"], w=f["tc"]["weight"]),
            dict(lm=f["tf"]["lm"], k1=f["tf"]["kf1"], k2=f["tf"]["kf2"], first=f["tf"]["first_ob"], ob=f["tf"]["ob"]),
            dict(kf=f["po"]["kf"], ob=f["po"]["ob"], pw=f["po"]["pw"]), f["inv_depth"])


@pytest.mark.parametrize("drop", [1, 2])
def test_slide_marginalize_with_landmarks_follows_the_rule(ctx, oracle, drop):
    """6 keyframes, 60 landmarks, lidar planes on keyframes 0 and 2; slide by `drop`, then by one more on top: the device's prior
    (get_dense_prior) against the hand-built sub-problem whose visual blocks come from tests/window_ref.py's assembly of the rule's mirror,
    eliminated in long double; the first prior must enter the second."""
    from lvio_fusion_amd import api
    n_kf = 6
    cfg = syn.config4_window(n_kf=n_kf, n_lm=60, n_prewindow=0, seed=808, imu_samples=4)
    pre = _pre(oracle, cfg)
    rng = np.random.default_rng(4)
    planes = _planes(cfg, rng, [0, 2])
    win = _window(api, ctx, cfg, pre, planes, True)
    opt = api.default_solver_options()
    o0 = api.default_solver_options(); o0.max_num_iterations = 0
    ids = [ID0 + t for t in range(n_kf)]
    first_prior = None
    try:
        for step, d in enumerate((drop, 1)):
            win.solve(o0)                                                  # the block lists at the current state
            blocks = _blocks(win)
            assert len(blocks[4][0]) == 0, "no weak-constraint prior in this scene"
            ids_sub = ids[:d + 1]
            tc, tf, po, invd = _rule(win, cfg, ids_sub, d)
            assert len(tc["kf"]) > 0 and (step == 0 or len(po["kf"]) > 0), "TwoCamera blocks, and PoseOnly blocks of frozen landmarks on the second slide"
            if d == 2:
                assert len(tf["k2"]) > 0
            prior = win.get_dense_prior()
            assert (prior is None) == (step == 0)
            hand = Hand(api, ctx, win, ids_sub, pre, {k: v for k, v in planes.items() if k in ids_sub[:d]}, prior=prior, visual=(tc, tf, po), n_lm=len(invd),
                        inv_depth=invd, w_kf=np.array([cfg["w_kf"][i - ID0] for i in ids_sub]), cams=(cfg["cam0"], cfg["cam1"]), win_imu=cfg["imu"])
            try:
                ri, re, rc0, rst = hand.prob.marginal_prior(opt, [d])
                assert rst["fail"] == 0
                S, g, c = hand.system(api, oracle)
                sel = dp.natural_index(d + 1, [d])
                A_star = dp.augmented(*dp.marginal_prior(S, g, c, sel))
                n_blocks = len(tc["kf"]) + len(tf["k2"]) + len(po["kf"]) + d + 80 + 1
                tol = dp.propagated(S, g, c, sel, A_star, n_blocks * 2.0 ** -53 + 2.0 ** -52) + M * max(dp.err64_bound(S, g, c, sel, A_star, 9), (15 * (d + 1) + 1) * 2.0 ** -53)
                # the landmarks' share of the constant (tests/test_gpu_dense_prior.py: 1e-9 c / c0*), and the TwoCamera weight: the window forms
                # 5 w_visual as a FLOAT product (the reference's arithmetic), the numpy dense system in double — one float rounding of a weight,
                # 2^-24, twice in H_ll, on a share that is at most c
                tol += (1e-9 + 2.0 ** -23) * hand.c_full / float(A_star[-1, -1] / 2)
                st = win.slide_marginalize(ids[d], opt)
                got = win.get_dense_prior()
                assert st["fail"] == 0 and list(got["kf_ids"]) == [ids[d]]
                err = dp.aug_err(dp.augmented(got["info"], got["eta"], got["c0"]), A_star)
                err_hand = dp.aug_err(dp.augmented(ri, re, rc0), A_star)
                print(f"drop {drop} step {step}: window prior err {err:.3e}, hand-built problem's {err_hand:.3e}, tol {tol:.3e}; blocks tc {len(tc['kf'])} tf {len(tf['k2'])} po {len(po['kf'])}")
                assert err <= tol and err_hand <= tol
                if step == 1:
                    hand.prob.set_dense_prior(None)
                    wi, we, wc, _ = hand.prob.marginal_prior(opt, [d])
                    assert dp.aug_err(dp.augmented(wi, we, wc), A_star) > 1e3 * tol, "the first prior must enter the second"
            finally:
                hand.close()
            ids = ids[d:]
            first_prior = got
        # the window solves on with its prior
        s = win.solve(opt)
        assert s.termination in (0, 1) and s.final_cost <= s.initial_cost and win.get_dense_prior() is not None and first_prior is not None
    finally:
        win.close()


# ------------------------------------------------------------------------------------------------ argument errors
def test_window_prior_argument_errors(ctx, oracle):
    from lvio_fusion_amd import api
    cfg = lc.imu_only(syn.config4_window(n_kf=3, n_lm=8, n_prewindow=4, seed=11, imu_samples=3))
    win = _window(api, ctx, cfg, _pre(oracle, cfg), {}, False)
    try:
        x0 = np.zeros((9, 16)); x0[:, 3] = 1.0
        info = np.eye(135)
        ids = [ID0, ID0 + 1, ID0 + 2]
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            win.set_dense_prior(list(range(ID0, ID0 + 9)), x0, info)                 # more than 8
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            win.set_dense_prior([ID0, ID0], x0[:2], info[:30, :30])                   # listed twice
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            win.set_dense_prior([ID0 + 7], x0[:1], info[:15, :15])                    # not in the window
        for bad in ("info", "eta", "x0"):
            a = dict(x0=x0[:1].copy(), info=info[:15, :15].copy(), eta=np.zeros(15))
            a[bad].flat[5 if bad != "info" else 15 * 5 + 2] = np.nan
            with pytest.raises(api.LvfError, match="lvf error 1:"):
                win.set_dense_prior([ID0], a["x0"], a["info"], a["eta"])
        assert win.get_dense_prior() is None
        win.set_dense_prior(ids[1:], x0[:2], info[:30, :30])
        with pytest.raises(api.LvfError, match="lvf error 1:"):
            win.slide_marginalize(ID0 + 1, api.default_solver_options())              # the prior reaches beyond the first kept keyframe
        assert win.counts()["kf"] == 3
        win.set_dense_prior(None)
        assert win.get_dense_prior() is None
    finally:
        win.close()


# ------------------------------------------------------------------------------------------------ the benefit, stated not tuned
def _run_device(api, ctx, sc, pre, marginalize):
    from tests import slide_benefit_ref as sb
    base = sc["base"]
    win = api.Window(ctx, base["cam0"], base["cam1"], baseline=syn.baseline(), weak_visual_threshold=0)
    opt = api.default_solver_options()
    opt.max_num_iterations = sb.ITERATIONS
    opt.function_tolerance = opt.gradient_tolerance = opt.parameter_tolerance = 0.0
    z3 = np.zeros(3)

    def add(k, ba, bg):
        win.add_keyframe(ID0 + k, sc["poses0"][k], base["w_kf"][k])
        win.set_imu(ID0 + k, sc["vel0"][k], ba, bg, pre[k - 1] if k > 0 else None)
        win.set_lidar_planes(ID0 + k, *sc["planes"][k], weight=np.full(sb.PER_KF, sb.PLANE_WEIGHT))

    try:
        for k in range(sb.WINDOW - 1):
            add(k, z3, z3)
        for t in range(sb.TICKS):
            new = sb.WINDOW - 1 + t
            _, ba, bg = win.imu(ID0 + new - 1)
            add(new, ba, bg)
            s = win.solve(opt)
            assert s.num_iterations == sb.ITERATIONS
            if marginalize:
                assert win.slide_marginalize(ID0 + new - 1, opt)["fail"] == 0
            else:
                win.slide(ID0 + new - 1)
        return _x_of(win, ID0 + sb.N_KF - 1), win.get_dense_prior()
    finally:
        win.close()


def test_marginalising_slide_keeps_the_bias_and_velocity_better(ctx, oracle):
    """tests/slide_benefit_ref.py's drive (a gyroscope bias the estimator does not know, a window of three keyframes, ten ticks) on the
    device: both runs equal the reference's (the bound of every state comparison here, helpers.assert_parity per field), and the
    marginalising run's error of the newest keyframe's bg and v is below the plain run's by the factor the REFERENCE shows, less 1e-3 of it
    for rounding.  Reference figures (seed 2024, the scene's default; seeds 7 and 99 give 1.46 / 1.33 and 3.71 / 1.31):
    |bg - truth| 1.83e-3 rad/s plain, 4.94e-4 marginalising (3.71 x); |v - truth| 0.0728 m/s plain, 0.0509 marginalising (1.43 x)."""
    from lvio_fusion_amd import api
    from tests import slide_benefit_ref as sb
    from tests.helpers import assert_parity
    sc = sb.scene()
    pre = sb.preintegrations(oracle, sc)
    out = {}
    for marg in (False, True):
        x_ref, prior_ref = sb.run_reference(oracle, sc, marg)
        x_dev, prior_dev = _run_device(api, ctx, sc, pre, marg)
        e_ref, e_dev = sb.errors(sc, x_ref), sb.errors(sc, x_dev)
        print(f"marginalize {marg}: reference |dbg| {e_ref[0]:.6e} |dv| {e_ref[1]:.6e}; device {e_dev[0]:.6e} {e_dev[1]:.6e}; max |x_dev - x_ref| {np.abs(x_dev - x_ref).max():.3e}")
        for name, a, b in (("pose", 0, 7), ("v", 7, 10), ("ba", 10, 13), ("bg", 13, 16)):
            assert_parity(x_dev[a:b], x_ref[a:b], f"marginalize {marg}: {name} of the newest keyframe")
        assert (prior_dev is None) == (not marg)
        if marg:
            assert list(prior_dev["kf_ids"]) == [ID0 + prior_ref["kf"]]
        out[marg] = (e_ref, e_dev)
    for q, name in ((0, "bg"), (1, "v")):
        factor_ref = out[False][0][q] / out[True][0][q]
        factor_dev = out[False][1][q] / out[True][1][q]
        print(f"{name}: the reference's factor {factor_ref:.4f}, the device's {factor_dev:.4f}")
        assert factor_ref > 1.0, "the scene must show a benefit on the reference"
        assert factor_dev >= factor_ref * (1.0 - 1e-3)
