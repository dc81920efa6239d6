"""The persistent sliding window (lvf_window_*) replayed tick by tick over a synthetic drive, against the
same ticks assembled FROM SCRATCH each time with Backend::BuildProblem's rules (src/lvio_fusion/src/backend.cpp:96-183) in
python and solved through the flat batch API.  Both run the same kernels, so the comparison pins the incremental
bookkeeping: block sets and order, TwoFrame -> PoseOnly conversion when a birth frame leaves, the Far / weak-prior rule."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu


def to_world(right, rob, inv_depth, pose):
    d = 1.0 / inv_depth
    ps = np.array([(rob[0] - right["cx"]) * d / right["fx"], (rob[1] - right["cy"]) * d / right["fy"], d])
    return syn.se3_apply(pose, syn.se3_apply(right["extrinsic"], ps))


def is_far(cam0, baseline, pw, pose):
    pc = syn.se3_apply(syn.se3_inv(cam0["extrinsic"]), syn.se3_apply(syn.se3_inv(pose), pw))
    return pc[2] > 50.0 * baseline


@pytest.mark.parametrize("device_assembly", [True, False])     # block lists assembled on the device / by the host walk
@pytest.mark.parametrize("with_imu,weak_thr", [(True, 20), (False, 10 ** 6), (False, 8)])
def test_ticks_match_from_scratch_assembly(oracle, with_imu, weak_thr, device_assembly):
    from lvio_fusion_amd import api
    N, W, max_it = 12, 6, 3
    cfg = syn.config4_window(n_kf=N, n_lm=150, n_prewindow=0, seed=606, imu_samples=4)
    cam0, cam1 = cfg["cam0"], cfg["cam1"]
    baseline = syn.baseline()
    tc, tf = cfg["tc"], cfg["tf"]
    pre = [oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]
    ctx = api.Context(0)
    win = api.Window(ctx, cam0, cam1, baseline=baseline, weak_visual_threshold=weak_thr, device_assembly=device_assembly)
    opt = api.default_solver_options(); opt.max_num_iterations = max_it
    # ---- from-scratch mirror state
    pose = {}; vel = {}; ba = {}; bg = {}; invd = {}; departed = {}; fixed_pw = {}
    obs = {k: {} for k in range(N)}          # kf -> {lm: ob}
    birth = {int(l): int(k) for l, k in zip(tc["lm_idx"], tc["kf_idx"])}
    right_ob = {int(l): tc["right_ob"][i] for i, l in enumerate(tc["lm_idx"])}
    left_ob = {int(l): tc["left_ob"][i] for i, l in enumerate(tc["lm_idx"])}
    seen_po = seen_prior = 0
    for t in range(N):
        # front-end adds keyframe t, its IMU state, the landmarks it triangulated and its observations of older landmarks
        win.add_keyframe(100 + t, cfg["poses"][t], cfg["w_kf"][t]); pose[t] = cfg["poses"][t].copy()
        if with_imu:
            win.set_imu(100 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
            vel[t], ba[t], bg[t] = cfg["vel"][t].copy(), cfg["ba"][t].copy(), cfg["bg"][t].copy()
        for l in sorted(l for l, k in birth.items() if k == t):
            win.add_landmark(5000 + l, 100 + t, left_ob[l], right_ob[l], cfg["inv_depth"][l]); invd[l] = float(cfg["inv_depth"][l])
            obs[t][l] = left_ob[l]
        for i in np.nonzero(tf["kf2_idx"] == t)[0]:
            l = int(tf["lm_idx"][i])
            win.add_observation(5000 + l, 100 + t, tf["ob"][i]); obs[t][l] = tf["ob"][i]
        if with_imu and t == 7:
            # an older pair is re-integrated (Repropagate after a bias change: preintegration.cpp:100-121): the window must factor ITS
            # information matrix again and keep re-using the untouched pairs' (the per-keyframe cache of lvf_window_solve)
            f5 = cfg["imu"][5]
            noise2 = dict(syn.IMU_NOISE) if isinstance(syn.IMU_NOISE, dict) else tuple(2.0 * x for x in syn.IMU_NOISE)
            if isinstance(noise2, dict):
                noise2 = {k: 2.0 * v for k, v in noise2.items()}
            pre[5] = oracle.imu_preintegrate(f5["samples"], f5["acc0"], f5["gyr0"], f5["ba"], f5["bg"], noise2)
            win.set_imu(100 + 6, vel[6], ba[6], bg[6], pre[5])
        if t in (5, 8):      # an older frame loses a tracked feature (what the outlier gate does): its device-side feature segment is re-sent
            k_old = t - 2
            cand = [l for l in sorted(obs[k_old]) if birth[l] != k_old]
            if cand:
                win.remove_observation(5000 + cand[len(cand) // 2], 100 + k_old); del obs[k_old][cand[len(cand) // 2]]
        first = max(0, t - W + 1)
        win.slide(100 + first)
        for k in [k for k in pose if k < first and k not in departed]:
            departed[k] = pose[k].copy()
        for l, b in birth.items():
            if b < first and l in invd and l not in fixed_pw:
                fixed_pw[l] = to_world(cam1, right_ob[l], invd[l], departed[b])
        s_win = win.solve(opt)

        # ---- the same tick assembled from scratch with BuildProblem's rules
        act = list(range(first, t + 1)); pos = {k: i for i, k in enumerate(act)}
        slot = {}; b_tc = [[], [], [], []]; b_tf = [[], [], [], [], []]; b_po = [[], [], []]; pw_tab = []
        pr = dict(kf_a=[], kf_b=[], target=[], weight=[], v=[]); imu_i, imu_j, imu_pre = [], [], []
        for k in act:
            near = 0
            for l in sorted(obs[k]):
                ob = obs[k][l]
                if birth[l] == k:
                    b_tc[0].append(ob); b_tc[1].append(right_ob[l]); b_tc[2].append(slot.setdefault(l, len(slot))); b_tc[3].append(pos[k]); continue
                if birth[l] < first:
                    pw = fixed_pw[l]
                    b_po[0].append(ob); b_po[1].append(pos[k]); b_po[2].append(len(pw_tab)); pw_tab.append(pw)
                else:
                    pw = to_world(cam1, right_ob[l], invd[l], pose[birth[l]])
                    b_tf[0].append(right_ob[l]); b_tf[1].append(ob); b_tf[2].append(slot.setdefault(l, len(slot))); b_tf[3].append(pos[birth[l]]); b_tf[4].append(pos[k])
                near += 0 if is_far(cam0, baseline, pw, pose[k]) else 1
            has_imu = with_imu and k > first
            if has_imu:
                imu_i.append(pos[k] - 1); imu_j.append(pos[k]); imu_pre.append(pre[k - 1])
            if not has_imu and near < weak_thr:
                if k > first:
                    pr["kf_a"].append(pos[k] - 1); pr["target"].append(np.concatenate([oracle.pose_graph_target(pose[k - 1], pose[k]), [0.0]]))
                else:
                    pr["kf_a"].append(-1); pr["target"].append(pose[k])
                pr["kf_b"].append(pos[k]); pr["weight"].append(100.0); pr["v"].append(0.0)
        cnt = win.counts()
        assert (cnt["kf"], cnt["lm"], cnt["tc"], cnt["tf"], cnt["po"], cnt["imu"], cnt["prior"]) == \
               (len(act), len(slot), len(b_tc[2]), len(b_tf[2]), len(b_po[1]), len(imu_i), len(pr["kf_b"])), f"tick {t}: block census"
        seen_po += len(b_po[1]); seen_prior += len(pr["kf_b"])
        st = api.State(ctx, len(act), max(len(slot), 1))
        st.set(api.POSES, np.array([pose[k] for k in act])); st.set(api.W_VISUAL, np.array([cfg["w_kf"][k] for k in act]))
        if with_imu:
            st.set(api.VEL, np.array([vel[k] for k in act])); st.set(api.BA, np.array([ba[k] for k in act])); st.set(api.BG, np.array([bg[k] for k in act]))
        inv_arr = np.ones(max(len(slot), 1))
        for l, sidx in slot.items():
            inv_arr[sidx] = invd[l]
        st.set(api.INV_DEPTH, inv_arr)
        z2 = np.zeros((0, 2)); zi = np.zeros(0, np.int32)
        arr = lambda x, w: np.array(x).reshape(-1, w) if len(x) else np.zeros((0, w))
        hs = []
        btc = api.two_camera_batch(ctx, cam0, cam1, arr(b_tc[0], 2), arr(b_tc[1], 2), np.array(b_tc[2], np.int32), np.array(b_tc[3], np.int32)); hs.append(btc)
        if len(b_tc[3]):     # the window forms the TwoCamera weight as the reference does, `5 * frame->weights.visual` in FLOAT (backend.cpp:123, adapt/weights.h:10)
            btc.set_block_weights((np.float32(5) * np.array([cfg["w_kf"][act[p]] for p in b_tc[3]], np.float32)).astype(np.float64))
        btf = api.two_frame_batch(ctx, cam0, cam1, arr(b_tf[0], 2), arr(b_tf[1], 2), np.array(b_tf[2], np.int32), np.array(b_tf[3], np.int32), np.array(b_tf[4], np.int32)); hs.append(btf)
        bpo = api.pose_only_batch(ctx, cam0, arr(b_po[0], 2), np.array(b_po[1], np.int32), np.array(b_po[2], np.int32), arr(pw_tab, 3) if pw_tab else np.zeros((1, 3))); hs.append(bpo)
        bim = api.imu_batch(ctx, np.array(imu_pre), imu_i, imu_j) if imu_i else None
        prob = api.Problem(ctx, st, btc, btf, bpo, bim)
        bpr = None
        if pr["kf_b"]:
            bpr = api.pose_prior_batch(ctx, pr["kf_a"], pr["kf_b"], np.array(pr["target"]), pr["weight"], pr["v"]); prob.set_pose_priors(bpr)
        s_ref = prob.solve(opt)
        assert abs(s_win.initial_cost - s_ref.initial_cost) <= 1e-8 * abs(s_ref.initial_cost) + 1e-12, f"tick {t}: initial cost"
        assert abs(s_win.final_cost - s_ref.final_cost) <= 1e-6 * abs(s_ref.final_cost) + 1e-12, f"tick {t}: final cost"
        assert s_win.num_successful_steps == s_ref.num_successful_steps and s_win.num_residual_blocks == s_ref.num_residual_blocks
        P = st.get(api.POSES).reshape(-1, 7); D = st.get(api.INV_DEPTH)
        for k in act:
            pose[k] = P[pos[k]].copy()
            assert_parity(win.pose(100 + k), pose[k], f"tick {t} pose {k}")
        for l, sidx in slot.items():
            invd[l] = float(D[sidx])
            assert abs(win.inv_depth(5000 + l) - invd[l]) <= 1e-6 * abs(invd[l])
        if with_imu:
            V, A, G = st.get(api.VEL).reshape(-1, 3), st.get(api.BA).reshape(-1, 3), st.get(api.BG).reshape(-1, 3)
            for k in act:
                vel[k], ba[k], bg[k] = V[pos[k]].copy(), A[pos[k]].copy(), G[pos[k]].copy()
                wv, wa, wg = win.imu(100 + k)
                assert_parity(wv, vel[k], f"tick {t} vel {k}")
        for h in [prob, bim, bpr, st] + hs:
            if h is not None:
                h.close()
    assert seen_po > 0, "the replay never exercised the TwoFrame -> PoseOnly conversion"
    if not with_imu:
        assert seen_prior > 0
    # a departed frame stays queryable exactly while a live landmark was born there (its pose anchors the frozen world point);
    # afterwards the window forgets it (bounded host mirror)
    act_now = list(range(max(0, N - W), N))
    for k0 in (0, N - W - 1):
        anchors = any(birth[l] == k0 for k in act_now for l in obs[k])
        if anchors:
            assert_parity(win.pose(100 + k0), departed[k0], "departed pose")
        else:
            with pytest.raises(api.LvfError):
                win.pose(100 + k0)
    live = {l for k in act_now for l in obs[k]}
    assert win.counts()["lm_known"] == len(live)
    win.close(); ctx.close()


def test_window_crosses_the_device_assembly_limit_and_back(oracle):
    """A window made with device_assembly=True assembles on the device only while it holds at most 64 keyframes (kDaMaxKf); above that it
    takes the host walk, and it comes back once it has slid below.  The strategy is selected BY THE KEYFRAME COUNT ALONE and nothing the
    API reports names it, so the crossing is pinned against a twin made with device_assembly=False (always the host walk) that is fed the
    same drive: solves at 63, 64 (device), 65, 66 (host) keyframes without sliding, four more keyframes and a re-integrated IMU pair while
    the host walk owns the window, a slide to 60 keyframes, and two more solves — the first back on the device must send the whole landmark
    table again and factor every ImuError information matrix again (the host ticks tracked neither), the second runs resident.  At every
    solve: the same census, the same block lists (which blocks, in which order, on which landmarks / keyframes, with which observations
    and weights), and states that agree within the bounds test_ticks_match_from_scratch_assembly holds a window to.  The frozen world
    point of a PoseOnly block is Landmark::ToWorld of the two windows' own solved states at the slide — R(pose) (ray / inv_depth) + t with
    inv_depth within 1e-6 and the pose within assert_parity's 1e-6 of each other — so it is compared to 3e-6 of the largest coordinate."""
    from lvio_fusion_amd import api
    from tests import window_replay as wr
    N, GROW_TO, KEEP = 70, 66, 60
    cfg = syn.config4_window(n_kf=N, n_lm=70, n_prewindow=0, seed=606, imu_samples=4, p_geom=0.2)
    tc, tf = cfg["tc"], cfg["tf"]
    assert len(tc["lm_idx"]) + len(tf["lm_idx"]) < 500
    pre = [oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]
    ctx = api.Context(0)
    wins = [api.Window(ctx, cfg["cam0"], cfg["cam1"], baseline=syn.baseline(), device_assembly=d) for d in (True, False)]
    opt = api.default_solver_options(); opt.max_num_iterations = 2
    ids = {"kf": [], "lm": set()}

    def add_keyframe(t):
        for win in wins:
            win.add_keyframe(100 + t, cfg["poses"][t], cfg["w_kf"][t])
            win.set_imu(100 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
            for i in np.nonzero(tc["kf_idx"] == t)[0]:
                win.add_landmark(5000 + int(tc["lm_idx"][i]), 100 + t, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][tc["lm_idx"][i]])
            for i in np.nonzero(tf["kf2_idx"] == t)[0]:
                win.add_observation(5000 + int(tf["lm_idx"][i]), 100 + t, tf["ob"][i])
        ids["kf"].append(100 + t)
        ids["lm"].update(5000 + int(l) for l in tc["lm_idx"][tc["kf_idx"] == t])

    seen = dict(po=0, tf=0, imu=0)

    def solve_and_compare(what):
        for win in wins:
            win.solve(opt)
        dev, host = wins
        cd, ch = dev.counts(), host.counts()
        assert cd == ch, f"{what}: census {cd} vs {ch}"
        ld, lh = wr.window_lists(dev), wr.window_lists(host)
        for kind in wr.KINDS:
            g, h = ld[kind], lh[kind]
            assert g["ids"].shape == h["ids"].shape and np.array_equal(g["ids"], h["ids"]), f"{what} {kind}: block set / order / indices"
            if kind in ("TwoCamera", "TwoFrame"):
                assert np.array_equal(g["vals"][:, :5], h["vals"][:, :5]), f"{what} {kind}: weight / observations"
            elif kind == "PoseOnly":
                assert np.array_equal(g["vals"][:, :3], h["vals"][:, :3]), f"{what} {kind}: weight / observation"
                if len(h["ids"]):
                    assert np.abs(g["vals"][:, 5:8] - h["vals"][:, 5:8]).max() <= 3e-6 * np.abs(h["vals"][:, 5:8]).max(), f"{what} {kind}: frozen world point"
            elif kind in ("PoseGraphError", "PoseError"):
                assert np.array_equal(g["vals"][:, :2], h["vals"][:, :2]), f"{what} {kind}: prior weight / v"
        for k in ids["kf"]:
            assert_parity(dev.pose(k), host.pose(k), f"{what} pose {k}")
            assert_parity(dev.imu(k)[0], host.imu(k)[0], f"{what} vel {k}")
        for l in sorted(ids["lm"]):
            a, b = dev.inv_depth(l), host.inv_depth(l)
            assert abs(a - b) <= 1e-6 * abs(b), f"{what} inverse depth {l}"
        assert cd["kf"] == len(ids["kf"]) and cd["imu"] == cd["kf"] - 1
        seen["po"] += cd["po"]; seen["tf"] += cd["tf"]; seen["imu"] += cd["imu"]

    for t in range(GROW_TO):
        add_keyframe(t)
        if t + 1 >= 63:
            solve_and_compare(f"{t + 1} keyframes")         # 63, 64: device assembly; 65, 66: the host walk
    for t in range(GROW_TO, N):
        add_keyframe(t)
    # an older pair that stays in the window is re-integrated while the host walk owns it (Repropagate after a bias change): back on the
    # device its information matrix must not come from what the device path cached before the crossing
    f39 = cfg["imu"][39]
    noise2 = {k: 2.0 * v for k, v in syn.IMU_NOISE.items()} if isinstance(syn.IMU_NOISE, dict) else tuple(2.0 * x for x in syn.IMU_NOISE)
    pre39 = oracle.imu_preintegrate(f39["samples"], f39["acc0"], f39["gyr0"], f39["ba"], f39["bg"], noise2)
    for win in wins:
        v, a, g = win.imu(100 + 40)
        win.set_imu(100 + 40, v, a, g, pre39)
    first = N - KEEP
    for win in wins:
        win.slide(100 + first)
    ids["kf"] = ids["kf"][first:]
    born = {5000 + int(l): int(k) for l, k in zip(tc["lm_idx"], tc["kf_idx"])}
    last_seen = dict(born)
    for l, k in zip(tf["lm_idx"], tf["kf2_idx"]):
        last_seen[5000 + int(l)] = max(last_seen[5000 + int(l)], int(k))
    ids["lm"] = {l for l in ids["lm"] if last_seen[l] >= first}            # (the slide prunes landmarks nobody in the window observes)
    solve_and_compare("back at 60 keyframes")
    solve_and_compare("resident again")
    assert seen["po"] > 0 and seen["tf"] > 0 and seen["imu"] > 0
    assert wins[0].counts()["lm_known"] == len(ids["lm"])
    for win in wins:
        win.close()
    ctx.close()


def test_reject_outliers_matches_the_reference_gate(oracle):
    """Backend::Optimize's outlier rejection (backend.cpp:229-245): features that are not their landmark's first observation and whose
    unit-weight reprojection error exceeds 10 px are removed; the device gate must pick exactly the set the oracle's PoseOnly residuals
    pick at the window's solved state, and the next tick must be assembled without them."""
    from lvio_fusion_amd import api
    from tests.helpers import ocam
    N = 7
    cfg = syn.config4_window(n_kf=N, n_lm=200, n_prewindow=0, seed=4711, imu_samples=4)
    cam0, cam1 = cfg["cam0"], cfg["cam1"]
    tc, tf = cfg["tc"], cfg["tf"]
    rng = np.random.default_rng(3)
    bad = rng.choice(len(tf["lm_idx"]), 25, replace=False)
    tf_ob = tf["ob"].copy(); tf_ob[bad] += rng.choice([-1, 1], (25, 2)) * rng.uniform(25, 60, (25, 2))     # gross outliers
    ctx = api.Context(0)
    win = api.Window(ctx, cam0, cam1, baseline=syn.baseline())
    birth = {int(l): int(k) for l, k in zip(tc["lm_idx"], tc["kf_idx"])}
    right_ob = {int(l): tc["right_ob"][i] for i, l in enumerate(tc["lm_idx"])}
    for t in range(N):
        win.add_keyframe(t, cfg["poses"][t], cfg["w_kf"][t])
        for i in np.nonzero(tc["kf_idx"] == t)[0]:
            win.add_landmark(int(tc["lm_idx"][i]), t, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][tc["lm_idx"][i]])
        for i in np.nonzero(tf["kf2_idx"] == t)[0]:
            win.add_observation(int(tf["lm_idx"][i]), t, tf_ob[i])
    opt = api.default_solver_options(); opt.max_num_iterations = 6
    win.solve(opt)
    cnt0 = win.counts()
    # expected set from the oracle at the solved state
    poses = np.array([win.pose(t) for t in range(N)])
    pw = np.array([to_world(cam1, right_ob[int(l)], win.inv_depth(int(l)), poses[birth[int(l)]]) for l in tf["lm_idx"]])
    r, _ = oracle.pose_only(tf_ob, tf["kf2_idx"], np.arange(len(pw), dtype=np.int32), pw, poses, np.ones(N), ocam(oracle, cam0), jac=False)
    err = np.linalg.norm(r, axis=1)
    assert np.abs(err - 10.0).min() > 1e-6, "a feature sits on the threshold: pick another seed"
    expect = sorted((int(tf["lm_idx"][i]), int(tf["kf2_idx"][i])) for i in np.nonzero(err > 10.0)[0])
    assert len(expect) >= 20
    removed, n = win.reject_outliers(10.0)
    assert n == len(expect) and sorted(removed) == expect
    # idempotent, and the next tick no longer contains them
    removed2, n2 = win.reject_outliers(10.0)
    assert n2 == 0 and removed2 == []
    win.solve(opt)
    cnt1 = win.counts()
    assert cnt1["tf"] == cnt0["tf"] - n and cnt1["tc"] == cnt0["tc"]
    # a tight gate removes every non-birth feature; landmarks keep their birth observation, nothing else
    removed3, n3 = win.reject_outliers(0.0, capacity=8)
    assert n3 == cnt1["tf"] and len(removed3) == 8
    win.solve(opt)
    assert win.counts()["tf"] == 0
    win.close(); ctx.close()


@pytest.mark.parametrize("device_assembly", [True, False])
@pytest.mark.parametrize("with_imu", [True, False])
def test_block_lists_equal_the_references_build_problem(oracle, with_imu, device_assembly):
    """the block lists lvf_window assembles — by its device kernels and by its host walk — against the lists the REFERENCE's
    own Backend::BuildProblem produced for the same 12 ticks (src/backend.cpp:96-183 compiled unmodified: oracle/ref_driver_backend.cpp ->
    tests/golden/ref_v4.npz, tests/window_replay.py's drive).  BIT FOR BIT: which blocks, in which order, on which landmark / keyframes, with
    which observations and which weight (TwoCamera: the reference's FLOAT product 5 * weights.visual); the frozen world point of PoseOnly
    blocks to 1e-12 (Landmark::ToWorld is floating-point arithmetic in another operation order); the weak-constraint priors exactly where
    the reference's VisualError census puts them."""
    import os
    from lvio_fusion_amd import api
    from tests import window_replay as wr
    R4 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_v4.npz"))
    tag = f"imu{int(with_imu)}"
    ctx = api.Context(0)
    drive = wr.Drive(with_imu)
    seen = {k: 0 for k in wr.KINDS}
    for t, first, win in wr.replay_window(api, ctx, drive, device_assembly, oracle.imu_preintegrate):
        got = wr.window_lists(win)
        for kind in wr.KINDS:
            ids, vals = R4[f"{tag}_t{t}_{kind}_ids"], R4[f"{tag}_t{t}_{kind}_vals"]
            g = got[kind]
            what = f"{tag} device_assembly={device_assembly} tick {t} {kind}"
            assert g["ids"].shape == ids.shape and np.array_equal(g["ids"], ids), f"{what}: block set / order / indices differ from the reference's BuildProblem"
            if kind in ("TwoCamera", "TwoFrame"):
                assert np.array_equal(g["vals"][:, :5], vals[:, :5]), f"{what}: weight / observations"
            elif kind == "PoseOnly":
                assert np.array_equal(g["vals"][:, :3], vals[:, :3]), f"{what}: weight / observation"
                if len(ids):
                    assert np.abs(g["vals"][:, 5:8] - vals[:, 5:8]).max() <= 1e-12 * np.abs(vals[:, 5:8]).max(), f"{what}: frozen world point"
            elif kind in ("PoseGraphError", "PoseError"):
                assert np.array_equal(g["vals"][:, :2], vals[:, :2]), f"{what}: prior weight / v"
            seen[kind] += len(ids)
        meta = R4[f"{tag}_meta"][t]
        cnt = win.counts()
        assert cnt["kf"] == meta[0] and cnt["tc"] + cnt["tf"] + cnt["po"] + cnt["imu"] + cnt["prior"] == meta[3]
    assert seen["PoseOnly"] > 0 and seen["TwoFrame"] > 0 and (with_imu or (seen["PoseGraphError"] > 0 and seen["PoseError"] > 0))
    ctx.close()
