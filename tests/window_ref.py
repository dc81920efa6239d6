"""A tick of the persistent window (lvf_window_solve's assembly) restated in plain numpy, from a mirror of the window to the six block
lists in the form tests/window_replay.window_lists returns.  The rules are the ones test_gpu_window.py's
test_ticks_match_from_scratch_assembly writes out as a python walk:
  * the keyframes in order, within a keyframe the features in ascending landmark id;
  * a feature in its landmark's birth keyframe -> TwoCamera, weight = the FLOAT product 5 * w_visual;
  * a feature whose landmark's birth keyframe is active -> TwoFrame(birth keyframe, keyframe);
  * a feature whose landmark's birth keyframe departed -> PoseOnly on the landmark's frozen world point;
  * the landmarks that some TwoCamera or TwoFrame block uses get dense slots in ascending landmark-TABLE index;
  * consecutive good_imu keyframes, the later one holding a pre-integration -> ImuError;
  * a keyframe without an ImuError block and with fewer than `weak_visual_threshold` near visual blocks (TwoFrame / PoseOnly blocks whose
    point is NOT far: z in cam0 > 50 baselines) -> PoseGraphError(previous, keyframe), the first keyframe PoseError(keyframe).
Everything is array arithmetic over all features at once (no python loop over features): it is called at ~200 k features."""
import numpy as np

from lvio_fusion_amd import synthetic as syn

KINDS = ("TwoCamera", "PoseOnly", "TwoFrame", "ImuError", "PoseGraphError", "PoseError")


def to_world(right, right_ob, inv_depth, pose):
    """the world point of landmarks given by their right-camera pixel and inverse depth in a keyframe at `pose` ([n][7] or [7])"""
    right_ob = np.asarray(right_ob, np.float64).reshape(-1, 2)
    d = 1.0 / np.asarray(inv_depth, np.float64).reshape(-1)
    ps = np.stack([(right_ob[:, 0] - right["cx"]) * d / right["fx"], (right_ob[:, 1] - right["cy"]) * d / right["fy"], d], -1)
    return syn.se3_apply(np.asarray(pose, np.float64), syn.se3_apply(np.asarray(right["extrinsic"], np.float64), ps))


def depth_in_cam0(left, pose, pw):
    """z of world points in the left camera of keyframes at `pose` ([n][7])"""
    pb = syn.se3_apply(syn.se3_inv(np.asarray(pose, np.float64)), pw)
    return syn.se3_apply(syn.se3_inv(np.asarray(left["extrinsic"], np.float64)), pb)[..., 2]


def _lists(ids, vals):
    return dict(ids=np.asarray(ids, np.int64).reshape(-1, 3), vals=np.asarray(vals, np.float64).reshape(-1, 8))


def assemble(left, right, baseline, weak_visual_threshold, kf, lm, obs, prior_weight=100.0, prior_v=0.0):
    """kf  : id [K] (ascending), pose [K][7], w_visual [K], good_imu [K], has_pre [K] (a pre-integration from the previous keyframe)
    lm  : id [M], index [M] (place in the window's landmark table), birth [M] (keyframe id), right_ob [M][2], inv_depth [M],
          fixed [M] (birth keyframe departed), pw [M][3] (the frozen point of a fixed landmark)
    obs : kf [n] (position in kf), lm [n] (row of lm), xy [n][2]
    Returns dict(lists = {kind: dict(ids [n][3], vals [n][8])}, counts = lvf_window_counts' first seven entries,
                 flat = the same blocks as index arrays for the flat batch API, slot_lm = rows of lm in slot order)."""
    kid = np.asarray(kf["id"], np.int64); K = len(kid)
    pose = np.asarray(kf["pose"], np.float64).reshape(K, 7)
    wv = np.asarray(kf["w_visual"], np.float64).reshape(K)
    good = np.asarray(kf["good_imu"], bool).reshape(K); has_pre = np.asarray(kf["has_pre"], bool).reshape(K)
    lid = np.asarray(lm["id"], np.int64); M = len(lid)
    lindex = np.asarray(lm["index"], np.int64).reshape(M); lbirth = np.asarray(lm["birth"], np.int64).reshape(M)
    lright = np.asarray(lm["right_ob"], np.float64).reshape(M, 2); linvd = np.asarray(lm["inv_depth"], np.float64).reshape(M)
    lfixed = np.asarray(lm["fixed"], bool).reshape(M); lpw = np.asarray(lm["pw"], np.float64).reshape(M, 3)
    okf = np.asarray(obs["kf"], np.int64).reshape(-1); olm = np.asarray(obs["lm"], np.int64).reshape(-1)
    oxy = np.asarray(obs["xy"], np.float64).reshape(-1, 2)
    assert np.all(np.diff(kid) > 0), "keyframe ids ascend"
    # the walk's order: keyframe position, then landmark id
    order = np.lexsort((lid[olm], okf))
    okf, olm, oxy = okf[order], olm[order], oxy[order]
    # where each landmark's birth keyframe sits in the window (-1: not active)
    at = np.searchsorted(kid, lbirth)
    bpos = np.where((at < K) & (kid[np.minimum(at, K - 1)] == lbirth), at, -1)
    ob_bpos = bpos[olm]
    is_tc = ob_bpos == okf
    is_tf = (ob_bpos >= 0) & ~is_tc
    is_po = (ob_bpos < 0) & lfixed[olm]
    # dense slots: the used landmarks in ascending table index
    used = np.zeros(M, bool); used[olm[is_tc | is_tf]] = True
    rows = np.flatnonzero(used)
    slot_lm = rows[np.argsort(lindex[rows], kind="stable")]
    slot = np.full(M, -1, np.int64); slot[slot_lm] = np.arange(len(slot_lm))
    # near visual blocks per keyframe
    tf_lm, tf_k1, tf_k2 = olm[is_tf], ob_bpos[is_tf], okf[is_tf]
    po_lm, po_kf = olm[is_po], okf[is_po]
    pw_tf = to_world(right, lright[tf_lm], linvd[tf_lm], pose[tf_k1]) if len(tf_lm) else np.zeros((0, 3))
    pw_po = lpw[po_lm]
    far_z = 50.0 * baseline
    near = np.zeros(K, np.int64)
    if len(tf_lm):
        near += np.bincount(tf_k2[~(depth_in_cam0(left, pose[tf_k2], pw_tf) > far_z)], minlength=K)
    if len(po_lm):
        near += np.bincount(po_kf[~(depth_in_cam0(left, pose[po_kf], pw_po) > far_z)], minlength=K)
    # ImuError pairs and weak-constraint priors (K entries: a loop over keyframes, not features)
    imu_j = np.array([k for k in range(1, K) if good[k] and good[k - 1] and has_pre[k]], np.int64)
    has_block = np.zeros(K, bool); has_block[imu_j] = True
    pr_b = np.flatnonzero(~has_block & (near < weak_visual_threshold))
    pr_a = np.where(pr_b > 0, pr_b - 1, -1)
    # ---- the lists
    z = lambda n: np.zeros(n)
    tc_lm, tc_kf = olm[is_tc], okf[is_tc]
    w_tc = (np.float32(5) * wv[tc_kf].astype(np.float32)).astype(np.float64)
    m1 = lambda n: np.full(n, -1, np.int64)
    L = {}
    L["TwoCamera"] = _lists(np.stack([lid[tc_lm], m1(len(tc_lm)), kid[tc_kf]], -1),
                            np.stack([w_tc, oxy[is_tc, 0], oxy[is_tc, 1], lright[tc_lm, 0], lright[tc_lm, 1], z(len(tc_lm)), z(len(tc_lm)), z(len(tc_lm))], -1))
    L["PoseOnly"] = _lists(np.stack([m1(len(po_lm)), m1(len(po_lm)), kid[po_kf]], -1),
                           np.stack([wv[po_kf], oxy[is_po, 0], oxy[is_po, 1], z(len(po_lm)), z(len(po_lm)), pw_po[:, 0], pw_po[:, 1], pw_po[:, 2]], -1))
    L["TwoFrame"] = _lists(np.stack([lid[tf_lm], kid[tf_k1], kid[tf_k2]], -1),
                           np.stack([wv[tf_k2], oxy[is_tf, 0], oxy[is_tf, 1], lright[tf_lm, 0], lright[tf_lm, 1], z(len(tf_lm)), z(len(tf_lm)), z(len(tf_lm))], -1))
    L["ImuError"] = _lists(np.stack([m1(len(imu_j)), kid[imu_j - 1], kid[imu_j]], -1), np.zeros((len(imu_j), 8)))
    pvals = np.zeros((len(pr_b), 8)); pvals[:, 0] = prior_weight; pvals[:, 1] = prior_v
    pids = np.stack([m1(len(pr_b)), np.where(pr_a >= 0, kid[np.maximum(pr_a, 0)], -1), kid[pr_b]], -1)
    pg = pr_a >= 0
    L["PoseGraphError"] = _lists(pids[pg], pvals[pg]); L["PoseError"] = _lists(pids[~pg], pvals[~pg])
    counts = dict(kf=K, lm=len(slot_lm), tc=len(tc_lm), tf=len(tf_lm), po=len(po_lm), imu=len(imu_j), prior=len(pr_b))
    flat = dict(tc=dict(left_ob=oxy[is_tc], right_ob=lright[tc_lm], lm=slot[tc_lm].astype(np.int32), kf=tc_kf.astype(np.int32), weight=w_tc),
                tf=dict(first_ob=lright[tf_lm], ob=oxy[is_tf], lm=slot[tf_lm].astype(np.int32), kf1=tf_k1.astype(np.int32), kf2=tf_k2.astype(np.int32)),
                po=dict(ob=oxy[is_po], kf=po_kf.astype(np.int32), pw=pw_po),
                imu_i=(imu_j - 1).astype(np.int32), imu_j=imu_j.astype(np.int32), prior_a=pr_a.astype(np.int32), prior_b=pr_b.astype(np.int32),
                inv_depth=linvd[slot_lm], near=near)
    return dict(lists=L, counts=counts, flat=flat, slot_lm=slot_lm)


def compare_lists(got, want, what, pw_bound=1e-12):
    """`got` against `want` the way test_block_lists_equal_the_references_build_problem compares: ids, order and indices exact, weight and
    observation columns exact, frozen world points to `pw_bound` of the largest coordinate"""
    for kind in KINDS:
        g, h = got[kind], want[kind]
        assert g["ids"].shape == h["ids"].shape and np.array_equal(g["ids"], h["ids"]), f"{what} {kind}: block set / order / indices"
        if kind in ("TwoCamera", "TwoFrame"):
            assert np.array_equal(g["vals"][:, :5], h["vals"][:, :5]), f"{what} {kind}: weight / observations"
        elif kind == "PoseOnly":
            assert np.array_equal(g["vals"][:, :3], h["vals"][:, :3]), f"{what} {kind}: weight / observation"
            if len(h["ids"]):
                err, top = np.abs(g["vals"][:, 5:8] - h["vals"][:, 5:8]).max(), np.abs(h["vals"][:, 5:8]).max()
                assert err <= pw_bound * top, f"{what} {kind}: frozen world point off by {err / top:.3e} of the largest coordinate"
        elif kind in ("PoseGraphError", "PoseError"):
            assert np.array_equal(g["vals"][:, :2], h["vals"][:, :2]), f"{what} {kind}: prior weight / v"
