"""CPU checks of the visual-relocalisation restatement (tests/reloc_ref.py).  What overlaps existing code is pinned to it (Hamming
distances to orb_ref, the reprojection error to pyoracle.pose_only, the LM loop to the oracle's ceres::Solve restatement); what is declared is
checked for its own properties; and every condition tests/test_gpu_reloc.py relies on is asserted here on the committed seeds with the
restatement alone."""
import math

import numpy as np
import pytest

from tests import orb_ref, reloc_cases as rc, reloc_ref as rr

SOLVE_SCENES = [k for k in rc.SCENES if k != "n20_early"]
P3P_REPROJ_BOUND = 1e-2      # px; measured: 2.9e-3 worst over the 2 000 committed triples (ill-conditioned roots, two Newton steps)
P3P_MAX_MISS = 0.005         # a condition (the issue's), not a measurement; found: 1 of 2 000


# ---- matching -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt,cross", [(130, 70, 1), (130, 70, 0), (1, 2, 1), (5, 1, 1), (64, 64, 1), (65, 129, 0)])
def test_match_equals_double_loop(nq, nt, cross):
    q, t = rc.match_sets(100 + nq + nt, nq, nt, duplicate=nt > 9, identical=nt > 5 and nq > 1)
    m, b, s = rr.match(q, t, dict(cross_check=cross))
    best_q = np.full(nt, -1)
    for j in range(nt):
        d = [int(orb_ref.hamming(q[i], t[j])) for i in range(nq)]
        best_q[j] = d.index(min(d))
    accepted = 0
    for i in range(nq):
        d = [int(orb_ref.hamming(q[i], t[j])) for j in range(nt)]
        order = sorted(range(nt), key=lambda j: (d[j], j))
        assert b[i] == d[order[0]]
        assert s[i] == (d[order[1]] if nt >= 2 else -1)
        ok = nt >= 2 and d[order[0]] < 50 and np.float32(d[order[0]]) < np.float32(0.8) * np.float32(d[order[1]]) and (not cross or best_q[order[0]] == i)
        assert m[i] == (order[0] if ok else -1)
        accepted += ok
    if nt >= 2 and nq > 1:
        assert accepted > 0
    if nt > 9:
        assert m[0] == -1 and b[0] == s[0] == 2          # the duplicated train descriptor: tie, the ratio test fails
    if nt > 5 and nq > 1:
        assert b[1] == 0 and m[1] == 5


def test_match_empty_sides():
    q, t = rc.match_sets(1, 4, 3)
    for a, b in ((q[:0], t), (q, t[:0])):
        m, bb, s = rr.match(a, b)
        assert len(m) == len(a) and (m == -1).all() and (bb == -1).all() and (s == -1).all()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
def test_sampler_matches_big_int_hash_and_never_repeats():
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d % 2 ** 32
        x ^= x >> 15; x = x * 0x846ca68b % 2 ** 32
        return x ^ (x >> 16)
    for seed, n in ((0, 3), (7, 21), (7, 71), (0xDEADBEEF, 300), (2 ** 32 - 1, 8192)):
        for h in list(range(40)) + [255, 4095]:
            tr = rr.sample_triple(seed, h, n)
            assert tr is not None and len(set(tr)) == 3 and all(0 <= v < n for v in tr)
            want, c = [], 0
            while len(want) < 3:
                d = mix(seed ^ mix((h * 0x9E3779B1 + c) % 2 ** 32)) % n
                if d not in want:
                    want.append(d)
                c += 1
            assert tr == want


# ---- the reprojection error against the oracle ------------------------------------------------------------------------------------------------
def test_reproj_error_equals_pose_only_residual(oracle):
    s = rc.named_scene("third_behind")
    cam = oracle.Camera.make(s["cam0"]["fx"], s["cam0"]["fy"], s["cam0"]["cx"], s["cam0"]["cy"], s["cam0"]["extrinsic"])
    n = len(s["pw"])
    for pose in (s["pose"], s["init"], s["pose"] * np.array([1.3, 1.3, 1.3, 1.3, 1, 1, 1])):
        r, _ = oracle.pose_only(s["pt"].astype(np.float64), np.zeros(n, np.int32), np.arange(n, dtype=np.int32), s["pw"], pose.reshape(1, 7), np.ones(1), cam, jac=False)
        e2 = rr.reproj_err2(s["cam0"], pose, s["pw"], s["pt"])
        front = np.isfinite(e2)
        assert front.sum() == n - 30 and (rr.project(s["cam0"], pose, s["pw"])[1][~front] <= 0).all()
        assert np.abs(np.sqrt(e2[front]) - np.linalg.norm(r[front], axis=1)).max() <= 1e-12 * max(1.0, np.sqrt(e2[front]).max())


# ---- P3P ------------------------------------------------------------------------------------------------------------------------------------
def test_p3p_property():
    miss, worst = 0, 0.0
    for pose, P, px in rc.p3p_triples():
        poses, _ = rr.hypothesis_poses(rc.CAM0, P, px)
        assert len(poses) <= 4
        found = False
        for p in poses:
            e2 = rr.reproj_err2(rc.CAM0, p, P, px)
            assert np.isfinite(e2).all()                      # positive depth at the three points
            worst = max(worst, float(np.sqrt(e2).max()))
            found |= np.abs(rr.rot_of(p[:4]) - rr.rot_of(pose[:4])).max() < 1e-6 and np.abs(p[4:] - pose[4:]).max() < 1e-5
        miss += not found
    print(f"P3P: planted pose missing in {miss} of {rc.P3P_TRIPLES}, worst reprojection of a sample point {worst:.3e} px")
    assert worst <= P3P_REPROJ_BOUND
    assert miss <= P3P_MAX_MISS * rc.P3P_TRIPLES


def test_quartic_roots_of_a_known_polynomial():
    for roots in ((0.5, 1.5, 2.0, 4.0), (-1.0, 0.25, 3.0, 3.5)):
        c = np.poly(roots)
        got, _ = rr.quartic_real_roots(c[1], c[2], c[3], c[4])
        assert np.allclose(sorted(got), sorted(roots), rtol=0, atol=1e-12)
    got, _ = rr.quartic_real_roots(*np.poly((1.0, 2.0, 0.3 + 1j, 0.3 - 1j)).real[1:])
    assert np.allclose(sorted(got), [1.0, 2.0], rtol=0, atol=1e-12)


# ---- the refinement against the oracle's ceres::Solve restatement -------------------------------------------------------------------------------
def _oracle_refine(oracle, s, x0, inl, iters):
    n = int(inl.sum())
    empty2 = np.zeros((0, 2))
    cfg = dict(n_kf=1, n_lm=1, poses=np.asarray(x0, float).reshape(1, 7), vel=np.zeros((1, 3)), ba=np.zeros((1, 3)), bg=np.zeros((1, 3)), inv_depth=np.ones(1), w_kf=np.ones(1),
               cam0=s["cam0"], cam1=s["cam0"],
               tc=dict(left_ob=empty2, right_ob=empty2, lm_idx=np.zeros(0, np.int32), kf_idx=np.zeros(0, np.int32)),
               tf=dict(first_ob=empty2, ob=empty2, lm_idx=np.zeros(0, np.int32), kf1_idx=np.zeros(0, np.int32), kf2_idx=np.zeros(0, np.int32)),
               po=dict(ob=s["pt"][inl].astype(np.float64), kf_idx=np.zeros(n, np.int32), pw_idx=np.arange(n, dtype=np.int32), pw=s["pw"][inl]), imu=[])
    win = oracle.Window(cfg, np.zeros((0, 467)), vbb_const=np.array([7], np.uint8), use=("po",))
    return win.solve(max_num_iterations=iters, huber_a=1.0), win.poses[0].copy()


@pytest.mark.parametrize("name", ["n71_w40", "n300_w50", "third_behind"])
def test_refine_equals_oracle_lm(oracle, name):
    """LocalMap::LocalBA's problem from a drifted start (several accepted steps, Huber's linear zone in play): equal counts and termination, costs and
    pose to the tolerances of the sibling one-launch solves"""
    s = rc.named_scene(name)
    inl = s["good"].copy()
    inl[np.flatnonzero(~s["good"])[:3]] = True            # three wrong matches among the blocks: |r| > huber_a by far
    x0 = s["init"].copy()
    x0[4:7] = s["pose"][4:7] + (s["init"][4:7] - s["pose"][4:7]) * 0.05
    xs, summ = rr.refine_lm(s["cam0"], x0, s["pw"][inl], s["pt"][inl], 1.0, 10)
    ref, xr = _oracle_refine(oracle, s, x0, inl, 10)
    assert (summ["num_iterations"], summ["num_successful_steps"], summ["termination"], summ["why"]) == \
        (ref["num_iterations"], ref["num_successful_steps"], ref["termination"], ref["why"])
    assert summ["num_successful_steps"] >= 2
    assert abs(summ["initial_cost"] - ref["initial_cost"]) <= 1e-9 * ref["initial_cost"]
    assert abs(summ["final_cost"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    assert np.abs(np.array([float(v) for v in xs]) - xr).max() <= 1e-9


# ---- the conditions of the GPU tests, on the committed seeds ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    out = {}
    for name in SOLVE_SCENES:
        s = rc.named_scene(name)
        keep = {}
        out[name] = (s, rr.pnp_ransac(s["cam0"], s["pw"], s["pt"], None, s["opt"], keep), keep)
    return out


@pytest.mark.parametrize("name", SOLVE_SCENES)
def test_scene_conditions(solved, name):
    s, r, _ = solved[name]
    sc = r["scored"]
    assert sc["min_margin"] >= 1e-6, "a match within 1e-6 px of the gate at a scored pose"
    assert sc["flagged"].sum() <= 0.02 * len(sc["flagged"])
    final = rr.reproj_err2(s["cam0"], r["pose"], s["pw"], s["pt"])
    assert np.abs(np.sqrt(final[np.isfinite(final)]) - 3.0).min() >= 1e-6
    if name == "all_wrong":
        assert r["score"] < 21
        return
    assert sc["winner"] is not None and sc["winner"] >= 0
    win_inl = rr.reproj_err2(s["cam0"], sc["winner_pose"], s["pw"], s["pt"]) < 9.0
    assert not (win_inl & ~s["good"]).any(), "the winning hypothesis holds a wrong match"
    assert (r["inlier"].astype(bool) == s["good"]).all() and r["score"] == int(s["good"].sum())
    if name == "noise_free":
        assert np.abs(r["pose"] - s["pose"]).max() <= 1e-6      # float32 pixels: 3e-5 px at 750 px


def test_early_exit_and_initial_pose():
    s = rc.named_scene("n20_early")
    r = rr.pnp_ransac(s["cam0"], s["pw"], s["pt"], s["init"], s["opt"])
    assert r["pose"] is None and r["score"] == 0 and not r["inlier"].any()
    s = rc.named_scene("n71_w40")
    sc = rr.score_hypotheses(s["cam0"], s["pw"], s["pt"], dict(num_hypotheses=1, seed=3), init_pose=s["pose"])
    assert sc["winner"] == -1 and sc["winner_count"] == int(s["good"].sum())      # the planted pose as hypothesis -1 beats (or ties) any triple


@pytest.mark.parametrize("H", [1, 64, 256])
@pytest.mark.parametrize("n", [21, 71, 300])
def test_hypothesis_conditions(n, H):
    s = rc.scene(40 + n, n, 0.4)
    sc = rr.score_hypotheses(s["cam0"], s["pw"], s["pt"], dict(num_hypotheses=H, seed=rc.PNP_SEED))
    assert sc["flagged"].sum() <= 0.02 * H and sc["min_margin"] >= 1e-6
    assert (sc["triples"] >= 0).all()


def test_image_pair_conditions():
    for same in (False, True):
        c = rc.image_pair(31 + same, same_pose=same, exact=same)
        r = rr.relocate_by_image(c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, c["opt"])
        assert (r["match"] == c["truth"]).all()
        assert r["score"] == 100 and (r["inlier"].astype(bool) == (c["truth"] >= 0)).all()
        sc = r["pnp"]["scored"]
        assert sc["min_margin"] >= 1e-6 and sc["flagged"].sum() <= 0.02 * len(sc["flagged"])
        want = rr.sophus_mul(rr.sophus_inverse(c["old_pose"]), c["pose"])
        assert np.abs(r["relative_o_c"] - want).max() <= 2e-3
        if same:
            assert np.abs(r["relative_o_c"] - [0, 0, 0, 1, 0, 0, 0]).max() <= 1e-12      # measured 3.2e-13 (pixels exact in float32)


def _mp_round(mp, s, x, inl):
    return rr.refine_lm(s["cam0"], x, s["pw"][inl], s["pt"][inl], 1.0, 10, M=mp, F=mp.mpf)


# ---- e_ref: the float64 refinement against a 50-digit run of the same text -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n71_w40", "noise_free"])
def test_refine_float64_deviation_from_extended_precision(solved, name):
    import mpmath as mp
    mp.mp.dps = 50
    s, r, keep = solved[name]
    x64, xmp, total = keep["start"], [mp.mpf(float(v)) for v in keep["start"]], 0
    for inl in keep["inliers"]:                            # every round on the float64 run's inlier set, the 50-digit pose carried through
        x64, s64 = rr.refine_lm(s["cam0"], x64, s["pw"][inl], s["pt"][inl], 1.0, 10)
        xmp, smp = _mp_round(mp, s, xmp, inl)
        assert (s64["num_iterations"], s64["why"]) == (smp["num_iterations"], smp["why"])
        total += s64["num_successful_steps"]
    assert total >= 1 and np.array_equal(np.array([float(v) for v in x64]), r["pose"])
    e_ref = max(abs(float(mp.mpf(a) - b)) for a, b in zip(x64, xmp))
    print(f"e_ref[{name}] = {e_ref:.3e}")
    assert e_ref <= rc.E_REF                                # the constant the GPU tolerance max(1e-12, 8 e_ref) is computed from


# ---- the score arithmetic of Relocator::Relocate ---------------------------------------------------------------------------------------------------
def test_combined_score_modes():
    from lvio_fusion_amd import relocalize as rl
    assert rl.combined_score(35, 50, rl.MODE_NONE) == 0
    assert rl.combined_score(35, 50, rl.MODE_VISUAL_ONLY) == 15
    assert rl.combined_score(35, 50, rl.MODE_LIDAR_ONLY) == 30
    assert rl.combined_score(35, 50, rl.MODE_VISUAL_AND_LIDAR) == 45
    assert rl.combined_score(0, 50, rl.MODE_VISUAL_AND_LIDAR) == 10          # a rejected image candidate still subtracts its base score
    assert rl.combined_score(35, None, rl.MODE_VISUAL_AND_LIDAR) == 15       # no LiDAR features on either frame: RelocateByPoints is not called
    assert rl.combined_score(None, 50, rl.MODE_VISUAL_AND_LIDAR) == 30       # orientation check failed: RelocateByImage is not called
    with pytest.raises(ValueError):
        rl.combined_score(1, 1, 7)
