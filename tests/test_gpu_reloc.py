"""GPU parity of the visual relocalisation (lvio_fusion_amd/csrc/reloc_kernels.hip) through the C-ABI against the CPU restatement
tests/reloc_ref.py.  Integer results (matches, distances, sample triples, inlier counts, masks, scores) are bit-equal; poses agree within
max(1e-12, 8 e_ref), e_ref = the restatement's own float64 deviation from its 50-digit run (tests/test_reloc_ref.py measures 4e-16 .. 9e-16, so
the bound is 1e-12).  Quaternions are compared up to their common sign.  The conditions the equalities rest on (no error within 1e-6 px of
the gate, at most 2 % ill-conditioned hypotheses, the planted inlier sets) are asserted on the CPU in tests/test_reloc_ref.py."""
import numpy as np
import pytest

from tests import klt_ref as kr, reloc_cases as rc, reloc_ref as rr

pytestmark = pytest.mark.gpu

POSE_TOL = max(1e-12, 8 * rc.E_REF)


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def pose_diff(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a[:4] @ b[:4] < 0:
        a = np.concatenate([-a[:4], a[4:]])
    return float(np.abs(a - b).max())


def pnp_opt(api, d):
    return api.pnp_options(**d)


# ---- match ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt", [(130, 70), (1, 2), (5, 1), (64, 64), (65, 129)])
@pytest.mark.parametrize("cross", [1, 0])
def test_match_bit_equal(ctx, nq, nt, cross):
    from lvio_fusion_amd import api
    q, t = rc.match_sets(100 + nq + nt, nq, nt, duplicate=nt > 9, identical=nt > 5 and nq > 1)
    got = api.orb_match(ctx, q, t, api.match_options(cross_check=cross))
    want = rr.match(q, t, dict(cross_check=cross))
    for g, w, what in zip(got, want, ("match", "best", "second")):
        assert np.array_equal(g, w), what
    if nt > 9:
        assert got[0][0] == -1 and got[1][0] == got[2][0] == 2      # the same descriptor at two train indices: a tie, the ratio test fails
    if nt > 5 and nq > 1:
        assert got[1][1] == 0 and got[0][1] == 5                    # a query identical to a train row
    if nt == 1:
        assert (got[0] == -1).all() and (got[2] == -1).all()        # no second neighbour, so no match
    assert all(np.array_equal(a, b) for a, b in zip(api.orb_match(ctx, q, t, api.match_options(cross_check=cross)), got))


def test_match_empty_and_limits(ctx):
    from lvio_fusion_amd import api
    q, t = rc.match_sets(1, 4, 3)
    m, b, s = api.orb_match(ctx, q[:0], t)
    assert len(m) == 0
    m, b, s = api.orb_match(ctx, q, t[:0])
    assert (m == -1).all() and (b == -1).all() and (s == -1).all()
    with pytest.raises(api.LvfError):
        api.orb_match(ctx, np.zeros((8193, 32), np.uint8), t)
    with pytest.raises(api.LvfError):
        api.orb_match(ctx, q, t, api.match_options(max_distance=-1))


# ---- hypotheses -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 64, 256])
@pytest.mark.parametrize("n", [21, 71, 300])
def test_hypotheses_through_the_tap(ctx, n, H):
    from lvio_fusion_amd import api
    s = rc.scene(40 + n, n, 0.4)
    o = dict(num_hypotheses=H, seed=rc.PNP_SEED)
    tri, npo, cnt, poses = api.pnp_debug_hypotheses(ctx, s["cam0"], s["pw"], s["pt"], pnp_opt(api, o))
    ref = rr.score_hypotheses(s["cam0"], s["pw"], s["pt"], o)
    assert np.array_equal(tri, ref["triples"])
    ok = ~ref["flagged"]
    assert ok.sum() >= 0.98 * H
    assert np.array_equal(npo[ok], ref["n_poses"][ok]) and np.array_equal(cnt[ok], ref["count"][ok])
    for h in np.flatnonzero(ok & (ref["n_poses"] > 0)):
        e_dev, e_ref = rr.reproj_err2(s["cam0"], poses[h], s["pw"], s["pt"]), rr.reproj_err2(s["cam0"], ref["pose"][h], s["pw"], s["pt"])
        assert np.array_equal(e_dev < 9.0, e_ref < 9.0), f"hypothesis {h}: the device's pose classifies differently"


# ---- the whole solve ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references():
    return {}


def reference(references, name):
    if name not in references:
        s = rc.named_scene(name)
        references[name] = (s, rr.pnp_ransac(s["cam0"], s["pw"], s["pt"], None, s["opt"]))
    return references[name]


@pytest.mark.parametrize("name", ["n71_w40", "n300_w50", "n21_clean", "all_wrong", "third_behind", "noise_free"])
def test_pnp_ransac_scene(ctx, references, name):
    from lvio_fusion_amd import api
    s, ref = reference(references, name)
    got = api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], None, pnp_opt(api, s["opt"]))
    assert got["score"] == ref["score"] and np.array_equal(got["inlier"], ref["inlier"])
    d = pose_diff(got["pose"], ref["pose"])
    print(f"{name}: score {got['score']}, |pose - restatement| = {d:.3e}")
    assert d <= POSE_TOL
    rs = ref["summary"]
    assert (got["summary"].num_iterations, got["summary"].num_successful_steps, got["summary"].termination) == \
        (rs["num_iterations"], rs["num_successful_steps"], rs["termination"])
    if name == "all_wrong":
        assert got["score"] < 21
    else:
        assert np.array_equal(got["inlier"].astype(bool), s["good"])
    if name == "noise_free":
        assert pose_diff(got["pose"], s["pose"]) <= 1e-6          # float32 pixels
    again = api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], None, pnp_opt(api, s["opt"]))
    assert again["score"] == got["score"] and np.array_equal(again["inlier"], got["inlier"]) and again["pose"].tobytes() == got["pose"].tobytes()
    assert again["summary"].final_cost == got["summary"].final_cost


def test_pnp_ransac_early_exit_and_initial_pose(ctx):
    from lvio_fusion_amd import api
    s = rc.named_scene("n20_early")
    got = api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], s["init"], pnp_opt(api, s["opt"]))
    assert got["pose"] is None and got["score"] == 0 and not got["inlier"].any()      # 20 < min_matches: the pose is left untouched
    s = rc.named_scene("n71_w40")
    o = dict(num_hypotheses=1, seed=3)
    got = api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], s["pose"], pnp_opt(api, o))
    ref = rr.pnp_ransac(s["cam0"], s["pw"], s["pt"], s["pose"], o)
    assert ref["scored"]["winner"] == -1
    assert got["score"] == ref["score"] and np.array_equal(got["inlier"], ref["inlier"]) and pose_diff(got["pose"], ref["pose"]) <= POSE_TOL
    with pytest.raises(api.LvfError):
        api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], None, api.pnp_options(num_hypotheses=4097))
    with pytest.raises(api.LvfError):
        api.pnp_ransac(ctx, s["cam0"], s["pw"], s["pt"], None, api.pnp_options(min_matches=2))


# ---- lvf_relocate_by_image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same_pose", [False, True])
def test_relocate_by_image(ctx, same_pose):
    from lvio_fusion_amd import api
    c = rc.image_pair(31 + same_pose, same_pose=same_pose, exact=same_pose)
    po = pnp_opt(api, c["opt"])
    got = api.relocate_by_image(ctx, c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, po)
    ref = rr.relocate_by_image(c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, c["opt"])
    assert np.array_equal(got["match"], ref["match"]) and np.array_equal(got["match"], c["truth"])
    assert got["score"] == ref["score"] == 100 and np.array_equal(got["inlier"], ref["inlier"])
    d = pose_diff(got["relative_o_c"], ref["relative_o_c"])
    print(f"relocate_by_image(same_pose={same_pose}): |relative_o_c - restatement| = {d:.3e}")
    assert d <= POSE_TOL
    if same_pose:                                          # pixels exact in float32, landmarks projected back from them: the identity itself
        d0 = pose_diff(got["relative_o_c"], [0, 0, 0, 1, 0, 0, 0])
        print(f"relocate_by_image: old_pose == pose, |relative_o_c - identity| = {d0:.3e}")
        assert d0 <= POSE_TOL
    # the same as lvf_orb_match followed by lvf_pnp_ransac on the matched pairs, bit for bit
    m, _, _ = api.orb_match(ctx, c["cur_desc"], c["old_desc"])
    assert np.array_equal(m, got["match"])
    q = np.flatnonzero(m >= 0)
    init = api.forward_update(ctx, c["old_pose"], c["relative_o_c"].reshape(1, 7))[0][0]
    two = api.pnp_ransac(ctx, c["cam0"], c["old_pw"][m[q]], c["cur_pt"][q], init, po)
    inv = rr.sophus_inverse(c["old_pose"])
    assert two["score"] == got["score"] and np.array_equal(two["inlier"], got["inlier"][q])
    rel = api.forward_update(ctx, inv, two["pose"].reshape(1, 7))[0][0]      # (old_pose^-1 is formed on the host here, inside the kernel there)
    assert pose_diff(rel, got["relative_o_c"]) <= POSE_TOL
    again = api.relocate_by_image(ctx, c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, po)
    assert again["relative_o_c"].tobytes() == got["relative_o_c"].tobytes() and again["score"] == got["score"]


def test_relocate_by_image_equals_the_two_calls_bit_for_bit(ctx):
    """An old pose whose inverse is exact (identity quaternion, a translation of few bits): the host's old_pose^-1 IS the kernel's, both products go
    through forward_update_pose on the device, so the fused call and lvf_orb_match + lvf_pnp_ransac are compared in every bit of relative_o_c."""
    from lvio_fusion_amd import api
    old_pose = np.array([0.0, 0.0, 0.0, 1.0, 16.0, -8.0, 1.5])
    inv = np.array([-0.0, -0.0, -0.0, 1.0, -16.0, 8.0, -1.5])
    assert rr.sophus_inverse(old_pose).tobytes() == inv.tobytes()
    c = rc.image_pair(35, old_pose=old_pose)
    po = pnp_opt(api, c["opt"])
    got = api.relocate_by_image(ctx, c["cam0"], old_pose, c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, po)
    assert got["score"] == 100
    m, _, _ = api.orb_match(ctx, c["cur_desc"], c["old_desc"])
    q = np.flatnonzero(m >= 0)
    init = api.forward_update(ctx, old_pose, c["relative_o_c"].reshape(1, 7))[0][0]
    two = api.pnp_ransac(ctx, c["cam0"], c["old_pw"][m[q]], c["cur_pt"][q], init, po)
    rel = api.forward_update(ctx, inv, two["pose"].reshape(1, 7))[0][0]
    assert np.array_equal(m, got["match"]) and two["score"] == got["score"] and np.array_equal(two["inlier"], got["inlier"][q])
    assert rel.tobytes() == got["relative_o_c"].tobytes(), f"differs by {np.abs(rel - got['relative_o_c']).max():.3e}"
    assert (two["summary"].num_iterations, two["summary"].final_cost) == (got["summary"].num_iterations, got["summary"].final_cost)
    ref = rr.relocate_by_image(c["cam0"], old_pose, c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, c["opt"])
    assert got["score"] == ref["score"] and pose_diff(got["relative_o_c"], ref["relative_o_c"]) <= POSE_TOL


def test_relocate_by_image_rejects_unrelated_frames(ctx):
    from lvio_fusion_amd import api
    c = rc.image_pair(33, n_common=10)
    got = api.relocate_by_image(ctx, c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"])
    assert got["score"] == 0 and not got["inlier"].any() and np.array_equal(got["relative_o_c"], c["relative_o_c"])      # 10 pairs < min_matches: untouched
    assert (got["match"] >= 0).sum() == 10 and np.array_equal(got["match"], c["truth"])
    from lvio_fusion_amd import relocalize as rl
    assert rl.combined_score(got["score"], None, rl.MODE_VISUAL_ONLY) == -20
    assert rl.evaluate_candidate_visual(api, ctx, c)["score"] == 0


# ---- images, end to end -----------------------------------------------------------------------------------------------------------------------
IMG_W, IMG_H, PLANE_Z = 320, 240, 6.0
IMG_CAM = dict(fx=300.0, fy=300.0, cx=IMG_W / 2.0, cy=IMG_H / 2.0, extrinsic=rc.CAM0["extrinsic"])


def _image_pair():
    """a fronto-parallel textured plane at PLANE_Z seen by the old camera, and the view of a camera yawed by 0.03 rad and shifted by 0.25 m:
    the plane-induced homography, sampled from the texture (not interpolated)"""
    tex = kr.Texture(5)
    th = 0.03
    R_oc = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])      # current camera -> old camera
    t_oc = np.array([0.25, 0.02, 0.0])
    c = IMG_CAM

    def coords(x, y):
        d = np.stack([(x - c["cx"]) / c["fx"], (y - c["cy"]) / c["fy"], np.ones_like(x)], -1) @ R_oc.T
        lam = (PLANE_Z - t_oc[2]) / d[..., 2]
        X = t_oc + lam[..., None] * d
        return c["fx"] * X[..., 0] / PLANE_Z + c["cx"], c["fy"] * X[..., 1] / PLANE_Z + c["cy"]
    Re = rr.rot_of(c["extrinsic"][:4])
    te = np.asarray(c["extrinsic"][4:7])
    # T_body(old <- current) = T_bc T_oc T_bc^-1
    R_b = Re @ R_oc @ Re.T
    rel = np.concatenate([rr.quat_of(R_b), te + Re @ t_oc - R_b @ te])
    return tex.image(IMG_W, IMG_H), tex.image(IMG_W, IMG_H, coords), rel


def test_images_end_to_end(ctx):
    from lvio_fusion_amd import api
    old_img, cur_img, rel_true = _image_pair()
    old_pose = rc.true_pose(np.random.default_rng(3))
    orb = api.Orb(ctx)
    feats = []
    for img in (old_img, cur_img):
        im = api.Image(ctx, img, 0)
        d = orb.detect(im)
        assert d["level_count"].min() > 0, "a pyramid level without keypoints"
        d["desc"] = orb.compute(d["pt"], d["octave"], d["angle"])
        feats.append(d)
        im.close()
    orb.close()
    A, B = feats
    c = rr.cam_derived(IMG_CAM)
    pc = np.stack([(A["pt"][:, 0] - c["cx"]) / c["fx"] * PLANE_Z, (A["pt"][:, 1] - c["cy"]) / c["fy"] * PLANE_Z, np.full(len(A["pt"]), PLANE_Z)], axis=1)
    old_pw = (pc @ c["Re"].T + c["te"]) @ rr.rot_of(old_pose[:4]).T + old_pose[4:7]
    rel0 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])      # the caller's initial value: no motion
    o = dict(num_hypotheses=128, seed=rc.PNP_SEED)
    got = api.relocate_by_image(ctx, IMG_CAM, old_pose, old_pw, A["desc"], B["pt"], B["desc"], rel0, None, pnp_opt(api, o))
    ref = rr.relocate_by_image(IMG_CAM, old_pose, old_pw, A["desc"], B["pt"], B["desc"], rel0, None, o)
    sc = ref["pnp"]["scored"]
    assert sc is not None and sc["min_margin"] >= 1e-6, "condition: an error within 1e-6 px of the gate"
    print(f"images: {len(A['pt'])} x {len(B['pt'])} keypoints, {(got['match'] >= 0).sum()} pairs, score {got['score']}, "
          f"|relative_o_c - planted| = {pose_diff(got['relative_o_c'], rel_true):.3e}")
    assert np.array_equal(got["match"], ref["match"])
    assert got["score"] >= 21 and got["score"] == ref["score"] and np.array_equal(got["inlier"], ref["inlier"])
    assert pose_diff(got["relative_o_c"], ref["relative_o_c"]) <= POSE_TOL
    assert pose_diff(got["relative_o_c"], rel_true) <= 0.05
