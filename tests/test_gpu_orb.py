"""GPU parity of the ORB front-end (lvio_fusion_amd/csrc/orb_kernels.hip) through the C-ABI against the numpy restatement tests/orb_ref.py
(itself checked against independent statements in tests/test_orb_ref.py).  The device is never compared with truth.

Rules:
  * every pyramid level, blurred level and FAST score map: bit equality;
  * detection: the keypoint set of every level, the bits of `pt`, `response`, `size`, `level_count`: equality; `angle` within one float32 ulp
    (np.spacing) of the restatement's (the moments are exact integers; atan2 is evaluated in fp64 by two different libraries);
  * descriptors: bit equality, the DEVICE's own angles fed to both sides; before the device's descriptors are looked at it is asserted that no
    rotated pattern coordinate lies within 1e-9 of a half-integer, where rint would depend on the last bit of cos / sin;
  * search: match / best / second equal on every feature that is not marginal in the restatement (a candidate's |angle difference - 15| or
    |distance - radius| below 1e-3, or |pc.z| < 1e-9); marginal features are at most 2 % of a case, asserted before the device is looked at;
  * two runs are bit-identical."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import klt_cases as kc
from tests import klt_ref as kr
from tests import orb_cases as oc
from tests import orb_ref as R
from tests import reloc_cases as rc
from tests.helpers import bad_cameras, bad_poses

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


CASES = {
    "rect200": dict(img=lambda: oc.rectangles(1, 200, 150), kw=dict(num_features=60)),
    "rect253": dict(img=lambda: oc.rectangles(5, 253, 131), kw=dict(num_features=60)),          # level 3 (146 x 76) has no cell: empty
    "tex640": dict(img=lambda: oc.texture(3, 640, 376), kw=dict(num_features=500)),
    "tex1241": dict(img=lambda: oc.texture(7, 1241, 376), kw=dict(num_features=500)),
    "rect200_padded": dict(img=lambda: oc.rectangles(1, 200, 150), kw=dict(num_features=60), pad=13),
    "rect200_one_level": dict(img=lambda: oc.rectangles(6, 200, 150), kw=dict(num_features=60, num_levels=1)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's detection of a case, computed once and shared (never modified)"""
    c = CASES[name]
    opt = R.Options(**c["kw"])
    d = R.detect(opt, c["img"]())
    d["blurred"] = [R.blur(g) for g in d["levels"]]
    return opt, d


def device_image(ctx, name, max_level=0):
    from lvio_fusion_amd import api
    c = CASES[name]
    img = c["img"]()
    if c.get("pad"):
        buf = np.zeros((img.shape[0], img.shape[1] + c["pad"]), np.uint8)
        buf[:, :img.shape[1]] = img
        img = buf[:, :-c["pad"]]                                   # a view with a padded row stride
    return api.Image(ctx, img, max_level)


def device_orb(ctx, name, pattern=None, **extra):
    from lvio_fusion_amd import api
    return api.Orb(ctx, api.orb_options(**dict(CASES[name]["kw"], **extra)), pattern)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_angles(dev, ref, what):
    ulp = np.abs(dev.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30))).astype(np.float64)
    print(f"{what}: {len(ref)} angles, max |device - restatement| = {ulp.max() if len(ulp) else 0:.2f} ulp, {int((ulp > 0).sum())} differ")
    assert len(dev) == len(ref) and (len(ulp) == 0 or ulp.max() <= 1.0), f"{what}: angle differs by {ulp.max()} ulp"


@pytest.mark.parametrize("name", list(CASES))
def test_detect_parity(ctx, name):
    opt, ref = reference(name)
    h, w = ref["levels"][0].shape
    img, orb = device_image(ctx, name), device_orb(ctx, name)
    for L in range(opt.num_levels):
        assert orb.level_info(L) == (opt.scale[L], opt.num_desired[L])
    assert orb.capacity(w, h) == R.capacity(opt, w, h)
    d1 = orb.detect(img)
    for L in range(opt.num_levels):
        g, b, s = orb.level(L)
        assert g.shape == ref["levels"][L].shape and np.array_equal(g, ref["levels"][L]), f"pyramid level {L}"
        assert np.array_equal(s, ref["scores"][L]), f"score map of level {L}: {int((s != ref['scores'][L]).sum())} pixels differ"
        assert np.array_equal(b, ref["blurred"][L]), f"blurred level {L}"
    print(f"{name}: level_count device {d1['level_count']} restatement {ref['level_count']} (num_desired {opt.num_desired})")
    assert np.array_equal(d1["level_count"], ref["level_count"])
    for k in ("pt", "response", "size"):
        assert same_bits(d1[k], ref[k]), k
    assert np.array_equal(d1["octave"], ref["octave"])
    assert_angles(d1["angle"], ref["angle"], name)
    assert len(d1["pt"]) <= orb.capacity(w, h)
    d2 = orb.detect(img)
    assert all(same_bits(d1[k], d2[k]) for k in d1), "two runs differ"
    # the stand-alone orientation call gives what detect gives
    assert same_bits(orb.orientation(d1["pt"], d1["octave"]), d1["angle"])
    img.close(); orb.close()


@pytest.mark.parametrize("name", ["rect200", "tex640", "rect200_one_level"])
@pytest.mark.parametrize("pattern_seed", [None, 12345])
def test_descriptor_parity(ctx, name, pattern_seed):
    opt, ref = reference(name)
    pattern = R.builtin_pattern() if pattern_seed is None else R.builtin_pattern(pattern_seed)
    assert R.half_integer_margin(pattern, ref["angle"]) > 1e-9      # before the device is looked at
    img, orb = device_image(ctx, name), device_orb(ctx, name, None if pattern_seed is None else pattern)
    assert np.array_equal(orb.pattern(), pattern)
    d = orb.detect(img)
    assert np.array_equal(d["octave"], ref["octave"]) and same_bits(d["pt"], ref["pt"])
    moved = d["angle"] != ref["angle"]
    assert not moved.any() or R.half_integer_margin(pattern, d["angle"][moved]) > 1e-9
    want = R.compute(opt, ref["levels"], d["pt"], d["octave"], d["angle"], pattern, dict(enumerate(ref["blurred"])))
    got = orb.compute(d["pt"], d["octave"], d["angle"])
    bad = np.nonzero((got != want).any(1))[0]
    print(f"{name} / pattern {pattern_seed}: {len(want)} descriptors, {len(bad)} differ")
    assert len(bad) == 0, f"descriptors differ at {bad[:10]}"
    assert np.array_equal(orb.compute(d["pt"], d["octave"], d["angle"]), got), "two runs differ"
    # keypoints that were not detected (tracked points) on an image that was only set, in another order
    orb.set_image(img)
    pt, octave = oc.random_keypoints(opt, ref["levels"][0].shape[1], ref["levels"][0].shape[0], 97, 5)
    ang = orb.orientation(pt, octave)
    assert_angles(ang, R.orientation(opt, ref["levels"], pt, octave), "tracked points")
    assert R.half_integer_margin(pattern, ang) > 1e-9
    assert np.array_equal(orb.compute(pt, octave, ang), R.compute(opt, ref["levels"], pt, octave, ang, pattern, dict(enumerate(ref["blurred"]))))
    img.close(); orb.close()


def test_errors_leave_the_object_usable(ctx):
    from lvio_fusion_amd import api
    opt, ref = reference("tex640")
    img, small = device_image(ctx, "tex640"), api.Image(ctx, oc.rectangles(2, 116, 87), 0)
    orb = device_orb(ctx, "tex640")
    with pytest.raises(api.LvfError, match=f"lvf error {api.ERR_ORB_CAPACITY}"):
        orb.detect(img, capacity=100)
    d = orb.detect(img)
    assert same_bits(d["pt"], ref["pt"])
    tight = device_orb(ctx, "tex640", max_candidates=64)                # the texture holds thousands of corners per level
    with pytest.raises(api.LvfError, match=f"lvf error {api.ERR_ORB_OVERFLOW}"):
        tight.detect(img)
    want = R.detect(R.Options(num_features=500), oc.rectangles(2, 116, 87))
    got = tight.detect(small)                                          # 21 corners: fits
    assert np.array_equal(got["level_count"], want["level_count"]) and same_bits(got["pt"], want["pt"])
    # argument checks: a keypoint too close to the edge, options the library refuses, calls before an image
    with pytest.raises(api.LvfError):
        orb.compute(np.array([[5.0, 5.0]], np.float32), [0], [0.0])
    with pytest.raises(api.LvfError):
        api.Orb(ctx, api.orb_options(patch_size=25))
    with pytest.raises(api.LvfError):
        api.Orb(ctx, api.orb_options(num_levels=9))
    fresh = api.Orb(ctx)
    with pytest.raises(api.LvfError):
        fresh.level(0)
    assert len(fresh.compute(np.zeros((0, 2), np.float32), [], [])) == 0      # n == 0 returns at once
    for x in (img, small, orb, tight, fresh):
        x.close()


# ---- search --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def search_case(seed=21):
    """two Texture views related by klt_cases.tracking_case's warp: features of A are the last keyframe's, features of B the current ones, whose
    landmarks project into A (through last_pose) where the warp says they were"""
    c = kc.tracking_case(seed)
    opt = R.Options()
    pattern = R.builtin_pattern()
    A, B = R.detect(opt, c["A"]), R.detect(opt, c["B"])
    A["desc"] = R.compute(opt, A["levels"], A["pt"], A["octave"], A["angle"], pattern)
    B["desc"] = R.compute(opt, B["levels"], B["pt"], B["octave"], B["angle"], pattern)
    rng = np.random.default_rng(seed + 1)
    cam0, _, _ = kc.rig()
    from lvio_fusion_amd.synthetic import quat_from_ypr
    last_pose = np.concatenate([quat_from_ypr(0.3, -0.05, 0.02), [4.0, -2.0, 0.5]])
    # B(x, y) = A(inv(x, y)): the scene point at pt in B was at inv(pt) in A
    r2 = np.random.default_rng(seed)
    angle, scale = r2.uniform(-0.02, 0.02), r2.uniform(0.98, 1.02)
    shift = r2.uniform(-6, 6, 2) / np.sqrt(2)
    _, inv = kr.similarity(angle, scale, shift, (kc.W / 2, kc.H / 2))
    in_a = np.stack(inv(B["pt"][:, 0].astype(np.float64), B["pt"][:, 1].astype(np.float64)), 1) + rng.normal(0, 2.0, (len(B["pt"]), 2))
    depth = rng.uniform(2.0, 40.0, len(in_a))
    pw = kr.se3_apply(last_pose, kr.se3_apply(cam0["extrinsic"], kr.pixel2sensor(cam0, in_a, 1.0) * depth[:, None]))
    return dict(opt=opt, cam0=cam0, last_pose=last_pose, A=A, B=B, pw=pw)


def run_search(ctx, c, last=slice(None), skip=None, pw=None):
    from lvio_fusion_amd import api
    A, B = c["A"], c["B"]
    pw = c["pw"] if pw is None else pw
    args = (c["cam0"], c["last_pose"], A["pt"][last], A["octave"][last], A["angle"][last], A["desc"][last], pw, B["octave"], B["angle"], B["desc"])
    m, b, s, marg = R.search(c["opt"], *args, skip=skip)
    assert marg.mean() <= 0.02, f"{int(marg.sum())} of {len(marg)} features are marginal in the restatement"        # before the device is looked at
    dm, db, ds = api.orb_search(ctx, *args, skip=skip)
    keep = ~marg
    assert np.array_equal(dm[keep], m[keep]) and np.array_equal(db[keep], b[keep]) and np.array_equal(ds[keep], s[keep])
    dm2, db2, ds2 = api.orb_search(ctx, *args, skip=skip)
    assert np.array_equal(dm, dm2) and np.array_equal(db, db2) and np.array_equal(ds, ds2), "two runs differ"
    return m, b, s, marg


def test_search_parity(ctx):
    c = search_case()
    m, b, s, marg = run_search(ctx, c)
    print(f"search: {len(m)} current x {len(c['A']['pt'])} last features, {int((m >= 0).sum())} matched, {int((b >= 0).sum())} with a candidate, {int(marg.sum())} marginal")
    assert (m >= 0).sum() >= 50, "the case matches almost nothing: it would not tell a broken search from a working one"
    # a skip mask: the skipped features report nothing
    skip = (np.arange(len(m)) % 3 == 0).astype(np.uint8)
    ms, bs, ss, _ = run_search(ctx, c, skip=skip)
    assert (ms[skip > 0] == -1).all() and (bs[skip > 0] == -1).all() and np.array_equal(ms[skip == 0], m[skip == 0])
    # fewer than two last features: nothing can be accepted
    m1, b1, s1, _ = run_search(ctx, c, last=slice(0, 1))
    assert (m1 == -1).all() and (s1 == -1).all()
    m0, b0, s0, _ = run_search(ctx, c, last=slice(0, 0))
    assert (m0 == -1).all() and (b0 == -1).all()
    # landmarks behind the last camera: mirrored through the camera centre
    centre = kr.se3_apply(c["last_pose"], kr.se3_apply(c["cam0"]["extrinsic"], np.zeros(3)))
    pw = c["pw"].copy()
    pw[::2] = 2 * centre - pw[::2]
    mb, bb, _, _ = run_search(ctx, c, pw=pw)
    assert (mb[::2] == -1).all() and (bb[::2] == -1).all() and np.array_equal(mb[1::2], m[1::2])


@functools.lru_cache(maxsize=None)
def small_search(n_cur, n_last):
    """n_cur current features of search_case() that the whole case matches, and the n_last last features nearest to their matches (the matches
    themselves and what competes with them), in index order; with the restatement's result (computed once and shared, never modified)"""
    c = search_case()
    A, B = c["A"], c["B"]
    m_full = R.search(c["opt"], c["cam0"], c["last_pose"], A["pt"], A["octave"], A["angle"], A["desc"], c["pw"], B["octave"], B["angle"], B["desc"])[0]
    cur = np.nonzero(m_full >= 0)[0][:n_cur]
    centre = A["pt"][m_full[cur]].astype(np.float64)
    dist = np.sqrt(((A["pt"].astype(np.float64)[:, None, :] - centre[None]) ** 2).sum(-1)).min(axis=1)
    last = np.sort(np.argsort(dist, kind="stable")[:n_last])
    args = (c["cam0"], c["last_pose"], A["pt"][last], A["octave"][last], A["angle"][last], A["desc"][last], c["pw"][cur], B["octave"][cur], B["angle"][cur], B["desc"][cur])
    return args, R.search(c["opt"], *args)


# one wave per current feature, four per workgroup: 1 = a single wave, 5 = a second workgroup with one wave, 4 = exactly one workgroup;
# the lanes stride the last features by 64: 1, 64 (every lane exactly once) and 65 (lane 0 a second time)
@pytest.mark.parametrize("n_cur,n_last", [(1, 1), (5, 65), (4, 64)])
def test_search_small_shapes(ctx, n_cur, n_last):
    from lvio_fusion_amd import api
    args, (m, b, s, marg) = small_search(n_cur, n_last)
    assert len(m) == n_cur and len(args[2]) == n_last and not marg.any()                                         # before the device is looked at
    assert (b >= 0).all(), "a feature without a candidate tests nothing"
    assert n_last == 1 or ((m >= 0).sum() >= n_cur - 1 and (s >= 0).sum() >= n_cur - 1), "the shape must exercise the second distance and the ratio gate"
    dm, db, ds = api.orb_search(ctx, *args)
    for name, g, w in (("match", dm, m), ("best", db, b), ("second", ds, s)):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, g, w)
    again = api.orb_search(ctx, *args)
    assert all(np.array_equal(x, y) for x, y in zip((dm, db, ds), again)), "two runs differ"


def test_non_finite_cameras_and_poses_are_refused(ctx):
    """lvf_orb_search and lvf_pnp_ransac: LVF_ERR_INVALID with the entry point's name, nothing written, and the same call works after"""
    from lvio_fusion_amd import api
    INVALID = 1
    L = ctx.L
    fp, u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    args, (m, b, s, _) = small_search(5, 65)
    cam, pose, lpt, loct, lang, ldesc, pw, coct, cang, cdesc = args
    lpt, lang, cang, pw = (np.ascontiguousarray(lpt, np.float32), np.ascontiguousarray(lang, np.float32), np.ascontiguousarray(cang, np.float32),
                           np.ascontiguousarray(pw, np.float64))
    loct, coct, ldesc, cdesc = np.ascontiguousarray(loct, np.int32), np.ascontiguousarray(coct, np.int32), np.ascontiguousarray(ldesc), np.ascontiguousarray(cdesc)
    outs = [np.full(len(pw), 7, np.int32) for _ in range(3)]

    def search(cam0, last_pose):
        a, p = api.make_camera(cam0), np.ascontiguousarray(last_pose, np.float64)
        return L.lvf_orb_search(ctx.h, None, C.byref(a), dp(p), len(lpt), fp(lpt), ip(loct), fp(lang), u8(ldesc), len(pw), dp(pw), ip(coct), fp(cang), u8(cdesc), None,
                                ip(outs[0]), ip(outs[1]), ip(outs[2]))

    for what, cam0, p in [(w, bad, pose) for w, bad in bad_cameras(cam)] + [(w, cam, bad) for w, bad in bad_poses(pose)]:
        assert search(cam0, p) == INVALID, what
        assert L.lvf_last_error().startswith(b"lvf_orb_search:"), (what, L.lvf_last_error())
    assert all((o == 7).all() for o in outs), "a refused call wrote its outputs"
    assert search(cam, pose) == 0
    assert np.array_equal(outs[0], m) and np.array_equal(outs[1], b) and np.array_equal(outs[2], s)

    # lvf_pnp_ransac (strict before this): a scene of tests/reloc_cases.py with its pose as the initial one
    sc = rc.named_scene("n71_w40")
    n = len(sc["pw"])
    pw3, pt, opt = np.ascontiguousarray(sc["pw"], np.float64), np.ascontiguousarray(sc["pt"], np.float32), api.pnp_options(**sc["opt"])
    out_pose, score, inl = np.full(7, 7.0), C.c_int32(7), np.full(n, 7, np.uint8)

    def pnp(cam0, init):
        a, i = api.make_camera(cam0), np.ascontiguousarray(init, np.float64)
        return L.lvf_pnp_ransac(ctx.h, C.byref(a), n, dp(pw3), fp(pt), dp(i), C.byref(opt), dp(out_pose), C.byref(score), u8(inl), None)

    for what, cam0, init in [(w, bad, sc["pose"]) for w, bad in bad_cameras(sc["cam0"])] + [(w, sc["cam0"], bad) for w, bad in bad_poses(sc["pose"])]:
        assert pnp(cam0, init) == INVALID, what
        assert L.lvf_last_error().startswith(b"lvf_pnp_ransac:"), (what, L.lvf_last_error())
    assert (out_pose == 7).all() and score.value == 7 and (inl == 7).all(), "a refused call wrote its outputs"
    assert pnp(sc["cam0"], sc["pose"]) == 0
    want = api.pnp_ransac(ctx, sc["cam0"], sc["pw"], sc["pt"], sc["pose"], opt)
    assert score.value == want["score"] > 0 and inl.tobytes() == want["inlier"].tobytes() and out_pose.tobytes() == want["pose"].tobytes()


def test_detect_to_window_chain(ctx):
    """detect on klt_cases.stereo_case's left image -> lvf_stereo_triangulate -> compute of the accepted -> lvf_window_add_landmark.
    A wiring check, not a parity test."""
    from lvio_fusion_amd import api
    c = kc.stereo_case(31)
    left, right = api.Image(ctx, c["left"], 3), api.Image(ctx, c["right"], 3)
    orb = api.Orb(ctx)
    d = orb.detect(left)
    assert len(d["pt"]) > 300
    kps_right, st, inv, pb = api.stereo_triangulate(left, right, c["cam0"], c["cam1"], c["baseline"], d["pt"])
    ok = np.nonzero(st == 1)[0]
    assert len(ok) > 100
    desc = orb.compute(d["pt"][ok], d["octave"][ok], d["angle"][ok])
    assert desc.shape == (len(ok), 32) and len(np.unique(desc, axis=0)) > 0.9 * len(ok)
    win = api.Window(ctx, c["cam0"], c["cam1"], baseline=c["baseline"])
    win.add_keyframe(0, np.array([0, 0, 0, 1.0, 0, 0, 0]), 46.0)
    for i in ok:
        win.add_landmark(int(i), 0, d["pt"][i], kps_right[i], inv[i])
    print(f"chain: {len(d['pt'])} detected, {len(ok)} triangulated and described")
    for x in (win, orb, left, right):
        x.close()
