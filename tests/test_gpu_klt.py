"""GPU parity of the feature tracker (lvio_fusion_amd/csrc/klt_kernels.hip) through the C-ABI against the CPU restatement tests/klt_ref.py
(itself checked against exact truth, scipy and a 50-digit DLT in tests/test_klt_ref.py).  The device is never compared with truth.

Rules (the same for optical_flow, stereo_triangulate and track_last_frame):
  * pyramid and derivative levels: bit equality;
  * two runs, and a run with the points permuted, are bit-identical;
  * `next` against the float64 restatement where both accept: 0.02 px, twice the termination step 0.01 of utility.cpp:65 (two trackers that
    stop on |delta| <= eps near the same fixed point differ by at most one last step each; coarse-level differences are re-converged);
  * status equal on every point that is not MARGINAL in the float64 restatement (klt_ref.marginal): |fb - 0.5| < 0.02, minEig at level 0
    within 1 % of min_eig, the final point within 0.02 px of an image edge, a window-bounds test that flips under a 0.02 px shift, or the
    float32 and float64 restatements disagreeing.  Marginal points are at most 5 % of a case, asserted BEFORE the device is looked at."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import klt_cases as kc
from tests import klt_ref as kr
from tests.helpers import assert_parity, bad_cameras, bad_poses

pytestmark = pytest.mark.gpu

TOL = 0.02


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def images(ctx, *arrays, max_level=3):
    from lvio_fusion_amd import api
    return [api.Image(ctx, a, max_level) for a in arrays]


def ref_kw(o):
    return dict(win=o.win, levels=o.max_level, back_win=o.back_win, back_levels=o.back_max_level, max_iter=o.max_iter, eps=o.eps, min_eig=o.min_eig,
                fb_max=o.fb_max)


def compare_flow(what, A, B, prev, init, nxt, st, kw=None, status_of=lambda s: s):
    """the point / status rules of the module docstring; returns the mask of compared (non-marginal) points"""
    n64, s64, f64, m = kr.marginal(A, B, prev, init, TOL, **(kw or {}))
    assert m.mean() <= 0.05, f"{what}: {m.sum()} of {len(m)} points are marginal in the restatement"        # before the device is looked at
    keep = ~m
    s_dev = status_of(st) > 0
    bad = keep & (s_dev != (s64 > 0))
    both = keep & s_dev & (s64 > 0)
    err = np.abs(nxt[both].astype(np.float64) - n64[both].astype(np.float64)).max() if both.any() else 0.0
    print(f"{what}: {len(m)} points, {int(m.sum())} marginal, {int(both.sum())} accepted by both, status differs on {int(bad.sum())}, max |next - ref| = {err:.5f} px")
    assert not bad.any(), f"{what}: status differs off the marginal set at {np.nonzero(bad)[0][:10]}"
    assert both.sum() > 0 and err <= TOL, f"{what}: next differs by {err} px"
    return keep, n64, s64


# ---- image object ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pad", [(640, 376, 0), (1241, 376, 0), (75, 53, 0), (75, 53, 21), (1241, 376, 7), (8, 5, 3)])
def test_pyramid_and_derivatives_bit_equal(ctx, w, h, pad):
    from lvio_fusion_amd import api
    rng = np.random.default_rng(w + 7 * h + pad)
    buf = rng.integers(0, 256, (h, w + pad), dtype=np.uint8)
    view = buf[:, :w]                                   # padded row stride when pad > 0
    img = api.Image(ctx, view, 3)
    assert img.size() == (w, h, 4)
    ref = kr.Pyramid(np.ascontiguousarray(view), 3)
    for L in range(4):
        g, d = img.level(L)
        assert g.shape == ref.gray[L].shape and np.array_equal(g, ref.gray[L]), f"gray level {L}"
        assert np.array_equal(d, ref.deriv[L]), f"derivative level {L}"
    img.close()


# ---- optical_flow ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
def test_optical_flow_parity(ctx, seed):
    from lvio_fusion_amd import api
    c = kc.tracking_case(seed)
    ia, ib = images(ctx, c["A"], c["B"])
    nxt, st, fb = api.optical_flow(ia, ib, c["prev"], c["init"])
    keep, n64, s64 = compare_flow(f"tracking seed {seed}", kr.Pyramid(c["A"]), kr.Pyramid(c["B"]), c["prev"], c["init"], nxt, st)
    assert np.all(fb[st > 0] <= 0.5) and st.sum() > 0.9 * len(st)
    ia.close(); ib.close()


def test_optical_flow_at_the_image_edge(ctx):
    """points whose windows hang over the border (reflect-101 for the images, zero for the derivatives) and points off the image"""
    from lvio_fusion_amd import api
    c = kc.tracking_case(13, n=300, border=-8.0)
    ia, ib = images(ctx, c["A"], c["B"])
    nxt, st, _ = api.optical_flow(ia, ib, c["prev"], c["init"])
    compare_flow("edge", kr.Pyramid(c["A"]), kr.Pyramid(c["B"]), c["prev"], c["init"], nxt, st)
    w, h = kc.W, kc.H
    off = np.array([[-12.5, 50.0], [w + 10.5, 50.0], [100.0, -12.5], [100.0, h + 10.5]], np.float32)
    _, st2, fb2 = api.optical_flow(ia, ib, off, off)
    assert st2.tolist() == [0, 0, 0, 0] and np.all(np.isinf(fb2))
    ia.close(); ib.close()


def test_optical_flow_is_deterministic_and_order_free(ctx):
    from lvio_fusion_amd import api
    c = kc.tracking_case(12)
    ia, ib = images(ctx, c["A"], c["B"])
    a = api.optical_flow(ia, ib, c["prev"], c["init"])
    b = api.optical_flow(ia, ib, c["prev"], c["init"])
    perm = np.random.default_rng(0).permutation(len(c["prev"]))
    p = api.optical_flow(ia, ib, c["prev"][perm], c["init"][perm])
    for x, y, z in zip(a, b, p):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        u = np.empty_like(z); u[perm] = z
        assert np.array_equal(x.view(np.uint8), u.view(np.uint8))
    ia.close(); ib.close()


def test_optical_flow_options(ctx):
    """window 15, 2 levels, 5 iterations follow the restatement"""
    from lvio_fusion_amd import api
    c = kc.tracking_case(11, n=300)
    ia, ib = images(ctx, c["A"], c["B"])
    o = api.flow_options(win=15, max_level=2, max_iter=5)
    init = (c["truth"] + np.random.default_rng(3).normal(0, 1.0, c["truth"].shape)).astype(np.float32)
    nxt, st, _ = api.optical_flow(ia, ib, c["prev"], init, o)
    compare_flow("options", kr.Pyramid(c["A"]), kr.Pyramid(c["B"]), c["prev"], init, nxt, st, ref_kw(o))
    d = api.flow_options()
    assert (d.win, d.max_level, d.back_win, d.back_max_level, d.max_iter, d.eps, d.min_eig, d.fb_max) == (21, 3, 3, 1, 30, 0.01, 1e-4, 0.5)
    ia.close(); ib.close()


def test_optical_flow_sizes(ctx):
    """N = 0 returns at once, N = 1 and N = 5000 work"""
    from lvio_fusion_amd import api
    c = kc.tracking_case(11, n=5000)
    ia, ib = images(ctx, c["A"], c["B"])
    nxt, st, fb = api.optical_flow(ia, ib, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert nxt.shape == (0, 2) and st.shape == (0,)
    assert ctx.L.lvf_optical_flow(ia.h, ib.h, 0, None, None, None, None, None) == 0
    n1, s1, _ = api.optical_flow(ia, ib, c["prev"][:1], c["init"][:1])
    nxt, st, fb = api.optical_flow(ia, ib, c["prev"], c["init"])
    assert np.array_equal(n1, nxt[:1]) and s1[0] == st[0]
    assert st.mean() > 0.9
    sub = np.arange(0, 5000, 25)                        # the restatement on every 25th point: points are independent
    compare_flow("N = 5000 (every 25th)", kr.Pyramid(c["A"]), kr.Pyramid(c["B"]), c["prev"][sub], c["init"][sub], nxt[sub], st[sub])
    ia.close(); ib.close()


def test_invalid_arguments(ctx):
    from lvio_fusion_amd import api
    c = kc.tracking_case(11, n=4)
    ia, = images(ctx, c["A"])
    small, = images(ctx, c["A"][:100, :200])
    shallow, = images(ctx, c["B"], max_level=1)
    L = ctx.L
    p, q = c["prev"].copy(), c["init"].copy()
    st = np.zeros(4, np.uint8)
    fp, u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    INVALID = 1
    assert L.lvf_optical_flow(None, ia.h, 4, fp(p), fp(q), u8(st), None, None) == INVALID
    assert L.lvf_optical_flow(ia.h, None, 4, fp(p), fp(q), u8(st), None, None) == INVALID
    assert L.lvf_optical_flow(ia.h, small.h, 4, fp(p), fp(q), u8(st), None, None) == INVALID
    assert b"sizes differ" in L.lvf_last_error()
    assert L.lvf_optical_flow(ia.h, shallow.h, 4, fp(p), fp(q), u8(st), None, None) == INVALID          # 4 levels asked, 2 held
    assert L.lvf_optical_flow(ia.h, ia.h, 4, None, fp(q), u8(st), None, None) == INVALID
    assert L.lvf_optical_flow(ia.h, ia.h, -1, fp(p), fp(q), u8(st), None, None) == INVALID
    big = api.flow_options(win=23)
    assert L.lvf_optical_flow(ia.h, ia.h, 4, fp(p), fp(q), u8(st), None, C.byref(big)) == INVALID
    assert np.array_equal(q, c["init"]) and not st.any()                                                # outputs untouched on failure
    out = C.c_void_p()
    g = np.ascontiguousarray(c["A"])
    assert L.lvf_image_create(None, u8(g), 640, 376, 640, 3, C.byref(out)) == INVALID
    assert L.lvf_image_create(ctx.h, u8(g), 640, 376, 600, 3, C.byref(out)) == INVALID                  # stride < width
    assert L.lvf_image_create(ctx.h, u8(g), 640, 376, 640, 8, C.byref(out)) == INVALID
    assert L.lvf_image_create(ctx.h, u8(g), 0, 376, 640, 3, C.byref(out)) == INVALID
    assert L.lvf_image_size(None, None, None, None) == INVALID
    assert L.lvf_image_download_level(ia.h, 4, None, None, None, None) == INVALID
    with pytest.raises(api.LvfError):
        api.stereo_triangulate(ia, small, *kc.rig()[:2], 0.54, c["prev"])
    with pytest.raises(api.LvfError):
        api.track_last_frame(ia, small, kc.rig()[0], 0.54, np.array([0, 0, 0, 1.0, 0, 0, 0]), np.ones((4, 3)), c["prev"])
    for im in (ia, small, shallow):
        im.close()


# ---- stereo_triangulate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,lo", [(21, 6.0), (23, -10.0)])
def test_stereo_triangulate_parity(ctx, seed, lo):
    """lo < 0 plants points of negative disparity: tracked, but behind the cameras (status 2)"""
    from lvio_fusion_amd import api
    c = kc.stereo_case(seed, lo=lo)
    il, ir = images(ctx, c["left"], c["right"])
    right, st, inv, pb = api.stereo_triangulate(il, ir, c["cam0"], c["cam1"], c["baseline"], c["kps"])
    pred = kr.stereo_predict(c["cam0"], c["cam1"], c["baseline"], c["kps"])
    compare_flow(f"stereo seed {seed}", kr.Pyramid(c["left"]), kr.Pyramid(c["right"]), c["kps"], pred, right, st)
    # depth from the DEVICE's own right pixels, so that the 0.02 px does not leak into a depth tolerance
    pb_ref, z0, inv_ref = kr.stereo_depth(c["cam0"], c["cam1"], c["kps"], right)
    t = st > 0
    assert t.sum() > 400 and np.abs(z0[t]).min() > 1e-6                        # no planted point within 1e-6 of zero depth
    assert np.array_equal(st[t], np.where(z0[t] > 0, 1, 2)), "depth-sign gate"
    if lo < 0:
        assert (st == 2).sum() >= 20 and (st == 1).sum() >= 200
    else:
        assert not (st == 2).any()
    assert_parity(pb[t], pb_ref[t], "p_robot")
    assert_parity(inv[t], inv_ref[t], "inv_depth")
    assert not inv[~t].any() and not pb[~t].any()
    again = api.stereo_triangulate(il, ir, c["cam0"], c["cam1"], c["baseline"], c["kps"])
    for x, y in zip((right, st, inv, pb), again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    il.close(); ir.close()


# Feature counts around the launch shapes: one wave per feature and four features per workgroup in k_klt_flow (1: one wave of a workgroup, 5: a second
# workgroup with one wave), 256 threads per workgroup in k_klt_stereo_predict / k_klt_dlt / k_klt_track_predict / k_klt_track_classify (257: one
# thread into the second workgroup, and the second trip of the classify loop).  Features are independent, so the first n of a case are a case.
COUNTS = [1, 5, 257]


@functools.lru_cache(maxsize=None)
def stereo_small():
    """klt_cases.stereo_case(21) with its pyramids of the restatement, built once and shared (never modified)"""
    c = kc.stereo_case(21)
    return c, kr.Pyramid(c["left"]), kr.Pyramid(c["right"])


@functools.lru_cache(maxsize=None)
def track_small():
    c = kc.track_case(31)
    return c, kr.Pyramid(c["A"]), kr.Pyramid(c["B"])


@pytest.mark.parametrize("n", COUNTS)
def test_stereo_triangulate_feature_counts(ctx, n):
    """test_stereo_triangulate_parity's rules on the first n features"""
    from lvio_fusion_amd import api
    c, L, R = stereo_small()
    kps = c["kps"][:n]
    il, ir = images(ctx, c["left"], c["right"])
    right, st, inv, pb = api.stereo_triangulate(il, ir, c["cam0"], c["cam1"], c["baseline"], kps)
    assert right.shape == (n, 2) and st.shape == (n,) and inv.shape == (n,) and pb.shape == (n, 3)
    pred = kr.stereo_predict(c["cam0"], c["cam1"], c["baseline"], kps)
    compare_flow(f"stereo, first {n}", L, R, kps, pred, right, st)
    pb_ref, z0, inv_ref = kr.stereo_depth(c["cam0"], c["cam1"], kps, right)        # from the DEVICE's own right pixels, as above
    t = st > 0
    assert t.any() and np.abs(z0[t]).min() > 1e-6
    assert np.array_equal(st[t], np.where(z0[t] > 0, 1, 2)), "depth-sign gate"
    assert_parity(pb[t], pb_ref[t], "p_robot")
    assert_parity(inv[t], inv_ref[t], "inv_depth")
    assert not inv[~t].any() and not pb[~t].any()
    again = api.stereo_triangulate(il, ir, c["cam0"], c["cam1"], c["baseline"], kps)
    for x, y in zip((right, st, inv, pb), again):
        assert x.tobytes() == y.tobytes()
    il.close(); ir.close()


@pytest.mark.parametrize("n", COUNTS)
def test_track_last_frame_feature_counts(ctx, n):
    """test_track_last_frame_parity's rules on the first n features (the case with a pose and world points is klt_cases.track_case)"""
    from lvio_fusion_amd import api
    c, A, B = track_small()
    b, pw, prev = c["baseline"], c["pw"][:n], c["prev"][:n]
    ia, ib = images(ctx, c["A"], c["B"])
    cur, cls, good, pred = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], pw, prev)
    assert cur.shape == (n, 2) and cls.shape == (n,) and pred.shape == (n, 2)
    assert np.abs(pred.astype(np.float64) - kr.track_predict(c["cam0"], c["pose"], pw)).max() <= 1e-4
    keep, n64, s64 = compare_flow(f"track, first {n}", A, B, prev, pred, cur, cls)
    cls_ref, _, norm, z = kr.classify(c["cam0"], b, c["pose"], pw, pred, n64, s64)
    keep &= ~(np.abs(norm - 30) < 0.05) & ~(np.abs(z - 50 * b) <= 1e-9 * 50 * b)
    assert np.array_equal(cls[keep], cls_ref[keep])
    # the count: the restatement's on the device's own tracks, at the default threshold of 20 and with none
    _, good_own, _, _ = kr.classify(c["cam0"], b, c["pose"], pw, pred, cur, cls > 0)
    _, count_own, _, _ = kr.classify(c["cam0"], b, c["pose"], pw, pred, cur, cls > 0, num_features_tracking_bad=0)
    assert good == good_own and count_own >= 1 and (good_own > 0) == (n > 20)
    again = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], pw, prev, num_features_tracking_bad=0)
    assert again[2] == count_own
    for x, y in zip((cur, cls, pred), (again[0], again[1], again[3])):
        assert x.tobytes() == y.tobytes()
    ia.close(); ib.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_cameras_and_poses_are_refused(ctx):
    """lvf_stereo_triangulate and lvf_track_last_frame: LVF_ERR_INVALID with the entry point's name, nothing written, and the same call works after"""
    from lvio_fusion_amd import api
    INVALID = 1
    L = ctx.L
    fp, u8, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    n = 5
    c, _, _ = stereo_small()
    il, ir = images(ctx, c["left"], c["right"])
    kps = np.ascontiguousarray(c["kps"][:n])
    outs = [np.full((n, 2), 7, np.float32), np.full(n, 7, np.uint8), np.full(n, 7.0), np.full((n, 3), 7.0)]

    def stereo(cam0, cam1):
        a, b = api.make_camera(cam0), api.make_camera(cam1)
        return L.lvf_stereo_triangulate(il.h, ir.h, C.byref(a), C.byref(b), C.c_double(c["baseline"]), n, fp(kps), fp(outs[0]), u8(outs[1]), dp(outs[2]), dp(outs[3]), None)

    for what, cams in [(w, (bad, c["cam1"])) for w, bad in bad_cameras(c["cam0"])] + [(w, (c["cam0"], bad)) for w, bad in bad_cameras(c["cam1"])]:
        assert stereo(*cams) == INVALID, what
        assert L.lvf_last_error().startswith(b"lvf_stereo_triangulate:"), (what, L.lvf_last_error())
    assert all((o == 7).all() for o in outs), "a refused call wrote its outputs"
    assert stereo(c["cam0"], c["cam1"]) == 0
    want = api.stereo_triangulate(il, ir, c["cam0"], c["cam1"], c["baseline"], kps)
    for o, w in zip(outs, want):
        assert o.tobytes() == w.tobytes()
    il.close(); ir.close()

    t, _, _ = track_small()
    ia, ib = images(ctx, t["A"], t["B"])
    prev, pw = np.ascontiguousarray(t["prev"][:n]), np.ascontiguousarray(t["pw"][:n])
    touts = [np.full((n, 2), 7, np.float32), np.full((n, 2), 7, np.float32), np.full(n, 7, np.uint8)]
    good = C.c_int32(7)

    def track(cam0, pose):
        a, p = api.make_camera(cam0), np.ascontiguousarray(pose, np.float64)
        return L.lvf_track_last_frame(ia.h, ib.h, C.byref(a), C.c_double(t["baseline"]), dp(p), n, dp(pw), fp(prev), 1, 0, fp(touts[0]), fp(touts[1]), u8(touts[2]),
                                      C.byref(good), None)

    for what, cam0, pose in [(w, bad, t["pose"]) for w, bad in bad_cameras(t["cam0"])] + [(w, t["cam0"], bad) for w, bad in bad_poses(t["pose"])]:
        assert track(cam0, pose) == INVALID, what
        assert L.lvf_last_error().startswith(b"lvf_track_last_frame:"), (what, L.lvf_last_error())
    assert all((o == 7).all() for o in touts) and good.value == 7, "a refused call wrote its outputs"
    assert track(t["cam0"], t["pose"]) == 0
    cur, cls, g, pred = api.track_last_frame(ia, ib, t["cam0"], t["baseline"], t["pose"], pw, prev, num_features_tracking_bad=0)
    assert touts[0].tobytes() == cur.tobytes() and touts[1].tobytes() == pred.tobytes() and touts[2].tobytes() == cls.tobytes() and good.value == g
    ia.close(); ib.close()


# ---- track_last_frame --------------------------------------------------------------------------------------------------------------------------
def test_track_last_frame_parity(ctx):
    from lvio_fusion_amd import api
    c = kc.track_case(31)
    b = c["baseline"]
    ia, ib = images(ctx, c["A"], c["B"])
    cur, cls, good, pred = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], c["pw"], c["prev"])
    pred_ref = kr.track_predict(c["cam0"], c["pose"], c["pw"])
    assert np.abs(pred.astype(np.float64) - pred_ref).max() <= 1e-4             # float32 roundings of one fp64 projection
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(c["B"])
    keep, n64, s64 = compare_flow("track", A, B, c["prev"], pred, cur, cls)
    # classes: the restatement's, marginal where the deviation norm is within 0.05 of 30 or the depth within 1e-9 (relative) of 50 baselines
    cls_ref, good_ref, norm, z = kr.classify(c["cam0"], b, c["pose"], c["pw"], pred, n64, s64)
    keep &= ~(np.abs(norm - 30) < 0.05) & ~(np.abs(z - 50 * b) <= 1e-9 * 50 * b)
    assert np.array_equal(cls[keep], cls_ref[keep])
    assert np.bincount(cls, minlength=4).min() >= 1                             # every class occurs
    # the count: exactly the restatement's on the device's own tracks, on both sides of num_features_tracking_bad
    _, good_own, _, _ = kr.classify(c["cam0"], b, c["pose"], c["pw"], pred, cur, cls > 0)
    assert good == good_own and good > 20
    if keep.all():
        assert good == good_ref
    _, cls_hi, none, _ = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], c["pw"], c["prev"], num_features_tracking_bad=good)
    assert none == 0 and np.array_equal(cls_hi, cls)
    _, _, edge, _ = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], c["pw"], c["prev"], num_features_tracking_bad=good - 1)
    assert edge == good
    _, cls_keep, good_keep, _ = api.track_last_frame(ia, ib, c["cam0"], b, c["pose"], c["pw"], c["prev"], remove_moving_points=False)
    assert not (cls_keep == 3).any() and good_keep == int((cls > 0).sum())
    ia.close(); ib.close()


# ---- hand-over to the sliding window ------------------------------------------------------------------------------------------------------------
def test_hand_over_to_the_window(ctx):
    """A small synthetic rig: keyframe 0 triangulates landmarks from its stereo pair, keyframe 1 (moved sideways) tracks them; the accepted tracks
    go through lvf_window_add_landmark / lvf_window_add_observation and lvf_window_solve.  A wiring check, not a parity test."""
    from lvio_fusion_amd import api
    w, h = kc.W, kc.H
    cam0, cam1, b = kc.rig()
    tex = kr.Texture(41)
    step = 0.3                                                    # metres along camera x between the keyframes
    disp = lambda y: kc.disparity(y, h, 8.0, 36.0)
    left0 = tex.image(w, h)
    right0 = tex.image(w, h, lambda x, y: (x + disp(y), y))
    left1 = tex.image(w, h, lambda x, y: (x + disp(y) * step / b, y))
    i0, r0, i1 = images(ctx, left0, right0, left1)
    rng = np.random.default_rng(4)
    kps = np.stack([rng.uniform(60, w - 20, 200), rng.uniform(20, h - 20, 200)], 1).astype(np.float32)
    right, st, inv, pb = api.stereo_triangulate(i0, r0, cam0, cam1, b, kps)
    lm = np.nonzero(st == 1)[0]
    assert len(lm) > 150
    pose0 = np.array([0, 0, 0, 1.0, 0, 0, 0])
    R = kr.rot(cam0["extrinsic"][:4])
    pose1_true = np.concatenate([[0, 0, 0, 1.0], R @ np.array([step, 0.0, 0.0])])
    pose1_guess = pose1_true + np.array([0, 0, 0, 0, 0.05, -0.04, 0.02])
    cur, cls, good, _ = api.track_last_frame(i0, i1, cam0, b, pose1_guess, pb[lm], kps[lm])          # pose 0 is the identity: p_robot = p_world
    assert good > 100
    win = api.Window(ctx, cam0, cam1, baseline=b)
    win.add_keyframe(0, pose0, 46.0)
    for i in lm:
        win.add_landmark(int(i), 0, kps[i], right[i], inv[i])
    win.add_keyframe(1, pose1_guess, 46.0)
    for k, i in enumerate(lm):
        if cls[k] in (1, 2):
            win.add_observation(int(i), 1, cur[k])
    opt = api.default_solver_options(); opt.max_num_iterations = 10
    s = win.solve(opt)
    print(f"hand-over: {len(lm)} landmarks, {good} tracked, cost {s.initial_cost:.4e} -> {s.final_cost:.4e}, |t1 - truth| = {np.linalg.norm(win.pose(1)[4:] - pose1_true[4:]):.4f} m")
    assert s.num_residual_blocks > 0 and s.final_cost < s.initial_cost
    win.close()
    for im in (i0, r0, i1):
        im.close()
