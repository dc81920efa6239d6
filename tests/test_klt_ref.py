"""The declared feature tracker (tests/klt_ref.py) on the CPU: against the exact truth of analytic images, against a second formulation of
its integer stages (scipy), against a 50-digit statement of the DLT (mpmath), and on planted structure (window off the image, flat patch,
occlusion stripe).  The device is never compared with truth; it is compared with this restatement (tests/test_gpu_klt.py).

Measured with the restatement itself (float64, 640 x 376, 600 points per case; tests/klt_cases.py), and the bounds asserted below, which
are those figures with a 1.5x margin on the error or on the failing fraction:

  tracking (seeds 11, 12, 13)   status = 1: 98.8 / 96.3 / 95.3 %      -> >= 93 %      (1 - 1.5 * 4.7 %)
                                median error 0.035 / 0.052 / 0.048 px -> <= 0.078 px
                                p90 error    0.069 / 0.094 / 0.086 px -> <= 0.141 px
                                within 0.25 px 99.7 / 98.1 / 99.3 %   -> >= 97.15 %   (1 - 1.5 * 1.9 %)
  stereo (seeds 21, 22)         status = 1: 98.3 / 97.3 %             -> >= 95.9 %
                                median error 0.119 / 0.138 px         -> <= 0.207 px  (the window spans a disparity gradient)
                                p90 error    0.228 / 0.265 px         -> <= 0.40 px
  marginal points (the set the GPU test may leave out): 0 - 2 of 600 per case."""
import numpy as np
import pytest

from tests import klt_cases as kc
from tests import klt_ref as kr
from tests.helpers import assert_parity


def errors(nxt, st, truth):
    return np.linalg.norm(nxt.astype(np.float64) - truth, axis=1)[st > 0]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_tracking_against_truth(seed):
    c = kc.tracking_case(seed)
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(c["B"])
    nxt, st, _ = kr.optical_flow(A, B, c["prev"], c["init"])
    e = errors(nxt, st, c["truth"])
    print(f"tracking seed {seed}: status {st.mean():.4f} median {np.median(e):.4f} p90 {np.percentile(e, 90):.4f} within 0.25 px {(e < 0.25).mean():.4f}")
    assert st.mean() >= 0.93
    assert np.median(e) <= 0.078
    assert np.percentile(e, 90) <= 0.141
    assert (e < 0.25).mean() >= 0.9715


@pytest.mark.parametrize("seed", [21, 22])
def test_stereo_against_truth(seed):
    c = kc.stereo_case(seed)
    L, R = kr.Pyramid(c["left"]), kr.Pyramid(c["right"])
    pred = kr.stereo_predict(c["cam0"], c["cam1"], c["baseline"], c["kps"])
    # the reference's own prediction: depth 50 baselines = fx / 50 px of disparity (local_map.cpp:240-242)
    assert np.abs((c["kps"] - pred)[:, 0] - c["cam0"]["fx"] / 50).max() < 1e-3 and np.abs((c["kps"] - pred)[:, 1]).max() < 1e-3
    nxt, st, _ = kr.optical_flow(L, R, c["kps"], pred)
    e = errors(nxt, st, c["truth"])
    print(f"stereo seed {seed}: status {st.mean():.4f} median {np.median(e):.4f} p90 {np.percentile(e, 90):.4f}")
    assert st.mean() >= 0.959
    assert np.median(e) <= 0.207
    assert np.percentile(e, 90) <= 0.40


def test_float32_and_float64_agree():
    """The arithmetic precision is a parameter; the two agree far inside the 0.02 px the device is held to."""
    c = kc.tracking_case(12, n=200)
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(c["B"])
    n64, s64, _ = kr.optical_flow(A, B, c["prev"], c["init"], dtype=np.float64)
    n32, s32, _ = kr.optical_flow(A, B, c["prev"], c["init"], dtype=np.float32)
    both = (s64 > 0) & (s32 > 0)
    assert (s64 != s32).mean() <= 0.01
    assert np.abs(n64[both] - n32[both]).max() <= 5e-3


# ---- integer stages against a second formulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(640, 376), (1241, 376), (75, 53), (8, 5)])
def test_pyramid_and_scharr_against_scipy(w, h):
    from scipy.ndimage import correlate1d          # mode='mirror' is BORDER_REFLECT_101
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    p = kr.Pyramid(img, 3)
    g = img
    for L in range(4):
        assert p.gray[L].shape == g.shape and np.array_equal(p.gray[L], g), f"level {L}"
        i = g.astype(np.int64)
        sx = correlate1d(correlate1d(i, [-1, 0, 1], axis=1, mode="mirror"), [3, 10, 3], axis=0, mode="mirror")
        sy = correlate1d(correlate1d(i, [-1, 0, 1], axis=0, mode="mirror"), [3, 10, 3], axis=1, mode="mirror")
        assert p.deriv[L].dtype == np.int16
        assert np.array_equal(p.deriv[L][..., 0], sx) and np.array_equal(p.deriv[L][..., 1], sy), f"level {L}"
        s = correlate1d(correlate1d(i, [1, 4, 6, 4, 1], axis=0, mode="mirror"), [1, 4, 6, 4, 1], axis=1, mode="mirror")[::2, ::2]
        g = ((s + 128) >> 8).astype(np.uint8)
        assert g.shape == ((i.shape[0] + 1) // 2, (i.shape[1] + 1) // 2)


# ---- DLT against 50 digits ---------------------------------------------------------------------------------------------------------------------
def test_triangulate_against_mpmath():
    import mpmath as mp
    cam0, cam1, b = kc.rig()
    P0, P1 = kr.inv_matrix3x4(cam0["extrinsic"]), kr.inv_matrix3x4(cam1["extrinsic"])
    rng = np.random.default_rng(5)
    got, want = [], []
    with mp.workdps(50):
        for depth in np.concatenate([[2.0, 60.0], rng.uniform(2.0, 60.0, 30)]):
            ps = np.array([rng.uniform(-0.6, 0.6) * depth, rng.uniform(-0.35, 0.35) * depth, depth])
            s1 = ps - np.array([b, 0.0, 0.0])
            p0 = ps / ps[2] + np.append(rng.normal(0, 1e-4, 2), 0)          # rays that do not meet exactly, as tracked pixels give
            p1 = s1 / s1[2] + np.append(rng.normal(0, 1e-4, 2), 0)
            got.append(kr.triangulate(P0, P1, p0, p1))
            M = mp.matrix(kr.dlt_matrix(P0, P1, p0, p1).tolist())
            E, Q = mp.eigsy(M.T * M)                                         # 50 digits: squaring the condition number costs nothing here
            k = min(range(4), key=lambda i: E[i])
            want.append([float(Q[r, k] / Q[3, k]) for r in range(3)])
    assert_parity(np.array(got), np.array(want), "triangulate vs 50-digit DLT")
    # and the triangulated point is where it was put (rays nearly meet)
    pb, z0, inv = kr.stereo_depth(cam0, cam1, np.array([[300.0, 200.0]]), np.array([[300.0 - 460.0 * b / 12.5, 200.0]]))
    assert abs(z0[0] - 12.5) < 1e-4 and abs(inv[0] - 1 / 12.5) < 1e-6          # (the pixel is a float32: 1e-6 px of disparity)


# ---- structure ---------------------------------------------------------------------------------------------------------------------------------
def test_window_off_the_image_is_lost():
    c = kc.tracking_case(11, n=4)
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(c["B"])
    w, h = A.size
    prev = np.array([[-12.5, 50.0], [w + 10.5, 50.0], [100.0, -12.5], [100.0, h + 10.5], [100.0, 100.0]], np.float32)
    nxt, st = kr.lk(A, B, prev, prev, 21, 3)
    assert st.tolist()[:4] == [0, 0, 0, 0] and st[4] == 1
    _, ok, _ = kr.optical_flow(A, B, prev, prev)
    assert ok.tolist()[:4] == [0, 0, 0, 0]


def test_flat_patch_is_lost_through_min_eig():
    c = kc.tracking_case(12, n=4)
    A_img, B_img = c["A"].copy(), c["B"].copy()
    A_img[100:180, 200:280] = 128
    B_img[100:180, 200:280] = 128
    A, B = kr.Pyramid(A_img), kr.Pyramid(B_img)
    prev = np.array([[240.0, 140.0], [400.0, 250.0]], np.float32)
    d = {}
    _, st = kr.lk(A, B, prev, prev, 21, 3, detail=d)
    assert st.tolist() == [0, 1]
    assert d["min_eig0"][0] < 1e-4 < d["min_eig0"][1]


def test_occlusion_stripe_is_gated():
    c = kc.tracking_case(13, n=600)
    B_img = c["B"].copy()
    B_img[:, 300:380] = kr.Texture(99).image(kc.W, kc.H)[:, 300:380]
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(B_img)
    d = {}
    nxt, ok, fb = kr.optical_flow(A, B, c["prev"], c["init"], detail=d)
    inside = (c["truth"][:, 0] > 315) & (c["truth"][:, 0] < 365)
    both = (d["st"] > 0) & (d["rst"] > 0)
    gated = inside & both & (fb > kr.FB_MAX)
    print(f"stripe: {inside.sum()} points, {int((inside & both).sum())} with both passes alive, {int(gated.sum())} gated by fb, {int(ok[inside].sum())} accepted")
    assert gated.sum() >= 1 and not ok[gated].any()
    assert np.all(fb[ok > 0] <= kr.FB_MAX)
    # away from the stripe nothing changed
    # (a 21-px window at level 3 spans 168 px of level 0, and the decimation taps widen it further)
    clear = (np.abs(c["truth"][:, 0] - 340) > 180) & (np.abs(c["prev"][:, 0] - 340) > 180)
    assert clear.sum() > 100
    n0, ok0, _ = kr.optical_flow(kr.Pyramid(c["A"]), kr.Pyramid(c["B"]), c["prev"][clear], c["init"][clear])
    assert np.array_equal(ok0, ok[clear]) and np.array_equal(n0, nxt[clear])


def test_track_last_frame_classes_and_gate():
    c = kc.track_case(31, n=300)
    A, B = kr.Pyramid(c["A"]), kr.Pyramid(c["B"])
    cur, cls, good = kr.track_last_frame(A, B, c["cam0"], c["baseline"], c["pose"], c["pw"], c["prev"])
    counts = np.bincount(cls, minlength=4)
    assert counts.min() >= 1, counts                       # every class occurs
    assert good == counts[kr.FAR] + counts[kr.NEAR]
    _, _, none = kr.track_last_frame(A, B, c["cam0"], c["baseline"], c["pose"], c["pw"], c["prev"], num_features_tracking_bad=int(good))
    assert none == 0                                       # the gate is a strict >
    _, cls2, _ = kr.track_last_frame(A, B, c["cam0"], c["baseline"], c["pose"], c["pw"], c["prev"], remove_moving_points=False)
    assert not (cls2 == kr.MOVING).any() and np.array_equal(cls2 == kr.FAR, cls == kr.FAR)
    z = kr.world2sensor(c["cam0"], c["pw"], c["pose"])[:, 2]
    assert np.array_equal((cls == kr.FAR), (cls != kr.LOST) & (z > 50 * c["baseline"]))
