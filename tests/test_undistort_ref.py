"""The declared image undistortion (tests/undistort_ref.py) on the CPU: its map against an exact rational evaluation of the distortion model,
its remap against the fp64 bilinear value at the quantised coordinate, planted border structure, the identity for zero coefficients and the
exact truth of an analytic image.  The device is never compared with truth; it is compared with this restatement
(tests/test_gpu_undistort.py).

Analytic truth (test_analytic_truth), measured with the restatement itself at 253 x 131, focal length 0.45 of the width, texture seed 5,
over the pixels whose four taps are inside; the bounds asserted are these figures times 1.5:

  set          max |error|   mean |error|   (grey levels)
  barrel         12            1.3399        -> <= 18.0, <= 2.010
  pincushion      7            0.5529        -> <= 10.5, <= 0.830
  euroc          11            1.3040        -> <= 16.5, <= 1.956

The error is that of bilinear interpolation between uint8-rounded samples of a texture with wavelengths down to 8 px, not of the map: a
barrel lens compresses the scene in the raw frame (shorter wavelengths there, a larger error), a pincushion lens stretches it."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import klt_ref as kr
from tests import undistort_cases as uc
from tests import undistort_ref as ur

W, H = 67, 45
TRUTH_BOUNDS = {"barrel": (18.0, 2.010), "pincushion": (10.5, 0.830), "euroc": (16.5, 1.956)}


@pytest.fixture(scope="module")
def maps():
    """the 67 x 45 maps of every set, with (iu, iv); shared and left unchanged"""
    out = {}
    for name, d in uc.SETS.items():
        detail = {}
        xy, frac = ur.build_map(uc.camera(W, H), d, W, H, detail)
        out[name] = (xy, frac, detail["iu"], detail["iv"])
    return out


@pytest.fixture(scope="module", autouse=True)
def not_vacuous(maps):
    """before anything else: every non-zero set leaves at least 1 % zero-filled pixels and at least 50 % with all four taps inside"""
    for name in uc.NONZERO:
        xy = maps[name][0]
        sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
        none = (sx + 1 < 0) | (sx >= W) | (sy + 1 < 0) | (sy >= H)
        _, full = ur.coverage(xy, W, H)
        print(f"{name}: {100 * none.mean():.1f} % zero-filled, {100 * full:.1f} % fully inside")
        assert none.mean() >= 0.01 and full >= 0.50, name
        assert np.all(ur.remap(uc.raw_image(W, H) | 1, xy, maps[name][1])[none] == 0)


def test_header_and_ctypes_surface():
    from lvio_fusion_amd import _lib
    assert C.sizeof(_lib.Distortion) == 4 * 8
    names = ("lvf_undistort_create", "lvf_undistort_destroy", "lvf_undistort_download_map", "lvf_image_create_undistorted", "lvf_image_pair_create_undistorted")
    assert set(names) <= set(_lib.declared_symbols()) and set(names) <= set(_lib._SIGS)
    _lib.build()
    so = C.CDLL(_lib.SO_PATH)
    assert all(hasattr(so, n) for n in names)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 45), (253, 131), (4096, 8), (8, 4096)])
def test_zero_distortion_is_the_identity(w, h):
    raw = uc.raw_image(w, h)
    cam = uc.camera(w, h)
    assert cam["cx"] != np.floor(cam["cx"]) and cam["cy"] != np.floor(cam["cy"])
    for cam in (cam, dict(cam, fx=718.856, fy=718.856, cx=w * 0.4893, cy=h * 0.4927)):
        xy, frac = ur.build_map(cam, uc.ZERO, w, h)
        assert not frac.any()
        assert np.array_equal(xy[..., 0], np.broadcast_to(np.arange(w, dtype=np.int16)[None, :], (h, w)))
        assert np.array_equal(xy[..., 1], np.broadcast_to(np.arange(h, dtype=np.int16)[:, None], (h, w)))
        assert np.array_equal(ur.remap(raw, xy, frac), raw)
        assert np.array_equal(ur.undistort(raw, cam, None), raw)


@pytest.mark.parametrize("name", uc.NONZERO)
def test_map_against_exact_rational_model(maps, name):
    """the distortion model evaluated in exact rational arithmetic on the same (binary) inputs: the fixed-point coordinate is within half a
    step (1 / 64 px) of it"""
    cam = uc.camera(W, H)
    fx, fy, cx, cy = (Fraction(float(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2 = (Fraction(float(c)) for c in uc.SETS[name])
    _, _, iu, iv = maps[name]
    worst = Fraction(0)
    for i in range(H):
        y = (i - cy) / fy
        for j in range(W):
            x = (j - cx) / fx
            r2 = x * x + y * y
            kr_ = 1 + (k2 * r2 + k1) * r2
            u = fx * (x * kr_ + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
            v = fy * (y * kr_ + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
            worst = max(worst, abs(Fraction(int(iu[i, j]), 32) - u), abs(Fraction(int(iv[i, j]), 32) - v))
    print(f"{name}: max |iu / 32 - u_exact| = {float(worst):.9f} px")
    assert float(worst) <= 1 / 64 + 1e-9


@pytest.mark.parametrize("name", uc.NONZERO)
def test_remap_against_fp64_bilinear(maps, name):
    """a second formulation: floating-point bilinear interpolation at (sx + a / 32, sy + b / 32), exact in fp64 (dyadic weights)"""
    xy, frac = maps[name][:2]
    raw = uc.raw_image(W, H, seed=3)
    out = ur.remap(raw, xy, frac)
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = raw
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    near = (sx >= -1) & (sx < W) & (sy >= -1) & (sy < H)                   # (elsewhere all four taps are outside: exact value 0)
    px, py = np.clip(sx, -1, W - 1) + 1, np.clip(sy, -1, H - 1) + 1
    fa, fb = (frac & 31) / 32.0, ((frac >> 5) & 31) / 32.0
    exact = (1 - fb) * ((1 - fa) * pad[py, px] + fa * pad[py, px + 1]) + fb * ((1 - fa) * pad[py + 1, px] + fa * pad[py + 1, px + 1])
    exact = np.where(near, exact, 0.0)
    assert np.abs(out - exact).max() <= 0.5
    tie = (exact * 1024) % 1024 == 512
    assert np.array_equal(out[~tie], np.floor(exact + 0.5).astype(np.uint8)[~tie])
    assert np.array_equal(out[tie], (exact[tie] + 0.5).astype(np.uint8))   # (a tie rounds up)
    assert near.mean() > 0.5 and (~near).any()


def test_planted_border_structure():
    raw = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)                 # 3 x 2
    half = 16 * 32 + 16                                                    # a = b = 16: all four weights 256
    cases = [((-5, 0), half, 0), ((3, 0), half, 0), ((0, -2), half, 0), ((0, 2), half, 0), ((-2, -2), 0, 0),     # fully outside
             ((-1, -1), half, (10 * 256 + 512) >> 10),                                                       # one tap: p11 = raw[0, 0]
             ((2, 1), half, (60 * 256 + 512) >> 10),                                                         # one tap: p00 = raw[1, 2]
             ((-1, 0), half, ((10 + 40) * 256 + 512) >> 10),                                                 # two taps: the left column
             ((1, 1), half, ((50 + 60) * 256 + 512) >> 10),                                                  # two taps: the bottom row
             ((2, 0), 0, 30), ((0, 1), 0, 40),                                                                # fraction 0 at the edge: the pixel itself
             ((0, 0), half, (10 + 20 + 40 + 50 + 2) >> 2),                                                   # all four
             ((1, 0), 31, (20 * 32 + 30 * 992 + 512) >> 10)]                                                 # a = 31, b = 0
    xy = np.array([c[0] for c in cases], np.int16).reshape(1, -1, 2)
    frac = np.array([c[1] for c in cases], np.uint16).reshape(1, -1)
    assert ur.remap(raw, xy, frac)[0].tolist() == [c[2] for c in cases]
    # every position of the tap square around and across a 9 x 7 image: a 2 x 2 square meets a rectangle in 0, 1, 2 or 4 pixels (never in
    # three: that needs a concave corner), and whatever is inside keeps its weight
    big = uc.raw_image(9, 7, seed=1)
    seen = set()
    for sy in range(-3, 9):
        for sx in range(-3, 11):
            at = np.array([[[sx, sy]]], np.int16)
            p, inside = ur.taps(big, at)
            seen.add(sum(int(m[0, 0]) for m in inside))
            want = sum((int(big[sy + dy, sx + dx]) if 0 <= sx + dx < 9 and 0 <= sy + dy < 7 else 0) * wt
                       for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (17 * 27, 15 * 27, 17 * 5, 15 * 5)))      # a = 15, b = 5
            assert int(ur.remap(big, at, np.array([[5 * 32 + 15]], np.uint16))[0, 0]) == (want + 512) >> 10
    assert seen == {0, 1, 2, 4}


def test_saturated_coordinates_give_zero():
    """coefficients that throw the corners past the int16 (and the int32) range: the map saturates and the pixel is 0"""
    cam = uc.camera(W, H)
    raw = uc.raw_image(W, H) | 1
    for dist in ((4.0e3, 0.0, 0.0, 0.0), (0.0, -6.0e9, 0.0, 0.0), (1e300, 1e300, 0.0, 0.0)):
        detail = {}
        xy, frac = ur.build_map(cam, dist, W, H, detail)
        sat = (np.abs(detail["iu"] >> 5) > 32767) | (np.abs(detail["iv"] >> 5) > 32767)
        assert sat.any()
        assert np.all((xy[sat] == 32767).any(-1) | (xy[sat] == -32768).any(-1))
        assert np.all(ur.remap(raw, xy, frac)[sat] == 0)
    assert (detail["iu"] == ur.INT32_MIN).any() or (detail["iu"] == ur.INT32_MAX).any()


@pytest.mark.parametrize("name", uc.NONZERO)
def test_analytic_truth(name):
    """a raw frame = the texture seen through the lens (sampled at the undistorted position of every raw pixel); undistorting it gives the
    texture sampled on the pixel grid"""
    w, h = 253, 131
    cam, dist = uc.camera(w, h, f=0.45), uc.SETS[name]
    tex = kr.Texture(5)
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ux, uy, res = uc.undistort_points(cam, dist, jj, ii)
    assert res.max() < 1e-9                                                 # the inverse map is exact to 1e-9 px on the whole raw frame
    raw = tex.image(w, h, lambda x, y: (ux, uy))
    xy, frac = ur.build_map(cam, dist, w, h)
    out = ur.remap(raw, xy, frac)
    _, full_fraction = ur.coverage(xy, w, h)
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    full = (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
    assert full.mean() == full_fraction and full.mean() > 0.5
    err = np.abs(out.astype(np.float64) - tex.image(w, h).astype(np.float64))[full]
    print(f"{name}: {full.sum()} pixels, max |error| {err.max():.3f}, mean {err.mean():.4f}")
    assert err.max() <= TRUTH_BOUNDS[name][0] and err.mean() <= TRUTH_BOUNDS[name][1]
