"""The declared image undistortion in numpy: what lvio_fusion_amd/csrc/undistort_kernels.hip is bit equal to.

It restates the cv::undistort of Estimator::InputImage (estimator.cpp:178-179) for the K, D of Camera (camera.h:22-26, 81-89), keeping
OpenCV's structure: initUndistortRectifyMap with R = I and the new camera matrix = K into a fixed-point map (integer source pixel as
CV_16SC2 plus 5-bit fractions), then remap(INTER_LINEAR, BORDER_CONSTANT 0).  The semantics are DECLARED, not pinned: OpenCV is not
compared with, and where this file leaves OpenCV it does so on purpose:

  * the map is evaluated DIRECTLY per pixel.  OpenCV advances x and y along a row by running sums (x += ir[0], ...); those are sequential,
    they differ from the direct evaluation by rounding noise of a few ulp, and that changes nothing that matters: a source coordinate
    moves by 1 / 32 px only where 32 u lies within that noise of a half-integer.
  * every fp64 operation is rounded separately, in the order written in build_map (no fused multiply-add; OpenCV's SIMD paths may fuse).
  * D = (k1, k2, p1, p2, 0) as camera.h:89 has it: k3, the rational and the thin-prism terms are zero and are not evaluated.
  * the four bilinear weights are the exact integers (32 - a)(32 - b), a (32 - b), (32 - a) b, a b, which sum to 1024, and
    out = (sum + 512) >> 10.  OpenCV's table holds saturate_cast<short>(w * 32768) (these same products times 32) and then adjusts one
    entry where the rounded floats do not sum to 32768; with 5-bit fractions the products are exact, so there is nothing to adjust and
    no adjustment is reproduced.  out is the round-half-up of the exact bilinear value at the quantised coordinate.
  * the border is per TAP: a tap outside the image reads 0 and a pixel half outside keeps its inside taps (what BORDER_CONSTANT does in
    remap's slow path; OpenCV's fast path agrees where all four taps are inside).
  * rint(32 u) is half-to-even and saturates to int32 (NaN -> INT32_MIN, as the x86 conversion gives); the integer part saturates to int16.
    A saturated coordinate is far outside any image this library takes (sides <= 4096), so such a pixel is 0.

With all four coefficients zero, u = fx ((j - cx) / fx) + cx differs from j by a few ulp, rint(32 u) = 32 j, the fractions are 0 and the
output equals the input bit for bit."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def distort(cam, dist, px, py):
    """(u, v) in fp64 of the declared model at the pixel coordinates (px, py): every operation separately rounded, in this order."""
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2 = (np.float64(c) for c in dist)
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    with np.errstate(all="ignore"):
        x = (px - cx) / fx
        y = (py - cy) / fy
        r2 = x * x + y * y
        kr = 1.0 + (k2 * r2 + k1) * r2
        xy2 = 2.0 * x * y
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x * x)
        yd = y * kr + p1 * (r2 + 2.0 * y * y) + p2 * xy2
        u = fx * xd + cx
        v = fy * yd + cy
    return u, v


def fix5(v):
    """rint(32 v), half to even, saturated to int32 (NaN -> INT32_MIN)"""
    with np.errstate(all="ignore"):
        r = np.rint(32.0 * v)
    nan = np.isnan(r)
    r = np.clip(np.where(nan, 0.0, r), float(INT32_MIN), float(INT32_MAX))
    return np.where(nan, INT32_MIN, r.astype(np.int64)).astype(np.int64)


def build_map(cam, dist, w, h, detail=None):
    """xy [h, w, 2] int16 = the top-left tap (sx, sy); frac [h, w] uint16 = b * 32 + a.  detail (a dict) receives iu, iv (int64)."""
    dist = (0.0, 0.0, 0.0, 0.0) if dist is None else dist
    j, i = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    u, v = distort(cam, dist, j, i)
    iu, iv = np.broadcast_to(fix5(u), (h, w)), np.broadcast_to(fix5(v), (h, w))
    if detail is not None:
        detail.update(iu=iu, iv=iv)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], -1).astype(np.int16)
    frac = (((iv & 31) << 5) | (iu & 31)).astype(np.uint16)
    return xy, frac


def taps(raw, xy):
    """The four taps p00, p01, p10, p11 [h, w] int64 (0 outside the image) and their inside masks."""
    sh, sw = raw.shape
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    vals, inside = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = sx + dx, sy + dy
            ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
            vals.append(np.where(ok, raw[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64), 0))
            inside.append(ok)
    return vals, inside


def remap(raw, xy, frac):
    """remap(INTER_LINEAR, BORDER_CONSTANT 0) of the uint8 image `raw` through the map: uint8 of the map's shape."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2
    (p00, p01, p10, p11), _ = taps(raw, xy)
    a, b = (frac & 31).astype(np.int64), ((frac >> 5) & 31).astype(np.int64)
    acc = p00 * ((32 - a) * (32 - b)) + p01 * (a * (32 - b)) + p10 * ((32 - a) * b) + p11 * (a * b)
    return ((acc + 512) >> 10).astype(np.uint8)


def coverage(xy, w, h):
    """(fraction of pixels with at least one tap outside a w x h source, fraction with all four inside)"""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    full = (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
    return 1.0 - full.mean(), full.mean()


def undistort(raw, cam, dist):
    raw = np.asarray(raw)
    xy, frac = build_map(cam, dist, raw.shape[1], raw.shape[0])
    return remap(raw, xy, frac)
