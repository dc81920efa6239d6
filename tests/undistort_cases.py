"""Cameras, coefficient sets and images for the undistortion tests (tests/test_undistort_ref.py on the CPU, tests/test_gpu_undistort.py on
the device).  The wide camera's focal length is 0.24 of the image width, so that the corners lie at a normalised radius above 2: there the
k2 r^4 term of the barrel sets has turned the map outwards and every non-zero set leaves both zero-filled corners and a fully-inside middle
(asserted in test_undistort_ref.py before anything else is looked at)."""
import numpy as np

BARREL = (-0.30, 0.08, 0.0, 0.0)
PINCUSHION = (0.25, -0.05, 0.0, 0.0)
EUROC = (-0.28, 0.07, 2e-3, -1.5e-3)          # EuRoC-like: radial plus tangential
ZERO = (0.0, 0.0, 0.0, 0.0)
SETS = {"barrel": BARREL, "pincushion": PINCUSHION, "euroc": EUROC, "zero": ZERO}
NONZERO = ("barrel", "pincushion", "euroc")


def camera(w, h, f=0.24):
    """non-integer principal point, fx != fy"""
    return dict(fx=f * w, fy=1.02 * f * w, cx=w / 2 - 0.3, cy=h / 2 + 0.2, extrinsic=np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))


def raw_image(w, h, seed=0, pad=0):
    """uniform random bytes (every tap matters to the result); pad > 0: a view with a padded row stride"""
    buf = np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w + pad), dtype=np.uint8)
    return buf[:, :w]


def undistort_points(cam, dist, u, v, iterations=40):
    """Inverse of undistort_ref.distort in pixel coordinates: (px, py) with distort(px, py) = (u, v), by Newton's method with a central-
    difference Jacobian (the step is self-correcting, so the Jacobian's accuracy only affects the speed).  Returns px, py and the residual."""
    from tests import undistort_ref as ur
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    px, py = u.copy(), v.copy()
    e = 1e-4
    for _ in range(iterations):
        fu, fv = ur.distort(cam, dist, px, py)
        au, av = ur.distort(cam, dist, px + e, py)
        bu, bv = ur.distort(cam, dist, px - e, py)
        cu, cv = ur.distort(cam, dist, px, py + e)
        du, dv = ur.distort(cam, dist, px, py - e)
        j00, j10 = (au - bu) / (2 * e), (av - bv) / (2 * e)
        j01, j11 = (cu - du) / (2 * e), (cv - dv) / (2 * e)
        ru, rv = fu - u, fv - v
        det = j00 * j11 - j01 * j10
        px = px - (j11 * ru - j01 * rv) / det
        py = py - (-j10 * ru + j00 * rv) / det
    fu, fv = ur.distort(cam, dist, px, py)
    return px, py, np.maximum(np.abs(fu - u), np.abs(fv - v))
