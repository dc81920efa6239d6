"""CPU restatement of the feature tracker: pyramidal Lucas-Kanade flow with the forward-backward gate (utility.cpp:55-89), the stereo
triangulation built on it (utility.cpp:7-18, local_map.cpp:233-269) and the numeric part of Frontend::TrackLastFrame (frontend.cpp:163-233).

The semantics are DECLARED here, not pinned to OpenCV bit for bit: OpenCV is neither installed nor vendored by the reference, so this file
writes down once what `cv::calcOpticalFlowPyrLK` is taken to compute and the device (lvio_fusion_amd/csrc/klt_kernels.hip) is
checked against it.  It follows the structure of OpenCV's tracker (pyramid by 5-tap decimation, unnormalised Scharr derivatives, the
2^-20 / 2^-15 scales of the normal equations, the level-skip and status rules, the oscillation stop) but interpolates in floating point:
OpenCV's fixed-point rounding of the interpolated patch (5 fractional bits, W_BITS = 14) is deliberately not reproduced.

Images are uint8, points are float32 (cv::Point2f); the arithmetic precision is the `dtype` parameter (float64 or float32).
Poses and extrinsics are Sophus SE3d::data() = [qx, qy, qz, qw, tx, ty, tz]."""
import numpy as np

FLT_EPSILON = 1.1920929e-07
TRACK_WIN, TRACK_LEVELS = 21, 3          # utility.cpp:64
BACK_WIN, BACK_LEVELS = 3, 1             # utility.cpp:71
FB_MAX = 0.5                             # utility.cpp:79


# ---- images --------------------------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    """BORDER_REFLECT_101 index (gfedcb|abcdefgh|gfedcba) for any integer i, any n >= 1."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = 2 * (n - 1)
    r = np.mod(i, m)
    return np.where(r >= n, m - r, r)


def pyr_down(img):
    """Separable [1 4 6 4 1] decimation, reflect-101, size ((w+1)/2, (h+1)/2), value (sum + 128) >> 8."""
    h, w = img.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int32)
    tmp = np.zeros((h2, w), np.int32)
    for t in range(5):
        tmp += k[t] * src[reflect101(2 * np.arange(h2) + t - 2, h), :]
    out = np.zeros((h2, w2), np.int32)
    for t in range(5):
        out += k[t] * tmp[:, reflect101(2 * np.arange(w2) + t - 2, w)]
    return ((out + 128) >> 8).astype(np.uint8)


def scharr(img):
    """Unnormalised Scharr pair on the uint8 image, exact int16, reflect-101 at the edge: [h, w, 2] = (Sx, Sy)."""
    h, w = img.shape
    s = img.astype(np.int32)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    g = lambda ys, xs: s[ys][:, xs]
    y0, x0 = np.arange(h), np.arange(w)
    sx = 3 * (g(ym, xp) - g(ym, xm)) + 10 * (g(y0, xp) - g(y0, xm)) + 3 * (g(yp, xp) - g(yp, xm))
    sy = 3 * (g(yp, xm) - g(ym, xm)) + 10 * (g(yp, x0) - g(ym, x0)) + 3 * (g(yp, xp) - g(ym, xp))
    return np.stack([sx, sy], axis=-1).astype(np.int16)


class Pyramid:
    """max_level + 1 levels of the uint8 image and their Scharr pairs (what the device image object holds)."""

    def __init__(self, img, max_level=TRACK_LEVELS):
        img = np.ascontiguousarray(img)
        assert img.dtype == np.uint8 and img.ndim == 2
        self.gray = [img]
        for _ in range(max_level):
            self.gray.append(pyr_down(self.gray[-1]))
        self.deriv = [scharr(g) for g in self.gray]
        self._pad = {}

    @property
    def size(self):
        return self.gray[0].shape[1], self.gray[0].shape[0]

    def padded(self, level, win, dtype):
        """Level image extended by reflect-101 and its derivative extended by zeros, far enough for every window that passes the bounds test."""
        key = (level, win, np.dtype(dtype).name)
        if key not in self._pad:
            g, d = self.gray[level], self.deriv[level]
            h, w = g.shape
            pad = win + 2
            iy, ix = reflect101(np.arange(-pad, h + pad), h), reflect101(np.arange(-pad, w + pad), w)
            gp = g[iy][:, ix].astype(dtype)
            dp = np.zeros((h + 2 * pad, w + 2 * pad, 2), dtype)
            dp[pad:pad + h, pad:pad + w] = d
            self._pad[key] = (gp, dp, pad)
        return self._pad[key]


def _bilinear(arr, pad, win, p, T):
    """win x win samples of arr (2-D or [.., 2]) at p + (x, y), x, y = 0 .. win-1."""
    ix, iy = int(np.floor(p[0])), int(np.floor(p[1]))
    a, b = T(p[0] - T(ix)), T(p[1] - T(iy))
    one = T(1)
    w00, w01, w10, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    y0, x0 = iy + pad, ix + pad
    t = arr[y0:y0 + win + 1, x0:x0 + win + 1]
    return w00 * t[:-1, :-1] + w01 * t[:-1, 1:] + w10 * t[1:, :-1] + w11 * t[1:, 1:]


def _outside(p, win, cols, rows):
    ix, iy = int(np.floor(p[0])), int(np.floor(p[1]))
    return ix < -win or ix >= cols or iy < -win or iy >= rows


def _margin(p, win, cols, rows):
    """distance of p to the nearest point where the bounds test flips"""
    return min(abs(float(p[0]) + win), abs(float(p[0]) - cols), abs(float(p[1]) + win), abs(float(p[1]) - rows))


# ---- one tracker pass ----------------------------------------------------------------------------------------------------------------------
def lk(A, B, prev, next_init, win, max_level, max_iter=30, eps=0.01, min_eig=1e-4, dtype=np.float64, detail=None):
    """calcOpticalFlowPyrLK(A, B, prev, next, status, err, (win, win), max_level, COUNT + EPS (max_iter, eps), USE_INITIAL_FLOW, min_eig) as
    declared: returns next [n, 2] float32 and status [n] uint8.  `detail`, if a dict, receives per point `min_eig0` (minEig at level 0, nan
    when not reached) and `margin` (the smallest distance of any tested window corner to a flip of its bounds test)."""
    T = np.dtype(dtype).type
    prev = np.asarray(prev, np.float32).reshape(-1, 2)
    next_init = np.asarray(next_init, np.float32).reshape(-1, 2)
    n = len(prev)
    out = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    mineig0 = np.full(n, np.nan)
    margin = np.full(n, np.inf)
    half = T((win - 1) * 0.5)
    eps2 = T(eps) * T(eps)
    sA, sb = T(2.0 ** -20), T(2.0 ** -15)
    for i in range(n):
        nxt = None
        for L in range(max_level, -1, -1):
            gA, dA, pad = A.padded(L, win, dtype)
            gB, _, _ = B.padded(L, win, dtype)
            rows, cols = A.gray[L].shape
            scale = T(2.0 ** -L)
            p = np.array([T(prev[i, 0]) * scale - half, T(prev[i, 1]) * scale - half], dtype)
            nxt = np.array([T(next_init[i, 0]) * scale, T(next_init[i, 1]) * scale], dtype) if L == max_level else nxt * T(2)
            margin[i] = min(margin[i], _margin(p, win, cols, rows))
            if _outside(p, win, cols, rows):
                if L == 0:
                    status[i] = 0
                continue
            I = _bilinear(gA, pad, win, p, T)
            S = _bilinear(dA, pad, win, p, T)
            Sx, Sy = S[..., 0], S[..., 1]
            A11, A12, A22 = np.sum(Sx * Sx) * sA, np.sum(Sx * Sy) * sA, np.sum(Sy * Sy) * sA
            D = A11 * A22 - A12 * A12
            me = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + T(4) * A12 * A12)) / T(2 * win * win)
            if L == 0:
                mineig0[i] = me
            if me < T(min_eig) or D < T(FLT_EPSILON):
                if L == 0:
                    status[i] = 0
                continue
            q = nxt - half
            dprev = np.zeros(2, dtype)
            for j in range(max_iter):
                margin[i] = min(margin[i], _margin(q, win, cols, rows))
                if _outside(q, win, cols, rows):
                    if L == 0:
                        status[i] = 0
                    break
                diff = _bilinear(gB, pad, win, q, T) - I
                b1, b2 = np.sum(diff * Sx) * sb, np.sum(diff * Sy) * sb
                d = np.array([(A12 * b2 - A22 * b1) / D, (A12 * b1 - A11 * b2) / D], dtype)
                q = q + d
                nxt = q + half
                if d[0] * d[0] + d[1] * d[1] <= eps2:
                    break
                if j > 0 and abs(d[0] + dprev[0]) < T(0.01) and abs(d[1] + dprev[1]) < T(0.01):
                    nxt = nxt - d * T(0.5)
                    break
                dprev = d
        out[i] = nxt.astype(np.float32)
    if detail is not None:
        detail["min_eig0"], detail["margin"] = mineig0, margin
    return out, status


def optical_flow(A, B, prev, next_init, win=TRACK_WIN, levels=TRACK_LEVELS, back_win=BACK_WIN, back_levels=BACK_LEVELS, max_iter=30, eps=0.01,
                 min_eig=1e-4, fb_max=FB_MAX, dtype=np.float64, detail=None):
    """optical_flow (utility.cpp:55-89): forward pass, 3x3 / 1-level backward pass started at prev, forward-backward and in-image gate.
    Returns next [n, 2] float32, status [n] uint8, fb [n] float64 (the forward-backward distance; inf where a pass failed)."""
    prev = np.asarray(prev, np.float32).reshape(-1, 2)
    df, db = ({}, {}) if detail is not None else (None, None)
    nxt, st = lk(A, B, prev, next_init, win, levels, max_iter, eps, min_eig, dtype, df)
    back, rst = lk(B, A, nxt, prev, back_win, back_levels, max_iter, eps, min_eig, dtype, db)
    d = (prev - back).astype(np.float32).astype(np.float64)           # cv_distance: float differences, double norm (utility.cpp:20-25)
    fb = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    cols, rows = A.size
    ok = (st > 0) & (rst > 0) & (fb <= fb_max) & (nxt[:, 0] >= 0) & (nxt[:, 0] < cols) & (nxt[:, 1] >= 0) & (nxt[:, 1] < rows)
    if detail is not None:
        detail.update(forward=df, backward=db, st=st, rst=rst)
    return nxt, ok.astype(np.uint8), np.where((st > 0) & (rst > 0), fb, np.inf)


def marginal(A, B, prev, next_init, tol=0.02, **kw):
    """float64 and float32 runs of optical_flow plus the set of points whose status is not decided with room (see tests/test_gpu_klt.py):
    returns (next64, status64, fb64, marginal mask)."""
    d64 = {}
    n64, s64, f64 = optical_flow(A, B, prev, next_init, dtype=np.float64, detail=d64, **kw)
    n32, s32, _ = optical_flow(A, B, prev, next_init, dtype=np.float32, **kw)
    cols, rows = A.size
    fb_max, min_eig = kw.get("fb_max", FB_MAX), kw.get("min_eig", 1e-4)
    m = np.abs(f64 - fb_max) < tol
    for d in (d64["forward"], d64["backward"]):
        me = d["min_eig0"]
        m |= np.isfinite(me) & (np.abs(me - min_eig) <= 0.01 * min_eig)
        m |= d["margin"] < tol
    edge = np.minimum.reduce([np.abs(n64[:, 0]), np.abs(n64[:, 0] - cols), np.abs(n64[:, 1]), np.abs(n64[:, 1] - rows)])
    m |= edge < tol
    m |= s32 != s64
    m |= (s64 > 0) & (s32 > 0) & (np.abs(n32.astype(np.float64) - n64).max(axis=1) > tol)
    return n64, s64, f64, m


# ---- geometry (fp64) -----------------------------------------------------------------------------------------------------------------------
def rot(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def se3_apply(T7, p):
    T7 = np.asarray(T7, np.float64)
    return np.asarray(p, np.float64) @ rot(T7[:4]).T + T7[4:]


def se3_inv_apply(T7, p):
    T7 = np.asarray(T7, np.float64)
    return (np.asarray(p, np.float64) - T7[4:]) @ rot(T7[:4])


def inv_matrix3x4(T7):
    """SE3d(T7).inverse().matrix3x4()"""
    T7 = np.asarray(T7, np.float64)
    R = rot(T7[:4]).T
    return np.hstack([R, (-R @ T7[4:])[:, None]])


def pixel2sensor(cam, px, depth=1.0):            # camera.h:51-57
    px = np.asarray(px, np.float64)
    return np.stack([(px[..., 0] - cam["cx"]) * depth / cam["fx"], (px[..., 1] - cam["cy"]) * depth / cam["fy"], np.full(px.shape[:-1], float(depth))], -1)


def sensor2pixel(cam, pc):                       # camera.h:44-49
    return np.stack([cam["fx"] * pc[..., 0] / pc[..., 2] + cam["cx"], cam["fy"] * pc[..., 1] / pc[..., 2] + cam["cy"]], -1)


def robot2sensor(cam, pb):                       # sensor.h:36-39
    return se3_inv_apply(cam["extrinsic"], pb)


def world2sensor(cam, pw, Twc):                  # sensor.h:16-19
    return se3_inv_apply(cam["extrinsic"], se3_inv_apply(Twc, pw))


def dlt_matrix(P0, P1, p0, p1):
    return np.stack([p0[0] * P0[2] - P0[0], p0[1] * P0[2] - P0[1], p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1]])


def triangulate(P0, P1, p0, p1):
    """triangulate (utility.cpp:7-18): right singular vector of the smallest singular value of the 4x4 DLT matrix, dehomogenised."""
    v = np.linalg.svd(dlt_matrix(P0, P1, p0, p1))[2][3]
    return v[:3] / v[3]


def stereo_predict(cam0, cam1, baseline, kps_left):
    """local_map.cpp:240-242: the left pixel at depth 50 * baseline, seen by camera 1 (rounded to cv::Point2f)."""
    pb = se3_apply(cam0["extrinsic"], pixel2sensor(cam0, np.asarray(kps_left, np.float32), baseline * 50))
    return sensor2pixel(cam1, robot2sensor(cam1, pb)).astype(np.float32)


def stereo_depth(cam0, cam1, kps_left, kps_right):
    """local_map.cpp:252-258 for every pair: p_robot [n, 3], the gated depth Robot2Sensor_0(pb).z and inv_depth = 1 / Robot2Sensor_1(pb).z —
    camera ONE in the last (local_map.cpp:258), as the reference has it."""
    P0, P1 = inv_matrix3x4(cam0["extrinsic"]), inv_matrix3x4(cam1["extrinsic"])
    s0, s1 = pixel2sensor(cam0, np.asarray(kps_left, np.float32)), pixel2sensor(cam1, np.asarray(kps_right, np.float32))
    pb = np.array([triangulate(P0, P1, a, b) for a, b in zip(s0, s1)]).reshape(-1, 3)
    z0 = robot2sensor(cam0, pb)[:, 2]
    return pb, z0, 1.0 / robot2sensor(cam1, pb)[:, 2]


LOST, FAR, NEAR, MOVING = 0, 1, 2, 3


def classify(cam0, baseline, pose, pw, predictions, tracked, status, remove_moving_points=True, num_features_tracking_bad=20):
    """frontend.cpp:195-256 given the flow's result: class per point, the number of good points, and the deviation norms."""
    predictions, tracked = np.asarray(predictions, np.float32), np.asarray(tracked, np.float32)
    ok = np.asarray(status) > 0
    dev = np.where(ok[:, None], (predictions - tracked).astype(np.float64), 0.0)        # Point2f difference
    dev = dev - dev.sum(axis=0) / max(1, int(ok.sum()))
    norm = np.sqrt(dev[:, 0] ** 2 + dev[:, 1] ** 2)
    z = world2sensor(cam0, pw, pose)[:, 2]
    far = z > baseline * 50                                                             # camera.h:38-41
    cls = np.where(far, FAR, np.where((not remove_moving_points) | (norm < 30), NEAR, MOVING))
    cls = np.where(ok, cls, LOST).astype(np.uint8)
    n = int(((cls == FAR) | (cls == NEAR)).sum())
    return cls, (n if n > num_features_tracking_bad else 0), norm, z


def track_predict(cam0, pose, pw):
    """frontend.cpp:168-170: World2Pixel(pw, current pose), rounded to cv::Point2f."""
    return sensor2pixel(cam0, world2sensor(cam0, pw, pose)).astype(np.float32)


def stereo_triangulate(L, R, cam0, cam1, baseline, kps_left, **kw):
    """LocalMap::Triangulate (local_map.cpp:233-269): right pixels, status (0 lost, 1 accepted, 2 tracked but behind camera 0), inv_depth, p_robot."""
    kps_left = np.asarray(kps_left, np.float32).reshape(-1, 2)
    right, st, _ = optical_flow(L, R, kps_left, stereo_predict(cam0, cam1, baseline, kps_left), **kw)
    pb, z0, inv = stereo_depth(cam0, cam1, kps_left, right)
    status = np.where(st > 0, np.where(z0 > 0, 1, 2), 0).astype(np.uint8)
    return right, status, inv, pb


def track_last_frame(last, cur, cam0, baseline, pose, pw, kps_last, remove_moving_points=True, num_features_tracking_bad=20, **kw):
    """Frontend::TrackLastFrame (frontend.cpp:163-256), numeric part: tracked pixels, class per point, number of good points."""
    pred = track_predict(cam0, pose, pw)
    cur_pts, st, _ = optical_flow(last, cur, kps_last, pred, **kw)
    cls, n_good, _, _ = classify(cam0, baseline, pose, pw, pred, cur_pts, st, remove_moving_points, num_features_tracking_bad)
    return cur_pts, cls, n_good


# ---- analytic test images ------------------------------------------------------------------------------------------------------------------
class Texture:
    """A seeded sum of ~60 sinusoids with wavelengths of 8-80 px, sigma ~ 45 grey levels around 128: a function of real coordinates, so a
    warped view is SAMPLED (not interpolated) and the true displacement of every point is known exactly."""

    def __init__(self, seed, n_waves=60, sigma=45.0):
        rng = np.random.default_rng(seed)
        lam = np.exp(rng.uniform(np.log(8.0), np.log(80.0), n_waves))
        th = rng.uniform(0, 2 * np.pi, n_waves)
        self.u, self.v = np.cos(th) / lam, np.sin(th) / lam
        self.phase = rng.uniform(0, 2 * np.pi, n_waves)
        self.amp = rng.uniform(0.5, 1.0, n_waves)
        self.amp *= sigma / np.sqrt(0.5 * np.sum(self.amp ** 2))

    def __call__(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        acc = np.zeros(np.broadcast(x, y).shape)
        for u, v, ph, a in zip(self.u, self.v, self.phase, self.amp):
            acc += a * np.sin(2 * np.pi * (u * x + v * y) + ph)
        return acc

    def image(self, w, h, coords=None):
        """uint8 image of size (w, h); coords(x, y) -> (x', y') maps its pixel grid into texture coordinates (identity when None)."""
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        if coords is not None:
            x, y = coords(x, y)
        return np.clip(np.rint(128.0 + self(x, y)), 0, 255).astype(np.uint8)


def similarity(angle, scale, shift, centre):
    """Forward map of points A -> B (rotation + scale about centre, then shift) and its inverse B -> A."""
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    cx, cy = centre

    def fwd(x, y):
        dx, dy = x - cx, y - cy
        return c * dx - s * dy + cx + shift[0], s * dx + c * dy + cy + shift[1]

    def inv(x, y):
        dx, dy = x - cx - shift[0], y - cy - shift[1]
        k = 1.0 / (scale * scale)
        return k * (c * dx + s * dy) + cx, k * (-s * dx + c * dy) + cy

    return fwd, inv
