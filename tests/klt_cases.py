"""Generated cases for the feature-tracker tests (tests/test_klt_ref.py on the CPU, tests/test_gpu_klt.py on the device).  Every image is
analytic (klt_ref.Texture): the second view is the same function sampled at warped coordinates, so the true displacement is exact."""
import numpy as np

from tests import klt_ref as kr

W, H = 640, 376


def tracking_case(seed, n=600, w=W, h=H, border=4.0):
    """Similarity warp with |rotation| <= 0.02 rad, scale within 2 %, shift <= 6 px; predictions = truth + N(0, 3 px)."""
    rng = np.random.default_rng(seed)
    angle, scale = rng.uniform(-0.02, 0.02), rng.uniform(0.98, 1.02)
    shift = rng.uniform(-6, 6, 2) / np.sqrt(2)
    fwd, inv = kr.similarity(angle, scale, shift, (w / 2, h / 2))
    tex = kr.Texture(seed)
    A, B = tex.image(w, h), tex.image(w, h, inv)
    prev = np.stack([rng.uniform(border, w - border, n), rng.uniform(border, h - border, n)], 1).astype(np.float32)
    truth = np.stack(fwd(prev[:, 0].astype(np.float64), prev[:, 1].astype(np.float64)), 1)
    init = (truth + rng.normal(0, 3, (n, 2))).astype(np.float32)
    return dict(A=A, B=B, prev=prev, truth=truth, init=init)


def rig(fx=460.0, baseline=0.54, w=W, h=H):
    """A rectified stereo pair mounted like the reference's (camera z = body x, camera x = -body y, camera y = -body z)."""
    R = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    from lvio_fusion_amd.synthetic import quat_from_rotmat
    q = quat_from_rotmat(R)
    t0 = np.array([1.1, -0.3, 0.75])
    cam0 = dict(fx=fx, fy=fx, cx=w / 2 - 0.5, cy=h / 2 - 0.5, extrinsic=np.concatenate([q, t0]))
    cam1 = dict(cam0, extrinsic=np.concatenate([q, t0 + R @ np.array([baseline, 0.0, 0.0])]))
    return cam0, cam1, baseline


def disparity(y, h=H, lo=6.0, hi=36.0):
    return lo + (hi - lo) * np.asarray(y, np.float64) / (h - 1)


def stereo_case(seed, n=600, w=W, h=H, lo=6.0, hi=36.0, border=4.0):
    """Disparity lo..hi px, linear in the row (a ground-like plane): right(x, y) = left(x + d(y), y); the prediction is the reference's own,
    fx / 50 px (depth 50 * baseline).  lo < 0 plants points behind the cameras (negative disparity)."""
    rng = np.random.default_rng(seed)
    cam0, cam1, b = rig(w=w, h=h)
    tex = kr.Texture(seed)
    left = tex.image(w, h)
    right = tex.image(w, h, lambda x, y: (x + disparity(y, h, lo, hi), y))
    kps = np.stack([rng.uniform(border + max(hi, 0), w - border, n), rng.uniform(border, h - border, n)], 1).astype(np.float32)
    truth = np.stack([kps[:, 0] - disparity(kps[:, 1].astype(np.float64), h, lo, hi), kps[:, 1].astype(np.float64)], 1)
    return dict(left=left, right=right, kps=kps, truth=truth, cam0=cam0, cam1=cam1, baseline=b)


def track_case(seed, n=600, w=W, h=H, moving_fraction=0.1):
    """tracking_case plus the 3-D side of Frontend::TrackLastFrame: a current pose and world points whose projections are the predictions;
    a third of the points deeper than 50 baselines (far), a tenth predicted 32-45 px off (moving, where the flow still finds them)."""
    c = tracking_case(seed, n, w, h)
    rng = np.random.default_rng(seed + 1000)
    cam0, _, b = rig(w=w, h=h)
    from lvio_fusion_amd.synthetic import quat_from_ypr
    pose = np.concatenate([quat_from_ypr(0.3, -0.05, 0.02), [4.0, -2.0, 0.5]])
    moving = rng.uniform(size=n) < moving_fraction
    ang = rng.uniform(0, 2 * np.pi, n)
    pred = c["init"].astype(np.float64) + np.where(moving, rng.uniform(32, 45, n), 0.0)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    depth = np.where(rng.uniform(size=n) < 1 / 3, rng.uniform(52 * b, 120 * b, n), rng.uniform(2.0, 48 * b, n))
    ps = np.stack([(pred[:, 0] - cam0["cx"]) * depth / cam0["fx"], (pred[:, 1] - cam0["cy"]) * depth / cam0["fy"], depth], 1)
    pw = kr.se3_apply(pose, kr.se3_apply(cam0["extrinsic"], ps))
    c.update(cam0=cam0, baseline=b, pose=pose, pw=pw, moving=moving)
    return c
