"""Declared semantics of the LiDAR sweep deskew, in numpy: float64 unless said otherwise.

The reference declares the step — the `deskew` key of its configs (estimator.cpp:152), FeatureAssociation::deskew_ (association.h:22,65), the
`//TODO:deskew` of AdjustDistortion (association.cpp:142-145) — and wrote its implementation, but never calls it:

    Map::ComputePose (map.cpp:92-102)
        frame1 = keyframes.lower_bound(time), frame2 = keyframes.upper_bound(time)
        s = (time - frame1->time) / (frame2->time - frame1->time)
        q = frame1->pose.unit_quaternion().slerp(s, frame2->pose.unit_quaternion())
        t = (1 - s) * frame1->t() + s * frame2->t();  return SE3d(q, t)
    FeatureAssociation::UndistortPoint (association.cpp:65-76)
        time_delta = point.intensity - int(point.intensity);  time = frame->time - cycle_time_ * 0.5 + time_delta
        p1 = Lidar::Sensor2World(p, ComputePose(time))   = Twc * extrinsic * p                    (sensor.h:21-24)
        p2 = Lidar::World2Sensor(p1, frame->pose)        = extrinsic.inverse() * Twc.inverse() * p1   (sensor.h:16-19)

This file restates those lines with TWO deviations, because the text cannot run as it stands:

  1. lower_bound(time) and upper_bound(time) name the SAME keyframe whenever `time` is not itself a stamp (the first key >= time and the first
     key > time), so t_t = 0 and s = 0/0.  Declared instead: the bracket is (the last stamp <= t, the stamp after it), clamped to the first and
     the last bracket; s is NOT clamped, so a time before the first or after the last stamp extrapolates the end bracket's constant velocity
     (the newest keyframe's sweep needs that for its second half).
  2. AdjustDistortion writes intensity = int(ring) + cycle_time * rel_time with rel_time in about [-0.25, 1.25]; `I - int(I)` truncates a
     negative offset on ring >= 1 to the ring below and returns a time one second off.  Declared instead (float32, like the reference's
     arithmetic on point.intensity): ring = floorf(I + 0.5f), delta = I - ring — equal to I - int(I) for every non-negative offset and
     unambiguous as long as |cycle_time * rel_time| < 0.5.

Quaternions are [qx, qy, qz, qw]; a pose is [qx, qy, qz, qw, tx, ty, tz]; every pose's quaternion is normalised on entry, as Sophus'
SE3d(q, t) constructor does."""
import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps


def normalized(poses):
    p = np.array(poses, np.float64, copy=True).reshape(-1, 7)
    p[:, :4] /= np.sqrt((p[:, :4] ** 2).sum(1))[:, None]
    return p


def rotmat(q):
    """[..., 4] unit quaternions -> [..., 3, 3]"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def apply(T, p):
    """T * p for poses [..., 7] and points [..., 3]"""
    return np.einsum("...ij,...j->...i", rotmat(T[..., :4]), p) + T[..., 4:]


def apply_inv(T, p):
    """T.inverse() * p"""
    return np.einsum("...ji,...j->...i", rotmat(T[..., :4]), p - T[..., 4:])


def bracket(stamps, times):
    """i = clamp(#{stamps <= t} - 1, 0, N - 2) for every time (deviation 1)"""
    n = len(stamps)
    return np.clip(np.searchsorted(stamps, times, side="right") - 1, 0, n - 2)


def compute_pose(stamps, poses, times):
    """Map::ComputePose for an array of times -> [m, 7]"""
    stamps = np.asarray(stamps, np.float64).reshape(-1)
    P = normalized(poses)
    times = np.atleast_1d(np.asarray(times, np.float64))
    if len(stamps) == 1:
        return np.repeat(P[:1], len(times), 0)
    i = bracket(stamps, times)
    a, b = P[i], P[i + 1]
    s = (times - stamps[i]) / (stamps[i + 1] - stamps[i])
    # Eigen::QuaternionBase::slerp
    d = (a[:, :4] * b[:, :4]).sum(1)
    ad = np.abs(d)
    lin = ad >= 1.0 - DBL_EPSILON
    th = np.arccos(np.where(lin, 0.5, ad))
    sn = np.sin(th)
    w0 = np.where(lin, 1.0 - s, np.sin((1.0 - s) * th) / sn)
    w1 = np.where(lin, s, np.sin(s * th) / sn)
    w1 = np.where(d < 0, -w1, w1)
    q = w0[:, None] * a[:, :4] + w1[:, None] * b[:, :4]
    q /= np.sqrt((q ** 2).sum(1))[:, None]                   # SE3d(q, t) normalises
    t = (1.0 - s)[:, None] * a[:, 4:] + s[:, None] * b[:, 4:]
    return np.concatenate([q, t], 1)


def point_times(intensity, frame_time, cycle_time):
    """(ring, delta, t): ring and delta in float32 arithmetic, t in double (deviation 2)"""
    I = np.asarray(intensity, np.float32)
    ring = np.floor(I + np.float32(0.5)).astype(np.float32)
    delta = (I - ring).astype(np.float32)
    t = (np.float64(frame_time) - 0.5 * np.float64(cycle_time)) + delta.astype(np.float64)
    return ring, delta, t


def deskew(cloud, stamps, poses, frame_time, frame_pose, cycle_time, extrinsic):
    """FeatureAssociation::UndistortPointCloud on a sensor-frame cloud [n, 4] float32 whose intensity carries ring + time offset.
    Returns (p2 [n, 3] float64 before rounding, out [n, 4] float32).  A point with a non-finite field is copied unchanged (its p2 is NaN);
    with a one-pose trajectory the cloud is copied."""
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    out = c.copy()
    p2 = np.full((len(c), 3), np.nan)
    if len(np.atleast_1d(stamps)) == 1 or len(c) == 0:
        p2[:] = c[:, :3]
        return p2, out
    E, Tf = normalized(extrinsic)[0], normalized(frame_pose)[0]
    ok = np.isfinite(c).all(1)
    _, _, t = point_times(c[ok, 3], frame_time, cycle_time)
    T = compute_pose(stamps, poses, t)
    p1 = apply(T, apply(E, c[ok, :3].astype(np.float64)))            # Sensor2World
    p2[ok] = apply_inv(E, apply_inv(Tf, p1))                         # World2Sensor
    out[ok, :3] = p2[ok].astype(np.float32)
    return p2, out
