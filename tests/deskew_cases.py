"""Trajectories, clouds and scans shared by test_deskew_ref.py (CPU) and test_gpu_deskew.py (GPU).  Everything is seeded and small."""
import functools

import numpy as np

from lvio_fusion_amd import synthetic as syn

CYCLE = 0.1036      # config/kitti.yaml:40


def trajectory(n, dt=0.1, speed=15.0, yaw_rate=0.3, origin=(0.0, 0.0, 0.0), t0=0.0, wobble=0.02, seed=0):
    """n keyframes dt apart: a vehicle at `speed` m/s along its heading, turning at yaw_rate rad/s, with a little pitch / roll.
    Returns (stamps [n], poses [n, 7])."""
    rng = np.random.default_rng(seed)
    stamps = t0 + dt * np.arange(n)
    yaw = 0.4 + yaw_rate * (stamps - t0)
    pitch, roll = wobble * rng.standard_normal(n), wobble * rng.standard_normal(n)
    q = syn.quat_from_ypr(yaw, pitch, roll).reshape(n, 4)
    pos = np.zeros((n, 3))
    pos[:, 0] = origin[0] + speed * np.cumsum(np.cos(yaw)) * dt
    pos[:, 1] = origin[1] + speed * np.cumsum(np.sin(yaw)) * dt
    pos[:, 2] = origin[2] + 0.05 * rng.standard_normal(n)
    return stamps, np.concatenate([q, pos], 1)


def far_trajectory(n, seed=1):
    """translations up to 1e3 m (the interpolation's tolerance scales with |t|; the cloud tests stay within 1e3 m)"""
    return trajectory(n, origin=(940.0, -870.0, 35.0), seed=seed)


def with_negative_dot(stamps, poses, k):
    """knot k's quaternion negated: the same rotation, but q_k-1 . q_k < 0 and q_k . q_k+1 < 0"""
    p = poses.copy(); p[k, :4] = -p[k, :4]
    return stamps, p


def with_identical_rotation(stamps, poses, k):
    """knots k and k + 1 share one quaternion bit for bit: |d| >= 1 - eps, the linear branch of slerp"""
    p = poses.copy(); p[k + 1, :4] = p[k, :4]
    return stamps, p


def query_times(stamps, per_bracket=3, seed=0):
    """before the first stamp, exactly on every stamp, inside every bracket, after the last stamp"""
    rng = np.random.default_rng(seed)
    s = np.asarray(stamps, np.float64)
    span = (s[-1] - s[0]) if len(s) > 1 else 1.0
    out = [s[0] - 0.37 * span - 0.01, s[0] - 1e-9, s[-1] + 1e-9, s[-1] + 0.21 * span + 0.01, s[-1] + 0.5]
    out += list(s)
    for a, b in zip(s[:-1], s[1:]):
        out += list(a + (b - a) * rng.uniform(0.01, 0.99, per_bracket))
    return np.array(out)


def sweep_cloud(n, cycle=CYCLE, seed=0, nan_every=0):
    """n sensor-frame points at 5 .. 30 m with intensity = ring + float32(cycle * rel_time), rel_time uniform in [-0.25, 1.25] (AdjustDistortion's
    range: about a sixth of the points carry a NEGATIVE offset, on every ring); nan_every > 0: every such point has a NaN coordinate"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1)[:, None] + 1e-300
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = (d * rng.uniform(5.0, 30.0, (n, 1))).astype(np.float32)
    ring = rng.integers(0, 64, n)
    rel = rng.uniform(-0.25, 1.25, n).astype(np.float32)
    c[:, 3] = (ring.astype(np.float64) + cycle * rel.astype(np.float64)).astype(np.float32)      # int(intensity) + cycle_time_ * rel_time (association.cpp:143)
    if nan_every:
        rows = np.arange(0, n, nan_every)
        c[rows, rows % 3] = np.nan
    return c


def negative_offset_cloud(cycle=CYCLE):
    """hand-made: the same direction on rings 1, 5, 17, 63 with offsets -0.25, -0.1, -0.001 cycle, and their positive twins"""
    rows = []
    for ring in (1, 5, 17, 63):
        for rel in (-0.25, -0.1, -0.001, 0.001, 0.1, 0.25):
            rows.append([12.0 + ring * 0.1, -7.0 + rel, 0.5, np.float32(ring + cycle * np.float32(rel))])
    return np.array(rows, np.float32)


def stray_offset_cloud(cycle=CYCLE):
    """hand-made: a sweep_cloud of 65 points in which six intensities carry an offset of +-0.4 s (still inside (-0.5, 0.5), so the ring is
    recoverable): their times fall well outside [frame_time - 0.75 cycle, frame_time + 0.75 cycle], the window the host narrows the trajectory
    to, while every other point's time falls inside it"""
    c = sweep_cloud(65, cycle=cycle, seed=21)
    for row, (ring, off) in zip((0, 7, 31, 32, 63, 64), ((0, 0.4), (5, -0.4), (17, 0.4), (40, -0.4), (63, 0.4), (63, -0.4))):
        c[row, 3] = np.float32(ring) + np.float32(off)
    return c


@functools.lru_cache(maxsize=None)
def scan600(seed):
    """a 600-firing revolution (38 400 points, horizon_scan = 600): the smallest scan that keeps the range image's row and column adjacency, so
    that segments, picks and both features come out non-empty"""
    a = syn.raw_scan(seed=seed, n_az=600)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scan_every_third(seed):
    """syn.raw_scan(seed)[::3]: every third point of the full revolution.  No firing keeps two adjacent rings and no two neighbouring columns
    keep one ring, so nothing is marked ground and no segment has two pixels: the picks are EMPTY and every launch behind the segmentation —
    the deskew's included — sees a count of zero on the device"""
    a = np.ascontiguousarray(syn.raw_scan(seed=seed)[::3])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scan_full(seed):
    a = syn.raw_scan(seed=seed)
    a.setflags(write=False)
    return a


def fast_drive(velocity=(650.0, 585.0, 520.0)):
    """3 keyframes 0.1 s apart at a constant heading and a constant world-frame velocity that is large on all three axes: 1015 m/s, 105 m across
    one 0.1036 s sweep.  Chosen on the CPU from oracle.lidar_extract's picks of scan600(31) pushed through deskew_ref.deskew about the middle
    keyframe: the deskewed ground picks then span 324 x 142 x 201 = 9.2e6 = 2^23.1 voxels of 0.4 m and the surf picks 217 x 90 x 139 = 2^21.4 —
    the ground box is past the 2^22 keys that two 11-bit digit passes sort (a factor 2.2) and within lvf_cloud_voxel_filter's 2^26 (a factor 7.3);
    600 m/s gives 2^22.8 and 700 m/s 2^23.4, so the case does not sit at an edge.  Positions stay within 130 m."""
    stamps = 0.1 * np.arange(3)
    q = syn.quat_from_ypr(np.array([0.4]), np.array([0.0]), np.array([0.0])).reshape(4)
    return stamps, np.stack([np.concatenate([q, np.asarray(velocity, np.float64) * t]) for t in stamps])


def tail_digit_passes(max_range, resolution):
    """the digit passes the device-counted tail enqueues, derived as dc_tail_begin derives them: coordinates in [-max_range, max_range], voxels of
    2 * resolution, in float32 like the voxel box below, two cells of slack, 11 bits per pass"""
    inv_leaf = np.float32(1) / (np.float32(2) * np.float32(resolution))
    span = float(np.floor(np.float32(max_range) * inv_leaf)) - float(np.floor(-np.float32(max_range) * inv_leaf)) + 1.0 + 2.0
    bits = 1
    while float(1 << bits) < span ** 3:
        bits += 1
    return (bits + 10) // 11


def voxel_cells(picks, resolution):
    """the voxel box of a pick cloud in float32, as k_dc_bounds and lvf_cloud_voxel_filter compute it: per axis
    floor(hi * inv_leaf) - floor(lo * inv_leaf) + 1 with inv_leaf = 1 / (2 * resolution); the product"""
    inv_leaf = np.float32(1.0) / (np.float32(2) * np.float32(resolution))
    lo, hi = picks[:, :3].min(0), picks[:, :3].max(0)
    assert lo.dtype == np.float32
    return int(np.prod(np.floor(hi * inv_leaf).astype(np.int64) - np.floor(lo * inv_leaf).astype(np.int64) + 1))


def drive(speed=15.0, yaw_rate=0.3, seed=3):
    """the extraction tests' trajectory: 3 keyframes 0.1 s apart"""
    return trajectory(3, dt=0.1, speed=speed, yaw_rate=yaw_rate, seed=seed)
