"""The deskew's restatement (tests/deskew_ref.py) pinned on the CPU: it is the yardstick of test_gpu_deskew.py, so its own
properties are checked here without a GPU — against an independent formulation in mpmath (rotation matrices, exp / log of the relative
rotation: nothing shared with the quaternion weights of slerp), against closed-form motion, and on the two deviations it declares."""
import mpmath as mp
import numpy as np

from lvio_fusion_amd import synthetic as syn
from tests import deskew_cases as dc
from tests import deskew_ref as dr
from tests import indep_mp as im


def quat_close(a, b):
    """max component difference of unit quaternions up to the common sign"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    sgn = np.where((a * b).sum(1) < 0, -1.0, 1.0)[:, None]
    return np.abs(a - sgn * b).max()


def test_pose_at_a_stamp_is_that_keyframe():
    for n in (1, 2, 3, 40):
        stamps, poses = dc.far_trajectory(n)
        got = dr.compute_pose(stamps, poses, stamps)
        assert quat_close(got[:, :4], poses[:, :4]) <= 4e-16
        assert np.abs(got[:, 4:] - poses[:, 4:]).max() <= 1e-12          # (1 - s) t_i + s t_i+1 with s = 0 or 1 exactly
    # one pose: every time returns it
    stamps, poses = dc.far_trajectory(1)
    assert np.array_equal(dr.compute_pose(stamps, poses, [-5.0, 0.0, 7.0]), np.repeat(dr.normalized(poses), 3, 0))


def mp_log_so3(R):
    """rotation vector of R (angle in [0, pi))"""
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = mp.acos(max(mp.mpf(-1), min(mp.mpf(1), c)))
    v = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < mp.mpf(10) ** -30:
        return v / 2
    return v * (th / (2 * mp.sin(th)))


def mp_exp_so3(w):
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < mp.mpf(10) ** -30:
        return mp.eye(3) + K
    return mp.eye(3) + K * (mp.sin(th) / th) + K * K * ((1 - mp.cos(th)) / th ** 2)


def test_agrees_with_independent_exp_log_formulation():
    """R(s) = R_i exp(s log(R_i^T R_i+1)) and the lerp, at 50 digits, against compute_pose to 1e-13 — inside the brackets and extrapolated, with a
    negative-dot-product bracket and an identical-rotation bracket among them"""
    stamps, poses = dc.trajectory(5, seed=2)
    stamps, poses = dc.with_negative_dot(stamps, poses, 2)
    stamps, poses = dc.with_identical_rotation(stamps, poses, 3)
    times = dc.query_times(stamps, per_bracket=2, seed=4)
    got = dr.compute_pose(stamps, poses, times)
    P = dr.normalized(poses)
    idx = dr.bracket(stamps, times)
    worst = 0.0
    for t, g, i in zip(times, got, idx):
        s = (mp.mpf(float(t)) - mp.mpf(float(stamps[i]))) / (mp.mpf(float(stamps[i + 1])) - mp.mpf(float(stamps[i])))
        Ra, Rb = im.R_of(im.vec(P[i, :4])), im.R_of(im.vec(P[i + 1, :4]))
        R = Ra * mp_exp_so3(mp_log_so3(Ra.T * Rb) * s)
        tr = im.vec(P[i, 4:]) * (1 - s) + im.vec(P[i + 1, 4:]) * s
        Rg = dr.rotmat(g[:4])
        worst = max(worst, max(abs(float(R[r, c]) - Rg[r, c]) for r in range(3) for c in range(3)), max(abs(float(tr[k]) - g[4 + k]) for k in range(3)))
    assert worst <= 1e-13, worst


def test_extrapolates_a_constant_twist_exactly_in_rotation():
    """keyframes on a constant angular velocity about a fixed axis: slerp with s outside [0, 1] continues the rotation exactly"""
    axis = np.array([0.2, -0.3, 0.93]); axis /= np.linalg.norm(axis)
    rate = 0.7
    quat = lambda t: np.concatenate([axis * np.sin(0.5 * rate * t), [np.cos(0.5 * rate * t)]])
    stamps = np.array([1.0, 1.1, 1.2])
    poses = np.array([np.concatenate([quat(t), [15.0 * t, 0.0, 0.0]]) for t in stamps])
    times = np.array([0.6, 0.95, 1.05, 1.17, 1.25, 1.9])
    got = dr.compute_pose(stamps, poses, times)
    assert quat_close(got[:, :4], np.array([quat(t) for t in times])) <= 1e-13
    assert np.abs(got[:, 4] - 15.0 * times).max() <= 1e-12          # (and the constant velocity of the end brackets)


def test_static_plane_under_constant_velocity():
    """A wall x_w = 20 seen from a sensor that moves at 15 m/s while the sweep is taken: every point is expressed in the sensor frame of ITS
    time.  Deskewed, the points lie on the wall as seen from the frame's pose to float32 rounding; left as they are they miss it by up to
    speed * cycle / 2 = 0.78 m."""
    rng = np.random.default_rng(9)
    E = syn.lidar_extrinsic()
    vel = np.array([15.0, 0.0, 0.0])
    q0 = syn.quat_from_ypr(0.1, -0.02, 0.03)
    stamps = np.array([0.0, 0.1, 0.2])
    poses = np.array([np.concatenate([q0, vel * t]) for t in stamps])
    frame_time, frame_pose = 0.1, poses[1]
    n = 2000
    ring = rng.integers(0, 64, n)
    rel = rng.uniform(0.0, 1.0, n)
    I = (ring + dc.CYCLE * rel).astype(np.float32)
    _, _, t = dr.point_times(I, frame_time, dc.CYCLE)                  # the acquisition time the intensity really encodes
    pw = np.stack([np.full(n, 20.0), rng.uniform(-8, 8, n), rng.uniform(-1.5, 3, n)], 1)
    T = np.concatenate([np.repeat(q0[None], n, 0), vel[None] * t[:, None]], 1)
    ps = dr.apply_inv(dr.normalized(E)[0], dr.apply_inv(T, pw))
    cloud = np.concatenate([ps, I[:, None]], 1).astype(np.float32)
    wall = lambda p: dr.apply(dr.normalized(frame_pose)[0], dr.apply(dr.normalized(E)[0], p.astype(np.float64)))[:, 0] - 20.0
    p2, out = dr.deskew(cloud, stamps, poses, frame_time, frame_pose, dc.CYCLE, E)
    r_max = np.linalg.norm(cloud[:, :3], axis=1).max()
    assert r_max < 40.0
    tol = 4 * 2.0 ** -24 * r_max          # float32 rounding of the three input and the three output coordinates, 2^-24 relative each
    assert np.abs(wall(out[:, :3])).max() <= tol, (np.abs(wall(out[:, :3])).max(), tol)
    assert np.array_equal(out[:, 3].view(np.uint32), cloud[:, 3].view(np.uint32))
    off = np.abs(wall(cloud[:, :3]))
    assert off.max() > 0.5 and np.median(off) > 0.05


def test_negative_offset_keeps_its_ring():
    """ring 5, offset -0.02 s: the time lies just before the sweep's start; the reference's int() would read ring 4 and offset +0.98 s"""
    I = np.float32(5 - 0.02)
    ring, delta, t = dr.point_times([I], 10.0, dc.CYCLE)
    assert ring[0] == 5.0 and abs(float(delta[0]) + 0.02) < 1e-6
    start = 10.0 - 0.5 * dc.CYCLE
    assert t[0] < start and abs(t[0] - (start - 0.02)) < 1e-6
    assert abs((float(I) - int(I)) - 0.98) < 1e-6          # what UndistortPoint computes: one second later
    # non-negative offsets: the two readings agree bit for bit
    I = dc.sweep_cloud(500, seed=5)[:, 3]
    _, delta, _ = dr.point_times(I, 0.0, dc.CYCLE)
    pos = delta >= 0
    assert pos.sum() > 300 and (~pos).sum() > 30
    assert np.array_equal(delta[pos], (I[pos] - I[pos].astype(np.int32).astype(np.float32)))


def test_cloud_edge_cases_of_the_restatement():
    stamps, poses = dc.drive()
    E = syn.lidar_extrinsic()
    c = dc.sweep_cloud(100, seed=6, nan_every=7)
    p2, out = dr.deskew(c, stamps, poses, 0.1, poses[1], dc.CYCLE, E)
    bad = ~np.isfinite(c).all(1)
    assert bad.sum() == 15 and np.array_equal(out[bad].view(np.uint32), c[bad].view(np.uint32)) and np.isfinite(out[~bad]).all()
    assert np.abs(out[~bad, :3] - c[~bad, :3]).max() > 0.3          # 15 m/s over half a sweep
    _, same = dr.deskew(c, stamps[:1], poses[:1], 0.1, poses[1], dc.CYCLE, E)
    assert np.array_equal(same.view(np.uint32), c.view(np.uint32))
    # at the frame's own time and pose the map is the identity: a point with offset cycle / 2 moves by rounding only
    c2 = dc.sweep_cloud(50, seed=7)
    c2[:, 3] = np.float32(3.0) + np.float32(0.5 * dc.CYCLE)
    _, d, _ = dr.point_times(c2[:, 3], 0.0, dc.CYCLE)
    p2, _ = dr.deskew(c2, stamps, poses, 0.1, dr.compute_pose(stamps, poses, [0.1 - 0.5 * dc.CYCLE + float(d[0])])[0], dc.CYCLE, E)
    assert np.abs(p2 - c2[:, :3]).max() <= 1e-12


def test_fast_drive_sits_inside_the_hand_over_window(oracle):
    """deskew_cases.fast_drive is chosen on the CPU: the oracle's picks of the 600-firing scan, deskewed by the restatement, must need more voxel
    keys than the digit passes planned for (max_range 30, resolution 0.2) sort — so the device-counted tail raises its verdict — and fewer than
    lvf_cloud_voxel_filter's 2^26 — so the host-counted path finishes — with a factor two to spare on either side (test_gpu_deskew.py's
    test_tail_verdict_hands_the_scan_over asserts the window itself on the device's own picks)"""
    ref = oracle.lidar_extract(dc.scan600(31), syn.lidar_extrinsic(), horizon_scan=600)
    stamps, poses = dc.fast_drive()
    passes = dc.tail_digit_passes(30.0, 0.2)
    assert passes == 2
    cells = [dc.voxel_cells(dr.deskew(ref[key], stamps, poses, stamps[1], poses[1], dc.CYCLE, syn.lidar_extrinsic())[1], 0.2) for key in ("ground_raw", "surf_raw")]
    print("deskewed boxes: 2^%.2f (ground), 2^%.2f (surf) voxels; displacement across one sweep %.1f m" %
          (np.log2(cells[0]), np.log2(cells[1]), np.linalg.norm((poses[2, 4:] - poses[0, 4:]) / 0.2) * dc.CYCLE))
    assert 2 << (11 * passes) < max(cells) < (1 << 26) // 2
    assert np.abs(poses[:, 4:]).max() <= 1e3
