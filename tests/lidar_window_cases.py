"""Scenes for the LiDAR-plane window tests (tests/test_lidar_window_ref.py on the CPU, tests/test_gpu_lidar_window.py on the device).

    plane_blocks    plane correspondences of every keyframe of a trajectory on three mutually non-parallel planes (ground, a side wall, a
                    slanted wall ahead), taken at the TRUE poses: p in the body frame, pa / pb / pc three points of the plane near the hit
    far_scene       the window that shows what the planes are for: landmarks too far for their depth to be observed, every free pose off
    imu_only        config4_window without any visual block or landmark (a LiDAR-inertial window)
"""
import numpy as np

from lvio_fusion_amd import synthetic as syn
from tests import lidar_window_ref as lw

# (unit normal, offset): n . x = d
PLANES = ((np.array([0.0, 0.0, 1.0]), -1.7), (np.array([0.0, 1.0, 0.0]), 6.0), (np.array([0.8, 0.0, 0.6]), 28.0))


def _basis(n):
    a = np.cross(n, [1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.cross(n, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return a, np.cross(n, a)


def plane_blocks(poses_true, per_kf, rng, noise=0.01, kfs=None):
    """per_kf blocks on each keyframe of `kfs` (default: all), a third on each plane, sorted by keyframe.  Returns the arrays of
    lidar_window_ref.make_lidar: (p, pa, pb, pc, kf)."""
    kfs = range(len(poses_true)) if kfs is None else kfs
    P, PA, PB, PC, KF = [], [], [], [], []
    for k in kfs:
        T = poses_true[k]
        R, t = syn.rotmat(T[:4]), T[4:]
        for j in range(per_kf):
            n, d = PLANES[j % 3]
            a, b = _basis(n)
            foot = t + (d - n @ t) * n                                # the keyframe's foot point on the plane
            hit = foot + rng.uniform(-8.0, 8.0) * a + rng.uniform(-8.0, 8.0) * b
            tri = [hit + rng.uniform(-0.4, 0.4) * a + rng.uniform(-0.4, 0.4) * b for _ in range(3)]
            tri[1] = tri[0] + 0.3 * a + rng.uniform(-0.1, 0.1) * b   # (never collinear)
            tri[2] = tri[0] + 0.3 * b + rng.uniform(-0.1, 0.1) * a
            P.append(R.T @ (hit + rng.normal(0, noise, 3) - t)); PA.append(tri[0]); PB.append(tri[1]); PC.append(tri[2]); KF.append(k)
    return np.array(P), np.array(PA), np.array(PB), np.array(PC), np.array(KF, np.int32)


def far_scene(seed=7, n_kf=5, n_lm=40, per_kf=150, offset=0.3):
    """5 keyframes, the first constant; 40 landmarks at 80-120 m — beyond 50 baselines (27 m), so a stereo depth says next to nothing and the
    translation of the window hangs on it; no IMU; every free pose starts `offset` metres off; `per_kf` plane blocks per keyframe with 1 cm of
    range noise, weighted by its reciprocal.  Returns (cfg, pre, lidar, pose_const)."""
    rng = np.random.default_rng(seed)
    cam0, cam1 = syn.kitti_cameras()
    poses = syn.drive_poses(n_kf, rng)
    birth = np.sort(rng.integers(0, n_kf - 1, n_lm)).astype(np.int32)
    depth = rng.uniform(80.0, 120.0, n_lm)
    assert depth.min() > 50 * syn.baseline()
    u1, v1 = rng.uniform(100, 1141, n_lm), rng.uniform(40, 336, n_lm)
    ps = np.stack([(u1 - syn.CX) / syn.FX * depth, (v1 - syn.CY) / syn.FY * depth, depth], -1)
    pw = syn.se3_apply(poses[birth], syn.se3_apply(cam1["extrinsic"], ps))
    right = np.stack([u1, v1], -1)
    left = syn.project(cam0, poses[birth], pw)[0] + rng.normal(0, 0.5, (n_lm, 2))
    lm, k1, k2 = [], [], []
    for l in range(n_lm):
        for k in range(birth[l] + 1, n_kf):
            lm.append(l); k1.append(birth[l]); k2.append(k)
    lm, k1, k2 = (np.array(x, np.int32) for x in (lm, k1, k2))
    order = np.lexsort((lm, k2))
    lm, k1, k2 = lm[order], k1[order], k2[order]
    ob = syn.project(cam0, poses[k2], pw[lm])[0] + rng.normal(0, 0.5, (len(lm), 2))
    est = poses.copy()
    for k in range(1, n_kf):
        dirn = rng.normal(size=3); est[k, 4:] += offset * dirn / np.linalg.norm(dirn)
    z3 = np.zeros((n_kf, 3))
    cfg = dict(cam0=cam0, cam1=cam1, n_kf=n_kf, n_lm=n_lm, poses_true=poses, poses=est, vel=z3.copy(), ba=z3.copy(), bg=z3.copy(),
               inv_depth=(1.0 / depth) * (1 + rng.normal(0, 0.05, n_lm)), inv_depth_true=1.0 / depth, w_kf=np.full(n_kf, syn.W_VISUAL),
               tc=dict(left_ob=left, right_ob=right, lm_idx=np.arange(n_lm, dtype=np.int32), kf_idx=birth),
               tf=dict(first_ob=right[lm], ob=ob, lm_idx=lm, kf1_idx=k1, kf2_idx=k2),
               po=dict(ob=np.zeros((0, 2)), kf_idx=np.zeros(0, np.int32), pw_idx=np.zeros(0, np.int32), pw=np.zeros((1, 3))), imu=[])
    noise = 0.01
    lidar = lw.make_lidar(*plane_blocks(poses, per_kf, rng, noise), weight=1.0 / noise)      # (whitened: the blocks' weight is 1 / sigma of the range noise)
    pc = np.zeros(n_kf, np.uint8); pc[0] = 1
    return cfg, np.zeros((0, 467)), lidar, pc


def imu_only(cfg):
    """the window without its visual blocks and landmarks (n_lm = 0): what an IMU + LiDAR window is made of"""
    c = dict(cfg)
    e2, ei = np.zeros((0, 2)), np.zeros(0, np.int32)
    c.update(n_lm=0, inv_depth=np.zeros(0), tc=dict(left_ob=e2, right_ob=e2, lm_idx=ei, kf_idx=ei),
             tf=dict(first_ob=e2, ob=e2, lm_idx=ei, kf1_idx=ei, kf2_idx=ei), po=dict(ob=e2, kf_idx=ei, pw_idx=ei, pw=np.zeros((1, 3))))
    return c


def state_of_cfg(cfg):
    return [np.array(cfg[k], dtype=np.float64) for k in ("poses", "vel", "ba", "bg", "inv_depth")]


def preint(oracle, cfg):
    if not cfg["imu"]:
        return np.zeros((0, 467))
    return np.stack([oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
