"""Committed scenes and seeds of the visual-relocalisation tests (tests/test_reloc_ref.py asserts on the CPU, with the restatement alone, every
condition tests/test_gpu_reloc.py relies on).  Everything is generated from the seeds below; nothing is read from disk."""
import numpy as np

from tests import reloc_ref as rr

CAM0 = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, extrinsic=np.array([-0.5, 0.5, -0.5, 0.5, 0.05, -0.02, 0.1]))      # sensor z = body x
WIDTH, HEIGHT = 752, 480
P3P_SEED, P3P_TRIPLES = 20240519, 2000
E_REF = 9e-16            # the restatement's float64 deviation from its 50-digit run: asserted in tests/test_reloc_ref.py, used by tests/test_gpu_reloc.py


def quat_zyx(yaw, pitch, roll):
    from tests import navsat_ref as nr
    return nr.quat_zyx(yaw, pitch, roll)


def true_pose(rng):
    return np.concatenate([quat_zyx(rng.uniform(-0.6, 0.6), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)), rng.uniform(-3, 3, 3) + [20.0, -8.0, 1.0]])


def landmarks_in_view(rng, pose, n, z_lo=4.0, z_hi=20.0, sign=1.0):
    """n world points whose sensor-frame coordinates fill the image at depths z_lo .. z_hi (sign -1: behind the camera)"""
    c = rr.cam_derived(CAM0)
    z = rng.uniform(z_lo, z_hi, n)
    u, v = rng.uniform(30, WIDTH - 30, n), rng.uniform(30, HEIGHT - 30, n)
    pc = np.stack([(u - c["cx"]) / c["fx"] * z, (v - c["cy"]) / c["fy"] * z, z], axis=1) * sign
    pb = pc @ c["Re"].T + c["te"]
    return pb @ rr.rot_of(pose[:4]).T + pose[4:7]


def scene(seed, n, wrong=0.0, noise=0.3, behind=0.0):
    """n 3D-2D correspondences: a fraction `wrong` carries a uniformly drawn pixel instead of the projection, a fraction `behind` (of the wrong
    ones' budget, taken first) lies behind the camera.  Returns dict(cam0, pose (planted), pw [n][3], pt [n][2] float32, good [n] bool,
    init (a drifted pose))."""
    rng = np.random.default_rng(seed)
    pose = true_pose(rng)
    pw = landmarks_in_view(rng, pose, n)
    px, _ = rr.project(CAM0, pose, pw)
    pt = px + rng.normal(0.0, noise, (n, 2)) if noise > 0 else px.copy()
    good = np.ones(n, bool)
    idx = rng.permutation(n)
    nb, nw = int(round(behind * n)), int(round(wrong * n))
    if nb:
        pw[idx[:nb]] = landmarks_in_view(rng, pose, nb, sign=-1.0)
    bad = idx[:max(nb, nw)]
    pt[bad] = np.stack([rng.uniform(0, WIDTH, len(bad)), rng.uniform(0, HEIGHT, len(bad))], axis=1)
    good[bad] = False
    init = pose.copy()
    init[4:7] += rng.normal(0.0, 0.5, 3)
    return dict(cam0=CAM0, pose=pose, pw=pw, pt=pt.astype(np.float32), good=good, init=init)


# name -> (seed, n, wrong, noise, behind, num_hypotheses)
SCENES = {
    "n71_w40": (11, 71, 0.4, 0.3, 0.0, 64),
    "n300_w50": (22, 300, 0.5, 0.3, 0.0, 256),
    "n21_clean": (13, 21, 0.0, 0.3, 0.0, 64),
    "n20_early": (14, 20, 0.0, 0.3, 0.0, 64),
    "all_wrong": (15, 60, 1.0, 0.3, 0.0, 64),
    "third_behind": (16, 90, 1.0 / 3.0, 0.3, 1.0 / 3.0, 64),
    "noise_free": (17, 71, 0.3, 0.0, 0.0, 64),
}
PNP_SEED = 7


def named_scene(name):
    seed, n, wrong, noise, behind, H = SCENES[name]
    s = scene(seed, n, wrong, noise, behind)
    s["opt"] = dict(num_hypotheses=H, seed=PNP_SEED)
    return s


def descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(rng, desc, k):
    out = desc.copy()
    for row in out:
        for b in rng.choice(256, k, replace=False):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def image_pair(seed, n_old=150, n_cur=180, n_common=100, noise=0.3, same_pose=False, exact=False, old_pose=None):
    """An old frame of n_old landmarks with descriptors and a current frame of n_cur features, n_common of them re-observations (the landmark's
    descriptor with up to 8 flipped bits), the rest independent draws.  Returns dict(cam0, old_pose, pose (planted current), old_pw, old_desc,
    cur_pt float32, cur_desc, relative_o_c (the caller's drifted initial value), truth [n_cur] (old index or -1)).  `exact`: the re-observed
    pixels are multiples of 1/8 (exact in float32) and their landmarks are those pixels projected back to a drawn depth, so the planted pose
    has residuals at the rounding level of fp64 and the estimate can be held to it."""
    rng = np.random.default_rng(seed)
    drawn = true_pose(rng)
    old_pose = drawn if old_pose is None else np.asarray(old_pose, float)
    pose = old_pose.copy()
    if not same_pose:
        pose[:4] = quat_zyx(rng.uniform(-0.05, 0.05), 0.0, 0.0)
        pose = rr.sophus_mul(old_pose, np.concatenate([pose[:4], rng.normal(0.0, 0.3, 3)]))
    old_pw = landmarks_in_view(rng, pose, n_old)
    old_desc = descriptors(rng, n_old)
    truth = np.full(n_cur, -1, np.int64)
    slots = rng.permutation(n_cur)[:n_common]
    truth[slots] = rng.permutation(n_old)[:n_common]
    cur_pt = np.stack([rng.uniform(0, WIDTH, n_cur), rng.uniform(0, HEIGHT, n_cur)], axis=1)
    cur_desc = descriptors(rng, n_cur)
    px, _ = rr.project(CAM0, pose, old_pw[truth[slots]])
    cur_pt[slots] = px + rng.normal(0.0, noise, (n_common, 2))
    if exact:
        c = rr.cam_derived(CAM0)
        uv, z = np.rint(px * 8.0) / 8.0, rng.uniform(4.0, 20.0, n_common)
        pc = np.stack([(uv[:, 0] - c["cx"]) / c["fx"] * z, (uv[:, 1] - c["cy"]) / c["fy"] * z, z], axis=1)
        old_pw[truth[slots]] = (pc @ c["Re"].T + c["te"]) @ rr.rot_of(pose[:4]).T + pose[4:7]
        cur_pt[slots] = uv
    for s in slots:
        cur_desc[s] = flip_bits(rng, old_desc[truth[s]][None], int(rng.integers(0, 9)))[0]
    drift = np.array([0.0, 0.0, 0.0, 1.0, 0.4, -0.3, 0.0])
    rel0 = rr.sophus_mul(rr.sophus_mul(rr.sophus_inverse(old_pose), pose), drift)
    return dict(cam0=CAM0, old_pose=old_pose, pose=pose, old_pw=old_pw, old_desc=old_desc, cur_pt=cur_pt.astype(np.float32), cur_desc=cur_desc, relative_o_c=rel0,
                truth=truth, opt=dict(num_hypotheses=128, seed=PNP_SEED))


def match_sets(seed, nq, nt, n_true=None, duplicate=False, identical=False):
    """query / train descriptor sets: n_true true pairs (a few flipped bits), the rest independent; `duplicate`: train rows 3 and 9 hold the same
    descriptor, which query 0 re-observes; `identical`: query 1 equals train row 5 bit for bit"""
    rng = np.random.default_rng(seed)
    q, t = descriptors(rng, nq), descriptors(rng, nt)
    k = min(nq, nt) // 2 if n_true is None else n_true
    qi, ti = rng.permutation(nq)[:k], rng.permutation(nt)[:k]
    for a, b in zip(qi, ti):
        q[a] = flip_bits(rng, t[b][None], int(rng.integers(0, 12)))[0]
    if duplicate:
        t[9] = t[3]
        q[0] = flip_bits(rng, t[3][None], 2)[0]
    if identical:
        q[1] = t[5]
    return q, t


def p3p_triples():
    """P3P_TRIPLES planted problems at the scales of the scenes: (pose, P [3][3] world, pt [3][2] exact pixels)"""
    rng = np.random.default_rng(P3P_SEED)
    out = []
    while len(out) < P3P_TRIPLES:
        pose = true_pose(rng)
        P = landmarks_in_view(rng, pose, 3)
        if np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])) / (np.linalg.norm(P[1] - P[0]) * np.linalg.norm(P[2] - P[0])) < 1e-2:
            continue
        px, _ = rr.project(CAM0, pose, P)
        out.append((pose, P, px))
    return out
