"""CPU restatement of the visual relocalisation — TEST INFRASTRUCTURE ONLY, numpy fp64.  The reference declares the step
(Relocator::RelocateByImage, relocator.cpp:164-173) and never builds it, so the semantics are DECLARED here and the device code
(lvio_fusion_amd/csrc/reloc_kernels.hip) follows this file:

  match             cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) + the gate of local_map.cpp:342-346 + an optional cross-check
  sample_triple     the counter-based sampler (mix32)
  p3p               Grunert's formulation (Haralick et al., "Review and analysis of solutions of the three point perspective pose estimation
                    problem", IJCV 1994): the quartic in v = s3 / s1 formed by polynomial arithmetic from the two law-of-cosine differences,
                    solved by Ferrari's factorisation (resolvent cubic in closed form), each root polished by two Newton steps; the pose from the
                    three depths by aligning the two orthonormal frames the triangles span
  reproj_err2       the squared norm of PoseOnlyReprojectionError's residual at weight 1 (pinned to pyoracle.pose_only in tests/test_reloc_ref.py)
  refine_lm         LocalMap::LocalBA's problem (local_map.cpp:158-181) under the declared Ceres loop (oracle/lm.h lm_solve), written over
                    scalars so that the same text runs in float64 and in 50-digit mpmath
  pnp_ransac, relocate_by_image   the two entry points

Poses are (qx, qy, qz, qw, tx, ty, tz), body -> world; cameras are dicts (fx, fy, cx, cy, extrinsic) with extrinsic = sensor -> body."""
import math

import numpy as np

from tests import orb_ref

MATCH_DEFAULT = dict(max_distance=50, ratio=np.float32(0.8), cross_check=1)
PNP_DEFAULT = dict(num_hypotheses=512, seed=0, max_reproj_px=3.0, min_matches=21, refine_rounds=2, refine_iterations=10, huber_a=1.0)
LM_DEFAULT = dict(function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, min_relative_decrease=1e-3, initial_trust_region_radius=1e4)
MAX_DRAWS = 64            # draws per hypothesis before it is given up (no triple: zero poses)
M32 = 0xFFFFFFFF


# ---- matching -------------------------------------------------------------------------------------------------------------------------------
def hamming_matrix(query, train):
    q, t = np.asarray(query, np.uint8).reshape(-1, 32), np.asarray(train, np.uint8).reshape(-1, 32)
    return orb_ref.hamming(q[:, None, :], t[None, :, :])


def match(query, train, opt=None):
    """returns match, best, second [nq] int32"""
    o = dict(MATCH_DEFAULT); o.update(opt or {})
    q, t = np.asarray(query, np.uint8).reshape(-1, 32), np.asarray(train, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    m, b, s = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    if nq == 0 or nt == 0:
        return m, b, s
    D = hamming_matrix(q, t)
    back = np.argmin(D, axis=0)                      # per train row: its best query, ties to the lower index (argmin takes the first)
    for i in range(nq):
        k = np.argsort(D[i], kind="stable")
        b[i] = D[i, k[0]]
        if nt < 2:
            continue
        s[i] = D[i, k[1]]
        if b[i] < o["max_distance"] and np.float32(b[i]) < np.float32(o["ratio"]) * np.float32(s[i]) and (not o["cross_check"] or back[k[0]] == i):
            m[i] = k[0]
    return m, b, s


# ---- sampling -------------------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, h, c, n):
    return mix32((seed & M32) ^ mix32((h * 0x9E3779B1 + c) & M32)) % n


def sample_triple(seed, h, n):
    """three distinct indices in draw order, or None when MAX_DRAWS draws do not hold three"""
    got = []
    for c in range(MAX_DRAWS):
        d = draw(seed, h, c, n)
        if d not in got:
            got.append(d)
            if len(got) == 3:
                return got
    return None


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
def rot_of(q):
    q = np.asarray(q, float)
    x, y, z, w = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_of(R):
    """Shepperd's method, (x, y, z, w)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4])
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        return np.array([s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s])
    if R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        return np.array([(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s])
    s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
    return np.array([(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s])


def cam_derived(cam):
    Re = rot_of(cam["extrinsic"][:4])
    te = np.asarray(cam["extrinsic"][4:7], float)
    return dict(fx=float(cam["fx"]), fy=float(cam["fy"]), cx=float(cam["cx"]), cy=float(cam["cy"]), Re=Re, te=te, E=Re.T, c0=-(Re.T @ te))


def project(cam, pose, pw):
    """pixels [n][2] and sensor-frame depth [n] of world points at body pose `pose`"""
    c = cam_derived(cam)
    R, t = rot_of(pose[:4]), np.asarray(pose[4:7], float)
    pc = ((np.asarray(pw, float).reshape(-1, 3) - t) @ R) @ c["E"].T + c["c0"]
    with np.errstate(all="ignore"):
        px = np.stack([c["fx"] * pc[:, 0] / pc[:, 2] + c["cx"], c["fy"] * pc[:, 1] / pc[:, 2] + c["cy"]], axis=1)
    return px, pc[:, 2]


def reproj_err2(cam, pose, pw, pt):
    """squared PoseOnly residual norm at weight 1; +inf where the sensor-frame depth is <= 0"""
    px, z = project(cam, pose, pw)
    with np.errstate(all="ignore"):
        e = ((px - np.asarray(pt, float).reshape(-1, 2)) ** 2).sum(1)
    return np.where(z > 0, e, np.inf)


def sophus_mul(A, B):
    """A * B: A's quaternion normalised, the Hamilton product re-normalised (as lvf_forward_update forms it)"""
    A, B = np.asarray(A, float), np.asarray(B, float)
    ux, uy, uz, uw = A[:4] / np.sqrt(A[:4] @ A[:4])
    bx, by, bz, bw = B[:4]
    q = np.array([uw * bx + ux * bw + uy * bz - uz * by, uw * by + uy * bw + uz * bx - ux * bz, uw * bz + uz * bw + ux * by - uy * bx,
                  uw * bw - ux * bx - uy * by - uz * bz])
    from tests import navsat_ref as nr
    return np.concatenate([q / np.sqrt(q @ q), A[4:7] + nr.quat_transform_vector(np.array([ux, uy, uz, uw]), B[4:7])])


def sophus_inverse(A):
    from tests import navsat_ref as nr
    return nr.sophus_inverse(A)


# ---- P3P ------------------------------------------------------------------------------------------------------------------------------------
def _cubic_largest_root(A, B, C):
    """largest real root of z^3 + A z^2 + B z + C, closed form + two Newton steps"""
    P, Q = B - A * A / 3.0, 2.0 * A * A * A / 27.0 - A * B / 3.0 + C
    disc = Q * Q / 4.0 + P * P * P / 27.0
    if disc > 0.0:
        sd = math.sqrt(disc)
        t = np.cbrt(-Q / 2.0 + sd) + np.cbrt(-Q / 2.0 - sd)
    elif P < 0.0:
        arg = min(1.0, max(-1.0, 3.0 * Q / (2.0 * P) * math.sqrt(-3.0 / P)))
        t = 2.0 * math.sqrt(-P / 3.0) * math.cos(math.acos(arg) / 3.0)
    else:
        t = 0.0
    z = float(t) - A / 3.0
    for _ in range(2):
        f, fp = ((z + A) * z + B) * z + C, (3.0 * z + 2.0 * A) * z + B
        if fp != 0.0:
            z -= f / fp
    return z


def quartic_real_roots(a, b, c, d):
    """real roots of x^4 + a x^3 + b x^2 + c x + d in the solver's order (first quadratic factor +, -, second +, -), each polished by two
    Newton steps; returns (roots, marginal) — marginal: a quadratic factor's discriminant lies within 1e-12 of zero"""
    p, q, r = b - 3.0 * a * a / 8.0, c - a * b / 2.0 + a * a * a / 8.0, d - a * c / 4.0 + a * a * b / 16.0 - 3.0 * a * a * a * a / 256.0
    z = _cubic_largest_root(2.0 * p, p * p - 4.0 * r, -q * q)
    roots, marginal = [], False
    if not (z > 0.0) or not math.isfinite(z):
        return roots, True
    s = math.sqrt(z)
    for sg, u in ((1.0, (p + z - q / s) / 2.0), (-1.0, (p + z + q / s) / 2.0)):      # y^2 + sg s y + u
        disc = z - 4.0 * u
        marginal |= abs(disc) < 1e-12
        if disc >= 0.0:
            sd = math.sqrt(disc)
            for y in ((-sg * s + sd) / 2.0, (-sg * s - sd) / 2.0):
                x = y - a / 4.0
                for _ in range(2):
                    f, fp = (((x + a) * x + b) * x + c) * x + d, ((4.0 * x + 3.0 * a) * x + 2.0 * b) * x + c
                    if fp != 0.0:
                        x -= f / fp
                roots.append(x)
    return roots, marginal


def _frame(p1, p2, p3):
    e1 = (p2 - p1) / np.linalg.norm(p2 - p1)
    e3 = np.cross(e1, p3 - p1)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)          # columns


def p3p(f, P):
    """f [3][3]: unit bearings in the camera frame; P [3][3]: the points in the world frame.  Returns (poses, info): poses = [(R_cw, t_cw)] with
    X_cam = R_cw X_world + t_cw and positive depth at the three points, in the solver's order; info = dict(roots, marginal)"""
    f, P = np.asarray(f, float), np.asarray(P, float)
    a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
    ca, cb, cg = float(f[1] @ f[2]), float(f[0] @ f[2]), float(f[0] @ f[1])
    info = dict(roots=[], marginal=False)
    if not (b2 > 0.0):
        info["marginal"] = True
        return [], info
    k, m = (a2 - c2) / b2, c2 / b2
    # u = N(v) / D(v) from the difference of the two law-of-cosine ratios; substituted into b^2 (1 + u^2 - 2 u cos g) = c^2 (1 + v^2 - 2 v cos b)
    n0, n1, n2 = 1.0 + k, -2.0 * k * cb, k - 1.0
    d0, d1 = 2.0 * cg, -2.0 * ca
    q0, q1, q2 = 1.0 - m, 2.0 * m * cb, -m
    A = [n0 * n0 + d0 * d0 * q0 - 2.0 * cg * (n0 * d0),
         2.0 * n0 * n1 + d0 * d0 * q1 + 2.0 * d0 * d1 * q0 - 2.0 * cg * (n0 * d1 + n1 * d0),
         n1 * n1 + 2.0 * n0 * n2 + d0 * d0 * q2 + 2.0 * d0 * d1 * q1 + d1 * d1 * q0 - 2.0 * cg * (n1 * d1 + n2 * d0),
         2.0 * n1 * n2 + 2.0 * d0 * d1 * q2 + d1 * d1 * q1 - 2.0 * cg * (n2 * d1),
         n2 * n2 + d1 * d1 * q2]
    if A[4] == 0.0 or not all(math.isfinite(x) for x in A):
        info["marginal"] = True
        return [], info
    roots, info["marginal"] = quartic_real_roots(A[3] / A[4], A[2] / A[4], A[1] / A[4], A[0] / A[4])
    info["roots"] = roots
    poses = []
    Fw = _frame(P[0], P[1], P[2])
    for v in roots:
        D = d1 * v + d0
        den = 1.0 + v * v - 2.0 * v * cb
        if D == 0.0 or not (den > 0.0):
            continue
        u = ((n2 * v + n1) * v + n0) / D
        if not (v > 0.0 and u > 0.0 and math.isfinite(u)):
            continue
        s1 = math.sqrt(b2 / den)
        X = np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
        Fc = _frame(X[0], X[1], X[2])
        R = Fc @ Fw.T
        t = X[0] - R @ P[0]
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            poses.append((R, t))
    return poses, info


def bearing(cam, pt):
    c = cam_derived(cam)
    pt = np.asarray(pt, float).reshape(-1, 2)
    v = np.stack([(pt[:, 0] - c["cx"]) / c["fx"], (pt[:, 1] - c["cy"]) / c["fy"], np.ones(len(pt))], axis=1)
    return v / np.sqrt((v * v).sum(1))[:, None]


def body_pose(cam, R_cw, t_cw):
    """the body pose Twb (7) of a camera pose X_cam = R_cw X_world + t_cw, through cam.extrinsic"""
    c = cam_derived(cam)
    R_wc = R_cw.T
    R_wb = R_wc @ c["Re"].T
    t_wb = -(R_wc @ t_cw) - R_wb @ c["te"]
    return np.concatenate([quat_of(R_wb), t_wb])


def hypothesis_poses(cam, pw3, pt3):
    poses, info = p3p(bearing(cam, pt3), pw3)
    return [body_pose(cam, R, t) for R, t in poses], info


# ---- hypotheses and scoring -----------------------------------------------------------------------------------------------------------------
def score_hypotheses(cam, pw, pt, opt=None, init_pose=None):
    """pw [n][3], pt [n][2] (float32 values).  Returns dict: triples [H][3] (-1: none), n_poses [H], count [H], pose [H][7], flagged [H] (bool),
    min_margin (the smallest | |error| - gate | seen at any scored pose, px), winner (h, -1 = the initial pose), winner_pose, winner_count"""
    o = dict(PNP_DEFAULT); o.update(opt or {})
    pw, pt = np.asarray(pw, float).reshape(-1, 3), np.asarray(pt, np.float32).reshape(-1, 2).astype(np.float64)
    n, H, gate = len(pw), int(o["num_hypotheses"]), float(o["max_reproj_px"])
    out = dict(triples=np.full((H, 3), -1, np.int32), n_poses=np.zeros(H, np.int32), count=np.zeros(H, np.int32), pose=np.zeros((H, 7)),
               flagged=np.zeros(H, bool), min_margin=np.inf)
    out["pose"][:, 3] = 1.0

    def count_at(pose):
        e2 = reproj_err2(cam, pose, pw, pt)
        with np.errstate(all="ignore"):
            margin = np.abs(np.sqrt(e2[np.isfinite(e2)]) - gate)
        mg = float(margin.min()) if len(margin) else np.inf
        return int((e2 < gate * gate).sum()), mg

    best_key = (-1, 0)
    if init_pose is not None:
        c, mg = count_at(init_pose)
        out["min_margin"] = min(out["min_margin"], mg)
        best_key, out["winner"], out["winner_pose"], out["winner_count"] = (c, 1), -1, np.asarray(init_pose, float).copy(), c
    for h in range(H):
        tr = sample_triple(int(o["seed"]), h, n)
        if tr is None:
            continue
        out["triples"][h] = tr
        P = pw[tr]
        cr = np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])) / max(np.linalg.norm(P[1] - P[0]) * np.linalg.norm(P[2] - P[0]), 1e-300)
        poses, info = hypothesis_poses(cam, P, pt[tr])
        r = sorted(info["roots"])
        flagged = info["marginal"] or cr < 1e-6 or any(b - a < 1e-6 for a, b in zip(r, r[1:]))
        out["n_poses"][h] = len(poses)
        best = -1                                            # ties to the pose the solver lists first, a count of 0 included
        for pose in poses:
            c, mg = count_at(pose)
            flagged |= mg < 1e-6
            out["min_margin"] = min(out["min_margin"], mg)
            if c > best:
                best, out["count"][h], out["pose"][h] = c, c, pose
        out["flagged"][h] = flagged
        if len(poses) and (int(out["count"][h]), 0) > best_key:          # ties: the initial pose, then the lowest h
            best_key, out["winner"], out["winner_pose"], out["winner_count"] = (int(out["count"][h]), 0), h, out["pose"][h].copy(), int(out["count"][h])
    if best_key[0] < 0:
        out["winner"], out["winner_pose"], out["winner_count"] = None, None, 0
    return out


# ---- refinement: scalar text, float64 (M = math, F = float) or mpmath (M = mp, F = mp.mpf) --------------------------------------------------
def _rot_s(u):
    x, y, z, w = u
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def pose_only_local(M, c, x, ob, pw, jac=True):
    """r [2] and the 2 x 6 Jacobian in the tangent of EigenQuaternionParameterization (+) Identity(3): rows 2 (A x d) | -A, A = R M_row"""
    n = M.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3])
    R = _rot_s([x[0] / n, x[1] / n, x[2] / n, x[3] / n])
    d = [pw[0] - x[4], pw[1] - x[5], pw[2] - x[6]]
    pb = [R[0][k] * d[0] + R[1][k] * d[1] + R[2][k] * d[2] for k in range(3)]
    E, c0 = c["E"], c["c0"]
    pc = [E[k][0] * pb[0] + E[k][1] * pb[1] + E[k][2] * pb[2] + c0[k] for k in range(3)]
    iz = 1 / pc[2]
    xp, yp = pc[0] * iz, pc[1] * iz
    r = [c["fx"] * xp + c["cx"] - ob[0], c["fy"] * yp + c["cy"] - ob[1]]
    if not jac:
        return r, None
    rows = [[c["fx"] * iz * (E[0][k] - xp * E[2][k]) for k in range(3)], [c["fy"] * iz * (E[1][k] - yp * E[2][k]) for k in range(3)]]
    L = []
    for m in rows:
        A = [R[k][0] * m[0] + R[k][1] * m[1] + R[k][2] * m[2] for k in range(3)]
        L.append([2 * (A[1] * d[2] - A[2] * d[1]), 2 * (A[2] * d[0] - A[0] * d[2]), 2 * (A[0] * d[1] - A[1] * d[0]), -A[0], -A[1], -A[2]])
    return r, L


def pose_plus(M, x, dl):
    """EigenQuaternionParameterization::Plus (q_delta * q) and t + dt"""
    nd = M.sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2])
    if nd == 0:
        q = list(x[:4])
    else:
        k = M.sin(nd) / nd
        ax, ay, az, aw = k * dl[0], k * dl[1], k * dl[2], M.cos(nd)
        bx, by, bz, bw = x[0], x[1], x[2], x[3]
        q = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
             aw * bw - ax * bx - ay * by - az * bz]
    return q + [x[4] + dl[3], x[5] + dl[4], x[6] + dl[5]]


def _huber_s(M, a, s):
    if a > 0 and s > a * a:
        r = M.sqrt(s)
        return 2 * a * r - a * a, a / r
    return s, s * 0 + 1


def refine_lm(cam, x0, pw, pt, huber_a=1.0, max_iters=10, lm=None, M=math, F=float):
    """the declared Ceres loop on one pose; returns (x [7] as a list of F, summary dict)"""
    o = dict(LM_DEFAULT); o.update(lm or {})
    cd = cam_derived(cam)
    c = dict(fx=F(cd["fx"]), fy=F(cd["fy"]), cx=F(cd["cx"]), cy=F(cd["cy"]), E=[[F(float(v)) for v in row] for row in cd["E"]], c0=[F(float(v)) for v in cd["c0"]])
    pw = [[F(float(v)) for v in p] for p in np.asarray(pw, float).reshape(-1, 3)]
    pt = [[F(float(v)) for v in p] for p in np.asarray(pt, float).reshape(-1, 2)]
    x = [F(float(v)) for v in x0]
    nb = len(pw)
    summ = dict(initial_cost=0.0, final_cost=0.0, num_iterations=0, num_successful_steps=0, termination=0, why="none")
    if nb == 0:
        return x, summ

    def cost_at(xx):                                         # the factor's own residual, as the linearisation has it: no depth test inside a solve
        cc = F(0.0)
        for i in range(nb):
            r, _ = pose_only_local(M, c, xx, pt[i], pw[i], False)
            cc += _huber_s(M, huber_a, r[0] * r[0] + r[1] * r[1])[0] / 2
        return cc

    x_start = list(x)
    radius, decrease = F(o["initial_trust_region_radius"]), F(2.0)
    iters = successes = invalid_run = 0
    termination, why = 1, "max_num_iterations"
    h0, cost, initial_cost = None, F(0.0), F(0.0)
    while True:
        H = [[F(0.0)] * 6 for _ in range(6)]
        g = [F(0.0)] * 6
        cost = F(0.0)
        for i in range(nb):
            r, L = pose_only_local(M, c, x, pt[i], pw[i])
            rho0, rho1 = _huber_s(M, huber_a, r[0] * r[0] + r[1] * r[1])
            cost += rho0 / 2
            for k in range(2):
                for u in range(6):
                    g[u] += rho1 * L[k][u] * r[k]
                    for v in range(u + 1):
                        H[u][v] += rho1 * L[k][u] * L[k][v]
        for u in range(6):
            for v in range(u + 1, 6):
                H[u][v] = H[v][u]
        if h0 is None:
            initial_cost, h0 = cost, [H[j][j] for j in range(6)]
        if iters >= max_iters:
            termination, why = 1, "max_num_iterations"; break
        if max(abs(v) for v in g) <= o["gradient_tolerance"]:
            termination, why = 0, "gradient_tolerance"; break
        if radius < 1e-32:
            termination, why = 0, "min_trust_region_radius"; break
        A = [row[:] for row in H]
        for j in range(6):
            s2 = (1 / (1 + M.sqrt(h0[j]))) ** 2
            A[j][j] += min(max(H[j][j] * s2, F(1e-6)), F(1e32)) / s2 / radius
        ok, Lc = True, [[F(0.0)] * 6 for _ in range(6)]
        for j in range(6):
            v = A[j][j] - sum((Lc[j][k] * Lc[j][k] for k in range(j)), F(0.0))
            if not v > 0:
                ok = False; break
            Lc[j][j] = M.sqrt(v)
            for i in range(j + 1, 6):
                Lc[i][j] = (A[i][j] - sum((Lc[i][k] * Lc[j][k] for k in range(j)), F(0.0))) / Lc[j][j]
        dx = [F(0.0)] * 6
        if ok:
            y = [F(0.0)] * 6
            for i in range(6):
                y[i] = (-g[i] - sum((Lc[i][k] * y[k] for k in range(i)), F(0.0))) / Lc[i][i]
            for i in range(5, -1, -1):
                dx[i] = (y[i] - sum((Lc[k][i] * dx[k] for k in range(i + 1, 6)), F(0.0))) / Lc[i][i]
        model = -sum((dx[u] * (g[u] + sum((H[u][v] * dx[v] for v in range(6)), F(0.0)) / 2) for u in range(6)), F(0.0))
        if not (ok and model > 0):
            iters += 1; invalid_run += 1
            if invalid_run >= 5:
                termination, why = 2, "consecutive_invalid_steps"; break
            radius = radius / 2
            continue
        invalid_run = 0
        xc = pose_plus(M, x, dx)
        sn = M.sqrt(sum(((xc[k] - x[k]) ** 2 for k in range(7)), F(0.0)))
        xn = M.sqrt(sum((x[k] ** 2 for k in range(7)), F(0.0)))
        if sn <= o["parameter_tolerance"] * (xn + o["parameter_tolerance"]):
            termination, why = 0, "parameter_tolerance"; break
        cand = cost_at(xc)
        if abs(cost - cand) <= o["function_tolerance"] * cost:
            termination, why = 0, "function_tolerance"; break
        iters += 1
        rho = (cost - cand) / model
        if rho > o["min_relative_decrease"]:
            x, cost = xc, cand
            successes += 1
            t = 2 * rho - 1
            radius, decrease = min(radius / max(F(1.0) / 3, 1 - t * t * t), F(1e16)), F(2.0)
        else:
            radius = radius / decrease; decrease = decrease * 2
    if termination == 2 or not M.isfinite(cost):
        termination, cost, x = 2, initial_cost, x_start
    summ.update(initial_cost=float(initial_cost), final_cost=float(cost), num_iterations=iters, num_successful_steps=successes, termination=termination, why=why)
    return x, summ


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------
def pnp_ransac(cam, pw, pt, init_pose=None, opt=None, keep=None):
    """returns dict(pose or None (untouched), score, inlier [n] uint8, summary (the last round's), n_matches, scored (score_hypotheses' dict));
    `keep` (a dict) receives the winner's pose and every round's inlier set (for the extended-precision run of the tests)"""
    o = dict(PNP_DEFAULT); o.update(opt or {})
    pw, pt = np.asarray(pw, float).reshape(-1, 3), np.asarray(pt, np.float32).reshape(-1, 2).astype(np.float64)
    n = len(pw)
    out = dict(pose=None, score=0, inlier=np.zeros(n, np.uint8), summary=None, n_matches=n, scored=None)
    if n < max(int(o["min_matches"]), 3):
        return out
    sc = score_hypotheses(cam, pw, pt, o, init_pose)
    out["scored"] = sc
    if sc["winner"] is None:
        return out
    gate2 = float(o["max_reproj_px"]) ** 2
    x = sc["winner_pose"].copy()
    if keep is not None:
        keep.update(start=x.copy(), inliers=[])
    for _ in range(int(o["refine_rounds"])):
        inl = reproj_err2(cam, x, pw, pt) < gate2
        if keep is not None:
            keep["inliers"].append(inl.copy())
        xs, out["summary"] = refine_lm(cam, x, pw[inl], pt[inl], float(o["huber_a"]), int(o["refine_iterations"]))
        x = np.array([float(v) for v in xs])
    inl = reproj_err2(cam, x, pw, pt) < gate2
    out.update(pose=x, inlier=inl.astype(np.uint8), score=int(inl.sum()))
    return out


def relocate_by_image(cam, old_pose, old_pw, old_desc, cur_pt, cur_desc, relative_o_c, match_opt=None, pnp_opt=None):
    """queries = the current features, train = the old frame's.  Returns dict(match [n_cur], inlier [n_cur], score, relative_o_c, pose, pnp)"""
    m, _, _ = match(cur_desc, old_desc, match_opt)
    q = np.nonzero(m >= 0)[0]
    cur_pt = np.asarray(cur_pt, np.float32).reshape(-1, 2)
    init = sophus_mul(old_pose, relative_o_c)
    r = pnp_ransac(cam, np.asarray(old_pw, float).reshape(-1, 3)[m[q]], cur_pt[q], init, pnp_opt)
    inl = np.zeros(len(m), np.uint8)
    inl[q] = r["inlier"]
    rel = np.asarray(relative_o_c, float).copy() if r["pose"] is None else sophus_mul(sophus_inverse(old_pose), r["pose"])
    return dict(match=m, inlier=inl, score=r["score"], relative_o_c=rel, pose=r["pose"], pnp=r)
