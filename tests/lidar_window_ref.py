"""Declared semantics of LiDAR plane factors on keyframe poses inside the window solve, in numpy (test infrastructure; the device is
tested against this file).

The factor is the reference's LidarPlaneError<1,7> (lidar_error.hpp:10-40): declared there, with a Create() nothing calls.  Block i sits on
the pose of keyframe k = kf[i]:

    r_i = w_i * n_i . (R(q_k / |q_k|) p_i + t_k - pa_i)

n_i the unit normal of (pa - pb) x (pa - pc) as the constructor forms it (a zero cross product stays zero: a null block), p_i in the
keyframe's body frame, pa, pb, pc in the world frame; the quaternion is normalised inside, as SE3TransformPoint does.  With w_i = 1 this is
the functor exactly (pinned to the oracle's Jet autodiff of it in tests/test_lidar_window_ref.py).

DEVIATION FROM THE REFERENCE — the only one: a per-block weight w_i and a per-block Huber a_i (<= 0: no loss; Ceres' corrector with
rho'' <= 0, as test_oracle_lm_numpy.huber_scale states it).  The reference scales its 3-DoF plane functors by one weight per problem and
gives a problem one loss; its conventions are ground w = 1 with no loss and surf w = 0.01 with a = 0.1, and a window holds both kinds.

    plane_normals / plane_rows      the factor: residuals, 1 x 7 ambient Jacobians (Ceres' layout), 1 x 6 tangent Jacobians
    lidar_rows                      the robustified rows of a block set in the dense Jacobian's column layout
    dense_system                    test_oracle_lm_numpy.dense_system with the lidar rows appended
    trial_step / lm_iteration       one trust-region trial, test_oracle_lm_numpy's one-iteration body
    lm_solve                        the full loop: oracle/lm.h lm_solve's order of tests restated
"""
import numpy as np

from tests.test_oracle_lm_numpy import dense_system as visual_imu_system
from tests.test_oracle_lm_numpy import huber_scale, quat_plus, quat_plus_jac

GROUND = dict(weight=1.0, huber_a=0.0)        # the reference's conventions (mapping.cpp: weights.lidar_ground / lidar_surf, HuberLoss(0.1) on surf)
SURF = dict(weight=0.01, huber_a=0.1)


def rotmat(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def plane_normals(pa, pb, pc):
    """LidarPlaneError's constructor: (pa - pb) x (pa - pc), normalised; Eigen's normalize() leaves a zero vector zero"""
    pa, pb, pc = (np.asarray(a, np.float64).reshape(-1, 3) for a in (pa, pb, pc))
    n = np.cross(pa - pb, pa - pc)
    z = (n * n).sum(axis=1)
    s = np.where(z > 0, np.sqrt(np.where(z > 0, z, 1.0)), 1.0)
    return n / s[:, None]


def _skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def drot_dq(q, p):
    """d (R(q/|q|) p) / dq, 3 x 4 in Eigen's coefficient order (x, y, z, w): the derivative at the unit quaternion times the projector
    of the normalisation, (I - u u^T) / |q|"""
    q = np.asarray(q, np.float64)
    nq = np.linalg.norm(q)
    u = q / nq
    v, w = u[:3], u[3]
    dv = 2.0 * (-w * _skew(p) + (v @ p) * np.eye(3) + np.outer(v, p) - 2.0 * np.outer(p, v))
    dw = 2.0 * np.cross(v, p)
    Ju = np.concatenate([dv, dw[:, None]], axis=1)
    return Ju @ (np.eye(4) - np.outer(u, u)) / nq


def make_lidar(p, pa, pb, pc, kf, weight=None, huber_a=None):
    """a block set: dict(p, pa, nrm [n][3], kf [n], weight, huber_a [n])"""
    p, pa = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(pa, np.float64).reshape(-1, 3)
    n = p.shape[0]
    full = lambda a, dflt: np.ascontiguousarray(np.broadcast_to(np.asarray(dflt if a is None else a, np.float64), (n,)))
    return dict(p=p, pa=pa, nrm=plane_normals(pa, pb, pc), kf=np.asarray(kf, np.int64).reshape(-1), weight=full(weight, 1.0), huber_a=full(huber_a, 0.0))


def empty_lidar():
    z = np.zeros((0, 3))
    return make_lidar(z, z, z, z, np.zeros(0, np.int64))


def take(lidar, idx):
    return {k: v[idx] for k, v in lidar.items()}


def plane_rows(lidar, poses):
    """(r [n], J7 [n][7]): the raw residuals (weight applied, no loss) and the ambient Jacobians, Ceres' layout [qx qy qz qw tx ty tz]"""
    n = len(lidar["kf"])
    r, J = np.zeros(n), np.zeros((n, 7))
    for i in range(n):
        T = poses[lidar["kf"][i]]
        w, nn, p = lidar["weight"][i], lidar["nrm"][i], lidar["p"][i]
        r[i] = w * nn @ (rotmat(T[:4]) @ p + T[4:] - lidar["pa"][i])
        J[i, :4] = w * nn @ drot_dq(T[:4], p)
        J[i, 4:] = w * nn
    return r, J


def plane_rows_local(lidar, poses):
    """(r [n], J6 [n][6]): the same in the tangent of ProductParameterization(EigenQuaternion, Identity3)"""
    r, J7 = plane_rows(lidar, poses)
    J6 = np.zeros((len(r), 6))
    for i in range(len(r)):
        J6[i, :3] = J7[i, :4] @ quat_plus_jac(poses[lidar["kf"][i]][:4])
        J6[i, 3:] = J7[i, 4:]
    return r, J6


def lidar_rows(lidar, poses, ncol):
    """(J [n][ncol], r [n], cost, outside [n] bool): the robustified rows in dense_system's column layout; `outside` marks the blocks beyond
    their Huber threshold"""
    r, J6 = plane_rows_local(lidar, poses)
    n = len(r)
    J, rr, cost, outside = np.zeros((n, ncol)), np.zeros(n), 0.0, np.zeros(n, bool)
    for i in range(n):
        rho, sc = huber_scale(lidar["huber_a"][i], r[i] * r[i])
        cost += 0.5 * rho
        outside[i] = sc != 1.0
        k = lidar["kf"][i]
        J[i, 6 * k:6 * k + 6] = sc * J6[i]
        rr[i] = sc * r[i]
    return J, rr, cost, outside


def dense_system(oracle, cfg, pre, state, lidar, huber_a=1.0, pose_const=None):
    """(J, r, cost) over [pose tangents 6 n_kf | (v, ba, bg) 9 n_kf | inverse depths n_lm]: the rows test_oracle_lm_numpy assembles, then
    the lidar rows.  pose_const [n_kf]: those keyframes' pose columns are zero (constant blocks are not in Ceres' program)."""
    n_kf, n_lm = cfg["n_kf"], cfg["n_lm"]
    J, r, cost = visual_imu_system(oracle, cfg, pre, state, huber_a)
    Jl, rl, cl, _ = lidar_rows(lidar, state[0], 15 * n_kf + n_lm)
    J, r, cost = np.concatenate([J, Jl]), np.concatenate([r, rl]), cost + cl
    if pose_const is not None:
        for k in np.flatnonzero(np.asarray(pose_const)):
            J[:, 6 * k:6 * k + 6] = 0.0
    return J, r, cost


def reduced(H, g, D, d):
    """the Schur complement of the damped normal equations on the inverse depths: (S [d][d], rhs [d])"""
    A = H + np.diag(D)
    if A.shape[0] == d:
        return A, -g
    ic = 1.0 / np.diag(A[d:, d:])
    return A[:d, :d] - (A[:d, d:] * ic) @ A[d:, :d], -g[:d] + A[:d, d:] @ (g[d:] * ic)


def apply_step(state, dx, n_kf):
    new = [s.copy() for s in state]
    for k in range(n_kf):
        new[0][k, :4] = quat_plus(state[0][k, :4], dx[6 * k:6 * k + 3]); new[0][k, 4:] += dx[6 * k + 3:6 * k + 6]
        o = 6 * n_kf + 9 * k
        new[1][k] += dx[o:o + 3]; new[2][k] += dx[o + 3:o + 6]; new[3][k] += dx[o + 6:o + 9]
    new[4] = state[4] + dx[15 * n_kf:]
    return new


def trial_step(oracle, cfg, pre, state, lidar, radius, jac, huber_a=1.0, pose_const=None):
    """One trial step at `radius`, Ceres literally (test_oracle_lm_numpy's body): Jacobi scaling s = 1 / (1 + |J_j|) taken at the solve's first
    linearisation and frozen (`jac`: a dict, start with {}), the diagonal of the SCALED normal equations clamped to [1e-6, 1e32], the scaled
    system solved, dx = s y.  Nothing is committed."""
    n_kf = cfg["n_kf"]
    J, r, cost = dense_system(oracle, cfg, pre, state, lidar, huber_a, pose_const)
    if "s" not in jac:
        jac["s"] = 1.0 / (1.0 + np.sqrt((J * J).sum(axis=0)))
    s = jac["s"]
    Js = J * s
    H, g = J.T @ J, J.T @ r
    Hs, gs = Js.T @ Js, Js.T @ r
    diag = np.minimum(np.maximum(np.diag(Hs), 1e-6), 1e32)
    D = diag / s ** 2 / radius
    out = dict(cost_before=cost, gradient_max_norm=float(np.abs(g).max()), H=H, g=g, D=D, state=state, solved=True, valid=False,
               cost_after=cost, model=0.0, rho=0.0, step_norm=0.0, x_norm=0.0)
    try:
        np.linalg.cholesky(Hs + np.diag(diag / radius))
        y = np.linalg.solve(Hs + np.diag(diag / radius), -gs)
    except np.linalg.LinAlgError:
        out["solved"] = False
        return out
    dx = s * y
    out["dx"] = dx
    out["model"] = float(-(Js @ y) @ (r + 0.5 * (Js @ y)))
    out["valid"] = out["model"] > 0.0
    new = apply_step(state, dx, n_kf)
    out["candidate"] = new
    out["cost_after"] = dense_system(oracle, cfg, pre, new, lidar, huber_a, pose_const)[2]
    out["rho"] = (cost - out["cost_after"]) / out["model"] if out["valid"] else -1.0
    # Ceres: |x - x_plus_delta| and |x| over the ambient parameter vector of the reduced program (constant poses are not in it)
    free = np.ones(n_kf, bool) if pose_const is None else ~np.asarray(pose_const, bool)
    sn = ((state[0][free] - new[0][free]) ** 2).sum() + sum(((state[q] - new[q]) ** 2).sum() for q in (1, 2, 3, 4))
    xn = (state[0][free] ** 2).sum() + sum((state[q] ** 2).sum() for q in (1, 2, 3, 4))
    out["step_norm"], out["x_norm"] = float(np.sqrt(sn)), float(np.sqrt(xn))
    return out


def lm_iteration(oracle, cfg, pre, state, lidar, radius, dec, jac, huber_a=1.0, min_relative_decrease=1e-3, pose_const=None):
    """one iteration with the radius handed in, no termination tests (oracle/lm.h lm_iteration): (trial, new state, radius, dec, accepted)"""
    t = trial_step(oracle, cfg, pre, state, lidar, radius, jac, huber_a, pose_const)
    if not (t["solved"] and t["valid"]):
        return t, state, radius * 0.5, dec, False
    if t["rho"] > min_relative_decrease:
        q = 2.0 * t["rho"] - 1.0
        return t, t["candidate"], min(radius / max(1.0 / 3.0, 1.0 - q ** 3), 1e16), 2.0, True
    return t, state, radius / dec, dec * 2.0, False


def lm_solve(oracle, cfg, pre, state, lidar, max_num_iterations=50, huber_a=1.0, initial_trust_region_radius=1e4, function_tolerance=1e-6,
             gradient_tolerance=1e-10, parameter_tolerance=1e-8, min_relative_decrease=1e-3, pose_const=None):
    """ceres::Solve's TrustRegionMinimizer loop in oracle/lm.h lm_solve's order: at the top the iteration cap, the gradient tolerance and the
    smallest radius; an invalid step halves the radius and counts (five in a row: failure); the parameter and then the function tolerance
    BEFORE the step-quality test (the candidate is not taken); then accept or reject.  Returns (summary dict, final state); trace rows are
    (cost_before, cost_after, radius used, accepted, valid, rho) per trial."""
    radius, dec = initial_trust_region_radius, 2.0
    s = dict(num_iterations=0, num_successful_steps=0, num_unsuccessful_steps=0, termination=1, why="max_num_iterations", initial_cost=None)
    jac, invalid_run, trace, cost = {}, 0, [], 0.0
    while True:
        t = trial_step(oracle, cfg, pre, state, lidar, radius, jac, huber_a, pose_const)
        if s["initial_cost"] is None:
            s["initial_cost"] = t["cost_before"]
        cost = t["cost_before"]
        if s["num_iterations"] >= max_num_iterations:
            s["termination"], s["why"] = 1, "max_num_iterations"; break
        if t["gradient_max_norm"] <= gradient_tolerance:
            s["termination"], s["why"] = 0, "gradient_tolerance"; break
        if radius < 1e-32:
            s["termination"], s["why"] = 0, "min_trust_region_radius"; break
        valid = t["solved"] and t["valid"]
        row = [t["cost_before"], t["cost_after"], radius, 0.0, float(valid), t["rho"]]
        trace.append(row)
        if not valid:
            s["num_iterations"] += 1; s["num_unsuccessful_steps"] += 1
            invalid_run += 1
            if invalid_run >= 5:
                s["termination"], s["why"] = 2, "consecutive_invalid_steps"; break
            radius *= 0.5
            continue
        invalid_run = 0
        if t["step_norm"] <= parameter_tolerance * (t["x_norm"] + parameter_tolerance):
            s["termination"], s["why"] = 0, "parameter_tolerance"; break
        if abs(t["cost_before"] - t["cost_after"]) <= function_tolerance * t["cost_before"]:
            s["termination"], s["why"] = 0, "function_tolerance"; break
        s["num_iterations"] += 1
        if t["rho"] > min_relative_decrease:
            state = t["candidate"]; cost = t["cost_after"]
            q = 2.0 * t["rho"] - 1.0
            radius, dec = min(radius / max(1.0 / 3.0, 1.0 - q ** 3), 1e16), 2.0
            s["num_successful_steps"] += 1; row[3] = 1.0
        else:
            radius, dec = radius / dec, dec * 2.0
            s["num_unsuccessful_steps"] += 1
    s.update(final_cost=cost, final_radius=radius, final_decrease_factor=dec, trace=np.array(trace).reshape(-1, 6))
    return s, state
