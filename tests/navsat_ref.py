"""CPU restatement of the GNSS (NavSat) alignment — TEST INFRASTRUCTURE ONLY, numpy fp64.  PARITY UNPINNED: the reference's
navsat_error.hpp does not compile over the stand-in headers of oracle/ref_shim (it needs SO3d::num_parameters, and cov2sqrt_info indexes a
3x3 matrix linearly), so there is no reference-compiled golden for it; this file is the statement of record the device code
(lvio_fusion_amd/csrc/navsat_kernels.hip) follows, and `mp_*` below is an independent 50-digit statement of the three residuals.

  functors     src/lvio_fusion/include/lvio_fusion/ceres/navsat_error.hpp:9-120, forward-mode duals over the functor text's operation order
  lm_dense     ceres::Solve(DENSE_QR) on <= 6 scalar parameter blocks with the solver semantics DECLARED in oracle/lm.h (header and lm_solve),
               oracle/robust.h and oracle/loop.h, plus what these problems add: a loss on whole 3-vector blocks, constant blocks, box bounds
  initialize   Navsat::Initialize   src/lvio_fusion/src/navsat.cpp:100-133
  optimize_bc  Navsat::OptimizeBC   src/lvio_fusion/src/navsat.cpp:192-269
  fix_chain    the loop of Navsat::Optimize / QuickFix  src/lvio_fusion/src/navsat.cpp:150-155, :171-176

Box bounds (SetParameterLowerBound / UpperBound; Ceres is un-vendored, DECLARED from upstream trust_region_minimizer.cc / line_search.cc):
the start point is projected onto the box before the first evaluation; Plus projects every candidate; the gradient test uses the projected
gradient max|P(x - g) - x|; after the trust-region step and before the candidate is evaluated, a projected Armijo search along the step
delta starts at step size 1 and accepts t when f(P(x + t delta)) <= f(x) + 1e-4 t g.delta, else contracts: t <- the minimiser of the
quadratic through f(0), g.delta and (t, f(t)), clamped to [1e-3 t, 0.6 t] (one CONTRACTION, counted); at most 20 samples, minimum step size
1e-9; an accepted t scales delta, a failed search leaves delta as it is; model_cost_change is that of the unscaled step.  Problems without
bounds take none of this path.

Pose products are Sophus' as oracle/loop.h forward_update states them (the `po` argument is the `oracle` fixture, oracle/pyoracle.py)."""
import numpy as np

DEFAULT_OPT = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, min_relative_decrease=1e-3,
                   initial_trust_region_radius=1e4)
WHY = ("none", "gradient_tolerance", "parameter_tolerance", "function_tolerance", "min_trust_region_radius", "max_num_iterations", "consecutive_invalid_steps")


# ---- forward-mode duals, vectorised over the blocks: a [nb], v [nb][P] --------------------------------------------------------------
class Dual:
    __slots__ = ("a", "v")

    def __init__(self, a, v):
        self.a, self.v = a, v

    @staticmethod
    def lift(x, like):
        return x if isinstance(x, Dual) else Dual(np.broadcast_to(np.asarray(x, dtype=np.float64), like.a.shape), np.zeros_like(like.v))

    def __add__(self, o):
        o = Dual.lift(o, self); return Dual(self.a + o.a, self.v + o.v)

    def __sub__(self, o):
        o = Dual.lift(o, self); return Dual(self.a - o.a, self.v - o.v)

    def __rsub__(self, o):
        return Dual.lift(o, self) - self

    def __neg__(self):
        return Dual(-self.a, -self.v)

    def __mul__(self, o):
        o = Dual.lift(o, self); return Dual(self.a * o.a, self.a[:, None] * o.v + self.v * o.a[:, None])

    __radd__ = __add__
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o, self)
        iy = 1.0 / o.a
        a = self.a * iy
        return Dual(a, (self.v - a[:, None] * o.v) * iy[:, None])


    def __rtruediv__(self, o):
        return Dual.lift(o, self) / self


def dsin(x):
    return Dual(np.sin(x.a), np.cos(x.a)[:, None] * x.v)


def dcos(x):
    return Dual(np.cos(x.a), -np.sin(x.a)[:, None] * x.v)


def dsqrt(x):
    r = np.sqrt(x.a)
    return Dual(r, (0.5 / r)[:, None] * x.v)


def _const(val, nb, P):
    return Dual(np.broadcast_to(np.asarray(val, dtype=np.float64), (nb,)).copy(), np.zeros((nb, P)))


def _seed(val, k, nb, P, jac):
    d = _const(val, nb, P)
    if jac:
        d.v[:, k] = 1.0
    return d


# ---- base.hpp helpers in the functor text's order ------------------------------------------------------------------------------------
def rpy_to_eigen_quat(rpy):
    z, y, x = rpy[0] / 2.0, rpy[1] / 2.0, rpy[2] / 2.0
    c_z, s_z, c_y, s_y, c_x, s_x = dcos(z), dsin(z), dcos(y), dsin(y), dcos(x), dsin(x)
    w = c_z * c_y * c_x + s_z * s_y * s_x
    qx = c_z * c_y * s_x - s_z * s_y * c_x
    qy = c_z * s_y * c_x + s_z * c_y * s_x
    qz = s_z * c_y * c_x - c_z * s_y * s_x
    return [qx, qy, qz, w]


def quat_rotate_wxyz(q, pt):
    scale = 1.0 / dsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    u0, u1, u2, u3 = scale * q[0], scale * q[1], scale * q[2], scale * q[3]
    t2, t3, t4, t5, t6, t7, t8, t9, t1 = u0 * u1, u0 * u2, u0 * u3, -(u1 * u1), u1 * u2, u1 * u3, -(u2 * u2), u2 * u3, -(u3 * u3)
    return [2.0 * ((t8 + t1) * pt[0] + (t6 - t4) * pt[1] + (t3 + t7) * pt[2]) + pt[0],
            2.0 * ((t4 + t6) * pt[0] + (t5 + t1) * pt[1] + (t9 - t2) * pt[2]) + pt[1],
            2.0 * ((t7 - t3) * pt[0] + (t2 + t9) * pt[1] + (t5 + t8) * pt[2]) + pt[2]]


def eigen_quat_rotate(eq, pt):
    return quat_rotate_wxyz([eq[3], eq[0], eq[1], eq[2]], pt)


def quat_product_wxyz(z, w):
    return [z[0] * w[0] - z[1] * w[1] - z[2] * w[2] - z[3] * w[3],
            z[0] * w[1] + z[1] * w[0] + z[2] * w[3] - z[3] * w[2],
            z[0] * w[2] - z[1] * w[3] + z[2] * w[0] + z[3] * w[1],
            z[0] * w[3] + z[1] * w[2] - z[2] * w[1] + z[3] * w[0]]


def se3_product(A, B):
    zw = quat_product_wxyz([A[3], A[0], A[1], A[2]], [B[3], B[0], B[1], B[2]])
    t = eigen_quat_rotate(A, B[4:7])
    return [zw[1], zw[2], zw[3], zw[0], A[4] + t[0], A[5] + t[1], A[6] + t[2]]


def se3_transform_point(se3, pt):
    r = eigen_quat_rotate(se3, pt)
    return [r[0] + se3[4], r[1] + se3[5], r[2] + se3[6]]


def cov2sqrt_info(cov):
    """navsat_error.hpp:9-15 for the diagonal covariance the reference passes (Eigen's inverse() + LLT may differ in the last bit)."""
    return np.sqrt(1.0 / np.asarray(cov, dtype=np.float64))


def _pack(rr, jac):
    r = np.stack([d.a for d in rr], axis=1)
    return r, (np.stack([d.v for d in rr], axis=1) if jac else None)


# ---- the three functors: r [nb][m], J [nb][m][P] --------------------------------------------------------------------------------------
def navsat_init(p0, p1, cov, x3, jac=True):
    """NavsatInitError <3,1,1,1> at x3 = (yaw, x, y) (navsat_error.hpp:27-40)."""
    p0, p1, sq = np.asarray(p0, float).reshape(-1, 3), np.asarray(p1, float).reshape(-1, 3), cov2sqrt_info(cov).reshape(-1, 3)
    nb = p0.shape[0]
    yaw, x, y = (_seed(x3[k], k, nb, 3, jac) for k in range(3))
    zero = _const(0.0, nb, 3)
    tf = rpy_to_eigen_quat([yaw, zero, zero]) + [x, y, zero]
    tp = se3_transform_point(tf, [_const(p1[:, k], nb, 3) for k in range(3)])
    return _pack([_const(sq[:, k], nb, 3) * (_const(p0[:, k], nb, 3) - tp[k]) for k in range(3)], jac)


def navsat_rx(p0, p1, pose, cov, x6, jac=True):
    """NavsatRXError <3,1,1,1,1,1,1> at x6 = (yaw, pitch, roll, x, y, z) (navsat_error.hpp:64-79)."""
    p0, p1, sq = np.asarray(p0, float).reshape(-1, 3), np.asarray(p1, float).reshape(-1, 3), cov2sqrt_info(cov).reshape(-1, 3)
    nb = p0.shape[0]
    prm = [_seed(x6[k], k, nb, 6, jac) for k in range(6)]
    rel = rpy_to_eigen_quat(prm[:3]) + prm[3:]
    tf = se3_product([_const(pose[k], nb, 6) for k in range(7)], rel)
    tp = se3_transform_point(tf, [_const(p1[:, k], nb, 6) for k in range(3)])
    return _pack([_const(sq[:, k], nb, 6) * (_const(p0[:, k], nb, 6) - tp[k]) for k in range(3)], jac)


def navsat_r(y3, pose, roll, jac=True):
    """NavsatRError <1,1> (navsat_error.hpp:98-110): r [1][1], J [1][1][1]."""
    rl = _seed(roll, 0, 1, 1, jac)
    zero = _const(0.0, 1, 1)
    rel = rpy_to_eigen_quat([zero, zero, rl])
    P = [_const(pose[k], 1, 1) for k in range(4)]
    zw = quat_product_wxyz([P[3], P[0], P[1], P[2]], [rel[3], rel[0], rel[1], rel[2]])
    tf_y = eigen_quat_rotate([zw[1], zw[2], zw[3], zw[0]], [_const(y3[k], 1, 1) for k in range(3)])
    return _pack([tf_y[2]], jac)


# ---- the solver --------------------------------------------------------------------------------------------------------------------------
def huber(a, s):
    """HuberLoss::Evaluate on s = |r_b|^2: (rho, rho'); a <= 0: no loss."""
    s = np.asarray(s, dtype=np.float64)
    if a <= 0.0:
        return s.copy(), np.ones_like(s)
    out = s > a * a
    r = np.sqrt(np.where(out, s, 1.0))
    return np.where(out, 2.0 * a * r - a * a, s), np.where(out, np.maximum(2.2250738585072014e-308, a / r), 1.0)


def _ordered_sum(a, reverse):
    a = a[::-1] if reverse else a
    out = np.zeros(a.shape[1:])
    for row in a:      # block by block, in order
        out = out + row
    return out


def lm_dense(evalf, x0, free, lo=None, hi=None, huber_a=0.0, opt=None, reverse=False):
    """The declared TrustRegionMinimizer loop.  evalf(x, jac) -> (r [nb][m], J [nb][m][P] or None) at the full parameter vector x [P];
    `free`: the indices of the non-constant parameters IN COLUMN ORDER (the order in which the reference adds the parameter blocks);
    lo / hi: per-parameter bounds (None or +-inf = none).  `reverse` sums the blocks in reverse order (a robustness probe for the tests).
    Returns (x, summary dict) — summary['contractions'] counts the line search's step-size contractions, ['huber_active'] the linearisations
    at which some block was in Huber's linear zone.  A FAILURE returns x0."""
    o = dict(DEFAULT_OPT); o.update(opt or {})
    x = np.array(x0, dtype=np.float64)
    P = x.size
    free = list(free)
    d = len(free)
    lo = np.full(P, -np.inf) if lo is None else np.array([-np.inf if v is None else v for v in lo], dtype=np.float64)
    hi = np.full(P, np.inf) if hi is None else np.array([np.inf if v is None else v for v in hi], dtype=np.float64)
    summ = dict(initial_cost=0.0, final_cost=0.0, num_iterations=0, num_successful_steps=0, termination=0, why="none", contractions=0, huber_active=0)

    def cost_at(xx):
        r, _ = evalf(xx, False)
        return 0.5 * float(_ordered_sum(huber(huber_a, (r * r).sum(axis=1))[0][:, None], reverse)[0])

    r, _ = evalf(x, False)
    if r.shape[0] == 0:      # no residual block: the unused parameter blocks are dropped, nothing moves
        return x, summ
    if d == 0:               # every block constant
        summ["initial_cost"] = summ["final_cost"] = cost_at(x)
        return x, summ
    fidx = np.array(free)
    bounded = bool(np.any(np.isfinite(lo[fidx])) or np.any(np.isfinite(hi[fidx])))

    def project(xx):
        xx = xx.copy()
        xx[fidx] = np.minimum(np.maximum(xx[fidx], lo[fidx]), hi[fidx])
        return xx

    x_start = x.copy()
    if bounded:
        x = project(x)
    radius, decrease = o["initial_trust_region_radius"], 2.0
    iters = successes = invalid_run = 0
    termination, why = 1, "max_num_iterations"
    h0 = None
    cost = initial_cost = 0.0
    while True:
        r, J = evalf(x, True)
        rho0, rho1 = huber(huber_a, (r * r).sum(axis=1))
        if huber_a > 0.0 and np.any(rho1 < 1.0):
            summ["huber_active"] += 1
        cost = 0.5 * float(_ordered_sum(rho0[:, None], reverse)[0])
        sc = np.sqrt(rho1)                                   # Corrector, rho'' <= 0
        rs = r * sc[:, None]
        Js = J[:, :, fidx] * sc[:, None, None]
        g = _ordered_sum(np.einsum("bkc,bk->bc", Js, rs), reverse)
        H = _ordered_sum(np.einsum("bku,bkv->buv", Js, Js), reverse)
        if h0 is None:
            initial_cost, h0 = cost, np.diag(H).copy()
        if iters >= o["max_num_iterations"]:
            termination, why = 1, "max_num_iterations"; break
        gn = float(np.max(np.abs(x[fidx] - np.minimum(np.maximum(x[fidx] - g, lo[fidx]), hi[fidx])))) if bounded else float(np.max(np.abs(g)))
        if gn <= o["gradient_tolerance"]:
            termination, why = 0, "gradient_tolerance"; break
        if radius < 1e-32:
            termination, why = 0, "min_trust_region_radius"; break
        A = H.copy()
        for j in range(d):
            s2 = (1.0 / (1.0 + np.sqrt(h0[j]))) ** 2
            A[j, j] += min(max(H[j, j] * s2, 1e-6), 1e32) / s2 / radius      # oracle/robust.h lm_damping
        ok, L = True, np.zeros((d, d))
        for j in range(d):
            v = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
            if not v > 0.0:
                ok = False; break
            L[j, j] = np.sqrt(v)
            for i in range(j + 1, d):
                L[i, j] = (A[i, j] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
        dx = np.zeros(d)
        if ok:
            y = np.zeros(d)
            for i in range(d):
                y[i] = (-g[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
            for i in range(d - 1, -1, -1):
                dx[i] = (y[i] - float(np.dot(L[i + 1:, i], dx[i + 1:]))) / L[i, i]
        model = -float(np.dot(dx, g + 0.5 * (H @ dx)))
        if not (ok and model > 0.0):                         # invalid step
            iters += 1
            invalid_run += 1
            if invalid_run >= 5:
                termination, why = 2, "consecutive_invalid_steps"; break
            radius *= 0.5
            continue
        invalid_run = 0
        if bounded:
            gd = float(np.dot(g, dx))
            if gd < 0.0:
                t, found = 1.0, False
                for _ in range(20):
                    xt = x.copy(); xt[fidx] = x[fidx] + t * dx
                    ft = cost_at(project(xt))
                    if ft <= cost + 1e-4 * t * gd:
                        found = True; break
                    tn = -gd * t * t / (2.0 * (ft - cost - gd * t))
                    tn = min(max(tn, 1e-3 * t), 0.6 * t)
                    summ["contractions"] += 1
                    if tn < 1e-9:
                        break
                    t = tn
                if found:
                    dx = dx * t
        xc = x.copy(); xc[fidx] = x[fidx] + dx
        if bounded:
            xc = project(xc)
        if np.sqrt(float(np.sum((xc[fidx] - x[fidx]) ** 2))) <= o["parameter_tolerance"] * (np.sqrt(float(np.sum(x[fidx] ** 2))) + o["parameter_tolerance"]):
            termination, why = 0, "parameter_tolerance"; break
        cand = cost_at(xc)
        if abs(cost - cand) <= o["function_tolerance"] * cost:
            termination, why = 0, "function_tolerance"; break
        iters += 1
        rho = (cost - cand) / model
        if rho > o["min_relative_decrease"]:
            x, cost = xc, cand
            successes += 1
            t = 2.0 * rho - 1.0
            radius, decrease = min(radius / max(1.0 / 3.0, 1.0 - t * t * t), 1e16), 2.0
        else:
            radius /= decrease; decrease *= 2.0
    if termination == 2 or not np.isfinite(cost):
        termination, cost, x = 2, initial_cost, x_start
    summ.update(initial_cost=initial_cost, final_cost=cost, num_iterations=iters, num_successful_steps=successes, termination=termination, why=why)
    return x, summ


# ---- Sophus operations (as lvio_fusion_amd/csrc/loop_dev.hpp) -----------------------------------------------------------------------------
def quat_transform_vector(q, v):
    """Eigen QuaternionBase::_transformVector, q (x,y,z,w) taken as it is; q [..][4], v [..][3]."""
    q, v = np.asarray(q, float), np.asarray(v, float)
    ux, uy, uz, uw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    cx, cy, cz = 2.0 * (uy * v2 - uz * v1), 2.0 * (uz * v0 - ux * v2), 2.0 * (ux * v1 - uy * v0)
    return np.stack([v0 + uw * cx + (uy * cz - uz * cy), v1 + uw * cy + (uz * cx - ux * cz), v2 + uw * cz + (ux * cy - uy * cx)], axis=-1)


def sophus_inverse(a):
    a = np.asarray(a, float)
    qn = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3])
    u = np.array([-(a[0] / qn), -(a[1] / qn), -(a[2] / qn), a[3] / qn])
    return np.concatenate([u, quat_transform_vector(u, -a[4:7])])


def sophus_mul(po, A, B):
    """A * B as PoseGraph::ForwardUpdate forms it (oracle/loop.h forward_update)."""
    return po.forward_update(A, np.asarray(B, float).reshape(1, 7))[0][0]


def sophus_transform_point(a, p):
    return quat_transform_vector(a[:4], p) + a[4:7]


# ---- the three procedures ---------------------------------------------------------------------------------------------------------------
def initialize(po, position, raw, cov, opt=None, reverse=False, scale=1.0):
    """Navsat::Initialize.  `scale` multiplies the fixes (position) — a robustness probe.  Returns (para6, extrinsic7, stage 1, stage 2)."""
    position, raw, cov = np.asarray(position, float).reshape(-1, 3) * scale, np.asarray(raw, float).reshape(-1, 3), np.asarray(cov, float).reshape(-1, 3)
    evalf = lambda x, jac: navsat_init(position, raw, cov, x, jac)
    x, s1 = lm_dense(evalf, np.zeros(3), [0], opt=opt, reverse=reverse)              # x, y constant (navsat.cpp:109-110)
    x, s2 = lm_dense(evalf, x, [0, 1, 2], opt=opt, reverse=reverse)                  # navsat.cpp:127-129
    para = np.array([x[0], 0.0, 0.0, x[1], x[2], 0.0])
    return para, po.rpyxyz_to_se3(para), s1, s2


def optimize_bc(po, poses, n_active, has_fix, fix_point, cov, mode, distance, trust_distance_yaw, trust_distance_pitch, z_lower, z_upper, huber_a=0.1,
                opt=None, reverse=False, scale=1.0):
    """Navsat::OptimizeBC.  poses [n_active + n_update][7], frame first.  Returns a dict: skipped, para, transform, poses (a copy), roll, main."""
    poses = np.array(poses, dtype=np.float64).reshape(-1, 7)
    n = int(n_active)
    out = dict(skipped=False, para=np.zeros(6), transform=np.array([0, 0, 0, 1.0, 0, 0, 0]), poses=poses, roll=None, main=None)
    if n == 0 or ((mode & 7) != 7 and distance < trust_distance_yaw):                # navsat.cpp:195-197
        out["skipped"] = True
        return out
    has = np.asarray(has_fix).astype(bool)[:n]
    fix, cov = np.asarray(fix_point, float).reshape(-1, 3)[:n] * scale, np.asarray(cov, float).reshape(-1, 3)[:n]
    frame = poses[0].copy()
    inv = sophus_inverse(frame)
    const = [bool(mode & (1 << i)) for i in range(6)]
    para = np.zeros(6)
    if not const[2]:                                                                 # navsat.cpp:216-234
        if distance > trust_distance_yaw:
            rel = po.forward_update(inv, poses[:n])[0]
            ys = quat_transform_vector(rel[:, :4], np.array([0.0, 1.0, 0.0]))
            y = _ordered_sum(ys, reverse)
            xr, out["roll"] = lm_dense(lambda x, jac: navsat_r(y, frame, x[0], jac), np.zeros(1), [0], opt=opt)
            para[2] = xr[0]
        const[2] = True
    if not const[1] and distance < trust_distance_pitch:                             # navsat.cpp:236-240
        const[1] = True
    lo, hi = [None] * 6, [None] * 6
    if not const[5]:                                                                 # navsat.cpp:242-247
        lo[5], hi[5] = z_lower, z_upper
    p1 = sophus_transform_point(inv, poses[:n, 4:7])[has]                            # frame^-1 * t_i (navsat.cpp:256)
    f, c = fix[has], cov[has]
    free = [i for i in (5, 4, 3, 2, 1, 0) if not const[i]]                           # the order of AddParameterBlock (navsat.cpp:204-209)
    para, out["main"] = lm_dense(lambda x, jac: navsat_rx(f, p1, frame, c, x, jac), para, free, lo, hi, huber_a, opt, reverse)
    fresh = sophus_mul(po, frame, po.rpyxyz_to_se3(para))                            # navsat.cpp:265
    T = sophus_mul(po, fresh, inv)                                                   # new * old^-1
    poses[0] = fresh
    if poses.shape[0] > 1:
        poses[1:] = po.forward_update(T, poses[1:])[0]
    out["para"], out["transform"] = para, T
    return out


def fix_chain(po, poses, has_fix, fix_point, cov, huber_a=0.1, opt=None, scale=1.0):
    """The per-keyframe loop: poses [n][7] = the keyframes strictly after B, C last.  Returns a dict: poses (a copy), x [n-1], iterations [n-1],
    huber_active (steps whose solve saw Huber's linear zone), summaries (per step, None where the keyframe has no fix)."""
    poses = np.array(poses, dtype=np.float64).reshape(-1, 7)
    n = poses.shape[0]
    steps = max(n - 1, 0)
    has = np.asarray(has_fix).astype(bool)
    fix, cov = np.asarray(fix_point, float).reshape(-1, 3) * scale, np.asarray(cov, float).reshape(-1, 3)
    x, its, summaries, huber_active = np.zeros(steps), np.zeros(steps, np.int32), [None] * steps, 0
    for k in range(steps):
        frame = poses[k].copy()
        inv = sophus_inverse(frame)
        para = np.zeros(6)
        if has[k]:
            p1 = sophus_transform_point(inv, frame[4:7])
            para, s = lm_dense(lambda xx, jac: navsat_rx(fix[k], p1, frame, cov[k], xx, jac), para, [3], None, None, huber_a, opt)
            x[k], its[k], summaries[k] = para[3], s["num_iterations"], s
            huber_active += s["huber_active"] > 0
        fresh = sophus_mul(po, frame, po.rpyxyz_to_se3(para))
        T = sophus_mul(po, fresh, inv)
        poses[k] = fresh
        poses[k + 1:] = po.forward_update(T, poses[k + 1:])[0]
    return dict(poses=poses, x=x, iterations=its, summaries=summaries, huber_active=int(huber_active))


# ---- independent statement: mpmath, 50 digits, rotation matrices instead of the quaternion polynomials -----------------------------------
def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def _mp_rot_unit_quat(mp, q):
    x, y, z, w = [mp.mpf(float(v)) for v in q]
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _mp_rot_zyx(mp, yaw, pitch, roll):
    cz, sz, cy, sy, cx, sx = mp.cos(yaw), mp.sin(yaw), mp.cos(pitch), mp.sin(pitch), mp.cos(roll), mp.sin(roll)
    Rz = mp.matrix([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = mp.matrix([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = mp.matrix([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz * Ry * Rx


def _mp_vec(mp, v):
    return mp.matrix([mp.mpf(float(t)) for t in v])


def mp_navsat_rx(p0, p1, pose, cov, x6):
    """One NavsatRXError block: r = sqrt(1 / cov) .* (p0 - (R(pose) (R_zyx(rpy) p1 + t_rel) + t_pose)); x6 may hold mpf."""
    mp = _mp()
    x6 = [mp.mpf(v) for v in x6]
    inner = _mp_rot_zyx(mp, x6[0], x6[1], x6[2]) * _mp_vec(mp, p1) + mp.matrix(x6[3:6])
    tp = _mp_rot_unit_quat(mp, pose[:4]) * inner + _mp_vec(mp, pose[4:7])
    return [mp.sqrt(1 / mp.mpf(float(cov[k]))) * (mp.mpf(float(p0[k])) - tp[k]) for k in range(3)]


def mp_navsat_init(p0, p1, cov, x3):
    mp = _mp()
    return mp_navsat_rx(p0, p1, [0, 0, 0, 1, 0, 0, 0], cov, [x3[0], mp.mpf(0), mp.mpf(0), x3[1], x3[2], mp.mpf(0)])


def mp_navsat_r(y3, pose, roll):
    mp = _mp()
    v = _mp_rot_unit_quat(mp, pose[:4]) * (_mp_rot_zyx(mp, mp.mpf(0), mp.mpf(0), mp.mpf(roll)) * _mp_vec(mp, y3))
    return [v[2]]


def mp_fd(fn, x, h=1e-20):
    """(r [m], J [m][len(x)]) as floats: central differences of the 50-digit residual (truncation ~h^2)."""
    mp = _mp()
    x = [mp.mpf(float(v)) for v in x]
    r0 = fn(x)
    J = np.zeros((len(r0), len(x)))
    hh = mp.mpf(h)
    for c in range(len(x)):
        xp, xm = list(x), list(x)
        xp[c] += hh; xm[c] -= hh
        rp, rm = fn(xp), fn(xm)
        for k in range(len(r0)):
            J[k, c] = float((rp[k] - rm[k]) / (2 * hh))
    return np.array([float(v) for v in r0]), J


# ---- synthetic sections for the tests ---------------------------------------------------------------------------------------------------
def quat_zyx(yaw, pitch, roll):
    """[n][4] (x,y,z,w) of R_z(yaw) R_y(pitch) R_x(roll), float arrays."""
    z, y, x = np.asarray(yaw, float) / 2, np.asarray(pitch, float) / 2, np.asarray(roll, float) / 2
    cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
    return np.stack([cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx, sz * cy * cx - cz * sy * sx, cz * cy * cx + sz * sy * sx], axis=-1)


def drive(n, seed, step=1.0):
    """n keyframes of a vehicle driving a gently winding, slightly hilly road: poses [n][7] (body x forward)."""
    if n == 0:
        return np.zeros((0, 7))
    rng = np.random.default_rng(seed)
    yaw = 0.3 + np.cumsum(rng.normal(0.0, 0.03, n))
    pitch = 0.05 * np.sin(np.arange(n) * 0.11 + rng.uniform(0, 6))
    roll = rng.normal(0.0, 0.01, n)
    q = quat_zyx(yaw, pitch, roll)
    fwd = quat_transform_vector(q, np.array([1.0, 0.0, 0.0]))
    t = np.concatenate([np.zeros((1, 3)), np.cumsum(step * fwd[:-1], axis=0)]) + np.array([10.0, -4.0, 1.5])
    return np.concatenate([q, t], axis=1)


def planted_section(po, n, seed, planted, noise=0.0, missing=0.0, n_update=0, step=1.0):
    """A section whose fixes are the true positions (+ noise) and whose poses are the true ones moved rigidly so that
    poses[0] * rpyxyz2se3(planted) is the true first pose.  Returns poses [n + n_update][7], has_fix [n], fix [n][3], cov [n][3]."""
    rng = np.random.default_rng(seed + 1000)
    true = drive(n + n_update, seed, step)
    planted = np.asarray(planted, float)
    est0 = sophus_mul(po, true[0], sophus_inverse(po.rpyxyz_to_se3(planted)))
    poses = po.forward_update(sophus_mul(po, est0, sophus_inverse(true[0])), true)[0]
    fix = true[:n, 4:7] + rng.normal(0.0, noise, (n, 3)) if noise > 0 else true[:n, 4:7].copy()
    has = (rng.uniform(size=n) >= missing).astype(np.int32)
    cov = np.tile(rng.uniform(0.02, 0.2, 3), (n, 1))
    return poses, has, fix, cov


def chain_section(n, seed, noise=0.15, outlier_every=7, outlier=1.5, missing=0.2, same_cov=False):
    """The keyframes after B (C last) with fixes for the first n - 1: noise on all three axes, every outlier_every-th fix far enough off for
    Huber's linear zone.  Returns poses [n][7], has_fix [n-1], fix [n-1][3], cov [n-1][3]."""
    rng = np.random.default_rng(seed + 2000)
    poses = drive(n, seed)
    m = max(n - 1, 0)
    fix = poses[:m, 4:7] + rng.normal(0.0, noise, (m, 3))
    fix[::outlier_every] += rng.normal(0.0, outlier, fix[::outlier_every].shape)
    has = (rng.uniform(size=m) >= missing).astype(np.int32)
    cov = np.full((m, 3), 0.04) if same_cov else rng.uniform(0.02, 0.2, (m, 3))
    return poses, has, fix, cov
