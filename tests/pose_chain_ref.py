"""CPU statement of the pose-chain solve — TEST INFRASTRUCTURE ONLY, numpy fp64 (lvio_fusion_amd/csrc/pose_chain_kernels.hip follows it).

  problem     n poses [qx,qy,qz,qw,tx,ty,tz], both ends constant, m = n - 2 free under EigenQuaternionParameterization (+) Identity(3);
              edge k = PoseGraphError <6,7,7>(target[k], weight[k], v[k]) between pose k and k + 1, no loss; one unary block per free pose:
              none, T = TError <3,7> under HuberLoss(huber_a), R = RError <4,7> without a loss
  functors    residuals and Jacobians are the oracle's (oracle.pose_graph, oracle.t_error, oracle.r_error, oracle.pose_jac_to_local;
              the `po` argument is the `oracle` fixture); the loss is navsat_ref.huber
  system      D [m][6][6], O [m-1][6][6] (O[i] = block-row i + 1, block-column i), g [6 m]: D_f = unary + edge(p-1).bb + edge(p).aa, p = f + 1
  linear      block-Thomas sweep in natural order (a Cholesky factor per pivot block); refine() corrects a solution with residuals in np.longdouble
  loop        the order of navsat_ref.lm_dense (oracle/lm.h lm_solve) plus the quaternion plus; parameter and step norms over the ambient
              coordinates of the free poses; the cost is 1/2 sum rho, edges first, then unaries
  margins     solve() records, per iteration, the relative margin |a - b| / max(|a|, |b|) of every comparison it decided by

navsat_ab() builds Navsat::OptimizeAB's problem (navsat.cpp:271-307)."""
import numpy as np

from tests.navsat_ref import DEFAULT_OPT, drive, huber

NONE, T, R = 0, 1, 2
LD = np.longdouble


def problem(po, poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight, huber_a=0.0):
    P = np.array(poses, dtype=np.float64).reshape(-1, 7)
    n = P.shape[0]
    if edge_target is None:                                # PoseGraphError(last_pose, pose): from the poses as they come
        edge_target = np.array([po.pose_graph_target(P[k], P[k + 1]) for k in range(n - 1)]).reshape(-1, 6)
    return dict(n=n, m=n - 2, poses=P, tg=np.asarray(edge_target, float).reshape(-1, 6), ew=np.asarray(edge_weight, float).ravel(),
                ev=np.asarray(edge_v, float).ravel(), kind=np.asarray(unary_kind, np.int32).ravel(), ut=np.asarray(unary_target, float).reshape(-1, 4),
                uw=np.asarray(unary_weight, float).ravel(), huber_a=float(huber_a))


def navsat_ab(po, poses, stamps, fix_point, relative_B, huber_a=0.1):
    """Navsat::OptimizeAB: poses = A, AB .., B; z of every fix interpolated between A and B by time; edges (1, 20) from the start poses, the
    last one PoseGraphError(relative_B, 10, 20); TError weight 1."""
    P = np.array(poses, dtype=np.float64).reshape(-1, 7)
    n = P.shape[0]
    t, fix = np.asarray(stamps, float).ravel(), np.asarray(fix_point, float).reshape(-1, 3)
    tg = np.array([po.pose_graph_target(P[k], P[k + 1]) for k in range(n - 1)]).reshape(-1, 6)
    tg[n - 2] = po.se3_to_rpyxyz(np.asarray(relative_B, float))
    ew, ev = np.ones(n - 1), np.full(n - 1, 20.0)
    ew[n - 2] = 10.0
    kind, ut = np.zeros(n, np.int32), np.zeros((n, 4))
    for i in range(1, n - 1):
        a = (t[i] - t[0]) / (t[n - 1] - t[0])
        kind[i] = T
        ut[i, :3] = fix[i]
        ut[i, 2] = a * P[n - 1, 6] + (1.0 - a) * P[0, 6]
    return problem(po, P, tg, ew, ev, kind, ut, np.ones(n), huber_a)


def from_priors(po, poses, pr):
    """The chain of tests/test_gpu_posegraph.py::chain (a pose-prior batch: PoseGraphError edges k -> k + 1 and RError blocks on the free
    poses) as a chain problem."""
    P = np.asarray(poses, float).reshape(-1, 7)
    n = P.shape[0]
    e = np.nonzero(pr["kf_a"] >= 0)[0]
    assert np.array_equal(pr["kf_a"][e], np.arange(n - 1)) and np.array_equal(pr["kf_b"][e], np.arange(1, n))
    kind, ut, uw = np.zeros(n, np.int32), np.zeros((n, 4)), np.zeros(n)
    for i in np.nonzero(pr["kf_a"] == -2)[0]:
        k = pr["kf_b"][i]
        kind[k], ut[k], uw[k] = R, pr["target"][i][:4], pr["weight"][i]
    return problem(po, P, pr["target"][e][:, :6], pr["weight"][e], pr["v"][e], kind, ut, uw, 0.0)


def pose_plus(x, d):
    """EigenQuaternionParameterization::Plus (q_delta * q) (+) Identity(3)"""
    nd = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    o = np.array(x, dtype=np.float64)
    if nd != 0.0:
        k = np.sin(nd) / nd
        ax, ay, az, aw = k * d[0], k * d[1], k * d[2], np.cos(nd)
        bx, by, bz, bw = x[0], x[1], x[2], x[3]
        o[0] = aw * bx + ax * bw + ay * bz - az * by
        o[1] = aw * by + ay * bw + az * bx - ax * bz
        o[2] = aw * bz + az * bw + ax * by - ay * bx
        o[3] = aw * bw - ax * bx - ay * by - az * bz
    o[4:7] = x[4:7] + d[3:6]
    return o


def plus(pb, X, dx):
    Xc = X.copy()
    for f in range(pb["m"]):
        Xc[f + 1] = pose_plus(X[f + 1], dx[6 * f:6 * f + 6])
    return Xc


def _unary(po, pb, X, p, jac):
    """(1/2 rho, H [6][6], g [6], in Huber's linear zone) of the unary block of pose p"""
    kind, w = pb["kind"][p], pb["uw"][p]
    H, g = np.zeros((6, 6)), np.zeros(6)
    if kind == T:
        r, J7 = po.t_error(pb["ut"][p, :3], w, X[p])
        rho0, rho1 = huber(pb["huber_a"], np.array([float(r @ r)]))
        if jac:
            sc = np.sqrt(rho1[0])                           # Corrector, rho'' <= 0
            L = sc * po.pose_jac_to_local(X[p], J7)
            H, g = L.T @ L, L.T @ (sc * r)
        return 0.5 * float(rho0[0]), H, g, bool(rho1[0] < 1.0)
    if kind == R:
        r, J7 = po.r_error(np.concatenate([pb["ut"][p], np.zeros(3)]), w, X[p])
        if jac:
            L = po.pose_jac_to_local(X[p], J7)
            H, g = L.T @ L, L.T @ r
        return 0.5 * float(r @ r), H, g, False
    return 0.0, H, g, False


def linearize(po, pb, X, jac=True):
    """dict(cost, D, O, g, huber_active) at the poses X (D, O, g only with jac)"""
    n, m = pb["n"], pb["m"]
    cost = 0.0
    aa, bb, ba, ga, gb = [], [], [], [], []
    for k in range(n - 1):
        r, J1, J2 = po.pose_graph(pb["tg"][k], pb["ew"][k], pb["ev"][k], X[k], X[k + 1])
        cost = cost + 0.5 * float(r @ r)
        if jac:
            La, Lb = po.pose_jac_to_local(X[k], J1), po.pose_jac_to_local(X[k + 1], J2)
            aa.append(La.T @ La); bb.append(Lb.T @ Lb); ba.append(Lb.T @ La); ga.append(La.T @ r); gb.append(Lb.T @ r)
    D, O, g = np.zeros((m, 6, 6)), np.zeros((max(m - 1, 0), 6, 6)), np.zeros(6 * m)
    active = False
    for f in range(m):
        p = f + 1
        c, H, gu, act = _unary(po, pb, X, p, jac)
        cost = cost + c
        active = active or act
        if jac:
            D[f] = (H + bb[p - 1]) + aa[p]
            g[6 * f:6 * f + 6] = (gu + gb[p - 1]) + ga[p]
            if f + 1 < m:
                O[f] = ba[p]
    return dict(cost=cost, D=D, O=O, g=g, huber_active=active)


def dense(D, O):
    m = D.shape[0]
    A = np.zeros((6 * m, 6 * m), dtype=D.dtype)
    for f in range(m):
        A[6 * f:6 * f + 6, 6 * f:6 * f + 6] = D[f]
        if f + 1 < m:
            A[6 * f + 6:6 * f + 12, 6 * f:6 * f + 6] = O[f]
            A[6 * f:6 * f + 6, 6 * f + 6:6 * f + 12] = O[f].T
    return A


def damp(D, h0, radius):
    """D + the damping term of oracle/robust.h lm_damping: clamped on the Jacobi-scaled diagonal, divided by the radius"""
    Dd = D.copy()
    for f in range(D.shape[0]):
        for c in range(6):
            s2 = (1.0 / (1.0 + np.sqrt(h0[6 * f + c]))) ** 2
            Dd[f, c, c] += min(max(D[f, c, c] * s2, 1e-6), 1e32) / s2 / radius
    return Dd


def _chol6(S):
    L = np.zeros((6, 6))
    for j in range(6):
        v = S[j, j] - float(L[j, :j] @ L[j, :j])
        if not v > 0.0:
            return False, L
        L[j, j] = np.sqrt(v)
        for i in range(j + 1, 6):
            L[i, j] = (S[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    return True, L


def _fwd(L, B):
    Y = np.array(B, dtype=np.float64)
    for i in range(6):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _bwd(L, Y):
    Xs = np.array(Y, dtype=np.float64)
    for i in range(5, -1, -1):
        Xs[i] = (Xs[i] - L[i + 1:, i] @ Xs[i + 1:]) / L[i, i]
    return Xs


def thomas(Dd, O, rhs, reverse=False):
    """Block-Thomas sweep of the block-tridiagonal system (Dd, O) x = rhs in natural order (`reverse`: from the other end).  Returns (ok, x):
    ok False when a pivot block is not positive definite (x = 0)."""
    m = Dd.shape[0]
    if reverse:
        ok, x = thomas(Dd[::-1], np.array([O[m - 2 - i].T for i in range(m - 1)]).reshape(-1, 6, 6), rhs.reshape(m, 6)[::-1].ravel())
        return ok, x.reshape(m, 6)[::-1].ravel()
    Ls, Us, ys = [], [], []
    S, r = Dd[0].copy(), rhs[0:6].copy()
    for i in range(m):
        ok, L = _chol6(S)
        if not ok:
            return False, np.zeros(6 * m)
        y = _fwd(L, r)
        Ls.append(L); ys.append(y)
        if i + 1 < m:
            U = _fwd(L, O[i].T)                            # L^-1 A[i][i+1]
            Us.append(U)
            S = Dd[i + 1] - U.T @ U
            r = rhs[6 * i + 6:6 * i + 12] - U.T @ y
    x = np.zeros(6 * m)
    for i in range(m - 1, -1, -1):
        t = ys[i] if i + 1 == m else ys[i] - Us[i] @ x[6 * i + 6:6 * i + 12]
        x[6 * i:6 * i + 6] = _bwd(Ls[i], t)
    return True, x


def matvec(D, O, x):
    """(D, O) x in the dtype of the arguments"""
    m = D.shape[0]
    X = x.reshape(m, 6, 1)
    y = D @ X
    if m > 1:
        y[1:] += O @ X[:-1]
        y[:-1] += np.transpose(O, (0, 2, 1)) @ X[1:]
    return y.reshape(6 * m)


def refine(Dd, O, rhs, x64, rounds=5):
    """x64 corrected `rounds` times: residual in np.longdouble, correction through the float64 sweep; returned as longdouble"""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here: the reference would not be one"
    Dl, Ol, bl = Dd.astype(LD), O.astype(LD), rhs.astype(LD)
    x = np.asarray(x64, np.float64).astype(LD)
    for _ in range(rounds):
        r = bl - matvec(Dl, Ol, x)
        ok, c = thomas(Dd, O, r.astype(np.float64))
        assert ok
        x = x + c.astype(LD)
    return x


def err(Dd, x, x_star):
    """||Ds (x - x_star)|| / ||Ds x_star||, Ds = sqrt(diag), in longdouble (as tests/reduced_cases.err)"""
    ds = np.sqrt(np.abs(np.einsum("fii->fi", Dd)).ravel().astype(LD))
    xs = np.asarray(x_star, LD)
    num, den = ds * (np.asarray(x, np.float64).astype(LD) - xs), ds * xs
    return float(np.sqrt(num @ num) / np.sqrt(den @ den))


def model_decrease(lin, dx):
    return -float(dx @ (lin["g"] + 0.5 * matvec(lin["D"], lin["O"], dx)))


def damped_step(lin, h0, radius):
    """(ok, dx, model) of one damped solve on a linearisation"""
    ok, dx = thomas(damp(lin["D"], h0, radius), lin["O"], -lin["g"])
    return ok, dx, model_decrease(lin, dx)


def lm_iteration(po, pb, X, radius, decrease, min_relative_decrease=1e-3):
    """One iteration at the radius handed in, Jacobi scaling from this linearisation, no termination tests (oracle/lm.h lm_iteration).
    Returns (X after, dict(accepted, valid, cost_before, cost_after, rho, radius, decrease_factor))."""
    lin = linearize(po, pb, X)
    ok, dx, model = damped_step(lin, np.einsum("fii->fi", lin["D"]).ravel().copy(), radius)
    out = dict(accepted=False, valid=bool(ok and model > 0.0), cost_before=lin["cost"], cost_after=lin["cost"], rho=0.0, radius=radius, decrease_factor=decrease)
    if not out["valid"]:
        out["radius"] = radius * 0.5
        return X, out
    Xc = plus(pb, X, dx)
    cand = linearize(po, pb, Xc, jac=False)["cost"]
    rho = (lin["cost"] - cand) / model
    out.update(cost_after=cand, rho=rho)
    if rho > min_relative_decrease:
        t = 2.0 * rho - 1.0
        out.update(accepted=True, radius=min(radius / max(1.0 / 3.0, 1.0 - t * t * t), 1e16), decrease_factor=2.0)
        return Xc, out
    out.update(radius=radius / decrease, decrease_factor=decrease * 2.0)
    return X, out


def _margin(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def solve(po, pb, opt=None):
    """The declared loop.  Returns (poses, summary): summary as navsat_ref.lm_dense's plus `rejected` (valid steps not taken) and `margins`, a
    list per pass of (name, relative margin) for every comparison that pass decided by.  A FAILURE returns the poses as they came."""
    o = dict(DEFAULT_OPT); o.update(opt or {})
    X0 = pb["poses"]
    X = X0.copy()
    n, m = pb["n"], pb["m"]
    summ = dict(initial_cost=0.0, final_cost=0.0, num_iterations=0, num_successful_steps=0, termination=0, why="none", huber_active=0, rejected=0, margins=[])
    if m == 0:                                             # no free pose: a cost and no unknown
        summ["initial_cost"] = summ["final_cost"] = linearize(po, pb, X, jac=False)["cost"]
        return X, summ
    free = slice(1, n - 1)
    radius, decrease = o["initial_trust_region_radius"], 2.0
    iters = successes = invalid_run = 0
    termination, why = 1, "max_num_iterations"
    h0 = None
    cost = initial_cost = 0.0
    while True:
        lin = linearize(po, pb, X)
        cost = lin["cost"]
        summ["huber_active"] += bool(lin["huber_active"])
        mg = []
        summ["margins"].append(mg)
        if h0 is None:
            initial_cost, h0 = cost, np.einsum("fii->fi", lin["D"]).ravel().copy()
        if iters >= o["max_num_iterations"]:
            termination, why = 1, "max_num_iterations"; break
        gn = float(np.max(np.abs(lin["g"])))
        mg.append(("gradient", _margin(gn, o["gradient_tolerance"])))
        if gn <= o["gradient_tolerance"]:
            termination, why = 0, "gradient_tolerance"; break
        mg.append(("radius", _margin(radius, 1e-32)))
        if radius < 1e-32:
            termination, why = 0, "min_trust_region_radius"; break
        ok, dx, model = damped_step(lin, h0, radius)
        if ok and np.isfinite(model):
            mg.append(("model", _margin(-float(dx @ lin["g"]), 0.5 * float(dx @ matvec(lin["D"], lin["O"], dx)))))
        if not (ok and model > 0.0):                       # invalid step
            iters += 1
            invalid_run += 1
            if invalid_run >= 5:
                termination, why = 2, "consecutive_invalid_steps"; break
            radius *= 0.5
            continue
        invalid_run = 0
        Xc = plus(pb, X, dx)
        sn, xn = np.sqrt(float(np.sum((Xc[free] - X[free]) ** 2))), np.sqrt(float(np.sum(X[free] ** 2)))
        mg.append(("parameter", _margin(sn, o["parameter_tolerance"] * (xn + o["parameter_tolerance"]))))
        if sn <= o["parameter_tolerance"] * (xn + o["parameter_tolerance"]):
            termination, why = 0, "parameter_tolerance"; break
        cand = linearize(po, pb, Xc, jac=False)["cost"]
        mg.append(("function", _margin(abs(cost - cand), o["function_tolerance"] * cost)))
        if abs(cost - cand) <= o["function_tolerance"] * cost:
            termination, why = 0, "function_tolerance"; break
        iters += 1
        rho = (cost - cand) / model
        mg.append(("rho", _margin(cost - cand, o["min_relative_decrease"] * model)))
        if rho > o["min_relative_decrease"]:
            X, cost = Xc, cand
            successes += 1
            t = 2.0 * rho - 1.0
            radius, decrease = min(radius / max(1.0 / 3.0, 1.0 - t * t * t), 1e16), 2.0
        else:
            summ["rejected"] += 1
            radius /= decrease; decrease *= 2.0
    if termination == 2 or not np.isfinite(cost):
        termination, cost, X = 2, initial_cost, X0.copy()
    summ.update(initial_cost=initial_cost, final_cost=cost, num_iterations=iters, num_successful_steps=successes, termination=termination, why=why)
    return X, summ


def min_margin(summ):
    return min((v for mg in summ["margins"] for _, v in mg), default=np.inf)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def _small_rot(po, pose, ypr):
    """pose * rpyxyz2se3([yaw, pitch, roll, 0, 0, 0])"""
    return po.se3_mul(pose, po.rpyxyz_to_se3(np.concatenate([ypr, np.zeros(3)])))


def ab_section(po, m, seed, drift=0.3, rot=0.01, noise=0.03, outlier_every=5, outlier=0.6, raw_z=0.0):
    """A section A .. B of m + 2 keyframes along navsat_ref.drive: the ends are the true poses, the interior has drifted (a smooth
    translation offset of size `drift` plus per-pose rotation noise `rot`), the fixes are the true positions plus `noise`, every
    outlier_every-th one moved by `outlier` (0: none); raw_z is added to z of every fix (OptimizeAB replaces z).  relative_B is the true
    relative pose of the last two keyframes, slightly off.  Returns poses [n][7], stamps [n], fix [n][3], relative_B [7]."""
    rng = np.random.default_rng(seed + 3000)
    n = m + 2
    true = drive(n, seed)
    poses = true.copy()
    s = np.linspace(0.0, np.pi, n)
    off = drift * np.sin(s)[:, None] * rng.normal(0.0, 1.0, 3)[None, :]
    for i in range(1, n - 1):
        poses[i] = _small_rot(po, true[i], rng.normal(0.0, rot, 3))
        poses[i, 4:7] += off[i] + rng.normal(0.0, 0.1 * drift, 3)
    stamps = 100.0 + np.arange(n) + rng.uniform(-0.2, 0.2, n)
    fix = true[:, 4:7] + rng.normal(0.0, noise, (n, 3))
    if outlier_every:
        fix[1::outlier_every] += rng.normal(0.0, outlier, fix[1::outlier_every].shape)
    fix[:, 2] += raw_z
    relB = po.se3_mul(po.se3_mul(po.se3_inv(true[n - 2]), true[n - 1]), po.rpyxyz_to_se3(rng.normal(0.0, 0.002, 6)))
    return poses, stamps, fix, relB


def step_case(po, m, seed):
    """A chain problem for the step-accuracy test: T unaries with weights 1 .. 400 and Huber zones mixed (drift and outliers beside small
    residuals), edge weights 1 .. 10, v 20."""
    rng = np.random.default_rng(seed + 4000)
    poses, stamps, fix, relB = ab_section(po, m, seed, drift=0.2, rot=0.01, noise=0.02, outlier_every=3, outlier=0.5)
    n = m + 2
    kind = np.zeros(n, np.int32); kind[1:n - 1] = T
    ut = np.zeros((n, 4)); ut[:, :3] = fix
    ut[1::2, :3] = poses[1::2, 4:7] + rng.normal(0.0, 1e-5, ut[1::2, :3].shape)      # every other pose sits on its fix: Huber's quadratic zone
    uw =np.exp(rng.uniform(0.0, np.log(400.0), n))
    ew = np.exp(rng.uniform(0.0, np.log(10.0), n - 1))
    true = drive(n, seed)
    tg = np.array([po.pose_graph_target(true[k], true[k + 1]) for k in range(n - 1)]).reshape(-1, 6)
    return problem(po, poses, tg, ew, np.full(n - 1, 20.0), kind, ut, uw, 0.1)


# the sections of the solve tests: (free poses, seed, ab_section keywords, exercises the loss).  QUIET keeps every TError inside Huber's
# quadratic zone (short: the interpolated z leaves the road after a few keyframes); SHARP starts far enough off for rejected steps.
QUIET = dict(drift=0.02, rot=0.002, noise=0.005, outlier_every=0)
SHARP = dict(drift=3.0, rot=0.8)
SOLVE_SCENES = [(1, 2, {}, True), (2, 1, QUIET, False), (7, 8, SHARP, True), (64, 1, {}, True), (200, 2, {}, True)]
