"""Declared semantics of the dense keyframe prior (lvf_dense_prior_*, lvf_problem_set_dense_prior) and of the marginalisation that
produces one (lvf_problem_marginal_prior), in numpy.

A prior sits on n_sel distinct keyframes (1 .. 8), m = 15 n_sel unknowns, per keyframe [rotation 3, translation 3, v 3, ba 3, bg 3]:

    cost(x) = c0 + eta^T e + 1/2 e^T info e,        e = x [-] x0

e is the local coordinate of x at x0 in the solver's parameterisation (EigenQuaternionParameterization (+) Identity: Plus(q, delta) =
(sin|delta| delta/|delta|, cos|delta|) (x) q, Eigen order x, y, z, w): with u = q/|q|, u0 = q0/|q0| and d = u (x) u0^-1 (negated if
d.w < 0), delta = atan2(|d.v|, d.w) d.v/|d.v| — so that Plus(q0, delta) = q — and plain differences elsewhere.  No loss function, no
first-estimate Jacobians: e is re-evaluated at every state.

Derivatives are taken in the tangent space at x: T = d e(Plus(x, eps)) / d eps at eps = 0 (the ambient derivative of the code above times
the plus-Jacobian, which is what quat_row_to_local applies).  T is block diagonal, identity except the 3 x 3 rotation block of every
keyframe, which has the closed form

    T_rot = I - [delta]x + (1 - theta cot theta) / theta^2 [delta]x^2,        theta = |delta| <= pi/2

(the inverse left Jacobian of the rotation by 2 theta about delta; I at delta = 0).  Gradient T^T (info e + eta), Gauss-Newton matrix
T^T info T; the columns of a constant block (pose_const bit 0: the 6 pose columns, bits 1 .. 3: v, ba, bg) are zero.
"""
import numpy as np

LD = np.longdouble


def qmul(a, b):
    """Hamilton product, Eigen order (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.result_type(a, b))


def qconj(a):
    return np.array([-a[0], -a[1], -a[2], a[3]], dtype=a.dtype)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=v.dtype)


def quat_plus(q, delta):
    """EigenQuaternionParameterization::Plus (pose_plus of lvf_math.hpp)."""
    q = np.asarray(q)
    delta = np.asarray(delta)
    dt = np.result_type(q, delta)
    nd = np.sqrt((delta * delta).sum())
    if nd == 0:
        return q.astype(dt)
    k = np.sin(nd) / nd
    return qmul(np.array([k * delta[0], k * delta[1], k * delta[2], np.cos(nd)], dtype=dt), q.astype(dt))


def rot_local(q, q0):
    """delta with Plus(q0, delta) = q up to the quaternion's sign and norm."""
    q = np.asarray(q)
    q0 = np.asarray(q0)
    u = q / np.sqrt((q * q).sum())
    u0 = q0 / np.sqrt((q0 * q0).sum())
    d = qmul(u, qconj(u0))
    if d[3] < 0:
        d = -d
    nv = np.sqrt((d[:3] * d[:3]).sum())
    if nv == 0:
        return np.zeros(3, dtype=d.dtype)
    return np.arctan2(nv, d[3]) * d[:3] / nv


def state_plus(x, eps):
    """x [n_sel][16] (pose 7, v 3, ba 3, bg 3) moved by eps [15 n_sel]."""
    x = np.asarray(x)
    eps = np.asarray(eps)
    out = np.array(x, dtype=np.result_type(x, eps))
    for k in range(x.shape[0]):
        e = eps[15 * k:15 * k + 15]
        out[k, :4] = quat_plus(x[k, :4], e[:3])
        out[k, 4:7] = x[k, 4:7] + e[3:6]
        out[k, 7:16] = x[k, 7:16] + e[6:15]
    return out


def local(x, x0):
    """e = x [-] x0, [15 n_sel]."""
    x = np.asarray(x)
    x0 = np.asarray(x0)
    e = np.zeros(15 * x.shape[0], dtype=np.result_type(x, x0))
    for k in range(x.shape[0]):
        e[15 * k:15 * k + 3] = rot_local(x[k, :4], x0[k, :4])
        e[15 * k + 3:15 * k + 6] = x[k, 4:7] - x0[k, 4:7]
        e[15 * k + 6:15 * k + 15] = x[k, 7:16] - x0[k, 7:16]
    return e


def rot_tangent(delta):
    delta = np.asarray(delta)
    th2 = (delta * delta).sum()
    K = skew(delta)
    if th2 < 1e-8:
        c = 1.0 / 3.0 + th2 / 45.0
    else:
        th = np.sqrt(th2)
        c = (1.0 - th * np.cos(th) / np.sin(th)) / th2
    return np.eye(3, dtype=delta.dtype) - K + c * (K @ K)


def tangent_jacobian(x, x0):
    e = local(x, x0)
    m = e.size
    T = np.eye(m, dtype=e.dtype)
    for k in range(m // 15):
        T[15 * k:15 * k + 3, 15 * k:15 * k + 3] = rot_tangent(e[15 * k:15 * k + 3])
    return T


def sym_lower(info):
    """The matrix the library reads: the lower triangle of `info`, mirrored."""
    L = np.tril(np.asarray(info))
    return L + np.tril(L, -1).T


def column_mask(const_bits):
    """const_bits [n_sel] (pose_const of the selected keyframes) -> 0 / 1 per column."""
    cm = np.ones(15 * len(const_bits))
    for k, b in enumerate(const_bits):
        if b & 1:
            cm[15 * k:15 * k + 6] = 0
        for j in range(3):
            if b & (2 << j):
                cm[15 * k + 6 + 3 * j:15 * k + 9 + 3 * j] = 0
    return cm


def evaluate(x0, info, eta, c0, x, const_bits=None):
    """cost, gradient [m], Gauss-Newton matrix [m][m] at x [n_sel][16]."""
    info = sym_lower(info)
    m = info.shape[0]
    eta = np.zeros(m, dtype=info.dtype) if eta is None else np.asarray(eta)
    e = local(x, x0)
    T = tangent_jacobian(x, x0)
    if const_bits is not None:
        T = T * column_mask(const_bits)[None, :].astype(T.dtype)
    y = info @ e + eta
    cost = c0 + eta @ e + 0.5 * (e @ (info @ e))
    return cost, T.T @ y, T.T @ info @ T


def natural_index(n_kf, kfs):
    """Row of each of the prior's m unknowns in the reduced system's natural order [pose tangent 6 n_kf | (v, ba, bg) 9 n_kf]."""
    idx = []
    for k in kfs:
        idx += [6 * k + c for c in range(6)] + [6 * n_kf + 9 * k + c for c in range(9)]
    return np.array(idx)


def scatter(n_kf, kfs, g, H):
    """The prior's terms as they enter the problem's gradient [15 n_kf] and Gauss-Newton matrix."""
    idx = natural_index(n_kf, kfs)
    gn = np.zeros(15 * n_kf, dtype=g.dtype)
    Hn = np.zeros((15 * n_kf, 15 * n_kf), dtype=H.dtype)
    gn[idx] = g
    Hn[np.ix_(idx, idx)] = H
    return gn, Hn


def marginal_prior(H, g, c, sel, dtype=LD, rest_order=None):
    """The local model c + g^T eps + 1/2 eps^T H eps minimised over the unknowns outside `sel`: (info, eta, c0) over sel, in `dtype` (long
    double: the reference).  An unknown with H_jj == 0 is absent (left out; zero rows / columns of the outputs).  rest_order permutes the
    elimination of the rest (the float64 error bound is taken over several orders, as marginal_ref.err64_bound does)."""
    H = _sym(np.asarray(H, np.float64)).astype(dtype)
    g = np.asarray(g, np.float64).astype(dtype)
    d = H.shape[0]
    present = np.diag(H) != 0
    sel = np.asarray(sel, np.int64)
    is_sel = np.zeros(d, bool)
    is_sel[sel] = True
    r = np.where(~is_sel & present)[0]
    if rest_order is not None:
        r = r[np.asarray(rest_order)]
    n, m = r.size, sel.size
    order = np.concatenate([r, sel])
    A = np.zeros((n + m + 1, n + m + 1), dtype)
    A[:n + m, :n + m] = H[np.ix_(order, order)]
    A[n + m, :n + m] = g[order]
    A[:n + m, n + m] = g[order]
    A[n + m, n + m] = 2 * dtype(c)
    for j in range(n):                               # right-looking elimination of the rest
        p = A[j, j]
        if not p > 0:
            raise np.linalg.LinAlgError("non-positive pivot %d" % j)
        col = A[j + 1:, j] / np.sqrt(p)
        A[j + 1:, j + 1:] -= np.outer(col, col)
    T = A[n:, n:]
    ps = np.concatenate([present[sel], [True]])
    T = T * ps[:, None] * ps[None, :]
    T = np.tril(T) + np.tril(T, -1).T
    return T[:m, :m], T[m, :m], T[m, m] / 2


def n_rest(H, sel):
    d = np.asarray(H).shape[0]
    is_sel = np.zeros(d, bool)
    is_sel[np.asarray(sel)] = True
    return int((~is_sel & (np.diag(H) != 0)).sum())


def _sym(S):
    return np.tril(S) + np.tril(S, -1).T


def augmented(info, eta, c0):
    """[info eta; eta^T 2 c0]: what the caller of a dense prior vouches is positive semi-definite"""
    m = len(eta)
    A = np.zeros((m + 1, m + 1), dtype=np.result_type(info, eta))
    A[:m, :m] = info
    A[m, :m] = eta
    A[:m, m] = eta
    A[m, m] = 2 * c0
    return A


def aug_scale(A_star):
    """1 / sqrt(diag) of the reference's augmented matrix, 0 where the diagonal is zero (absent unknowns): the scaling of marginal_ref.err"""
    dg = np.diag(np.asarray(A_star, LD)).copy()
    ok = dg > 0
    return np.where(ok, 1 / np.sqrt(np.where(ok, dg, 1)), 0)


def system_scale(H, c, sel):
    """The scaling for a gauge-free case, where diagonal entries of info* are exactly zero along the free directions (the rest follows a
    translation of the selection at no cost) and aug_scale has nothing to divide by: 1 / sqrt of the selection's own diagonal of H, and of 2c"""
    dg = np.concatenate([np.diag(np.asarray(H, np.float64))[np.asarray(sel)], [2.0 * float(c)]]).astype(LD)
    ok = dg > 0
    return np.where(ok, 1 / np.sqrt(np.where(ok, dg, 1)), 0)


def aug_err(A, A_star, D=None):
    """||D (A - A*) D||_F / ||D A* D||_F in long double (marginal_ref.err, on the matrix with the extra row)"""
    D = aug_scale(A_star) if D is None else D
    As = np.asarray(A_star, LD)
    E = D[:, None] * (np.asarray(A, np.float64).astype(LD) - As) * D[None, :]
    N = D[:, None] * As * D[None, :]
    return float(np.sqrt((E * E).sum()) / np.sqrt((N * N).sum()))


N_ORDERS = 8


def err64_bound(H, g, c, sel, A_star, seed, D=None):
    """marginal_ref.err64_bound extended to the extra row: the largest aug_err of the float64 host computation over the natural order of the
    rest and N_ORDERS - 1 seeded permutations of it"""
    rng = np.random.default_rng(1000 + seed)
    n = n_rest(H, sel)
    worst = 0.0
    for k in range(N_ORDERS):
        o = None if k == 0 else rng.permutation(n)
        worst = max(worst, aug_err(augmented(*marginal_prior(H, g, c, sel, np.float64, o)), A_star, D))
    assert np.isfinite(worst)
    return worst


def propagated(H, g, c, sel, A_star, rel_entry, D=None):
    """marginal_ref.propagated for the matrix with the extra row: what an entry-wise disagreement <= rel_entry * max|entry| between two
    assemblies of [H g; g^T 2c] can do to [info eta; eta^T 2 c0], to first order, in aug_err's norm.  d A = Z^T dS Z with
    Z = [-H_rr^-1 [H_rs g_r]; I]; only H_rr is inverted, so a gauge-free system (H singular, H_rr not) has a bound too."""
    H = _sym(np.asarray(H, np.float64)).astype(LD)
    g = np.asarray(g, np.float64).astype(LD)
    d = H.shape[0]
    present = np.diag(H) != 0
    sel = np.asarray(sel, np.int64)
    is_sel = np.zeros(d, bool)
    is_sel[sel] = True
    r = np.where(~is_sel & present)[0]
    n, m = r.size, sel.size
    Z = np.zeros((n + m + 1, m + 1), LD)
    Z[n:, :] = np.eye(m + 1, dtype=LD)
    if n:
        L = cholesky_ld(H[np.ix_(r, r)])
        rhs = np.concatenate([H[np.ix_(r, sel)], g[r][:, None]], axis=1)
        Y = solve_lower_ld(L, rhs)
        Z[:n, :] = -solve_lower_ld_t(L, Y)
    D = aug_scale(A_star) if D is None else D
    ZD = (Z * D[None, :]).astype(np.float64)
    N = (D[:, None] * np.asarray(A_star, LD) * D[None, :]).astype(np.float64)
    big = max(float(np.abs(H).max()), float(np.abs(g).max()), abs(2 * float(c)))
    dS = (d + 1) * rel_entry * big
    return float(np.linalg.norm(ZD, 2) * dS * np.linalg.norm(ZD, "fro") / np.linalg.norm(N, "fro"))


def solve_lower_ld_t(L, B):
    """L^-T B"""
    n = L.shape[0]
    X = np.zeros_like(B, dtype=LD)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def brute_force(H, g, c, sel):
    """The same three quantities by minimising the model over the rest for given selected increments: a least-squares fit of the quadratic
    eps_s -> min_r model through its values (long double), no Schur complement anywhere"""
    H = _sym(np.asarray(H, np.float64)).astype(LD)
    g = np.asarray(g, np.float64).astype(LD)
    d = H.shape[0]
    sel = np.asarray(sel, np.int64)
    is_sel = np.zeros(d, bool)
    is_sel[sel] = True
    r = np.where(~is_sel & (np.diag(H) != 0))[0]
    m = sel.size
    L = cholesky_ld(H[np.ix_(r, r)]) if r.size else None

    def value(es):
        eps = np.zeros(d, LD)
        eps[sel] = es
        if r.size:
            b = -(g[r] + H[np.ix_(r, sel)] @ es)     # gradient of the model in the rest = 0
            eps[r] = solve_lower_ld_t(L, solve_lower_ld(L, b[:, None]))[:, 0]
        return LD(c) + g @ eps + LD(0.5) * (eps @ (H @ eps))

    c0 = value(np.zeros(m, LD))
    E = np.eye(m, dtype=LD)
    vp = np.array([value(E[i]) for i in range(m)])
    vm = np.array([value(-E[i]) for i in range(m)])
    eta = (vp - vm) / 2
    info = np.zeros((m, m), LD)
    for i in range(m):
        info[i, i] = vp[i] + vm[i] - 2 * c0
        for j in range(i):
            info[i, j] = info[j, i] = value(E[i] + E[j]) - vp[i] - vp[j] + c0
    return info, eta, c0


def sqrt_rows(info, eta, c0):
    """The prior as least-squares rows: A, b, const with c0 + eta^T e + 1/2 e^T info e = 1/2 |A e + b|^2 + const (info = A^T A from its
    eigen-decomposition, eta = A^T b; eta must lie in the range of info, which a positive semi-definite [info eta; eta^T 2 c0] implies)"""
    w, V = np.linalg.eigh(sym_lower(info))
    keep = w > 1e-13 * max(w.max(), 1e-300)
    A = np.sqrt(w[keep])[:, None] * V[:, keep].T
    eta = np.zeros(info.shape[0]) if eta is None else np.asarray(eta, np.float64)
    b = (V[:, keep].T @ eta) / np.sqrt(w[keep])
    assert np.abs(A.T @ b - eta).max() <= 1e-9 * max(np.abs(eta).max(), 1e-300) + 1e-300, "eta is not in the range of info"
    return A, b, c0 - 0.5 * float(b @ b)


class in_dense_system:
    """Context manager: while active, tests.lidar_window_ref.dense_system (and so its trial_step / lm_iteration / lm_solve) carries the rows
    of a dense prior on keyframes `kfs` of the window — the prior's terms added to the reference loop, the loop itself untouched."""

    def __init__(self, kfs, x0, info, eta, c0, const_bits=None):
        self.kfs, self.x0, self.const_bits = list(kfs), np.asarray(x0, np.float64), const_bits
        self.A, self.b, self.const = sqrt_rows(info, eta, c0)

    def rows(self, state, ncol, n_kf):
        x = np.array([np.concatenate([state[0][k], state[1][k], state[2][k], state[3][k]]) for k in self.kfs])
        e = local(x, self.x0)
        T = tangent_jacobian(x, self.x0)
        if self.const_bits is not None:
            T = T * column_mask([self.const_bits[k] for k in self.kfs])[None, :]
        J = np.zeros((self.A.shape[0], ncol))
        J[:, natural_index(n_kf, self.kfs)] = self.A @ T
        return J, self.A @ e + self.b

    def __enter__(self):
        from tests import lidar_window_ref as lw
        self.lw, self.orig = lw, lw.dense_system

        def dense_system(oracle, cfg, pre, state, lidar, huber_a=1.0, pose_const=None):
            J, r, cost = self.orig(oracle, cfg, pre, state, lidar, huber_a, pose_const)
            Jp, rp = self.rows(state, J.shape[1], cfg["n_kf"])
            if pose_const is not None:
                for k in np.flatnonzero(np.asarray(pose_const)):
                    Jp[:, 6 * k:6 * k + 6] = 0.0
            return np.concatenate([J, Jp]), np.concatenate([r, rp]), cost + 0.5 * float(rp @ rp) + self.const

        lw.dense_system = dense_system
        return self

    def __exit__(self, *exc):
        self.lw.dense_system = self.orig
        return False


def cholesky_ld(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not s > 0:
            raise np.linalg.LinAlgError("not positive definite at %d" % j)
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, B):
    n = L.shape[0]
    X = np.zeros_like(B, dtype=LD)
    for i in range(n):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X
