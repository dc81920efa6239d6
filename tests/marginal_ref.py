"""Marginal information and covariance of selected unknowns of a reduced system: the declared semantics (lvf_marginal_dense,
lvf_problem_marginal, lvf_window_marginal) and their CPU reference.  Pure numpy.

    info = S_ss - S_sr S_rr^-1 S_rs        cov = info^-1 = (S^-1)_ss          (s = sel, r = the rest)

Unknown order of S: lvf_problem_download_reduced's, [pose tangent 6 x n_kf | (v, ba, bg) 9 x n_kf].  Only the lower triangle of S is read.
  * An unknown is ABSENT iff S_jj == 0 exactly (its Jacobian column is identically zero): it is left out of the system, and its rows and
    columns of both outputs are zero (ceres::Covariance's convention for constant blocks).  A NaN diagonal is present (and then fails).
  * The elimination order is [rest, ascending, absent unknowns keeping their place | padding to a multiple of 64 | sel in the caller's order];
    the rest is eliminated in block steps of 64 columns.  Output row i belongs to sel[i]; both outputs are exactly symmetric.
  * fail = 0, or 1 + kb of the block step that met a non-positive or NaN pivot (kb = position in the rest // 64), or 1 + (number of block
    steps of the rest) for a pivot inside the selection.  A failure leaves no outputs.
  * min_pivot_ratio = min L_jj^2 / S_jj over the present unknowns (L the Cholesky factor in that order): in (0, 1].

`marginal` computes all of it in np.longdouble (Cholesky of the permuted system, inverse of the trailing block's triangle); `marginal64`
is the float64 host computation of the same quantities, and `err64_bound` its error taken as a bound over elimination orders of the rest, as
reduced_cases.err64_bound does for the solve."""
import numpy as np

from tests import reduced_cases as rc

LD = rc.LD
NB = 64
MAX_SEL = 120


def _sym_lower(S, dtype):
    S = np.asarray(S, dtype)
    return np.tril(S) + np.tril(S, -1).T


def layout(S, sel):
    """(rest, present, nr): the rest in elimination order, the presence mask over all unknowns, the block steps of the rest"""
    S = np.asarray(S)
    d = S.shape[0]
    sel = [int(s) for s in sel]
    assert 1 <= len(sel) <= MAX_SEL and len(set(sel)) == len(sel) and all(0 <= s < d for s in sel)
    chosen = np.zeros(d, bool); chosen[sel] = True
    rest = [u for u in range(d) if not chosen[u]]
    present = ~(np.diag(S) == 0.0)
    return rest, present, (len(rest) + NB - 1) // NB


def _permuted(S, order, present, dtype):
    """S through `order` with absent unknowns as identity rows / columns"""
    A = _sym_lower(S, dtype)[np.ix_(order, order)]
    gone = ~present[order]
    A[gone, :] = 0; A[:, gone] = 0
    A[gone, gone] = 1
    return A


def _eliminate(A, n):
    """right-looking Cholesky of the first n columns of A in place (A's dtype); returns (index of the first bad pivot or -1, pivots L_jj^2).
    Afterwards A[n:, n:] is the Schur complement and A[:, :n] holds L."""
    piv = np.zeros(n, A.dtype)
    for j in range(n):
        p = A[j, j]
        piv[j] = p
        if not p > 0:
            return j, piv
        A[j, j] = np.sqrt(p)
        A[j + 1:, j] /= A[j, j]
        c = A[j + 1:, j]
        A[j + 1:, j + 1:] -= np.outer(c, c)
    return -1, piv


def _lower_inverse(L):
    """L^-1 of a lower-triangular L by forward substitution, row by row, in L's dtype"""
    m = L.shape[0]
    W = np.zeros_like(L)
    for i in range(m):
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = 1 / L[i, i]
    return W


def _marginal(S, sel, rest_order, dtype):
    S = np.asarray(S, np.float64)
    rest, present, nr = layout(S, sel)
    sel = [int(s) for s in sel]
    rest = list(rest) if rest_order is None else [rest[k] for k in rest_order]
    order = rest + sel
    n, m, d = len(rest), len(sel), S.shape[0]
    out = dict(fail=0, n_present=int(present.sum()), n_absent=int(d - present.sum()), info=None, cov=None, min_pivot_ratio=None, nr=nr)
    A = _permuted(S, order, present, dtype)
    diag0 = np.diag(A).copy()
    bad, piv_r = _eliminate(A, n)
    if bad >= 0:
        out["fail"] = 1 + bad // NB
        return out
    info = A[n:, n:].copy()
    info = np.tril(info) + np.tril(info, -1).T
    Ls = info.copy()
    bad, piv_s = _eliminate(Ls, m)
    if bad >= 0:
        out["fail"] = 1 + nr
        return out
    W = _lower_inverse(np.tril(Ls))
    cov = W.T @ W
    cov = np.tril(cov) + np.tril(cov, -1).T
    keep = present[sel]
    mask = np.outer(keep, keep)
    out["info"] = np.where(mask, info, 0)
    out["cov"] = np.where(mask, cov, 0)
    ratios = np.concatenate([piv_r, piv_s]) / diag0
    out["min_pivot_ratio"] = float(np.min(ratios[present[order]], initial=1.0))
    return out


def marginal(S, sel):
    """the reference: dict(fail, n_present, n_absent, nr, info, cov, min_pivot_ratio), info / cov in np.longdouble (None after a failure)"""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here: the reference would not be one"
    return _marginal(S, sel, None, LD)


def marginal64(S, sel, rest_order=None):
    """the same in float64; rest_order (a permutation of range(len(rest))) reorders the elimination of the rest"""
    return _marginal(S, sel, rest_order, np.float64)


def scales(info_star, present_sel):
    """(D_cov, D_info): sqrt(diag info*) and its reciprocal over the present selected unknowns, 0 on the absent ones"""
    dg = np.diag(np.asarray(info_star, LD)).copy()
    keep = np.asarray(present_sel, bool)
    dc = np.where(keep, np.sqrt(np.where(keep, dg, 1)), 0)
    di = np.where(keep, 1 / np.where(keep, dc, 1), 0)
    return dc, di


def err(X, X_star, D):
    """||D (X - X*) D||_F / ||D X* D||_F in longdouble"""
    Xs = np.asarray(X_star, LD)
    E = D[:, None] * (np.asarray(X, np.float64).astype(LD) - Xs) * D[None, :]
    N = D[:, None] * Xs * D[None, :]
    return float(np.sqrt((E * E).sum()) / np.sqrt((N * N).sum()))


def errors(got_info, got_cov, ref, present_sel):
    """(err_info, err_cov) of a float64 result against the reference dict"""
    dc, di = scales(ref["info"], present_sel)
    return err(got_info, ref["info"], di), err(got_cov, ref["cov"], dc)


N_ORDERS = rc.N_ORDERS


def err64_bound(S, sel, ref, seed):
    """(err64_info, err64_cov): the largest errors() of marginal64 over the natural order of the rest and N_ORDERS - 1 seeded permutations of it"""
    rest, present, _ = layout(S, sel)
    keep = present[[int(s) for s in sel]]
    rng = np.random.default_rng(1000 + seed)
    worst = [0.0, 0.0]
    for k in range(N_ORDERS):
        o = None if k == 0 else rng.permutation(len(rest))
        g = marginal64(S, sel, o)
        assert g["fail"] == 0, f"the float64 host computation fails (order {k}): fail {g['fail']}"
        e = errors(g["info"], g["cov"], ref, keep)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    assert np.isfinite(worst).all()
    return worst[0], worst[1]


def propagated(S, sel, ref, rel_entry):
    """(tol_info, tol_cov): what an entry-wise disagreement |dS_ij| <= rel_entry * max|S| between two assemblies of S can do to the two outputs,
    in the norm of err(), to first order.  With Z = (S^-1)[:, sel] info (= [I; -S_rr^-1 S_rs] in the natural order): d info = Z^T dS Z and
    d cov = -(S^-1)[:, sel]^T dS (S^-1)[:, sel]; ||dS||_2 <= d * rel_entry * max|S|, so ||D X^T dS X D||_F <= ||X D||_2 ||dS||_2 ||X D||_F.  The
    condition of the case enters through S^-1, computed here in longdouble from the present unknowns."""
    S = np.asarray(S, np.float64)
    d = S.shape[0]
    sel = [int(s) for s in sel]
    _, present, _ = layout(S, sel)
    alive = np.flatnonzero(present)
    A = _sym_lower(S, LD)[np.ix_(alive, alive)]
    bad, _ = _eliminate(A, len(alive))
    assert bad < 0
    W = _lower_inverse(np.tril(A))
    Sinv = np.zeros((d, d), LD)
    Sinv[np.ix_(alive, alive)] = W.T @ W
    keep = present[sel]
    dc, di = scales(ref["info"], keep)
    X = Sinv[:, sel]
    Z = X @ np.asarray(ref["info"], LD)
    dS = d * rel_entry * np.abs(S[np.ix_(alive, alive)]).max()
    out = []
    for Y, D, ref_x in ((Z, di, ref["info"]), (X, dc, ref["cov"])):
        YD = (Y * D[None, :]).astype(np.float64)
        N = (D[:, None] * np.asarray(ref_x, LD) * D[None, :]).astype(np.float64)
        out.append(float(np.linalg.norm(YD, 2) * dS * np.linalg.norm(YD, "fro") / np.linalg.norm(N, "fro")))
    return out[0], out[1]


def random_spd(d, cond, seed):
    """Q diag(w) Q^T with log-uniform eigenvalues in [1, cond] (both ends attained), exactly symmetric"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    w = np.exp(rng.uniform(0.0, np.log(cond), d))
    w[0] = 1.0
    if d > 1:
        w[-1] = cond
    S = (Q * w[None, :]) @ Q.T
    return np.tril(S) + np.tril(S, -1).T


def scattered(d, m, seed):
    """m distinct unknowns of d, scattered and unordered"""
    return np.random.default_rng(7000 + seed).permutation(d)[:m].astype(np.int32)


def kf_selection(n_kf, kfs):
    """the unknowns of keyframes `kfs` in the order of lvf_problem_marginal: per keyframe [pose 6, v 3, ba 3, bg 3]"""
    out = []
    for k in kfs:
        out += [6 * k + t for t in range(6)] + [6 * n_kf + 9 * k + t for t in range(9)]
    return np.asarray(out, np.int32)
