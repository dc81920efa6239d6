"""Reduced systems for the direct test of the linear solve (tests/test_gpu_reduced_solve.py) and their high-precision reference.

Pure numpy.  The reference is a float64 Cholesky factor with plain forward / back substitution loops, refined with residuals in
np.longdouble (80-bit extended here: asserted, not assumed).  np.linalg.solve is not used on the triangular factors: it pivots, which
breaks the exact scale invariance the `graded` case relies on (measured 1e-6 against 1e-13)."""
import numpy as np

LD = np.longdouble


def _forward(L, b):
    n = len(b)
    y = np.array(b, dtype=L.dtype)
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def _backward(L, y):
    n = len(y)
    x = np.array(y, dtype=L.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def chol_solve64(L, b):
    """L L^T x = b in float64 with plain substitution loops"""
    return _backward(L, _forward(L, np.asarray(b, np.float64)))


def ref_solve(S, b):
    """(x_star, x64): x64 = float64 Cholesky + substitution; x_star = x64 refined five times (residual in longdouble, correction through the
    same float64 factor), returned as longdouble"""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here: the reference would not be one"
    S = np.asarray(S, np.float64); b = np.asarray(b, np.float64)
    L = np.linalg.cholesky(S)
    x64 = chol_solve64(L, b)
    Sl, bl = S.astype(LD), b.astype(LD)
    x = x64.astype(LD)
    for _ in range(5):
        r = bl - Sl @ x
        x = x + chol_solve64(L, r.astype(np.float64)).astype(LD)
    return x, x64


def err(S, x, x_star):
    """||Ds (x - x_star)||_2 / ||Ds x_star||_2, Ds = sqrt(diag S), in longdouble: the error in the norm a Cholesky solve is stable in
    (invariant under the symmetric diagonal scalings of `graded`)"""
    ds = np.sqrt(np.abs(np.diag(np.asarray(S, np.float64))).astype(LD))
    xs = np.asarray(x_star, LD)
    num = ds * (np.asarray(x, np.float64).astype(LD) - xs)
    den = ds * xs
    return float(np.sqrt(num @ num) / np.sqrt(den @ den))


N_ORDERS = 8


def err64_bound(S, b, x_star, seed, x64=None):
    """The float64 solve's error as a BOUND instead of one sample: the largest err() over N_ORDERS float64 Cholesky solves of the same system
    that differ in elimination (hence summation) order only — the natural order and N_ORDERS - 1 seeded symmetric permutations P S P^T.  One
    solve's error is a single draw of a rounding error of size cond * eps: for the shifted systems it was seen to move 70-fold (2.0e-9 ..
    1.4e-7 at 32 keyframes) with the last bits of S.  Exact powers of two scale every one of these solves exactly, so `graded` and `own`
    still get the same number."""
    S = np.asarray(S, np.float64); b = np.asarray(b, np.float64)
    if x64 is None:
        x64 = chol_solve64(np.linalg.cholesky(S), b)
    worst = err(S, x64, x_star)
    rng = np.random.default_rng(1000 + seed)
    for _ in range(N_ORDERS - 1):
        p = rng.permutation(len(b))
        xp = np.empty(len(b))
        xp[p] = chol_solve64(np.linalg.cholesky(S[np.ix_(p, p)]), b[p])
        worst = max(worst, err(S, xp, x_star))
    return worst


def grading(d, seed):
    """D = 2^k, k random integers in [-20, 20]: scaling by it is exact in binary floating point"""
    rng = np.random.default_rng(seed)
    return np.ldexp(1.0, rng.integers(-20, 21, size=d))


def lambda_min(S):
    """The smallest eigenvalue of a positive definite S.  np.linalg.eigvalsh resolves it to eps * ||S|| in ABSOLUTE terms: enough for the
    ordinary windows (lambda_min ~ 1e2 under ||S|| ~ 1e9).  A window with an isolated (v, ba, bg) block — no ImuError factor touches it, its
    damped diagonal is 1e-6 / radius = 1e-10 — is below that resolution (eigvalsh returns +-1e-7 there), so where eigvalsh's value is not
    resolved the eigenvalue is taken by inverse iteration through the Cholesky factor, whose accuracy is relative (it depends on the
    condition number of the diagonally scaled matrix only).  The estimate is a Rayleigh quotient, i.e. never below lambda_min."""
    w, V = np.linalg.eigh(S)
    if w[0] > 1e4 * np.finfo(np.float64).eps * max(abs(w[0]), abs(w[-1])):
        return float(w[0])
    L = np.linalg.cholesky(S)
    x = V[:, 0] / np.linalg.norm(V[:, 0])
    lam = None
    for _ in range(6):
        y = chol_solve64(L, x)
        lam = float((x @ y) / (y @ y))                       # = y^T S y / y^T y
        x = y / np.linalg.norm(y)
    return lam


def cases(S0, b0, seed, names=("own", "graded", "shift3", "shift6", "dd")):
    """{name: (S, b)}; every S keeps the sparsity pattern S0 != 0 (the elimination plan of the window reads no other entry).
    `graded`'s reference is x_star(own) / grading(d, seed): a refined reference of the graded matrix itself is not accurate."""
    S0 = np.asarray(S0, np.float64); b0 = np.asarray(b0, np.float64)
    S0 = np.tril(S0) + np.tril(S0, -1).T                     # exactly symmetric
    d = len(b0)
    rng = np.random.default_rng(seed + 1)
    out = {"own": (S0, b0)}
    if "graded" in names:
        D = grading(d, seed)
        out["graded"] = (D[:, None] * S0 * D[None, :], D * b0)
    if "shift3" in names or "shift6" in names:
        lam = lambda_min(S0)
        assert lam > 0.0
        for k in (3, 6):
            out[f"shift{k}"] = (S0 - (1.0 - 10.0 ** -k) * lam * np.eye(d), b0)
    P = S0 != 0.0
    G = rng.standard_normal((d, d)); G = np.tril(G) + np.tril(G, -1).T
    M = np.where(P, G, 0.0)
    np.fill_diagonal(M, 0.0)
    np.fill_diagonal(M, 1.01 * np.abs(M).sum(axis=1) + 1e-3)
    out["dd"] = (M, rng.standard_normal(d))
    return {k: v for k, v in out.items() if k in names}


def poisoned(S0, j, kind):
    """S0 with unknown j made unfactorable: `neg` S[j,j] = -S0[j,j]; `zero` row, column and pivot j all 0; `nan` one structurally non-zero
    off-diagonal entry of row j is NaN: (j, j-1), or (j, j+1) where j = 0 or S0[j, j-1] is outside the pattern (an entry outside it, or right of
    the diagonal only, is never read and poisons nothing).  Symmetric: both mirror entries are set."""
    S = np.array(S0, np.float64)
    if kind == "neg":
        S[j, j] = -S[j, j]
    elif kind == "zero":
        S[j, :] = 0.0; S[:, j] = 0.0
    elif kind == "nan":
        k = j - 1 if (j > 0 and S[j, j - 1] != 0.0) else j + 1
        assert S[j, k] != 0.0, f"no structural neighbour next to unknown {j}"
        S[j, k] = np.nan; S[k, j] = np.nan
    else:
        raise ValueError(kind)
    return S
