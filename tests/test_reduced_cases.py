"""(CPU) tests/reduced_cases.py on the oracle's own damped reduced systems: every case factors in float64, the graded case is the exact
scaling it claims to be, the float64 solve sits where a backward-stable solve of that condition number sits against the refined reference,
and every poisoned system really is unfactorable."""
import numpy as np
import pytest

from tests import reduced_cases as rc

WINDOWS = [(3, 80, 103), (11, 200, 107), (24, 500, 55)]      # n_kf, n_lm, seed
_sys = {}


def system(oracle, w):
    """(S0, b0) of the window's first LM iteration at radius 1e4 (computed once, shared, never modified)"""
    if w not in _sys:
        from lvio_fusion_amd import synthetic as syn
        n_kf, n_lm, seed = w
        cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=40, seed=seed, imu_samples=5)
        pre = np.stack([oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
        ref = oracle.Window(cfg, pre, use=("tc", "tf", "po", "imu")).lm_iteration(1e4, 2.0)
        S0, b0 = np.array(ref["S"], np.float64), np.array(ref["rhs"], np.float64)
        S0 = np.tril(S0) + np.tril(S0, -1).T                 # the lower triangle, mirrored: what the device tap reads
        S0.setflags(write=False); b0.setflags(write=False)
        _sys[w] = (S0, b0)
    return _sys[w]


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("w", WINDOWS, ids=lambda w: f"kf{w[0]}")
def test_cases_factor_and_the_float64_solve_is_accurate(oracle, w):
    S0, b0 = system(oracle, w)
    cs = rc.cases(S0, b0, w[2])
    assert set(cs) == {"own", "graded", "shift3", "shift6", "dd"}
    sols = {}
    for name, (S, b) in cs.items():
        assert ((S != 0.0) == (cs["own"][0] != 0.0)).all(), f"{name}: the sparsity pattern changed"
        assert (S == S.T).all()
        sols[name] = rc.ref_solve(S, b)                      # np.linalg.cholesky raises if the case does not factor
    D = rc.grading(len(b0), w[2])
    assert (sols["graded"][1] == sols["own"][1] / D).all(), "graded: x64 is not bit-equal to own's x64 / D"
    for name, (S, b) in cs.items():
        x_star, x64 = sols[name]
        if name == "graded":
            x_star = sols["own"][0] / D.astype(np.longdouble)
        e = rc.err(S, x64, x_star)
        print(f"kf{w[0]} {name}: err(x64) = {e:.2e}")
        assert np.isfinite(e) and e < 1e-6, f"{name}: err(x64) = {e}"
    # the bound over elimination orders contains the natural order's sample, is of its size, and is the same for the graded system
    xs_own = sols["own"][0]
    b_own = rc.err64_bound(*cs["own"], xs_own, w[2])
    assert rc.err(cs["own"][0], sols["own"][1], xs_own) <= b_own < 1e-6
    assert rc.err64_bound(*cs["graded"], xs_own / D.astype(np.longdouble), w[2]) == pytest.approx(b_own, rel=1e-12)
    b6 = rc.err64_bound(*cs["shift6"], sols["shift6"][0], w[2])
    print(f"kf{w[0]} bound over {rc.N_ORDERS} orders: own {b_own:.2e} shift6 {b6:.2e}")
    assert rc.err(cs["shift6"][0], sols["shift6"][1], sols["shift6"][0]) <= b6 < 1e-5
    # the scaled norm is invariant under the grading
    assert rc.err(cs["graded"][0], sols["graded"][1], sols["own"][0] / D.astype(np.longdouble)) == pytest.approx(
        rc.err(cs["own"][0], sols["own"][1], sols["own"][0]), rel=1e-12)


@pytest.mark.parametrize("w", WINDOWS, ids=lambda w: f"kf{w[0]}")
def test_poisoned_systems_do_not_factor(oracle, w):
    S0, _ = system(oracle, w)
    n_kf = w[0]
    dp = 6 * n_kf
    for j in (0, dp - 1, dp, dp + 9 * (n_kf // 2) + 6, dp + 9 * (n_kf - 1) + 3):
        for kind in ("neg", "zero", "nan"):
            S = rc.poisoned(S0, j, kind)
            assert (np.isnan(S) | (S == S.T)).all()
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                continue
            assert kind == "nan" and not np.isfinite(L).all(), f"unknown {j}, {kind}: the system factored"
