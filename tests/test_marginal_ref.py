"""The CPU reference of the marginal information / covariance (tests/marginal_ref.py) against independent computations, and the pieces of the
feature that need no GPU: the exported symbols and the position gate."""
import numpy as np
import pytest

from tests import marginal_ref as mr
from tests import reduced_cases as rc

EPS = 2.0 ** -53


def tol(S, sel):
    """d * 2^-53 * cond(S) (relative, max norm): what a float64 inverse / Schur formula of S is good for"""
    S = np.asarray(S, np.float64)
    return S.shape[0] * EPS * np.linalg.cond(S)


@pytest.mark.parametrize("d,m,cond,seed", [(1, 1, 1e2, 1), (7, 6, 1e2, 2), (40, 15, 1e2, 3), (80, 15, 1e6, 4), (150, 64, 1e4, 5), (140, 120, 1e2, 6)])
def test_reference_against_inverse_and_schur(d, m, cond, seed):
    S = mr.random_spd(d, cond, seed)
    sel = mr.scattered(d, m, seed)
    ref = mr.marginal(S, sel)
    assert ref["fail"] == 0 and ref["n_present"] == d and ref["n_absent"] == 0
    t = 8.0 * tol(S, sel)
    cov = np.linalg.inv(S)[np.ix_(sel, sel)]
    assert np.abs(ref["cov"].astype(np.float64) - cov).max() <= t * np.abs(cov).max()
    rest = [u for u in range(d) if u not in set(sel.tolist())]
    info = S[np.ix_(sel, sel)]
    if rest:
        info = info - S[np.ix_(sel, rest)] @ np.linalg.solve(S[np.ix_(rest, rest)], S[np.ix_(rest, sel)])
    assert np.abs(ref["info"].astype(np.float64) - info).max() <= t * np.abs(S).max()
    assert 0.0 < ref["min_pivot_ratio"] <= 1.0
    for X in (ref["info"], ref["cov"]):
        assert np.array_equal(X, X.T)


def with_absent(S, gone):
    S = np.array(S)
    S[gone, :] = 0.0; S[:, gone] = 0.0
    return S


def test_identity_on_present_and_zero_on_absent():
    d, m = 90, 20
    S0 = mr.random_spd(d, 1e3, 11)
    sel = mr.scattered(d, m, 11)
    rest = [u for u in range(d) if u not in set(sel.tolist())]
    gone = [int(sel[3]), int(sel[17]), rest[0], rest[40], rest[-1]]      # absent unknowns among the selection and among the rest
    S = with_absent(S0, gone)
    ref = mr.marginal(S, sel)
    assert ref["fail"] == 0 and ref["n_absent"] == len(gone) and ref["n_present"] == d - len(gone)
    keep = np.array([int(s) not in gone for s in sel])
    P = (ref["info"] @ ref["cov"]).astype(np.float64)
    assert np.abs(P[np.ix_(keep, keep)] - np.eye(keep.sum())).max() <= 8.0 * tol(S0, sel)
    for X in (ref["info"], ref["cov"]):
        assert not X[~keep, :].any() and not X[:, ~keep].any()
    # the present part is the marginal of the system with the absent unknowns deleted
    alive = [u for u in range(d) if u not in gone]
    pos = {u: i for i, u in enumerate(alive)}
    small = mr.marginal(S0[np.ix_(alive, alive)], [pos[int(s)] for s in sel if int(s) not in gone])
    assert np.abs((ref["cov"][np.ix_(keep, keep)] - small["cov"]).astype(np.float64)).max() <= 1e-15 * np.abs(small["cov"]).max().astype(np.float64)


def test_permuting_the_selection_permutes_the_outputs():
    d, m = 100, 30
    S = mr.random_spd(d, 1e4, 21)
    sel = mr.scattered(d, m, 21)
    p = np.random.default_rng(5).permutation(m)
    a, b = mr.marginal(S, sel), mr.marginal(S, sel[p])
    # info does not depend on the order inside the selection beyond rounding; cov is recomputed from a differently ordered factor
    assert np.abs((b["info"] - a["info"][np.ix_(p, p)]).astype(np.float64)).max() <= 1e-15 * np.abs(S).max()
    assert np.abs((b["cov"] - a["cov"][np.ix_(p, p)]).astype(np.float64)).max() <= 1e-13 * np.abs(a["cov"]).max().astype(np.float64)


@pytest.mark.parametrize("kind", ["neg", "nan"])
def test_indefinite_matrix_reports_the_step(kind):
    d, m = 64 * 3 + 15, 15
    S0 = mr.random_spd(d, 1e2, 31)
    sel = mr.scattered(d, m, 31)
    rest, _, nr = mr.layout(S0, sel)
    assert nr == 3
    for want_block in (0, 2):
        # an unknown of that block of the rest whose left neighbour sits right in front of it in the elimination order (what `nan` poisons)
        pos = next(q for q in range(64 * want_block + 1, 64 * want_block + 64) if rest[q] - 1 == rest[q - 1])
        ref = mr.marginal(rc.poisoned(S0, rest[pos], kind), sel)
        assert ref["fail"] == 1 + want_block and ref["info"] is None and ref["cov"] is None
    j = next(int(s) for s in sel if s > 0)
    assert mr.marginal(rc.poisoned(S0, j, kind), sel)["fail"] == 1 + nr
    # everything selected: no elimination step, the failure is "one past" = 1
    assert mr.marginal(rc.poisoned(S0[:10, :10], 4, kind), np.arange(10)[::-1])["fail"] == 1


def test_float64_bound_is_finite_and_small():
    S = mr.random_spd(79, 1e10, 41)
    sel = mr.scattered(79, 15, 41)
    ref = mr.marginal(S, sel)
    e_info, e_cov = mr.err64_bound(S, sel, ref, 41)
    assert 0.0 < e_info < 1e-4 and 0.0 < e_cov < 1e-4


def test_symbols_declared_and_bound():
    from lvio_fusion_amd import _lib
    declared = _lib.declared_symbols()
    for n in ("lvf_marginal_dense", "lvf_problem_marginal", "lvf_window_marginal"):
        assert n in declared and n in _lib._SIGS, n
    assert [f[0] for f in _lib.MarginalStats._fields_] == ["fail", "n_present", "n_absent", "min_pivot_ratio"]


def test_position_gate():
    from lvio_fusion_amd import relocalize
    cov = np.zeros((15, 15))
    cov[:3, :3] = 100.0 * np.eye(3)                  # rotation: not part of the gate
    R, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))
    cov[3:6, 3:6] = R @ np.diag([0.04, 0.25, 0.01]) @ R.T
    assert abs(relocalize.position_gate(cov, 3.0) - 1.5) <= 1e-12
    assert abs(relocalize.position_gate(cov[:6, :6], 2.0) - 1.0) <= 1e-12
