"""Marginal information and covariance on device, dense entry (lvf_marginal_dense): accuracy against the extended-precision reference of
tests/marginal_ref.py on matrices of the test's own choosing (tests/marginal_cases.py), exactness, numeric failures and argument errors.

    accuracy    err(X_dev) <= M * max(err64(X), d * 2^-53)   for X = info and X = cov
                err(X) = ||D (X - X*) D||_F / ||D X* D||_F,  D = sqrt(diag info*) for cov, its reciprocal for info

err64 is the float64 host computation's error taken as a bound: the largest over the natural elimination order of the rest and seven seeded
permutations of it (marginal_ref.err64_bound, the construction of reduced_cases.err64_bound).

M = 16: the smallest power of two that is at least four times the largest ratio, 2.64 (the 7 x 7 matrix of condition 1e10, info: 5.1e-14
against the float64 bound 1.9e-14; next 2.52, its condition-1e2 twin, cov: 2.0e-15 against the floor d * 2^-53 = 7.8e-16), over the 70 case / quantity figures of one MI355X run of this file (DESIGN.md §24 has the table).

"Failure" below is the numeric flag of a matrix that cannot be factored — never a device fault."""
import ctypes as C

import numpy as np
import pytest

from tests import marginal_cases as mc
from tests import marginal_ref as mr
from tests import reduced_cases as rc

M = 16.0
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("cid", mc.ALL_IDS)
def test_accuracy_and_exactness(ctx, oracle, cid):
    from lvio_fusion_amd import api
    c = mc.case(oracle, cid)
    S, sel, ref, keep, d = c["S"], c["sel"], c["ref"], c["present_sel"], c["d"]
    info, cov, st = api.marginal_dense(ctx, S, sel)
    assert st["fail"] == 0
    e_info, e_cov = mr.errors(info, cov, ref, keep)
    worst = 0.0
    for name, e, e64 in (("info", e_info, c["e64_info"]), ("cov", e_cov, c["e64_cov"])):
        floor = max(e64, d * 2.0 ** -53)
        worst = max(worst, floor)
        print(f"ratio {cid} d={d} m={len(sel)} {name}: err_dev {e:.3e} err64 {e64:.3e} floor {floor:.3e} ratio {e / floor:.3f}")
    rel = abs(st["min_pivot_ratio"] - ref["min_pivot_ratio"]) / ref["min_pivot_ratio"]
    print(f"pivot {cid}: dev {st['min_pivot_ratio']:.6e} ref {ref['min_pivot_ratio']:.6e} rel {rel:.3e} (M * floor {M * worst:.3e})")
    assert e_info <= M * max(c["e64_info"], d * 2.0 ** -53), f"{cid}: info"
    assert e_cov <= M * max(c["e64_cov"], d * 2.0 ** -53), f"{cid}: cov"
    # exactness
    assert np.array_equal(info, info.T) and np.array_equal(cov, cov.T)
    assert st["n_present"] + st["n_absent"] == d and st["n_present"] == ref["n_present"]
    for X in (info, cov):
        assert not X[~keep, :].any() and not X[:, ~keep].any()
        assert np.isfinite(X).all()
    assert 0.0 < st["min_pivot_ratio"] <= 1.0
    assert rel <= max(1e-6, M * worst), f"{cid}: min_pivot_ratio {st['min_pivot_ratio']} against {ref['min_pivot_ratio']}"


def test_absent_case_has_both_kinds(oracle):
    c = mc.case(oracle, mc.ABSENT_ID)
    rest, present, _ = mr.layout(c["S"], c["sel"])
    assert (~present[rest]).sum() >= 2 and (~c["present_sel"]).sum() >= 2


def test_info_only_and_cov_only(ctx, oracle):
    """either output may be NULL; the other is bit-equal to the call that asks for both"""
    from lvio_fusion_amd import _lib, api
    c = mc.case(oracle, "spd-r65-m15-c1e+02")
    S, sel = np.ascontiguousarray(c["S"]), np.ascontiguousarray(c["sel"], np.int32)
    info, cov, _ = api.marginal_dense(ctx, S, sel)
    m = len(sel)
    a, b, st = np.empty((m, m)), np.empty((m, m)), _lib.MarginalStats()
    assert ctx.L.lvf_marginal_dense(ctx.h, api._dp(S), S.shape[0], api._ip(sel), m, api._dp(a), None, C.byref(st)) == 0 and st.fail == 0
    assert ctx.L.lvf_marginal_dense(ctx.h, api._dp(S), S.shape[0], api._ip(sel), m, None, api._dp(b), C.byref(st)) == 0 and st.fail == 0
    assert np.array_equal(a, info) and np.array_equal(b, cov)


FAIL_D, FAIL_M = 64 * 3 + 15, 15


@pytest.fixture(scope="module")
def failing():
    S0 = mr.random_spd(FAIL_D, 1e2, 31)
    sel = mr.scattered(FAIL_D, FAIL_M, 31)
    rest, _, nr = mr.layout(S0, sel)
    assert nr == 3
    # an unknown of the block whose left neighbour (what `nan` poisons) sits right in front of it in the elimination order
    pick = lambda blk: next(q for q in range(64 * blk + 1, 64 * blk + 64) if rest[q] - 1 == rest[q - 1])
    where = {"first": (rest[pick(0)], 1), "last": (rest[pick(nr - 1)], nr), "selection": (int(next(s for s in sel if s > 0)), 1 + nr)}
    return S0, sel, where


@pytest.mark.parametrize("kind", ["neg", "nan"])
@pytest.mark.parametrize("where", ["first", "last", "selection"])
def test_numeric_failure_is_a_flag(ctx, failing, where, kind):
    from lvio_fusion_amd import _lib, api
    S0, sel, places = failing
    j, want = places[where]
    S = np.ascontiguousarray(rc.poisoned(S0, j, kind))
    assert mr.marginal(S, sel)["fail"] == want
    sel32 = np.ascontiguousarray(sel, np.int32)
    info, cov = np.full((FAIL_M, FAIL_M), -7.25), np.full((FAIL_M, FAIL_M), -7.25)
    st = _lib.MarginalStats()
    rc_ = ctx.L.lvf_marginal_dense(ctx.h, api._dp(S), FAIL_D, api._ip(sel32), FAIL_M, api._dp(info), api._dp(cov), C.byref(st))
    assert rc_ == 0, "a numeric failure is soft: LVF_OK"
    assert st.fail == want, f"{where} / {kind}: fail {st.fail}, the step holding unknown {j} is {want}"
    assert (info == -7.25).all() and (cov == -7.25).all(), "outputs touched after a failure"
    assert st.n_present + st.n_absent == FAIL_D
    # the next call on a good matrix succeeds
    g_info, g_cov, g = api.marginal_dense(ctx, S0, sel)
    assert g["fail"] == 0 and np.isfinite(g_info).all() and np.isfinite(g_cov).all()
    ref = mr.marginal(S0, sel)
    e_info, e_cov = mr.errors(g_info, g_cov, ref, np.ones(FAIL_M, bool))
    assert max(e_info, e_cov) <= M * FAIL_D * 2.0 ** -53                          # (condition 1e2: the floor of the accuracy bound alone)


def test_argument_errors(ctx):
    from lvio_fusion_amd import _lib, api
    d = 130
    S = np.ascontiguousarray(mr.random_spd(d, 1e2, 5))
    buf = np.full((121, 121), -7.25)
    st = _lib.MarginalStats()

    def call(sel, m, info=True, cov=True):
        s = np.ascontiguousarray(sel, np.int32)
        return ctx.L.lvf_marginal_dense(ctx.h, api._dp(S), d, api._ip(s), m, api._dp(buf) if info else None, api._dp(buf) if cov else None, C.byref(st))

    INVALID = 1                                                                  # LVF_ERR_INVALID (include/lvf.h)
    assert call(np.arange(121), 0) == INVALID                                    # m = 0
    assert call(np.arange(121), 121) == INVALID                                  # m = 121
    assert call([3, 9, 3], 3) == INVALID                                         # a duplicate
    assert call([3, d], 2) == INVALID and call([-1, 4], 2) == INVALID            # out of range
    assert call([3, 9], 2, info=False, cov=False) == INVALID                     # both outputs NULL
    assert (buf == -7.25).all()
    assert call([3, 9], 2) == 0 and st.fail == 0                                 # (and the same call with valid arguments works)
