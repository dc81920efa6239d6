"""GPU parity of the GNSS (NavSat) alignment (lvio_fusion_amd/csrc/navsat_kernels.hip) through the C-ABI against the CPU restatement
tests/navsat_ref.py (itself checked against a 50-digit statement in tests/test_navsat_ref.py; there is no reference-compiled golden for
navsat_error.hpp: see that file's header).  Solver parity uses the tolerances of the sibling one-launch solve (tests/test_gpu_loop.py):
equal (num_iterations, num_successful_steps, termination), initial cost 1e-9 relative, final cost 1e-6 relative + 1e-15, parameters 1e-9.

Equal iteration counts are a CONDITION on the case, not a measurement: every case first asserts on the CPU that the restatement returns the
same counts with the fixes scaled by 1 +- 1e-12 and with the blocks summed in reverse order."""
import numpy as np
import pytest

from tests import navsat_ref as nr
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu

TRUST_YAW, TRUST_PITCH = 10.0, 30.0
BELOW, BETWEEN, ABOVE = 5.0, 20.0, 100.0


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def counts(s):
    return None if s is None else (s["num_iterations"], s["num_successful_steps"], s["termination"])


def assert_summary(s, ref, what):
    assert (s.num_iterations, s.num_successful_steps, s.termination) == counts(ref), what
    assert s.num_unsuccessful_steps == ref["num_iterations"] - ref["num_successful_steps"], what
    assert nr.WHY[s.termination_reason] == ref["why"], what
    assert abs(s.initial_cost - ref["initial_cost"]) <= 1e-9 * max(ref["initial_cost"], 1e-30), what
    assert abs(s.final_cost - ref["final_cost"]) <= 1e-6 * max(ref["final_cost"], 1e-12) + 1e-15, what


# ---- functors ------------------------------------------------------------------------------------------------------------------------------
def blocks(n, seed):
    rng = np.random.default_rng(seed)
    pose = np.concatenate([nr.quat_zyx(0.4, -0.1, 0.05) * 1.07, [3.0, -2.0, 0.5]])
    return rng.normal(0, 20, (n, 3)), rng.normal(0, 20, (n, 3)), rng.uniform(0.01, 0.3, (n, 3)), pose


@pytest.mark.parametrize("n,seed", [(1, 1), (12, 2), (300, 3)])
def test_navsat_init_error_parity(ctx, n, seed):
    from lvio_fusion_amd import api
    p0, p1, cov, _ = blocks(n, seed)
    for x3 in ((0.0, 0.0, 0.0), (0.7, 3.0, -2.0)):
        r, J = api.navsat_init_evaluate(ctx, p0, p1, cov, x3)
        r0, J0 = nr.navsat_init(p0, p1, cov, x3)
        for i in range(n):
            assert_parity(r[i], r0[i], f"NavsatInitError r[{i}]")
            for c in range(3):
                assert_parity(J[i][:, c], J0[i][:, c], f"NavsatInitError J[{i}] block {c}")
        r2, none = api.navsat_init_evaluate(ctx, p0, p1, cov, x3, jacobians=False)
        assert none is None and np.array_equal(r2, r)


@pytest.mark.parametrize("n,seed", [(1, 4), (12, 5), (300, 6)])
def test_navsat_rx_error_parity(ctx, n, seed):
    from lvio_fusion_amd import api
    p0, p1, cov, pose = blocks(n, seed)
    for x6 in ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.3, -0.1, 0.05, 0.8, -0.5, 0.2)):
        r, J = api.navsat_rx_evaluate(ctx, p0, p1, pose, cov, x6)
        r0, J0 = nr.navsat_rx(p0, p1, pose, cov, x6)
        for i in range(n):
            assert_parity(r[i], r0[i], f"NavsatRXError r[{i}]")
            for c in range(6):
                assert_parity(J[i][:, c], J0[i][:, c], f"NavsatRXError J[{i}] block {c}")
        r2, none = api.navsat_rx_evaluate(ctx, p0, p1, pose, cov, x6, jacobians=False)
        assert none is None and np.array_equal(r2, r)


def test_navsat_r_error_parity(ctx):
    from lvio_fusion_amd import api
    _, _, _, pose = blocks(1, 7)
    for y in (np.array([0.4, 11.5, -0.8]), np.array([-3.0, 280.0, 6.0])):
        for roll in (0.0, 0.2):
            r, J = api.navsat_r_evaluate(ctx, y, pose, roll)
            r0, J0 = nr.navsat_r(y, pose, roll)
            assert_parity([r], r0[0], "NavsatRError r"); assert_parity([J], J0[0, 0], "NavsatRError J")
            r2, none = api.navsat_r_evaluate(ctx, y, pose, roll, jacobians=False)
            assert none is None and r2 == r


# ---- Navsat::Initialize ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,noise,para", [(30, 5, 0.05, (0.7, 3.0, -2.0)), (300, 6, 0.2, (-1.2, -8.0, 5.0)), (2, 7, 0.01, (0.1, 0.5, 0.5))])
def test_navsat_initialize_matches_restatement(ctx, oracle, n, seed, noise, para):
    from lvio_fusion_amd import api
    rng = np.random.default_rng(seed)
    p6 = np.array([para[0], 0.0, 0.0, para[1], para[2], 0.0])
    raw = rng.normal(0, 25, (n, 3))
    position = np.array([oracle.se3_apply(oracle.rpyxyz_to_se3(p6), p) for p in raw]) + rng.normal(0, noise, (n, 3))
    cov = np.tile(rng.uniform(0.02, 0.2, 3), (n, 1))
    ref = nr.initialize(oracle, position, raw, cov)
    for kw in (dict(scale=1 + 1e-12), dict(scale=1 - 1e-12), dict(reverse=True)):
        probe = nr.initialize(oracle, position, raw, cov, **kw)
        assert (counts(probe[2]), counts(probe[3])) == (counts(ref[2]), counts(ref[3])), f"iteration counts are not robust for this case ({kw})"
    got = api.navsat_initialize(ctx, position, raw, cov)
    assert_summary(got[2], ref[2], "stage 1"); assert_summary(got[3], ref[3], "stage 2")
    assert got[2].num_residual_blocks == n
    assert np.abs(got[0] - ref[0]).max() <= 1e-9 and np.array_equal(got[0][[1, 2, 5]], np.zeros(3))
    assert_parity(got[1], ref[1], "extrinsic")
    if noise <= 0.05:
        assert np.abs(got[0] - p6).max() < 0.05


def test_navsat_initialize_empty_and_bad_covariance(ctx):
    from lvio_fusion_amd import api
    para, ext, s1, s2 = api.navsat_initialize(ctx, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert np.array_equal(para, np.zeros(6)) and np.array_equal(ext, [0, 0, 0, 1, 0, 0, 0]) and s2.num_iterations == 0
    with pytest.raises(api.LvfError):
        api.navsat_initialize(ctx, np.ones((3, 3)), np.ones((3, 3)), np.array([[0.1, 0.1, 0.1], [0.1, 0.0, 0.1], [0.1, 0.1, 0.1]]))


# ---- Navsat::OptimizeBC ----------------------------------------------------------------------------------------------------------------------
PLANTED = (0.05, -0.02, 0.0, 0.8, -0.5, 0.3)
STEEP = (0.3, 0.1, 0.0, 2.0, -1.0, 2.0)
WIDE, TIGHT, AWAY = (-100.0, 100.0), (-0.05, 0.05), (0.5, 0.6)
BC_CASES = [
    # id, planted, mode, distance, fraction without fix, z bounds, n, n_update, seed
    ("section-above", PLANTED, 0b000000, ABOVE, 0.2, WIDE, 40, 5, 3),
    ("section-between", PLANTED, 0b000000, BETWEEN, 0.2, WIDE, 40, 5, 4),
    ("section-above-bound-active", STEEP, 0b000000, ABOVE, 0.2, TIGHT, 40, 3, 3),
    ("section-above-no-fix", PLANTED, 0b000000, ABOVE, 1.0, WIDE, 25, 4, 5),
    ("roll-held-above", PLANTED, 0b000100, ABOVE, 0.2, WIDE, 300, 0, 6),
    ("roll-held-between", PLANTED, 0b000100, BETWEEN, 0.0, WIDE, 12, 700, 7),
    ("roll-held-above-bound-active", STEEP, 0b000100, ABOVE, 0.0, TIGHT, 40, 2, 3),
    ("roll-held-between-start-outside-box", PLANTED, 0b000100, BETWEEN, 0.2, AWAY, 40, 2, 8),
    ("roll-held-above-no-fix", PLANTED, 0b000100, ABOVE, 1.0, TIGHT, 9, 3, 9),
    ("x-only-below", PLANTED, 0b110111, BELOW, 0.2, WIDE, 40, 5, 10),
    ("x-only-between", PLANTED, 0b110111, BETWEEN, 0.0, TIGHT, 1, 30, 11),
    ("x-only-above", STEEP, 0b110111, ABOVE, 0.2, WIDE, 40, 5, 12),
    ("x-only-below-no-fix", PLANTED, 0b110111, BELOW, 1.0, WIDE, 6, 2, 13),
]
# The Armijo contraction path must be covered: these two are CONSTRUCTED for it (a z bound 2 m short of the optimum and a first step that
# the clipping shortens too much for the sufficient-decrease test); realistic sections with a loose bound never contract.
MUST_CONTRACT = {"section-above-bound-active", "roll-held-above-bound-active"}


def run_bc_ref(oracle, case, **kw):
    _, planted, mode, distance, missing, zb, n, n_update, seed = case
    poses, has, fix, cov = nr.planted_section(oracle, n, seed, planted, noise=0.05, missing=missing, n_update=n_update)
    return (poses, has, fix, cov), nr.optimize_bc(oracle, poses, n, has, fix, cov, mode, distance, TRUST_YAW, TRUST_PITCH, zb[0], zb[1], **kw)


@pytest.mark.parametrize("case", BC_CASES, ids=[c[0] for c in BC_CASES])
def test_navsat_optimize_bc_matches_restatement(ctx, oracle, case):
    from lvio_fusion_amd import api
    name, planted, mode, distance, missing, zb, n, n_update, seed = case
    (poses, has, fix, cov), ref = run_bc_ref(oracle, case)
    for kw in (dict(scale=1 + 1e-12), dict(scale=1 - 1e-12), dict(reverse=True)):
        probe = run_bc_ref(oracle, case, **kw)[1]
        assert (counts(probe["roll"]), counts(probe["main"])) == (counts(ref["roll"]), counts(ref["main"])), f"iteration counts are not robust for this case ({kw})"
        assert probe["main"]["contractions"] == ref["main"]["contractions"]
    assert not ref["skipped"]
    if name in MUST_CONTRACT:
        assert ref["main"]["contractions"] > 0
    if missing < 1.0 and mode != 0b110111:
        assert ref["main"]["huber_active"] > 0
    opt = api.navsat_bc_options(mode=mode, distance=distance, trust_distance_yaw=TRUST_YAW, trust_distance_pitch=TRUST_PITCH, z_lower=zb[0], z_upper=zb[1])
    P = poses.copy()
    res = api.navsat_optimize_bc(ctx, P, n, has, fix, cov, opt)
    assert res.skipped == 0
    assert_summary(res.main, ref["main"], "main solve")
    assert res.main.num_residual_blocks == int(has.sum())
    if ref["roll"] is None:
        assert res.roll.num_iterations == 0 and res.roll.num_residual_blocks == 0
    else:
        assert_summary(res.roll, ref["roll"], "roll pre-solve")
    assert res.line_search_contractions == ref["main"]["contractions"]
    assert np.abs(np.array(res.para) - ref["para"]).max() <= 1e-9
    assert_parity(np.array(res.transform), ref["transform"], "transform")
    assert_parity(P, ref["poses"], "poses")
    if zb is not WIDE and not (mode & 32) and missing < 1.0:
        assert zb[0] <= res.para[5] <= zb[1]


def test_navsat_optimize_bc_early_return_leaves_everything_untouched(ctx, oracle):
    from lvio_fusion_amd import api
    poses, has, fix, cov = nr.planted_section(oracle, 20, 3, PLANTED, noise=0.05, n_update=3)
    for mode in (0b000000, 0b000100, 0b110011):
        P, H, F, C = poses.copy(), has.copy(), fix.copy(), cov.copy()
        res = api.navsat_optimize_bc(ctx, P, 20, H, F, C, api.navsat_bc_options(mode=mode, distance=BELOW, trust_distance_yaw=TRUST_YAW, trust_distance_pitch=TRUST_PITCH))
        assert res.skipped == 1 and res.main.num_iterations == 0
        assert P.tobytes() == poses.tobytes() and H.tobytes() == has.tobytes() and F.tobytes() == fix.tobytes() and C.tobytes() == cov.tobytes()
    P = np.zeros((0, 7))
    assert api.navsat_optimize_bc(ctx, P, 0, np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3)), api.navsat_bc_options(distance=ABOVE)).skipped == 1


def test_navsat_optimize_bc_rejects_bad_input(ctx, oracle):
    from lvio_fusion_amd import api
    poses, has, fix, cov = nr.planted_section(oracle, 10, 3, PLANTED, noise=0.05, n_update=2)
    has[:] = 1
    opt = api.navsat_bc_options(mode=0b110111, distance=ABOVE, trust_distance_yaw=TRUST_YAW, trust_distance_pitch=TRUST_PITCH)
    bad = cov.copy(); bad[4, 1] = -0.1
    with pytest.raises(api.LvfError):
        api.navsat_optimize_bc(ctx, poses.copy(), 10, has, fix, bad, opt)
    P = poses.copy(); P[11, :4] = 0.0
    with pytest.raises(api.LvfError):
        api.navsat_optimize_bc(ctx, P, 10, has, fix, cov, opt)
    has[4] = 0                                               # a covariance nobody reads may be anything
    assert api.navsat_optimize_bc(ctx, poses.copy(), 10, has, fix, bad, opt).skipped == 0


# ---- the per-keyframe chain --------------------------------------------------------------------------------------------------------------------
def chain_ref(oracle, n, seed, **kw):
    poses, has, fix, cov = nr.chain_section(n, seed)
    return (poses, has, fix, cov), nr.fix_chain(oracle, poses, has, fix, cov, **kw)


@pytest.mark.parametrize("n,seed", [(2, 21), (64, 22), (700, 23), (3000, 24)])      # 3000 poses do not fit the LDS: the global-memory path
def test_navsat_fix_chain_matches_restatement(ctx, oracle, n, seed):
    from lvio_fusion_amd import api
    (poses, has, fix, cov), ref = chain_ref(oracle, n, seed)
    for scale in (1 + 1e-12, 1 - 1e-12):      # (one block per step: there is no order to reverse)
        probe = chain_ref(oracle, n, seed, scale=scale)[1]
        assert np.array_equal(probe["iterations"], ref["iterations"]), f"iteration counts are not robust for this case (scale {scale})"
    if n > 2:
        assert 0 < int(has.sum()) < n - 1 and abs(1.0 - has.mean() - 0.2) < 0.1      # about one keyframe in five has no fix
        assert ref["huber_active"] > 0
    costs = [s["final_cost"] for s in ref["summaries"] if s is not None]
    assert all(c > 0.0 for c in costs)                       # noise on all three axes: no block's cost vanishes
    P = poses.copy()
    x, it, summ = api.navsat_fix_chain(ctx, P, has, fix, cov)
    assert np.array_equal(it, ref["iterations"])
    assert np.abs(x - ref["x"]).max() <= 1e-9
    assert_parity(P, ref["poses"], "chain poses")
    assert summ.num_iterations == int(ref["iterations"].sum()) and summ.num_residual_blocks == int(has.sum()) and summ.termination == 0
    assert abs(summ.final_cost - sum(costs)) <= 1e-6 * sum(costs) + 1e-15


@pytest.mark.parametrize("n,seed", [(40, 31), (300, 32)])
def test_navsat_fix_chain_equals_separate_optimize_bc_calls(ctx, oracle, n, seed):
    from lvio_fusion_amd import api
    poses, has, fix, cov = nr.chain_section(n, seed)
    P = poses.copy()
    x, it, _ = api.navsat_fix_chain(ctx, P, has, fix, cov)
    Q = poses.copy()
    opt = api.navsat_bc_options(mode=0b110111, distance=0.0, trust_distance_yaw=TRUST_YAW, trust_distance_pitch=TRUST_PITCH)
    for k in range(n - 1):
        tail = Q[k:]                                         # a view: updated in place
        res = api.navsat_optimize_bc(ctx, tail, 1, has[k:k + 1], fix[k:k + 1], cov[k:k + 1], opt)
        assert res.skipped == 0 and res.main.num_iterations == it[k] and abs(res.para[3] - x[k]) <= 1e-9
    assert_parity(P, Q, "one launch against n - 1 launches")      # two kernels: not bit for bit


def test_navsat_fix_chain_small_and_bad_input(ctx, oracle):
    from lvio_fusion_amd import api
    for n in (0, 1):
        poses, has, fix, cov = nr.chain_section(n, 1)
        P = poses.copy()
        x, it, summ = api.navsat_fix_chain(ctx, P, has, fix, cov)
        assert P.tobytes() == poses.tobytes() and x.size == 0 and summ.num_iterations == 0
    poses, has, fix, cov = nr.chain_section(12, 2, missing=0.0)
    bad = cov.copy(); bad[3, 0] = 0.0
    with pytest.raises(api.LvfError):
        api.navsat_fix_chain(ctx, poses.copy(), has, fix, bad)
    P = poses.copy(); P[11, :4] = 0.0
    with pytest.raises(api.LvfError):
        api.navsat_fix_chain(ctx, P, has, fix, cov)


def test_navsat_quick_fix_composes_the_two_calls(ctx, oracle):
    from lvio_fusion_amd import api
    n = 50
    poses, has, fix, cov = nr.planted_section(oracle, n, 41, PLANTED, noise=0.05, missing=0.2)
    opt = api.navsat_bc_options(distance=ABOVE, trust_distance_yaw=TRUST_YAW, trust_distance_pitch=TRUST_PITCH, z_lower=-100.0, z_upper=100.0)
    seen = []
    P = poses.copy()
    res, x, it, summ = api.navsat_optimize(ctx, P, has, fix, cov, opt, lambda arr: seen.append(arr.copy()))
    Q = poses.copy()
    res2 = api.navsat_optimize_bc(ctx, Q, n, has, fix, cov, opt)
    assert len(seen) == 1 and seen[0].tobytes() == Q.tobytes() and np.array_equal(np.array(res.para), np.array(res2.para))
    x2, it2, _ = api.navsat_fix_chain(ctx, Q[1:], has[1:n - 1], fix[1:n - 1], cov[1:n - 1])
    assert P.tobytes() == Q.tobytes() and np.array_equal(x, x2) and np.array_equal(it, it2) and x.size == n - 2
    R = poses.copy()
    api.navsat_quick_fix(ctx, R, has, fix, cov, opt)
    assert R.tobytes() == P.tobytes()
