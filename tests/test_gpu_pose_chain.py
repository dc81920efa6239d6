"""The device pose-chain solve (lvio_fusion_amd/csrc/pose_chain_kernels.hip) against tests/pose_chain_ref.py: the block system,
the accuracy of one damped step of the odd-even block cyclic reduction, whole solves of Navsat::OptimizeAB sections, the pose-graph chain
against the window solver's route, the soft failures and the composition of Navsat::Optimize.

    step accuracy    err(x_dev) <= M * max(err64, d * 2^-53),   err = ||Ds (x - x_star)|| / ||Ds x_star||, Ds = sqrt(diag), d = 6 m

on the DEVICE's own damped system (downloaded; the linearisation is bit-reproducible): x_star is a float64 block-Thomas solution refined with
residuals in np.longdouble, err64 the largest error of three float64 solves of the same system (Thomas forward, Thomas from the other end,
dense).  M = 8: the smallest power of two that is at least four times the largest ratio, 1.16 (2 free poses, radius 1e4), over the 26
size / radius figures of one MI355X run of this file (DESIGN.md §23 has the table; the rule is §17's).

Iteration counts are compared for equality: tests/test_pose_chain_ref.py shows that every comparison the loop decides by has a relative margin
of at least 1e-6 on these scenes.  "Failure" below is the numerical flag, never a GPU fault."""
import numpy as np
import pytest

from tests import navsat_ref as nr
from tests import pose_chain_ref as pc
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu

M = 8.0
LDS_ROWS = 120                     # the working set of the reduction is in LDS up to here, in the workspace beyond
STEP_SIZES = [1, 2, 3, 4, 63, 64, 65, LDS_ROWS, LDS_ROWS + 1, 255, 256, 257, "capacity"]
RADII = [1e4, 1e-2]


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def chain_args(pb):
    return pb["poses"], pb["tg"], pb["ew"], pb["ev"], pb["kind"], pb["ut"], pb["uw"]


def assert_summary(s, ref, what):
    assert (s.num_iterations, s.num_successful_steps, s.termination) == (ref["num_iterations"], ref["num_successful_steps"], ref["termination"]), what
    assert s.num_unsuccessful_steps == ref["num_iterations"] - ref["num_successful_steps"], what
    assert nr.WHY[s.termination_reason] == ref["why"], what


@pytest.mark.parametrize("m", [1, 2, 5, 64])
def test_block_system_matches_ref_and_is_reproducible(ctx, oracle, m):
    from lvio_fusion_amd import api
    pb = pc.step_case(oracle, m, 20 + m)
    lin = pc.linearize(oracle, pb, pb["poses"])
    D, O, g = api.pose_chain_debug_system(ctx, *chain_args(pb), pb["huber_a"])
    assert_parity(D, lin["D"], "D"); assert_parity(O, lin["O"], "O"); assert_parity(g, lin["g"], "g")
    assert np.array_equal(D, np.transpose(D, (0, 2, 1)))
    D2, O2, g2 = api.pose_chain_debug_system(ctx, *chain_args(pb), pb["huber_a"])
    assert D.tobytes() == D2.tobytes() and O.tobytes() == O2.tobytes() and g.tobytes() == g2.tobytes()
    # edge targets taken from the start poses on the device
    pbs = pc.problem(oracle, pb["poses"], None, pb["ew"], pb["ev"], pb["kind"], pb["ut"], pb["uw"], pb["huber_a"])
    lins = pc.linearize(oracle, pbs, pbs["poses"])
    Ds, Os, gs = api.pose_chain_debug_system(ctx, pb["poses"], None, pb["ew"], pb["ev"], pb["kind"], pb["ut"], pb["uw"], pb["huber_a"])
    assert_parity(Ds, lins["D"], "D, targets from the poses"); assert_parity(Os, lins["O"], "O, targets from the poses")
    assert np.abs(gs - lins["g"]).max() <= 1e-9 * np.abs(lin["g"]).max()      # the edges are at their targets: g is what the unaries leave


_step_cache = {}


def step_system(api, ctx, oracle, m):
    """the case and the device's own undamped blocks, computed once per size"""
    if m not in _step_cache:
        pb = pc.step_case(oracle, m, 30 + m)
        D, O, g = api.pose_chain_debug_system(ctx, *chain_args(pb), pb["huber_a"])
        for a in (D, O, g):
            a.setflags(write=False)
        _step_cache.clear()                                # one size at a time: the capacity case holds a 6132 x 6132 matrix
        _step_cache[m] = (pb, D, O, g)
    return _step_cache[m]


@pytest.mark.parametrize("m,radius", [(m, r) for m in STEP_SIZES for r in RADII])
def test_step_accuracy(ctx, oracle, m, radius):
    from lvio_fusion_amd import api
    if m == "capacity":
        m = api.pose_chain_capacity()
        assert m >= 1022
    pb, D, O, g = step_system(api, ctx, oracle, m)
    got = api.pose_chain_debug_step(ctx, *chain_args(pb), pb["huber_a"], radius)
    assert not got["fail"] and np.all(np.isfinite(got["dx"]))
    Dd = pc.damp(D, np.einsum("fii->fi", D).ravel().copy(), radius)
    ok, x_fwd = pc.thomas(Dd, O, -g)
    ok2, x_rev = pc.thomas(Dd, O, -g, reverse=True)
    assert ok and ok2
    x_dense = np.linalg.solve(pc.dense(Dd, O), -g)
    x_star = pc.refine(Dd, O, -g, x_fwd)
    err64 = max(pc.err(Dd, x, x_star) for x in (x_fwd, x_rev, x_dense))
    floor = max(err64, 6 * m * 2.0 ** -53)
    e = pc.err(Dd, got["dx"], x_star)
    print(f"pose-chain step m={m} radius={radius:g}: err_dev {e:.3e} err64 {err64:.3e} floor {floor:.3e} ratio {e / floor:.3f}")
    assert e <= M * floor, (m, radius, e, err64, e / floor)
    lin = dict(D=D, O=O, g=g)
    model = pc.model_decrease(lin, got["dx"])
    assert got["model"] > 0 and abs(got["model"] - model) <= 1e-9 * abs(model)
    assert abs(got["cost"] - pc.linearize(oracle, pb, pb["poses"], jac=False)["cost"]) <= 1e-9 * got["cost"]
    again = api.pose_chain_debug_step(ctx, *chain_args(pb), pb["huber_a"], radius)
    assert again["dx"].tobytes() == got["dx"].tobytes() and again["model"] == got["model"]      # no atomics: bit-equal


@pytest.mark.parametrize("scene", pc.SOLVE_SCENES, ids=[f"m{s[0]}" for s in pc.SOLVE_SCENES])
def test_navsat_optimize_ab_matches_ref(ctx, oracle, scene):
    from lvio_fusion_amd import api
    m, seed, kw, loss = scene
    poses, stamps, fix, relB = pc.ab_section(oracle, m, seed, **kw)
    X, ref = pc.solve(oracle, pc.navsat_ab(oracle, poses, stamps, fix, relB, 0.1))
    P = poses.copy()
    s = api.navsat_optimize_ab(ctx, P, stamps, fix, relB, 0.1)
    print(f"OptimizeAB m={m}: iterations {s.num_iterations} ({ref['num_iterations']}), successful {s.num_successful_steps}, cost {s.initial_cost:.6g} -> {s.final_cost:.6g}")
    assert_summary(s, ref, f"m = {m}")
    assert_parity(s.initial_cost, ref["initial_cost"], "initial cost"); assert_parity(s.final_cost, ref["final_cost"], "final cost")
    assert_parity(P, X, "poses")
    assert P[0].tobytes() == poses[0].tobytes() and P[-1].tobytes() == poses[-1].tobytes()      # constant ends
    assert s.num_residual_blocks == (m + 1) + m
    assert np.abs(P[1:-1, 4:] - poses[1:-1, 4:]).max() > 1e-3                                    # something moved
    Q = poses.copy()
    api.navsat_optimize_ab(ctx, Q, stamps, fix, relB, 0.1)
    assert Q.tobytes() == P.tobytes()


def test_navsat_optimize_ab_interpolates_fix_z(ctx, oracle):
    """z of every fix is a B.z + (1 - a) A.z whatever GetFixPoint returned: a wildly wrong raw z changes nothing"""
    from lvio_fusion_amd import api
    poses, stamps, fix, relB = pc.ab_section(oracle, 7, 3)
    wild = fix.copy(); wild[:, 2] += 250.0 * np.arange(1, 10)
    X, ref = pc.solve(oracle, pc.navsat_ab(oracle, poses, stamps, wild, relB, 0.1))
    P, Q = poses.copy(), poses.copy()
    s = api.navsat_optimize_ab(ctx, P, stamps, wild, relB, 0.1)
    api.navsat_optimize_ab(ctx, Q, stamps, fix, relB, 0.1)
    assert P.tobytes() == Q.tobytes()
    assert_summary(s, ref, "wild z"); assert_parity(P, X, "poses")


def test_pose_graph_chain_against_the_window_route(ctx, oracle):
    """R unaries at n = 9: lvf_pose_chain_solve and the lvf_problem_* + pose-prior route, both run to convergence, and the ref"""
    from lvio_fusion_amd import api
    from tests.test_gpu_posegraph import chain
    n = 9
    P, before, pr = chain(oracle, n, 5)
    tight = dict(function_tolerance=1e-15, parameter_tolerance=1e-13, gradient_tolerance=1e-12, max_num_iterations=50)
    opt = api.default_solver_options()
    for k, v in tight.items():
        setattr(opt, k, v)
    st = api.State(ctx, n, 0); st.set(api.POSES, P)
    b = api.pose_prior_batch(ctx, pr["kf_a"], pr["kf_b"], pr["target"], pr["weight"], pr["v"])
    prob = api.Problem(ctx, st, None, None, None, None); prob.set_pose_priors(b)
    prob.set_pose_constant(0, True); prob.set_pose_constant(n - 1, True)
    sw = prob.solve(opt)
    Pw = st.get(api.POSES).reshape(-1, 7)
    pb = pc.from_priors(oracle, P, pr)
    Pc = P.copy()
    sc = api.pose_chain_solve(ctx, Pc, pb["tg"], pb["ew"], pb["ev"], pb["kind"], pb["ut"], pb["uw"], 0.0, opt)
    X, ref = pc.solve(oracle, pb, tight)
    print(f"pose graph n=9: chain {sc.num_iterations} iterations, cost {sc.final_cost:.9g}; window route {sw.num_iterations}, {sw.final_cost:.9g}; ref {ref['num_iterations']}, {ref['final_cost']:.9g}")
    assert sc.termination != 2 and sw.termination != 2
    assert_parity(sc.initial_cost, ref["initial_cost"], "initial cost"); assert_parity(sw.initial_cost, ref["initial_cost"], "initial cost (window route)")
    assert_parity(Pc, X, "chain vs ref"); assert_parity(Pw, X, "window route vs ref"); assert_parity(Pc, Pw, "chain vs window route")
    assert Pc[0].tobytes() == P[0].tobytes() and Pc[-1].tobytes() == P[-1].tobytes()
    assert sc.final_cost < 0.5 * sc.initial_cost and sc.num_residual_blocks == len(pr["kf_b"])
    prob.close(); b.close(); st.close()


def test_soft_failures_and_edge_cases(ctx, oracle):
    from lvio_fusion_amd import api
    poses, stamps, fix, relB = pc.ab_section(oracle, 7, 3)
    # a NaN fix point: five invalid steps, FAILURE, the poses stay as they came
    bad = fix.copy(); bad[3, 0] = np.nan
    P = poses.copy()
    s = api.navsat_optimize_ab(ctx, P, stamps, bad, relB, 0.1)
    assert s.termination == 2 and P.tobytes() == poses.tobytes() and s.num_successful_steps == 0
    X, ref = pc.solve(oracle, pc.navsat_ab(oracle, poses, stamps, bad, relB, 0.1))
    assert ref["termination"] == 2 and s.num_iterations == ref["num_iterations"] == 5
    pbn = pc.navsat_ab(oracle, poses, stamps, bad, relB, 0.1)
    got = api.pose_chain_debug_step(ctx, *chain_args(pbn), 0.1, 1e4)      # the blocks are finite (the fix is not in a Jacobian), g is not
    assert not got["fail"] and not got["model"] > 0.0
    # a NaN edge weight: NaN pivots, the reduction raises its flag, dx = 0
    pbn = pc.navsat_ab(oracle, poses, stamps, fix, relB, 0.1)
    pbn["ew"][2] = np.nan
    got = api.pose_chain_debug_step(ctx, *chain_args(pbn), 0.1, 1e4)
    assert got["fail"] and not np.any(got["dx"]) and not pc.damped_step(pc.linearize(oracle, pbn, poses), np.ones(42), 1e4)[0]
    P = poses.copy()
    s = api.pose_chain_solve(ctx, P, pbn["tg"], pbn["ew"], pbn["ev"], pbn["kind"], pbn["ut"], pbn["uw"], 0.1)
    assert s.termination == 2 and s.num_iterations == 5 and P.tobytes() == poses.tobytes()
    # one pose that no block holds (its two edges have weight 0, no unary): a zero row, rescued by the damping clamp
    pb = pc.navsat_ab(oracle, poses, stamps, fix, relB, 0.1)
    pb["ew"][3] = pb["ew"][4] = 0.0; pb["kind"][4] = pc.NONE
    X, ref = pc.solve(oracle, pb)
    assert ref["termination"] == 0 and pc.min_margin(ref) >= 1e-6
    P = poses.copy()
    s = api.pose_chain_solve(ctx, P, pb["tg"], pb["ew"], pb["ev"], pb["kind"], pb["ut"], pb["uw"], 0.1)
    assert_summary(s, ref, "zero row"); assert_parity(P, X, "zero row: poses"); assert_parity(s.final_cost, ref["final_cost"], "zero row: cost")
    assert P[4].tobytes() == poses[4].tobytes()             # g = 0 there: the step is exactly zero
    # n = 2: the cost only
    two = np.stack([poses[0], poses[-1]])
    pb2 = pc.problem(oracle, two, [oracle.pose_graph_target(poses[0], poses[1])], [2.0], [20.0], [0, 0], np.zeros((2, 4)), [0.0, 0.0])
    P = two.copy()
    s = api.pose_chain_solve(ctx, P, pb2["tg"], pb2["ew"], pb2["ev"], pb2["kind"], pb2["ut"], pb2["uw"])
    c = pc.linearize(oracle, pb2, two, jac=False)["cost"]
    assert P.tobytes() == two.tobytes() and s.num_iterations == 0 and s.termination == 0 and c > 0
    assert_parity(s.initial_cost, c, "n = 2"); assert s.final_cost == s.initial_cost
    # sizes outside the interface
    cap = api.pose_chain_capacity()
    n = cap + 3
    big = np.tile(poses[0], (n, 1))
    with pytest.raises(api.LvfError, match="capacity"):
        api.pose_chain_solve(ctx, big, None, np.ones(n - 1), np.ones(n - 1), np.zeros(n, np.int32), np.zeros((n, 4)), np.zeros(n))
    with pytest.raises(api.LvfError):
        api.pose_chain_solve(ctx, poses[:1].copy(), None, np.zeros(0), np.zeros(0), np.zeros(1, np.int32), np.zeros((1, 4)), np.zeros(1))
    with pytest.raises(api.LvfError):
        api.navsat_optimize_ab(ctx, poses[:1].copy(), stamps[:1], fix[:1], relB)
    Z = poses.copy(); Z[2, :4] = 0.0
    with pytest.raises(api.LvfError, match="quaternion"):
        api.navsat_optimize_ab(ctx, Z, stamps, fix, relB)


def test_navsat_optimize_section_composes_on_the_device(ctx, oracle):
    """Navsat::Optimize with the device OptimizeAB against the same composition with the ref's host solve in the middle"""
    from lvio_fusion_amd import api
    nb, m = 30, 12
    bc, has, fixb, cov = nr.chain_section(nb, 7)
    rng = np.random.default_rng(7)
    has = np.concatenate([has, [1]]).astype(np.int32); fixb = np.concatenate([fixb, bc[-1:, 4:7] + rng.normal(0, 0.1, (1, 3))]); cov = np.concatenate([cov, cov[-1:]])
    ab, stamps, fixa, relB = pc.ab_section(oracle, m, 9)
    Tm = oracle.se3_mul(bc[0], oracle.se3_inv(ab[-1]))       # the AB section moved rigidly so that it ends at B
    ab = oracle.forward_update(Tm, ab)[0]
    fixa = np.array([oracle.se3_apply(Tm, p) for p in fixa])
    opt = api.navsat_bc_options(distance=100.0, trust_distance_yaw=10.0, trust_distance_pitch=30.0, z_lower=-100.0, z_upper=100.0)
    refs = []

    def host_ab(arr):
        A = ab_h
        A[-1] = arr.reshape(-1, 7)[0]
        X, s = pc.solve(oracle, pc.navsat_ab(oracle, A, stamps, fixa, relB, opt.huber_a))
        A[:] = X
        refs.append(s)

    ab_h, bc_h = ab.copy(), bc.copy()
    api.navsat_optimize(ctx, bc_h, has, fixb, cov, opt, host_ab)
    ab_d, bc_d = ab.copy(), bc.copy()
    res, s_ab, x, it, summ = api.navsat_optimize_section(ctx, ab_d, stamps, fixa, relB, bc_d, has, fixb, cov, opt)
    assert res.skipped == 0 and len(refs) == 1 and pc.min_margin(refs[0]) >= 1e-6
    assert_summary(s_ab, refs[0], "OptimizeAB inside the section")
    assert bc_d.tobytes() == bc_h.tobytes()
    assert_parity(ab_d, ab_h, "AB poses")
    assert ab_d[-1].tobytes() == bc_d[0].tobytes()          # B as OptimizeBC left it (the per-keyframe chain starts after B)
    assert ab_d[0].tobytes() == ab[0].tobytes() and np.abs(ab_d[1:-1] - ab[1:-1]).max() > 1e-3
