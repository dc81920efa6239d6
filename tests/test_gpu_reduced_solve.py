"""The linear solve of an LM iteration — the (v, ba, bg) elimination levels, the blocked dense Cholesky, the riders that build G and the back
substitution — tested on its own through lvf_problem_debug_override_reduced / lvf_problem_debug_download_step: the production chain is handed
reduced systems with the window's sparsity (tests/reduced_cases.py) and the step it computes is compared with a float64 Cholesky solve
refined in extended precision.

    accuracy    err(S, x_dev, x_star) <= M * max(err64, d * 2^-53),   err = ||Ds (x - x_star)|| / ||Ds x_star||, Ds = sqrt(diag S)

err64 is the float64 Cholesky solve's error taken as a bound, not as one sample: the largest err(S, x64, x_star) over eight float64 solves of
the same system that differ in elimination order only (reduced_cases.err64_bound).  One solve's error is a single draw of a rounding error
of size cond * eps; for the shifted systems it moved between 2.0e-9 and 1.4e-7 from run to run at 32 keyframes (S0 changes in its last bits
with the summation order of the linearisation) while the device's error stayed at 0.95e-7 .. 1.5e-7.

M = 8: the smallest power of two that is at least four times the largest ratio, 1.89 (3 keyframes, shift6, sequential back substitution),
over the 87 window / case / switch figures of one MI355X run of this file (DESIGN.md §17 has the table) — two backward-stable solves of one
system differ by the direction of their rounding errors, hence the factor four.

Failure paths ("failure" = the numerical flag, never a GPU fault): a non-positive, zero or NaN pivot anywhere in the chain must leave an
INVALID step behind — state bit-equal, radius halved, decrease factor untouched, five in a row end a solve — and so must a step whose
model cost change is not positive."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import reduced_cases as rc

M = 8.0

# (n_kf, n_lm, seed, imu_drop): the stage and block edges of test_gpu_chol_subblocks.py; product form off (16); broken IMU chains and
# isolated blocks (24); five levels and ldE > 320 (50); top-level blocks kept dense (140: `own` and `dd` only)
EDGES = [(2, 60, 101, ()), (3, 80, 103, ()), (10, 200, 105, ()), (11, 200, 107, ()), (32, 300, 109, ()), (22, 300, 111, ())]
W16, W24, W50, W140 = (16, 400, 51, ()), (24, 500, 55, (5, 6, 17)), (50, 300, 61, ()), (140, 600, 41, ())
WINDOWS = EDGES + [W16, W24, W50, W140]
SWITCHED = [EDGES[1], EDGES[3], EDGES[4], W24]          # re-run with LVF_CHOL_SUBBLOCK=0 / LVF_BACK_PRODUCT=0, and poisoned
BACK_PRODUCT = {10: 1, 11: 1, 22: 1, 24: 1, 32: 1, 50: 1, 16: 0}
STATE = ("poses", "vel", "ba", "bg", "inv_depth")
RADIUS = 1e4


def wid(w):
    return f"kf{w[0]}"


def case_names(w):
    return ("own", "dd") if w[0] >= 140 else ("own", "graded", "shift3", "shift6", "dd")


def reset(api, st, cfg):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        st.set(field, cfg[key])


class Win:
    """A built window after ONE plain iteration at RADIUS from the start state: (S0, b0) its damped reduced system, x0 its step, `first` the
    iteration's result and `after` the state it left; the cases and their references are computed once and never modified."""

    def __init__(self, api, ctx, oracle, w):
        from tests.test_gpu_solver import build, state_of
        n_kf, n_lm, seed, drop = w
        self.w, self.api = w, api
        self.cfg, self.st, self.b, self.prob, _ = build(api, ctx, oracle, n_kf, n_lm, seed, imu_drop=drop)
        self.opt = api.default_solver_options()
        self.start = state_of(api, self.st)
        self.back_product = self.prob.debug_back_product()
        self.first = self.prob.lm_iteration(self.opt, RADIUS)
        self.first["solved"] = self.prob.debug_last_solved()
        self.nb, self.dense_kf = self.prob.debug_plan()
        self.S0, self.b0 = self.prob.reduced_system()
        self.x0, self.fail0 = self.prob.debug_step()
        self.after = state_of(api, self.st)
        self.d = len(self.b0)
        self._cases = None

    def cases(self):
        if self._cases is None:
            cs = rc.cases(self.S0, self.b0, self.w[2], case_names(self.w))
            out = {}
            for name in case_names(self.w):
                S, b = cs[name]
                x_star, x64 = rc.ref_solve(S, b)
                out[name] = [S, b, x_star, x64, None]
            if "graded" in out:                                  # the exact scaling of own's reference
                self.D = rc.grading(self.d, self.w[2])
                out["graded"][2] = out["own"][2] / self.D.astype(np.longdouble)
            for name, v in out.items():             # the float64 error as a bound over elimination orders (against the FINAL reference)
                v[4] = np.float64(rc.err64_bound(v[0], v[1], v[2], self.w[2], v[3]))
                for a in v[:4]:
                    a.setflags(write=False)
            self._cases = out
        return self._cases

    def iterate(self, S=None, b=None, radius=RADIUS):
        """one iteration from the START state, with (S, b) overridden if given; the override is always cleared again"""
        from tests.test_gpu_solver import state_of
        reset(self.api, self.st, self.cfg)
        if S is not None:
            self.prob.debug_override_reduced(S, b)
        try:
            got = self.prob.lm_iteration(self.opt, radius)
            got["solved"] = self.prob.debug_last_solved()
            x, fail = self.prob.debug_step()
        finally:
            self.prob.debug_clear_override()
        return got, x, fail, state_of(self.api, self.st)

    def accuracy(self):
        """{case: (err_dev, floor, ratio)} and the device steps, printed as the DESIGN table's rows"""
        out, xs = {}, {}
        for name, (S, b, x_star, x64, e64) in self.cases().items():
            got, x, fail, _ = self.iterate(S, b)
            assert fail == 0 and np.isfinite(x).all(), f"{wid(self.w)} {name}: fail flag {fail}"
            e_dev, e64 = rc.err(S, x, x_star), float(e64)
            floor = max(e64, self.d * 2.0 ** -53)
            out[name] = (e_dev, floor, e_dev / floor)
            xs[name] = x
            print(f"ratio {wid(self.w)} d={self.d} {name}: err_dev {e_dev:.3e} err64 {e64:.3e} floor {floor:.3e} ratio {e_dev / floor:.3f}")
        return out, xs

    def close(self):
        self.prob.close()
        for h in list(self.b.values()) + [self.st]:
            if h is not None:
                h.close()


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wins(ctx, oracle):
    from lvio_fusion_amd import api
    built = {}

    def get(w):
        if w not in built:
            built[w] = Win(api, ctx, oracle, w)
        return built[w]
    yield get
    for v in built.values():
        v.close()


def same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in STATE)


# ---------------------------------------------------------------------------------------------------------------- a. the tap is faithful
@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS, ids=wid)
def test_the_tap_reproduces_the_plain_step(wins, w):
    win = wins(w)
    assert win.fail0 == 0 and win.first["solved"]
    win.prob.debug_override_reduced(win.S0, win.b0)
    try:
        assert win.prob.debug_back_product() == win.back_product, "the override changed the back-substitution branch"
    finally:
        win.prob.debug_clear_override()
    if w[0] in BACK_PRODUCT:
        assert win.back_product == BACK_PRODUCT[w[0]]
    got, x, fail, state = win.iterate(win.S0, win.b0)
    assert fail == 0 and got["solved"]
    assert np.abs(x - win.x0).max() <= 1e-9 * np.abs(win.x0).max()       # summation order only
    assert win.prob.debug_back_product() == win.back_product


# ---------------------------------------------------------------------------------------------------------------- b. accuracy
@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS, ids=wid)
def test_the_step_is_as_accurate_as_a_float64_cholesky(wins, w):
    win = wins(w)
    acc, xs = win.accuracy()
    for name, (e_dev, floor, ratio) in acc.items():
        assert e_dev <= M * floor, f"{wid(w)} {name}: err {e_dev:.3e} > {M} x {floor:.3e} (ratio {ratio:.2f})"
    if "graded" in xs:
        assert np.abs(xs["graded"] * win.D - xs["own"]).max() <= 1e-9 * np.abs(xs["own"]).max()


# ---------------------------------------------------------------------------------------------------------------- c. both sweeps, both back substitutions
def child_accuracy():
    """The accuracy ratios of the SWITCHED windows in this process (its environment carries the switch); one JSON line."""
    from lvio_fusion_amd import api
    from oracle import pyoracle
    pyoracle.build()
    ctx = api.Context(0)
    out = {}
    for w in SWITCHED:
        win = Win(api, ctx, pyoracle, w)
        acc, _ = win.accuracy()
        out[wid(w)] = {"back_product": win.back_product, "cases": {k: list(v) for k, v in acc.items()}}
        win.close()
    ctx.close()
    print(json.dumps(out))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["LVF_CHOL_SUBBLOCK", "LVF_BACK_PRODUCT"])
def test_accuracy_of_the_other_sweep_and_the_other_back_substitution(switch):
    """The switches are read once per process, hence a fresh child per switch (one at a time)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env[switch] = "0"
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(switch + "=0\n" + "\n".join(ln for ln in p.stdout.splitlines() if ln.startswith("ratio ")))
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(out) == {wid(w) for w in SWITCHED}
    for name, r in out.items():
        if switch == "LVF_BACK_PRODUCT":
            assert r["back_product"] == 0
        for case, (e_dev, floor, ratio) in r["cases"].items():
            assert e_dev <= M * floor, f"{switch}=0 {name} {case}: err {e_dev:.3e} > {M} x {floor:.3e} (ratio {ratio:.2f})"


# ---------------------------------------------------------------------------------------------------------------- d. a failed factor is an INVALID step
def poisoned_unknowns(n_kf):
    dp = 6 * n_kf
    js = [("v", dp), ("bg", dp + 9 * (n_kf // 2) + 6), ("ba", dp + 9 * (n_kf - 1) + 3), ("pose", 0), ("pose", dp - 1)]
    if n_kf > 11:
        js.append(("pose", 6 * 11))      # keyframe 11: a pivot of the second 64-block (at 11 keyframes that is unknown dp - 1 above)
    return js


@pytest.mark.gpu
@pytest.mark.parametrize("w", SWITCHED, ids=wid)
def test_a_failed_factor_is_an_invalid_step(wins, w):
    from lvio_fusion_amd import api
    k_sparse, k_handover = api.fail_codes()
    win = wins(w)
    n_kf = w[0]
    sparse_seen = 0
    for what, j in poisoned_unknowns(n_kf):
        for kind in ("neg", "zero", "nan"):
            tag = f"{wid(w)} unknown {j} ({what}) {kind}"
            got, x, fail, state = win.iterate(rc.poisoned(win.S0, j, kind), win.b0)
            assert got["solved"] is False and got["accepted"] is False, tag
            assert got["radius"] == 0.5 * RADIUS and got["decrease_factor"] == 2.0, tag
            for k in STATE:
                assert np.array_equal(state[k], win.start[k]) and np.isfinite(state[k]).all(), f"{tag}: {k} changed"
            if what == "pose":                   # no elimination level sees a pose pivot: a block step of the dense corner raises it
                assert 1 <= fail <= win.nb, f"{tag}: fail flag {fail}"
            elif win.dense_kf[(j - 6 * n_kf) // 9]:   # the plan left this keyframe's block in the dense corner (the top of the dissection)
                assert 1 <= fail <= win.nb, f"{tag}: fail flag {fail}"
            else:
                sparse_seen += 1
                # The level that eliminates the poisoned keyframe's block must raise the flag itself: sparse base + keyframe.  The flag is a
                # maximum, and the bad factor spreads into the blocks coupled to it, which fail in later levels under their own keyframes:
                # the flag names the poisoned keyframe or a later one, never a dense block step and never a keyframe before it.
                kf = (j - 6 * n_kf) // 9
                assert k_sparse + kf <= fail < k_sparse + n_kf <= k_handover, f"{tag}: fail flag {fail}, poisoned keyframe {kf}"
    assert sparse_seen >= 3, "no poisoned (v, ba, bg) block of this window went through an elimination level"
    # nothing stale is left behind: the plain iteration again
    got, x, fail, state = win.iterate()
    assert fail == 0 and got["solved"] and got["accepted"] == win.first["accepted"]
    assert abs(got["cost_after"] - win.first["cost_after"]) <= 1e-9 * abs(win.first["cost_after"])
    assert abs(got["radius"] - win.first["radius"]) <= 1e-9 * win.first["radius"]
    for k in STATE:
        assert np.abs(state[k] - win.after[k]).max() <= 1e-9 * np.abs(win.after[k]).max(), k
    assert np.abs(x - win.x0).max() <= 1e-9 * np.abs(win.x0).max()


# ---------------------------------------------------------------------------------------------------------------- e. model <= 0 is INVALID too
@pytest.mark.gpu
@pytest.mark.parametrize("w", SWITCHED, ids=wid)
def test_a_step_against_the_gradient_is_an_invalid_step(wins, w):
    """(S0, -b0): the step is -x0, and the model cost change — formed on device from the problem's own gradient and blocks, not from the
    overridden system — is negative."""
    win = wins(w)
    assert win.b0 @ win.x0 > 0.0
    got, x, fail, state = win.iterate(win.S0, -win.b0)
    assert fail == 0 and got["solved"] is True
    assert np.abs(x + win.x0).max() <= 1e-9 * np.abs(win.x0).max()
    assert got["solved"] is True and got["accepted"] is False
    assert got["radius"] == 0.5 * RADIUS and got["decrease_factor"] == 2.0
    assert same_state(state, win.start)


# ---------------------------------------------------------------------------------------------------------------- f. five invalid steps end a solve
@pytest.mark.gpu
def test_five_invalid_steps_end_a_solve(wins):
    """oracle/lm.h lm_solve: every invalid step counts as an iteration and halves the radius; the fifth in a row is a FAILURE"""
    from lvio_fusion_amd import api
    from tests.test_gpu_solver import state_of
    win = wins(EDGES[3])
    opt = api.default_solver_options()
    opt.max_num_iterations = 20
    reset(api, win.st, win.cfg)
    win.prob.debug_override_reduced(rc.poisoned(win.S0, 0, "neg"), win.b0)
    try:
        s = win.prob.solve(opt)
        x, fail = win.prob.debug_step()
    finally:
        win.prob.debug_clear_override()
    assert fail != 0
    assert (s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps) == (5, 0, 5)
    assert s.why == "consecutive_invalid_steps" and s.termination == 2
    assert s.final_cost == s.initial_cost and np.isfinite(s.final_cost)
    assert same_state(state_of(api, win.st), win.start)
    # and the next plain solve of the window is the one it always was
    reset(api, win.st, win.cfg)
    opt.max_num_iterations = 1; opt.function_tolerance = 0.0; opt.parameter_tolerance = 0.0; opt.gradient_tolerance = 0.0
    s1 = win.prob.solve(opt)
    assert s1.num_successful_steps == 1 and abs(s1.final_cost - win.first["cost_after"]) <= 1e-9 * abs(s1.final_cost)


# ---------------------------------------------------------------------------------------------------------------- g. error paths, and the chain without an override
@pytest.mark.gpu
def test_error_paths(ctx, oracle):
    from lvio_fusion_amd import api
    from tests.test_gpu_solver import build
    cfg, st, b, prob, _ = build(api, ctx, oracle, 2, 40, 31)
    try:
        with pytest.raises(api.LvfError, match="no iteration yet"):
            prob.debug_step()
        d = 15 * 2
        S, rhs = np.eye(d), np.ones(d)
        with pytest.raises(ValueError):
            prob.debug_override_reduced(np.eye(d + 1), np.ones(d + 1))
        with pytest.raises(ValueError):
            prob.debug_override_reduced(S, np.ones(d - 1))
        with pytest.raises(api.LvfError):
            prob.debug_override_reduced(S, None)
        with pytest.raises(api.LvfError):
            prob.debug_override_reduced(None, rhs)
        prob.debug_clear_override(); prob.debug_clear_override()           # nothing set, twice
        opt = api.default_solver_options()
        prob.debug_override_reduced(S, rhs)
        batch = api.ProblemBatch(ctx, [prob])
        try:
            with pytest.raises(api.LvfError, match="overridden"):
                batch.lm_iteration(opt, [RADIUS], [2.0])
            with pytest.raises(api.LvfError, match="overridden"):
                batch.solve(opt)
            prob.debug_clear_override(); prob.debug_clear_override()
            r = batch.lm_iteration(opt, [RADIUS], [2.0])                   # the batch works again
            assert np.isfinite(r[0]["cost_after"])
        finally:
            batch.close()
    finally:
        prob.close()
        for h in list(b.values()) + [st]:
            if h is not None:
                h.close()


@pytest.mark.gpu
def test_the_chain_is_the_same_after_an_override_was_set_and_cleared(wins):
    win = wins(W50)
    reset(win.api, win.st, win.cfg)
    before = [(n, la) for n, _, la in win.prob.stage_times(win.opt, RADIUS, reps=2)]
    win.iterate(win.S0, win.b0)
    reset(win.api, win.st, win.cfg)
    after = [(n, la) for n, _, la in win.prob.stage_times(win.opt, RADIUS, reps=2)]
    assert before == after and sum(la for _, la in before) > 0


if __name__ == "__main__":
    child_accuracy()
