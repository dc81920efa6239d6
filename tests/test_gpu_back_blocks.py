"""The dense back substitution on stored block products, and the landmark / pose workgroups that request their operands before the wait.

a. Block form.  Riders of the block-step launches store T_kj = -Dinv_k L_jk^T; the back substitution then runs x_k = sum_{j > k} T_kj x_j
(DESIGN.md 10.4).  Tested as tests/test_gpu_reduced_solve.py tests the solve — the override tap, the systems of tests/reduced_cases.py, the
same norm and the same bound

    err(S, x_dev, x_star) <= M * max(err64_bound, d * 2^-53),      M = 8

— on both sides of every block count: 3 keyframes (one block: form off), 10 and 11 (two), 22 (three), 32 (four), 50 (five), 16 (sequential
levels beside the block form) and 24 with IMU gaps.  (A dense corner of a multiple of 64 unknowns keeps the S / Dinv form; the plan's cost
function steers away from it — 6 n_kf + 9 kept blocks = 192 k was met by no chain of up to 69 keyframes, nor with up to three IMU gaps
below 45 — so none of these windows has one (asserted); a forced plan, CORNER below, exercises the fall-back.)  The
references are computed once, in this process; the device steps come from child processes (the switches are read once per process):
LVF_BACK_BLOCKS unset, LVF_BACK_BLOCKS=0, LVF_CHOL_SUBBLOCK=0 (the riders of the pair-pivot kernel) and LVF_BACK_PRODUCT=0 (the body that
runs the sequential levels holds the products of three blocks only: 22 keyframes take the block form there, 32 and 50 fall back to S and
Dinv, and their steps meet the same bound).  On against off:
||Ds (x_on - x_off)|| <= 2 M max(err64_bound, d 2^-53) ||Ds x_star|| (triangle inequality through x_star).

b. Landmark pass.  lm_iteration against the oracle (tests/test_gpu_solver.py's comparison) for three iterations at 10 and 50 keyframes: 7
landmarks (less than one workgroup's 32), 300 (no multiple of 32), tracks longer than the register window (p_geom = 0.02, asserted), and a
child with LVF_BACK_TAIL_WGS=3 (300 landmarks in four passes, two of them read after the wait); against LVF_BACK_TAIL_MERGE=0 (two
launches) the states agree to tests/test_gpu_handover.py's same_state (1e-9), the costs to 1e-9 — tests/test_gpu_back_product.py's bound
between two paths that differ in summation order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import reduced_cases as rc

M = 8.0
# (n_kf, n_lm, seed, imu_drop): the windows of tests/test_gpu_reduced_solve.py at these keyframe counts
WINDOWS = [(3, 80, 103, ()), (10, 200, 105, ()), (11, 200, 107, ()), (22, 300, 111, ()), (32, 300, 109, ()), (50, 300, 61, ()),
           (16, 400, 51, ()), (24, 500, 55, (5, 6, 17))]
NB = {3: 1, 10: 2, 11: 2, 22: 3, 32: 4, 50: 5}
# 26 keyframes in four IMU segments of 6 / 7 / 6 / 7: after TWO elimination levels one block of each segment is left, 6 * 26 + 9 * 4 = 192
# dense unknowns — the augmented row has the fourth factor block to itself.  The plan's own choice is three levels (nothing left), hence
# LVF_FORCE_LEVELS=2 in the child.
CORNER = (26, 300, 113, (5, 12, 18))
CASES = ("own", "shift3", "shift6", "dd")
BLOCK_SWITCHES = {"corner": {"LVF_FORCE_LEVELS": "2"}, "on": {}, "off": {"LVF_BACK_BLOCKS": "0"}, "pair_pivot": {"LVF_CHOL_SUBBLOCK": "0"}, "levels": {"LVF_BACK_PRODUCT": "0"}}
# name: (n_kf, n_lm, seed, p_geom)
LM_WINDOWS = {"kf10_lm7": (10, 7, 211, 0.1), "kf50_lm7": (50, 7, 213, 0.1), "kf10_lm300": (10, 300, 215, 0.1), "kf50_lm300": (50, 300, 217, 0.1),
              "kf10_long": (10, 300, 219, 0.02), "kf50_long": (50, 300, 221, 0.02)}
LM_SWITCHES = {"merged": {}, "two_launches": {"LVF_BACK_TAIL_MERGE": "0"}, "three_workgroups": {"LVF_BACK_TAIL_WGS": "3"}}
FIELDS = ("poses", "vel", "ba", "bg", "inv_depth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wid(w):
    return f"kf{w[0]}"


def run_child(mode, env_extra, arg=None):
    env = dict(os.environ)
    for k in ("LVF_BACK_BLOCKS", "LVF_CHOL_SUBBLOCK", "LVF_BACK_TAIL_MERGE", "LVF_BACK_TAIL_WGS", "LVF_BACK_PRODUCT", "LVF_BACK_EARLY", "LVF_FORCE_LEVELS"):
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), mode] + ([arg] if arg else []), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------------------- a. block form
def child_blocks(path):
    """Every window's steps for the systems in `path`, in this process (its environment carries the switch); one JSON line."""
    from lvio_fusion_amd import api
    from oracle import pyoracle
    from tests.test_gpu_reduced_solve import Win
    pyoracle.build()
    ctx = api.Context(0)
    sys_ = np.load(path)
    out = {}
    for w in ([CORNER] if os.environ.get("LVF_FORCE_LEVELS") else WINDOWS):
        win = Win(api, ctx, pyoracle, w)
        r = {"nb": win.nb, "ndense": 6 * w[0] + 9 * int(np.sum(win.dense_kf)), "back_product": win.back_product, "blocks": win.prob.debug_back_blocks(), "x": {}}
        for name in CASES:
            S, b = sys_[f"{wid(w)}_{name}_S"], sys_[f"{wid(w)}_{name}_b"]
            win.prob.debug_override_reduced(S, b)
            try:
                assert win.prob.debug_back_blocks() == r["blocks"], "the override changed the form of the back substitution"
            finally:
                win.prob.debug_clear_override()
            got, x, fail, _ = win.iterate(S, b)
            assert fail == 0 and got["solved"] and np.isfinite(x).all(), f"{wid(w)} {name}: fail flag {fail}"
            r["x"][name] = np.asarray(x, np.float64).tolist()
        out[wid(w)] = r
        win.close()
    ctx.close()
    print(json.dumps(out))


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """{window: {case: (S, b, x_star, floor)}} and the file the children read the systems from; computed once, never modified"""
    from lvio_fusion_amd import api
    from tests.test_gpu_reduced_solve import Win
    ctx = api.Context(0)
    out, arrays = {}, {}
    for w in WINDOWS + [CORNER]:
        win = Win(api, ctx, oracle, w)
        cs = rc.cases(win.S0, win.b0, w[2], CASES)
        out[wid(w)] = {}
        for name in CASES:
            S, b = cs[name]
            x_star, x64 = rc.ref_solve(S, b)
            floor = max(float(rc.err64_bound(S, b, x_star, w[2], x64)), win.d * 2.0 ** -53)
            for a in (S, b, x_star):
                a.setflags(write=False)
            out[wid(w)][name] = (S, b, x_star, floor)
            arrays[f"{wid(w)}_{name}_S"], arrays[f"{wid(w)}_{name}_b"] = S, b
        win.close()
    ctx.close()
    path = str(tmp_path_factory.mktemp("back_blocks") / "systems.npz")
    np.savez(path, **arrays)
    return out, path


_block_runs = {}


def block_run(refs, switch):
    if switch not in _block_runs:
        _block_runs[switch] = run_child("blocks", BLOCK_SWITCHES[switch], refs[1])
    return _block_runs[switch]


@pytest.mark.gpu
def test_a_corner_of_a_multiple_of_64_unknowns_keeps_the_plain_form(refs):
    """The one plan-dependent branch of the choice: row d alone in the last factor block.  Four blocks with the G product on would take the
    block form; this corner must not, and its steps meet the bound."""
    r = block_run(refs, "corner")[wid(CORNER)]
    assert r["ndense"] == 192 and r["nb"] == 4 and r["back_product"] == 1, r["ndense"]
    assert r["blocks"] == 0
    for name in CASES:
        S, b, x_star, floor = refs[0][wid(CORNER)][name]
        e_dev = rc.err(S, np.array(r["x"][name]), x_star)
        print(f"ratio {wid(CORNER)} d={len(b)} {name} corner: err_dev {e_dev:.3e} floor {floor:.3e} ratio {e_dev / floor:.3f}")
        assert e_dev <= M * floor, f"{name}: err {e_dev:.3e} > {M} x {floor:.3e}"


SWITCHES = [k for k in BLOCK_SWITCHES if k != "corner"]


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_which_windows_take_the_block_form(refs, switch):
    """Two blocks or more, whether or not the G product is on (16 keyframes: off); beside the sequential levels two or three blocks."""
    got = block_run(refs, switch)
    for w in WINDOWS:
        r = got[wid(w)]
        if w[0] in NB:
            assert r["nb"] == NB[w[0]], f"{wid(w)}: nb {r['nb']}"
        held = 5 if r["back_product"] else 3      # blocks whose products the body that runs holds in registers
        assert r["blocks"] == (1 if switch != "off" and 2 <= r["nb"] <= held else 0), f"{wid(w)} {switch}: nb {r['nb']}, blocks {r['blocks']}"
    assert got["kf16"]["back_product"] == 0 and got["kf50"]["back_product"] == (0 if switch == "levels" else 1)
    if switch == "levels":
        assert got["kf22"]["blocks"] == 1 and got["kf32"]["blocks"] == 0 and got["kf50"]["blocks"] == 0
    assert all(got[wid(w)]["ndense"] % 64 != 0 for w in WINDOWS), "a dense corner of a multiple of 64 unknowns keeps the S / Dinv form: expect blocks == 0 there"


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("w", WINDOWS, ids=wid)
def test_the_step_is_as_accurate_as_a_float64_cholesky(refs, w, switch):
    got = block_run(refs, switch)[wid(w)]
    for name in CASES:
        S, b, x_star, floor = refs[0][wid(w)][name]
        e_dev = rc.err(S, np.array(got["x"][name]), x_star)
        print(f"ratio {wid(w)} d={len(b)} {name} {switch}: err_dev {e_dev:.3e} floor {floor:.3e} ratio {e_dev / floor:.3f}")
        assert e_dev <= M * floor, f"{wid(w)} {name} {switch}: err {e_dev:.3e} > {M} x {floor:.3e} (ratio {e_dev / floor:.2f})"


@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS, ids=wid)
def test_on_and_off_agree(refs, w):
    on, off = block_run(refs, "on")[wid(w)], block_run(refs, "off")[wid(w)]
    for name in CASES:
        S, b, x_star, floor = refs[0][wid(w)][name]
        ds = np.sqrt(np.abs(np.diag(S)).astype(rc.LD))
        diff = ds * (np.array(on["x"][name]).astype(rc.LD) - np.array(off["x"][name]).astype(rc.LD))
        den = ds * x_star
        rel = float(np.sqrt(diff @ diff) / np.sqrt(den @ den))
        print(f"on/off {wid(w)} {name}: {rel:.3e} (bound {2 * M * floor:.3e})")
        assert rel <= 2.0 * M * floor, f"{wid(w)} {name}: {rel:.3e} > 2 x {M} x {floor:.3e}"


# ---------------------------------------------------------------------------------------------------------------- b. landmark pass
def lm_cfg(name):
    from lvio_fusion_amd import synthetic as syn
    n_kf, n_lm, seed, p_geom = LM_WINDOWS[name]
    return syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=40, seed=seed, imu_samples=5, p_geom=p_geom)


def track_span(cfg):
    """(kmin, kmax) per landmark: the keyframes of its TwoCamera block and of both ends of its TwoFrame blocks"""
    n_lm = cfg["n_lm"]
    kmin, kmax = np.full(n_lm, 10 ** 9), np.full(n_lm, -1)
    for lm, kf in ((cfg["tc"]["lm_idx"], cfg["tc"]["kf_idx"]), (cfg["tf"]["lm_idx"], cfg["tf"]["kf1_idx"]), (cfg["tf"]["lm_idx"], cfg["tf"]["kf2_idx"])):
        np.minimum.at(kmin, np.asarray(lm, int), np.asarray(kf, int))
        np.maximum.at(kmax, np.asarray(lm, int), np.asarray(kf, int))
    return kmin, kmax


def lm_three_iterations(api, ctx, oracle, name):
    """Three lm_iterations of the window beside the oracle's, compared as tests/test_gpu_solver.py compares them; returns costs and states."""
    from tests.helpers import assert_parity
    from tests.test_gpu_solve_trajectory import close, make
    from tests.test_gpu_solver import state_of
    n_kf, n_lm, seed, _ = LM_WINDOWS[name]
    w = make(api, ctx, oracle, n_kf, n_lm, seed, cfg=lm_cfg(name))
    prob, win, opt = w["prob"], w["win"], api.default_solver_options()
    radius, dec, out = 1e4, 2.0, []
    for it in range(3):
        ref = win.lm_iteration(radius, dec)
        got = prob.lm_iteration(opt, radius, dec)
        assert prob.debug_last_solved() and got["accepted"] == ref["accepted"], f"{name} it{it}"
        assert abs(got["cost_before"] - ref["cost_before"]) <= 1e-8 * abs(ref["cost_before"])
        assert abs(got["cost_after"] - ref["cost_after"]) <= 1e-6 * abs(ref["cost_after"])
        assert abs(got["radius"] - ref["radius"]) <= 1e-5 * ref["radius"]
        s = state_of(api, w["st"])
        for k, shape in (("poses", (-1, 7)), ("inv_depth", (-1,)), ("vel", (-1, 3)), ("ba", (-1, 3)), ("bg", (-1, 3))):
            assert_parity(np.asarray(s[k]).reshape(shape), np.asarray(getattr(win, k)).reshape(shape), f"{name}: {k} it{it}")
        out.append({"cost_after": float(got["cost_after"]), "radius": float(got["radius"]), "accepted": bool(got["accepted"]),
                    "state": {k: np.asarray(s[k], np.float64).ravel().tolist() for k in FIELDS}})
        radius, dec = ref["radius"], ref["decrease_factor"]
    close(w)
    return out


def child_landmarks():
    from lvio_fusion_amd import api
    from oracle import pyoracle
    pyoracle.build()
    ctx = api.Context(0)
    out = {name: lm_three_iterations(api, ctx, pyoracle, name) for name in LM_WINDOWS}
    ctx.close()
    print(json.dumps(out))


_lm_runs = {}


def lm_run(switch):
    if switch not in _lm_runs:
        _lm_runs[switch] = run_child("landmarks", LM_SWITCHES[switch])
    return _lm_runs[switch]


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_the_long_tracks_exceed_the_register_window():
    """A lane's window holds the 16 kLmEPre entries from the 16-aligned start of the band: kf50_long has bands that end behind it, and the
    ordinary windows have bands that fit (both sides are run)."""
    from lvio_fusion_amd import api
    window = api.debug_landmark_window()
    assert window > 0 and window % 16 == 0
    beyond = {}
    for name in LM_WINDOWS:
        kmin, kmax = track_span(lm_cfg(name))
        beyond[name] = int(np.sum(6 * (kmax + 1) > ((6 * kmin) & ~15) + window))
    print("window", window, "landmarks whose band ends behind it:", beyond)
    assert beyond["kf50_long"] >= 10 and beyond["kf50_lm300"] < 300 - 10 and beyond["kf10_long"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LM_WINDOWS))
def test_three_iterations_against_the_oracle(ctx, oracle, name):
    from lvio_fusion_amd import api
    lm_three_iterations(api, ctx, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["two_launches", "three_workgroups"])
@pytest.mark.parametrize("name", list(LM_WINDOWS))
def test_the_merged_launch_against_the_other_paths(name, switch):
    """The children compare with the oracle themselves (three_workgroups: 300 landmarks take four passes of 96); here their states against
    the merged launch's at the default grid."""
    from tests.test_gpu_handover import same_state
    a, b = lm_run("merged")[name], lm_run(switch)[name]
    for it, (ra, rb) in enumerate(zip(a, b)):
        assert ra["accepted"] == rb["accepted"], f"{name} it{it}"
        assert abs(ra["cost_after"] - rb["cost_after"]) <= 1e-9 * abs(rb["cost_after"]) and abs(ra["radius"] - rb["radius"]) <= 1e-9 * rb["radius"]
        same_state({k: np.array(v) for k, v in ra["state"].items()}, {k: np.array(v) for k, v in rb["state"].items()})


if __name__ == "__main__":
    if sys.argv[1] == "blocks":
        child_blocks(sys.argv[2])
    else:
        child_landmarks()
