"""The matrices and selections of tests/test_gpu_marginal.py, with their references (tests/marginal_ref.py), built once per process.

Sizes (rest = d - m, m) at every boundary of the device path: nothing eliminated; one unknown; a rest of 63 / 64 / 65 (one block, exactly one,
one and a column); a selection of 64 / 65 (one tile, two) behind 128 / 129; the largest selection, 120, behind 15 * 22 - 120.  Every selection is
scattered over the unknowns and unordered.  Matrices: random SPD of condition 1e2 and 1e10 at every size; the damped reduced systems of small
synthetic windows (2, 3, 11, 24 keyframes; the CPU oracle's iteration at radius 1e4) in the `own`, `graded`, `shift3`, `shift6` families of
reduced_cases.cases; one matrix with absent unknowns among the rest and among the selection."""
import numpy as np

from tests import marginal_ref as mr
from tests import reduced_cases as rc

SIZES = [(0, 1), (1, 6), (63, 15), (64, 15), (65, 15), (128, 64), (129, 65), (15 * 22 - 120, 120)]
CONDS = [1e2, 1e10]
WINDOWS = {2: (40, 31, 15), 3: (80, 103, 30), 11: (200, 107, 15), 24: (500, 55, 120)}      # n_kf: (n_lm, seed, m)
FAMILIES = ("own", "graded", "shift3", "shift6")

RANDOM_IDS = [f"spd-r{r}-m{m}-c{c:.0e}" for (r, m) in SIZES for c in CONDS]
WINDOW_IDS = [f"kf{n}-{f}" for n in WINDOWS for f in FAMILIES] + ["kf24-newest8"]
ABSENT_ID = "spd-absent"
ALL_IDS = RANDOM_IDS + WINDOW_IDS + [ABSENT_ID]

_window_S0 = {}
_cases = {}


def window_system(oracle, n_kf):
    """the damped reduced system of the synthetic window at its start point (CPU oracle, radius 1e4), exactly symmetric"""
    if n_kf not in _window_S0:
        from lvio_fusion_amd import synthetic as syn
        n_lm, seed, _ = WINDOWS[n_kf]
        cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=40, seed=seed, imu_samples=5)
        pre = np.stack([oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
        it = oracle.Window(cfg, pre).lm_iteration(1e4, 2.0)
        S = np.asarray(it["S"], np.float64)
        _window_S0[n_kf] = (np.tril(S) + np.tril(S, -1).T, np.asarray(it["rhs"], np.float64))
    return _window_S0[n_kf]


def _matrix(oracle, cid):
    if cid == ABSENT_ID:
        d, m = 150, 20
        S = mr.random_spd(d, 1e4, 77)
        sel = mr.scattered(d, m, 77)
        rest = [u for u in range(d) if u not in set(sel.tolist())]
        gone = [int(sel[2]), int(sel[11]), rest[1], rest[63], rest[64], rest[-1]]
        S[gone, :] = 0.0; S[:, gone] = 0.0
        return S, sel, 77
    if cid.startswith("spd-"):
        k = RANDOM_IDS.index(cid)
        (r, m), cond = SIZES[k // len(CONDS)], CONDS[k % len(CONDS)]
        return mr.random_spd(r + m, cond, 500 + k), mr.scattered(r + m, m, 500 + k), 500 + k
    n_kf = int(cid[2:cid.index("-")])
    fam = cid[cid.index("-") + 1:]
    n_lm, seed, m = WINDOWS[n_kf]
    S0, b0 = window_system(oracle, n_kf)
    if fam == "newest8":
        return S0, mr.kf_selection(n_kf, list(range(n_kf - 1, n_kf - 9, -1))), seed
    S, _ = rc.cases(S0, b0, seed, (fam,))[fam]
    return S, mr.scattered(15 * n_kf, m, seed), seed


def case(oracle, cid):
    """dict(S, sel, ref, present_sel, e64_info, e64_cov, d): never modified"""
    if cid not in _cases:
        S, sel, seed = _matrix(oracle, cid)
        ref = mr.marginal(S, sel)
        assert ref["fail"] == 0, f"{cid}: the reference cannot factor its matrix (fail {ref['fail']})"
        e_info, e_cov = mr.err64_bound(S, sel, ref, seed)
        S.setflags(write=False); sel.setflags(write=False)
        _, present, _ = mr.layout(S, sel)
        _cases[cid] = dict(S=S, sel=sel, ref=ref, present_sel=present[sel], e64_info=e_info, e64_cov=e_cov, d=S.shape[0])
    return _cases[cid]
