"""Inputs that put BOTH branches of the Huber loss into one linearisation (tests/test_gpu_robust_loss.py), with the census that proves it
(tests/test_robust_cases.py).  numpy and the oracle only, no GPU.

The synthetic windows start with every visual residual norm far above the default huber_a = 1 (all linear); the LiDAR scenes keep
|r| <= weight * gate = 0.01 under huber_a = 0.1 (all quadratic).  Here the threshold is taken from the residuals themselves: pick_a() puts it
in the widest gap between consecutive sorted norms of the middle quantile band, so about half of the blocks sit on either side and none sits
within the returned relative margin of it.  One accepted LM step shrinks the norms below any threshold chosen before it, hence one threshold
per iteration (ladder()) for the per-iteration parity, and for whole solves the median norm at the state the default solve converges to
(a_fix()): such a solve starts all linear and ends mixed."""
import numpy as np

from lvio_fusion_amd import synthetic as syn
from tests import edge_ref as er
from tests.helpers import ocam

KINDS = ("tc", "tf", "po")
ALL = ("tc", "tf", "po", "imu")

# name -> (n_kf, n_lm, seed, use, TwoFrame blocks permuted): the shapes of test_gpu_solver.test_lm_iteration_parity that reach the sorted
# TwoFrame body, TwoCamera-only landmarks, the window without IMU factors, the pose-only window and the 2-keyframe window; `perm` is
# test_unsorted_two_frame_uses_generic_path's window (its blocks shuffled: the generic TwoFrame body).  Two seeds differ from those tests':
# with (8, 120, 3) and (7, 90, 41) only 3.3 % and 2.2 % of the TwoCamera blocks are linear at the first threshold (TwoCamera residuals
# depend on the inverse depths alone and start small), short of the census' 5 %; seeds 4 and 42 are the next ones up that meet it at every
# step (7.5 % and 7.8 % at the worst).
WINDOWS = {"kf8": (8, 120, 4, ALL, False), "kf6_noimu": (6, 80, 7, ("tc", "tf", "po"), False), "kf2": (2, 40, 31, ALL, False),
           "kf5_po": (5, 0, 9, ("po", "imu"), False), "perm": (7, 90, 42, ALL, True)}
LADDER_STEPS = 4                                     # test_lm_iteration_parity's four iterations
SOLVES = [(5, 120, 33), (8, 120, 3)]                 # n_kf, n_lm, seed of the whole solves (test_device_loop_equals_oracle_chain's smallest, and kf8)
_memo = {}


def window(name):
    """(cfg, use) — the cfg test_gpu_solver.build() generates for the same numbers, so a device problem built there is this window"""
    if ("cfg", name) not in _memo:
        n_kf, n_lm, seed, use, perm = WINDOWS[name]
        if perm:
            cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=20, seed=seed, imu_samples=4)
            p = np.random.default_rng(0).permutation(len(cfg["tf"]["lm_idx"]))
            cfg = dict(cfg); cfg["tf"] = {k: v[p] for k, v in cfg["tf"].items()}
        else:
            cfg = syn.config4_window(n_kf=n_kf, n_lm=max(n_lm, 1), n_prewindow=40, seed=seed, imu_samples=5)
        _memo["cfg", name] = (cfg, use)
    return _memo["cfg", name]


def solve_window(spec):
    """the cfg test_gpu_solve_trajectory.make() generates for (n_kf, n_lm, seed)"""
    if ("solve_cfg", spec) not in _memo:
        _memo["solve_cfg", spec] = syn.config4_window(n_kf=spec[0], n_lm=spec[1], n_prewindow=40, seed=spec[2], imu_samples=5)
    return _memo["solve_cfg", spec]


def preint(oracle, cfg):
    return np.stack([oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])


def state_of(x):
    """[poses, vel, ba, bg, inv_depth] copies of a cfg dict or an oracle.Window"""
    get = (lambda k: x[k]) if isinstance(x, dict) else (lambda k: getattr(x, k))
    return [np.array(get(k), dtype=np.float64) for k in ("poses", "vel", "ba", "bg", "inv_depth")]


def norms(oracle, cfg, state, use=ALL):
    """{kind: sqrt(r . r) per block} of the visual kinds in `use`, from the oracle's per-factor residuals at `state`"""
    poses, _, _, _, rho_l = state
    c0, c1 = ocam(oracle, cfg["cam0"]), ocam(oracle, cfg["cam1"])
    tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
    out = {}
    if "tc" in use:
        out["tc"] = oracle.two_camera(tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"], rho_l, cfg["w_kf"], c0, c1)[0]
    if "tf" in use:
        out["tf"] = oracle.two_frame(tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"], rho_l, poses, cfg["w_kf"], c0, c1)[0]
    if "po" in use:
        out["po"] = oracle.pose_only(po["ob"], po["kf_idx"], po["pw_idx"], po["pw"], poses, cfg["w_kf"], c0)[0]
    return {k: np.sqrt((np.asarray(r, np.float64).reshape(len(r), -1) ** 2).sum(axis=1)) for k, r in out.items()}


def shares(nrm, a):
    """fraction of the blocks in the LINEAR branch (s > a^2) per kind and over all of them (`all`); a <= 0 is the trivial loss"""
    lin = {k: (v > a) if a > 0 else np.zeros(len(v), bool) for k, v in nrm.items()}
    out = {k: float(v.mean()) if len(v) else 0.0 for k, v in lin.items()}
    out["all"] = float(np.concatenate(list(lin.values())).mean())
    return out


def pick_a(nrm, lo=0.4, hi=0.6):
    """(a, margin): a = the midpoint of the widest gap between consecutive sorted norms (all kinds together) within the quantile band
    [lo, hi]; margin = the distance from a to the nearest norm, relative to a"""
    v = np.sort(np.concatenate([np.ravel(x) for x in nrm.values()]) if isinstance(nrm, dict) else np.ravel(nrm))
    i0, i1 = int(np.floor(lo * (len(v) - 1))), int(np.ceil(hi * (len(v) - 1)))
    assert i1 > i0, "too few blocks for a band"
    gaps = np.diff(v[i0:i1 + 1])
    j = i0 + int(np.argmax(gaps))
    a = 0.5 * (v[j] + v[j + 1])
    return float(a), float(0.5 * (v[j + 1] - v[j]) / a)


def ladder(oracle, name, steps=LADDER_STEPS):
    """The per-iteration thresholds of window `name`: a list of dict(a, margin, shares, counts, state, radius, dec) — a_k = pick_a at the state
    the oracle is in before iteration k, having taken iterations 0 .. k-1 at a_0 .. a_{k-1} from radius 1e4 (each a one-iteration solve, as
    Problem.lm_iteration is)."""
    if ("ladder", name, steps) not in _memo:
        cfg, use = window(name)
        win = oracle.Window(cfg, preint(oracle, cfg), use=use)
        radius, dec, out = 1e4, 2.0, []
        for _ in range(steps):
            st = state_of(win)
            n = norms(oracle, cfg, st, use)
            a, margin = pick_a(n)
            out.append(dict(a=a, margin=margin, shares=shares(n, a), counts={k: len(v) for k, v in n.items()}, state=st, radius=radius, dec=dec))
            ref = win.lm_iteration(radius, dec, huber_a=a)
            radius, dec = ref["radius"], ref["decrease_factor"]
        _memo["ladder", name, steps] = out
    return _memo["ladder", name, steps]


def a_fix(oracle, spec):
    """dict(a, start, end, ref): a = the median visual norm at the state the oracle's solve with its default options ends in; start / end =
    the linear shares at that a at the initial state and at the state the solve WITH a ends in; ref = that second solve's summary"""
    if ("a_fix", spec) not in _memo:
        cfg = solve_window(spec)
        w = oracle.Window(cfg, preint(oracle, cfg))
        w.solve()
        a = float(np.median(np.concatenate(list(norms(oracle, cfg, state_of(w)).values()))))
        _memo["a_fix", spec] = dict(a=a, **solve_census(oracle, spec, a))
    return _memo["a_fix", spec]


def solve_census(oracle, spec, a):
    """dict(start, end, ref) of the oracle's solve of solve_window(spec) with huber_a = a and otherwise default options"""
    if ("solve_census", spec, a) not in _memo:
        cfg = solve_window(spec)
        w = oracle.Window(cfg, preint(oracle, cfg))
        start = shares(norms(oracle, cfg, state_of(w)), a)
        ref = w.solve(huber_a=a)
        _memo["solve_census", spec, a] = dict(start=start, end=shares(norms(oracle, cfg, state_of(w)), a), ref=ref)
    return _memo["solve_census", spec, a]


def batch_thresholds(oracle):
    """(a_solve, a_step): a batch call takes ONE huber_a for all its windows — a_fix of SOLVES[0] for the solves, and pick_a at SOLVES[0]'s
    initial state for the single iteration (test_robust_cases.py asserts the census of the other window under them)"""
    cfg = solve_window(SOLVES[0])
    return a_fix(oracle, SOLVES[0])["a"], pick_a(norms(oracle, cfg, state_of(cfg)))[0]


# ----------------------------------------------------------------------------- LiDAR
def icp_scene():
    """config3_icp with test_gpu_icp's 6 000-point subset of the scan: (c, query, query_ground)"""
    if "icp" not in _memo:
        c = syn.config3_icp()
        sel = np.sort(np.random.default_rng(1).choice(c["query"].shape[0], 6000, replace=False))
        _memo["icp"] = (c, c["query"][sel], c["query_ground"][sel])
    return _memo["icp"]


def icp_surf(oracle):
    """dict(mm, qq, thr, w, rpyxyz0, r, a): the surf sub-problem (mode 1) of icp_scene(), its residuals r at rpyxyz0 (association at pose0 with
    oracle.knn3, as icp_solve associates), and a = median |r|"""
    if "icp_surf" not in _memo:
        c, q, qg = icp_scene()
        qq, mm = q[~qg], c["map"][~c["map_ground"]]
        thr, w = c["thr_surf"], syn.W_LIDAR_SURF
        rp0 = oracle.se3_to_rpyxyz(oracle.se3_mul(oracle.se3_inv(c["map_pose"]), c["pose0"]))
        idx, _, valid = oracle.knn3(mm, qq, c["pose0"], thr)
        v = valid > 0
        p = qq[v, :3].astype(np.float64); pa, pb, pc = (mm[idx[v, k], :3].astype(np.float64) for k in range(3))
        nrm = oracle.plane_normals(pa, pb, pc)
        r, _ = oracle.lidar_plane(1, p, pa, nrm, c["map_pose"], rp0, w)
        r = np.abs(np.asarray(r, np.float64).ravel())
        _memo["icp_surf"] = dict(c=c, mm=mm, qq=qq, thr=thr, w=w, rpyxyz0=rp0, r=r, a=float(np.median(r)), p=p, pa=pa, n=nrm)
    return _memo["icp_surf"]


EDGE_RES = 0.2
EDGE_THR_SURF = float(np.float32(EDGE_RES * EDGE_RES * 25.0))
EDGE_W_SURF = float(np.float32(0.01))


def edge_scene():
    """dict(s, r_plane, r_edge, a_plane, a_edge): test_icp_solve_edges_parity's largest scene (300 planes, 257 lines), the norms of its plane and
    line residuals at rpyxyz0 through tests/edge_ref.py, and their medians"""
    if "edge" not in _memo:
        s = er.solve_scene(seed=21, n_surf=300, n_edge=257)
        ed = er.edge_defaults(EDGE_RES)
        p, a, n = er.plane_correspondences(s["map_surf"], s["scan_surf"], s["pose0"], EDGE_THR_SURF)
        rp = np.abs(er.plane_rows(1, p, a, n, s["map_pose"], s["rpyxyz0"], EDGE_W_SURF)[0])
        e = er.edge_associate(s["map_edge"], s["scan_edge"], s["pose0"], ed["thr"], ed["min_eigen_ratio"])
        v = e["valid"] > 0
        re_ = er.edge_block(1, np.asarray(s["scan_edge"], np.float32)[v, :3].astype(np.float64), e["c"][v], e["proj"][v], s["map_pose"], s["rpyxyz0"], ed["weight"])[0]
        re_ = np.sqrt((re_ * re_).sum(axis=1))
        _memo["edge"] = dict(s=s, r_plane=rp, r_edge=re_, a_plane=float(np.median(rp)), a_edge=float(np.median(re_)))
    return _memo["edge"]
