"""CPU checks of tests/edge_ref.py, the declared semantics of the LiDAR edge features: wherever it overlaps the oracle it must reproduce it
(the float transform and search, the factor's rows, the 3-DoF LM), its float64 line fit is measured against a 50-digit solve, and the seeded
scenes of the GPU tests are checked to keep clear of the line test's threshold."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import edge_ref as er


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def test_transform_and_search_match_oracle(oracle):
    """transform_f32 + knn_brute(3) are pyoracle.knn3's exact search: indices, d2 and the gate, bit for bit"""
    rng = np.random.default_rng(3)
    m = np.zeros((1500, 4), np.float32); m[:, :3] = rng.uniform(-5, 5, (1500, 3))
    m[100:200] = m[:100]                                                       # exact duplicates: ties go to the lower index
    q = np.zeros((400, 4), np.float32); q[:, :3] = rng.uniform(-5, 5, (400, 3))
    pose = np.array([0.1, -0.2, 0.3, 0.9, 0.5, -0.4, 0.2]); pose[:4] /= np.linalg.norm(pose[:4])
    i0, d0, v0 = oracle.knn3(m, q, pose, 0.3)
    idx, d2 = er.knn_brute(m, er.transform_f32(pose, q), 3)
    v = np.all(d2 < np.float32(0.3), axis=1)
    assert np.array_equal(v, v0 > 0) and 20 < v.sum() < 400
    assert np.array_equal(idx[v], i0[v]) and np.array_equal(d2[v].view(np.uint32), d0[v].view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_block_is_three_oracle_plane_rows(oracle, mode):
    """row k of the block = the oracle's LidarPlaneError with normal P[k,:] and anchor c (the oracle takes the normal as given)"""
    rng = np.random.default_rng(11 + mode)
    n = 200
    p, c = rng.uniform(-20, 20, (n, 3)), rng.uniform(-20, 20, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    proj = np.stack([er.proj6(P[i]) for i in range(n)])
    Twc1 = np.array([0.2, -0.1, 0.4, 0.8, 3.0, -2.0, 0.7])                    # (raw, not unit: the functor normalises)
    x = np.array([0.3, -0.05, 0.08, 0.7, -0.4, 0.2])
    r, J = er.edge_block(mode, p, c, proj, Twc1, x, 0.37)
    for k in range(3):
        r0, J0 = oracle.lidar_plane(mode, p, c, P[:, k, :], Twc1, x, 0.37)
        assert rel(r[:, k], r0) <= 1e-12 and rel(J[:, k, :], J0) <= 1e-12, (k, rel(r[:, k], r0), rel(J[:, k, :], J0))


def test_lm_with_zero_edges_is_the_oracle_icp_solve(oracle):
    c3 = syn.config3_icp(seed=77, n_query=4000, n_az=260)
    q, m = c3["query"][~c3["query_ground"]][:2000], c3["map"][~c3["map_ground"]]
    assert q.shape[0] == 2000
    rp0 = oracle.se3_to_rpyxyz(oracle.se3_mul(oracle.se3_inv(c3["map_pose"]), c3["pose0"]))
    for prior in (0.0, 3.0):
        x0, s0 = oracle.icp_solve(m, q, c3["map_pose"], c3["pose0"], rp0, 1, c3["thr_surf"], syn.W_LIDAR_SURF, 0.1, prior_w=prior, use_kdtree=False)
        x, s = er.icp_solve_edges(m, q, None, None, c3["map_pose"], c3["pose0"], rp0, c3["thr_surf"], syn.W_LIDAR_SURF, 0.1, prior_w=prior)
        assert s["num_residual_blocks"] == s0["num_residual_blocks"] > 500
        assert s["num_iterations"] == s0["num_iterations"] and s["num_successful_steps"] == s0["num_successful_steps"] and s0["num_successful_steps"] >= 1
        assert rel(x, x0) <= 1e-12 and rel(s["initial_cost"], s0["initial_cost"]) <= 1e-12 and rel(s["final_cost"], s0["final_cost"]) <= 1e-12, \
            (rel(x, x0), rel(s["initial_cost"], s0["initial_cost"]), rel(s["final_cost"], s0["final_cost"]))
        # the SE3 helpers of the chain are the oracle's
        assert rel(er.se3_to_rpyxyz(er.se3_mul(er.se3_inv(c3["map_pose"]), c3["pose0"])), rp0) <= 1e-14
        assert rel(er.se3_mul(c3["map_pose"], er.rpyxyz_to_se3(x)), oracle.se3_mul(c3["map_pose"], oracle.rpyxyz_to_se3(x0))) <= 1e-12


def test_line_fit_error_and_scene_margins():
    """e_ref: the largest entry error of the float64 (c, projector) against the 50-digit solve over every line of the GPU test's scenes; and the
    scenes leave no query within 1e-9 (relative) of the line test's threshold, so the GPU test has nothing to leave out"""
    e_ref, n_lines, n_valid = 0.0, 0, 0
    for name, sc in er.assoc_scenes().items():
        a = er.edge_associate(sc["map"], sc["scan"], sc["pose"], sc["thr"], sc["ratio"])
        g = a["gate"]
        assert not np.any(np.abs(a["margin"][g] - 1.0) <= 1e-9), name
        if name == "m4":
            assert not g.any() and not a["valid"].any()
        else:
            assert a["valid"].sum() >= 3 and (a["valid"] == 0).sum() >= 2, name
        if name in ("dups", "big"):
            assert (g & (a["valid"] == 0)).sum() >= 5, name                     # blobs: inside the gate, not a line
        if name == "dups":
            assert np.any(a["d2_5"][g][:, 1:] == a["d2_5"][g][:, :-1]), "no d2 tie among the neighbours"
        for i in np.nonzero(a["valid"])[0][:150]:
            x5 = sc["map"][a["idx5"][i], :3].astype(np.float64)
            c, P, _ = er.line_fit(x5)
            c_mp, P_mp, l1, l2 = er.line_fit_mp(x5)
            e_ref = max(e_ref, np.abs(c - c_mp).max(), np.abs(P - P_mp).max())
            n_lines += 1
        n_valid += int(a["valid"].sum())
    print(f"e_ref = {e_ref:.3e} over {n_lines} lines ({n_valid} valid queries)")
    assert n_lines >= 200 and e_ref <= er.E_REF


# ----------------------------------------------------------------------------- edge picks
def _taps(oracle, scan, kw):
    T = oracle.lidar_extract_taps(scan, **kw)
    rg, g, rings = er.seg_layout(T["label_mat"], T["ground_mat"], T["range_mat"])
    return T, rg, g, rings


@pytest.mark.parametrize("which", ["scan16", "edited"])
def test_pick_inputs_are_the_oracles(oracle, which):
    """the curvature array, the ground flags and the ring ranges the pick rule reads are the oracle's restatement of CalculateSmoothness /
    ExtractFeatures, bit for bit; and with the default threshold the edge set and the surf set are disjoint"""
    scan, kw = er.scan16() if which == "scan16" else er.edited_scan()
    T, rg, g, rings = _taps(oracle, scan, kw)
    assert np.array_equal(rg.view(np.uint32), T["seg_range"].view(np.uint32)) and np.array_equal(g, T["seg_ground"])
    assert [a for a, _ in rings] == list(T["start_ring"]) and [b for _, b in rings] == list(T["end_ring"])
    c = er.curvature(rg)
    assert np.array_equal(c.view(np.uint32), T["curvature"].view(np.uint32))
    fs, fl, per = er.edge_picks(c, g, rings)
    assert fl.sum() > 50 and fs.sum() > 30 and np.all(fl[fs == 1] == 1)
    # the oracle's surf picks are the points of the sectors with curvature < 1: none of them is an edge pick
    in_sector = np.zeros(len(c), bool)
    for start, end in rings:
        for sp, ep in er.ring_sectors(start, end):
            if sp < ep:
                in_sector[sp:ep + 1] = True
    surf = in_sector & (g == 0) & (c < np.float32(1.0))
    assert surf.sum() == len(T["surf_raw"]) and not np.any(surf & (fl == 1))


def test_edited_scan_has_the_cases(oracle):
    """the third scan of the GPU test: a sector whose two sharpest candidates have bit-equal curvature (the lower index is picked first),
    sectors with fewer candidates than n_sharp, sectors with none"""
    scan, kw = er.edited_scan()
    T, rg, g, rings = _taps(oracle, scan, kw)
    c = er.curvature(rg)
    fs, fl, per = er.edge_picks(c, g, rings, 1.0, 1, 20)
    ties = [(r, j, ls) for r, j, sh, ls in per if len(ls) >= 2 and c[ls[0]].view(np.uint32) == c[ls[1]].view(np.uint32)]
    assert ties and all(ls[0] < ls[1] and ls[1] - ls[0] > 5 and fs[ls[0]] == 1 and fs[ls[1]] == 0 for _, _, ls in ties)
    n_cand = []
    for start, end in rings:
        for sp, ep in er.ring_sectors(start, end):
            if sp < ep:
                n_cand.append(int(((g[sp:ep + 1] == 0) & (c[sp:ep + 1] >= np.float32(1.0))).sum()))
    assert sum(n == 0 for n in n_cand) > 10 and sum(n == 1 for n in n_cand) >= 1          # none; fewer than n_sharp = 2


def test_pick_rule_properties():
    rng = np.random.default_rng(5)
    for trial in range(40):
        m = int(rng.integers(30, 400))
        c = rng.choice([0.0, 0.5, 1.0, 2.0, 3.0, 7.5], m).astype(np.float32) if trial % 2 else rng.gamma(1.0, 1.5, m).astype(np.float32)
        g = (rng.uniform(size=m) < 0.2).astype(np.uint8)
        n_sharp, n_less = int(rng.integers(0, 4)), int(rng.integers(4, 9))
        sh, ls = er.pick_sector(c, g, 3, m - 4, 1.0, n_sharp, n_less)
        assert len(ls) <= n_less and len(sh) <= n_sharp and sh == ls[:len(sh)] and set(sh) <= set(ls)
        assert all(3 <= k <= m - 4 and g[k] == 0 and c[k] >= 1.0 for k in ls)
        assert all(abs(a - b) > 5 for i, a in enumerate(ls) for b in ls[:i])
        # greedy: every pick is the largest (curvature, then lower index) of the candidates no earlier pick suppresses
        for i, k in enumerate(ls):
            free = [q for q in range(3, m - 3) if g[q] == 0 and c[q] >= 1.0 and all(abs(q - p) > 5 for p in ls[:i])]
            assert k == min(free, key=lambda q: (-float(c[q]), q))
        if len(ls) < n_less:      # stopped because no candidate was left
            assert not [q for q in range(3, m - 3) if g[q] == 0 and c[q] >= 1.0 and all(abs(q - p) > 5 for p in ls)]
    # a curvature tie goes to the lower index
    c = np.zeros(40, np.float32); c[[10, 30]] = 4.0
    assert er.pick_sector(c, np.zeros(40, np.uint8), 0, 39, 1.0, 1, 20) == ([10], [10, 30])
    # the +-5 suppression stays inside the sector; a sector with sp >= ep contributes nothing
    c = np.zeros(40, np.float32); c[[18, 20, 26]] = [3.0, 5.0, 2.0]
    assert er.pick_sector(c, np.zeros(40, np.uint8), 19, 39, 1.0, 2, 20) == ([20, 26], [20, 26])
    assert er.pick_sector(c, np.zeros(40, np.uint8), 20, 20, 1.0, 2, 20) == ([], []) and er.pick_sector(c, np.zeros(40, np.uint8), 21, 20, 1.0, 2, 20) == ([], [])
    fs, fl, per = er.edge_picks(c, np.zeros(40, np.uint8), [(4, 34), (34, 34)], 1.0, 2, 20)
    assert fl.sum() == 3 and all(r == 0 for r, _, _, _ in per)                                # sectors are independent: 18 and 20 are 2 apart, in different sectors
