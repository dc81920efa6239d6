"""GPU parity of the LiDAR edge features against their declared semantics, tests/edge_ref.py (pinned on the CPU by
test_edge_ref.py): the 5-NN line association (integers and the centroid bit for bit), the point-to-line factor, the (yaw, x, y) solve over
planes and lines, and the frame update."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_ref as er

pytestmark = pytest.mark.gpu

RES = 0.2
THR_SURF = float(np.float32(RES * RES * 25.0))
W_SURF = float(np.float32(0.01))


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    return er.assoc_scenes()


def relerr(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


# ----------------------------------------------------------------------------- association
@pytest.mark.parametrize("name", ["m4", "m5", "dups", "big"])
def test_edge_associate(ctx, scenes, name):
    from lvio_fusion_amd import api, _lib
    sc = scenes[name]
    ref = er.edge_associate(sc["map"], sc["scan"], sc["pose"], sc["thr"], sc["ratio"])
    mp, sn = api.Map(ctx, sc["map"], sc["thr"]), api.Scan(ctx, sc["scan"])
    if name == "big":      # the search must cross pyramid levels here
        Q = sc["scan"].shape[0]
        stats = np.zeros((Q, 4), np.int32); lv = np.zeros((8, 4), np.float32); nl = C.c_int(0)
        pose = np.ascontiguousarray(sc["pose"], np.float64)
        api._chk(ctx.L.lvf_knn3_debug_stats(mp.h, sn.h, pose.ctypes.data_as(_lib.c_double_p), float(sc["thr"]), stats.ctypes.data_as(_lib.c_int_p),
                                            lv.ctypes.data_as(_lib.c_float_p), C.byref(nl)))
        assert nl.value >= 2, nl.value
    api.edge_associate(mp, sn, sc["pose"], sc["thr"], sc["ratio"])
    idx, d2, valid, p, c, proj = sn.download_edges()
    near = np.abs(ref["margin"] - 1.0) <= 1e-9                                  # the line test's rounding may decide these: left out of `valid`
    assert near.sum() <= 0.01 * len(near)
    keep = ~near
    assert np.array_equal(valid[keep], ref["valid"][keep])
    v = (ref["valid"] > 0) & keep
    if name == "m4":
        assert not valid.any()
    else:
        assert v.sum() >= 3
    assert np.array_equal(idx[v], ref["idx5"][v])
    assert np.array_equal(d2[v].view(np.uint32), ref["d2_5"][v].view(np.uint32))
    assert np.array_equal(c[v].view(np.uint64), ref["c"][v].view(np.uint64))                    # the centroid bit for bit
    assert np.array_equal(p[v], sc["scan"][v, :3].astype(np.float64))
    e = np.abs(proj[v] - ref["proj"][v]).max() if v.any() else 0.0
    print(f"{name}: {int(v.sum())} lines of {len(v)} queries, max projector entry error {e:.3e}")
    assert e <= max(1e-13, 8 * er.E_REF)
    assert not np.any(p[valid == 0]) and not np.any(c[valid == 0]) and not np.any(proj[valid == 0])      # an invalid point's record reads zero
    # the plane association of the same scan is untouched by the line association
    api.knn3(mp, sn, sc["pose"], sc["thr"])
    i3, d3, _ = sn.download()
    r3, rd3 = er.knn_brute(sc["map"], er.transform_f32(sc["pose"], sc["scan"]), 3)
    ok3 = np.all((r3 >= 0) & (rd3 < np.float32(sc["thr"])), axis=1)
    assert np.array_equal(i3[ok3], r3[ok3])
    idx_b = sn.download_edges()[0]
    assert np.array_equal(idx_b, idx)
    mp.close(); sn.close()


def test_line_association_starts_with_the_plane_association(ctx, scenes):
    """The two associations are one search with lists of three and of five: on the same (map, scan) the five neighbours begin with the three,
    indices and d2 bit for bit, and both are the brute-force lists.  300 points in [-2, 2]^3 on a 1 m grid, 41 of them one point (a cell
    longer than the cooperative scan's threshold, with 40-fold d2 ties), 37 queries (surplus groups in the one workgroup), no gate."""
    from lvio_fusion_amd import api
    rng = np.random.default_rng(518)
    m = np.zeros((300, 4), np.float32); m[:, :3] = rng.uniform(-2, 2, (300, 3))
    m[100:140] = m[7]
    pose = scenes["m5"]["pose"]
    q = rng.uniform(-3, 3, (37, 3))
    q[0] = (m[7, :3].astype(np.float64) - pose[4:]) @ er.rotmat(pose[:4])          # the duplicated point through the inverse pose
    q = er._pad(q)
    lo = m[:, :3].min(0)
    cell = np.floor((m[:, :3] - lo) / np.float32(1.0)).astype(int)
    assert (cell == cell[7]).all(1).sum() > 12                                     # kLongRange: the whole group scans this cell
    r5, rd5 = er.knn_brute(m, er.transform_f32(pose, q), 5)
    assert (r5 >= 0).all() and list(r5[0]) == [7, 100, 101, 102, 103] and len(set(rd5[0].view(np.uint32))) == 1
    mp, sn = api.Map(ctx, m, 4.0), api.Scan(ctx, q)
    api.knn3(mp, sn, pose, np.inf)
    i3, d3, v3 = sn.download()
    api.edge_associate(mp, sn, pose, np.inf, 3.0)
    i5, d5 = sn.download_edges()[:2]
    mp.close(); sn.close()
    assert v3.all()
    assert np.array_equal(i5[:, :3], i3) and np.array_equal(d5[:, :3].view(np.uint32), d3.view(np.uint32))
    assert np.array_equal(i5, r5) and np.array_equal(d5.view(np.uint32), rd5.view(np.uint32))
    assert np.array_equal(i3, r5[:, :3]) and np.array_equal(d3.view(np.uint32), rd5[:, :3].view(np.uint32))


# ----------------------------------------------------------------------------- factor
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_lidar_edge_evaluate(ctx, mode, n):
    from lvio_fusion_amd import api
    rng = np.random.default_rng(100 * mode + n)
    p, c = rng.uniform(-30, 30, (n, 3)), rng.uniform(-30, 30, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    proj = np.stack([er.proj6(P[i]) for i in range(n)])
    Twc1 = np.array([0.2, -0.1, 0.4, 0.8, 3.0, -2.0, 0.7])
    x = np.array([0.3, -0.05, 0.08, 0.7, -0.4, 0.2])
    r0, J0 = er.edge_block(mode, p, c, proj, Twc1, x, 0.37)
    r, J = api.lidar_edge_evaluate(ctx, mode, p, c, proj, Twc1, x, 0.37)
    assert relerr(r, r0) <= 1e-6 and relerr(J, J0) <= 1e-6, (relerr(r, r0), relerr(J, J0))
    r2, J2 = api.lidar_edge_evaluate(ctx, mode, p, c, proj, Twc1, x, 0.37, jacobians=False)
    assert J2 is None and np.array_equal(r2, r)


# ----------------------------------------------------------------------------- solve
def _solve_both(ctx, s, use_surf, use_edge, prior=0.0, edge_kw=None):
    """(device rpyxyz, device summary, reference rpyxyz, reference summary) of one sub-problem of scene s"""
    from lvio_fusion_amd import api
    edge = er.edge_defaults(RES)
    edge.update(edge_kw or {})
    eo = api.edge_icp_options(RES, **(edge_kw or {}))
    assert (eo.thr, eo.weight, eo.huber_a, eo.min_eigen_ratio) == (np.float32(edge["thr"]), edge["weight"], edge["huber_a"], edge["min_eigen_ratio"])
    ms = api.Map(ctx, s["map_surf"], THR_SURF) if use_surf else None
    ss = api.Scan(ctx, s["scan_surf"]) if use_surf else None
    me = api.Map(ctx, s["map_edge"], edge["thr"]) if use_edge else None
    se = api.Scan(ctx, s["scan_edge"]) if use_edge else None
    x = s["rpyxyz0"].copy()
    summ = api.icp_solve_edges(ms, ss, me, se, s["map_pose"], s["pose0"], x, THR_SURF, W_SURF, 0.1, eo if use_edge else None, prior_weight=prior)
    x_ref, ref = er.icp_solve_edges(s["map_surf"] if use_surf else None, s["scan_surf"], s["map_edge"] if use_edge else None, s["scan_edge"],
                                    s["map_pose"], s["pose0"], s["rpyxyz0"], THR_SURF, W_SURF, 0.1, edge, prior_w=prior)
    for h in (ms, ss, me, se):
        if h is not None:
            h.close()
    return x, summ, x_ref, ref


def _assert_parity(x, summ, x_ref, ref, x0):
    print(f"blocks {summ.num_residual_blocks}, iterations {summ.num_iterations} / {summ.num_successful_steps}, cost {summ.initial_cost:.6e} -> {summ.final_cost:.6e}, "
          f"|dx| {np.abs(x - x_ref).max():.2e}")
    assert summ.num_residual_blocks == ref["num_residual_blocks"]
    assert summ.num_iterations == ref["num_iterations"] and summ.num_successful_steps == ref["num_successful_steps"]
    assert abs(summ.initial_cost - ref["initial_cost"]) <= 1e-6 * abs(ref["initial_cost"])
    assert abs(summ.final_cost - ref["final_cost"]) <= 1e-6 * abs(ref["final_cost"])
    assert np.all(np.abs(x - x_ref) <= 1e-6 * np.abs(x_ref))
    assert np.array_equal(x[[1, 2, 5]], x0[[1, 2, 5]])                       # only (yaw, x, y) move


@pytest.mark.parametrize("case,n_surf,n_edge,prior", [("planes", 400, 0, 0.0), ("lines", 0, 200, 0.0), ("both-1", 300, 1, 0.0), ("both-255", 300, 255, 0.0),
                                                     ("both-257", 300, 257, 0.0), ("both-257-prior", 300, 257, 0.05)])
def test_icp_solve_edges_parity(ctx, case, n_surf, n_edge, prior):
    s = er.solve_scene(seed=21, n_surf=max(n_surf, 1), n_edge=n_edge)
    x, summ, x_ref, ref = _solve_both(ctx, s, n_surf > 0, n_edge > 0, prior)
    _assert_parity(x, summ, x_ref, ref, s["rpyxyz0"])
    assert summ.num_residual_blocks == n_surf + n_edge + (1 if prior > 0 else 0)         # every scan point of the scene finds its plane / its line
    assert summ.num_successful_steps >= 1 and summ.final_cost < summ.initial_cost


def test_icp_solve_edges_no_valid_line_with_prior(ctx):
    s = er.solve_scene(seed=22, n_surf=300, n_edge=40, far_edges=True)
    x, summ, x_ref, ref = _solve_both(ctx, s, True, True, prior=0.05)
    _assert_parity(x, summ, x_ref, ref, s["rpyxyz0"])
    assert summ.num_residual_blocks == 300 + 1
    # and with no plane either: the prior alone holds the pose
    x, summ, x_ref, ref = _solve_both(ctx, s, False, True, prior=0.05)
    assert summ.num_residual_blocks == ref["num_residual_blocks"] == 1 and summ.num_iterations == ref["num_iterations"]
    assert np.array_equal(x, s["rpyxyz0"]) and summ.final_cost == 0.0


def test_icp_solve_edges_without_edges_is_icp_solve(ctx):
    from lvio_fusion_amd import api
    s = er.solve_scene(seed=23, n_surf=400, n_edge=0)
    out = []
    for call in ("edges", "plain"):
        mp, sn = api.Map(ctx, s["map_surf"], THR_SURF), api.Scan(ctx, s["scan_surf"])
        x = s["rpyxyz0"].copy()
        if call == "edges":
            r = api.icp_solve_edges(mp, sn, None, None, s["map_pose"], s["pose0"], x, THR_SURF, W_SURF, 0.1, None, prior_weight=1.5)
        else:
            r = api.icp_solve(mp, sn, s["map_pose"], s["pose0"], x, 1, THR_SURF, W_SURF, 0.1, prior_weight=1.5)
        out.append((x, bytes(r)))
        mp.close(); sn.close()
    assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64)) and out[0][1] == out[1][1]


def test_lines_constrain_the_motion_along_a_wall(ctx):
    """a ground plane, ONE wall and four poles, the frame displaced along the wall: the planes leave that direction free, the poles do not"""
    s = er.solve_scene(seed=24, n_surf=400, n_edge=120, canyon=True)
    along = np.array([1.0, 0.0, 0.0])                                          # the wall y = 4 runs along the world's x
    err = {}
    for name, use_edge in (("planes", False), ("planes+lines", True)):
        x, summ, _, _ = _solve_both(ctx, s, True, use_edge)
        pose = er.se3_mul(s["map_pose"], er.rpyxyz_to_se3(x))
        err[name] = abs((pose[4:] - s["pose_true"][4:]) @ along)
    e0 = abs((s["pose0"][4:] - s["pose_true"][4:]) @ along)
    print(f"error along the wall: start {e0:.4f} m, planes {err['planes']:.4f} m, planes + lines {err['planes+lines']:.4f} m")
    assert err["planes+lines"] < err["planes"]


# ----------------------------------------------------------------------------- frame update
@pytest.mark.parametrize("outer", [1, 4])
def test_scan_match_edges_without_edges_is_scan_match(ctx, outer):
    from lvio_fusion_amd import api
    s = er.solve_scene(seed=25, n_surf=400, n_edge=0, n_ground=400)
    opt = api.scan_match_options(RES, outer_iterations=outer, prior_weight=0.0 if outer == 4 else 0.05)
    out = []
    for call in ("edges", "plain"):
        mg, sg = api.Map(ctx, s["map_ground"], opt.thr_ground), api.Scan(ctx, s["scan_ground"])
        ms, ss = api.Map(ctx, s["map_surf"], opt.thr_surf), api.Scan(ctx, s["scan_surf"])
        if call == "edges":
            r = api.scan_match_edges(mg, sg, ms, ss, None, None, s["map_pose"], s["pose0"], opt, None, last_pose=s["map_pose"])
        else:
            r = api.scan_match(mg, sg, ms, ss, s["map_pose"], s["pose0"], opt, last_pose=s["map_pose"])
        out.append(bytes(r))
        for h in (mg, sg, ms, ss):
            h.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("outer,prior", [(1, 0.05), (2, 0.0)])
def test_scan_match_edges_parity(ctx, outer, prior):
    from lvio_fusion_amd import api
    s = er.solve_scene(seed=26, n_surf=400, n_edge=150, n_ground=400)
    opt = api.scan_match_options(RES, outer_iterations=outer, prior_weight=prior)
    eo = api.edge_icp_options(RES)
    mg, sg = api.Map(ctx, s["map_ground"], opt.thr_ground), api.Scan(ctx, s["scan_ground"])
    ms, ss = api.Map(ctx, s["map_surf"], opt.thr_surf), api.Scan(ctx, s["scan_surf"])
    me, se = api.Map(ctx, s["map_edge"], eo.thr), api.Scan(ctx, s["scan_edge"])
    r = api.scan_match_edges(mg, sg, ms, ss, me, se, s["map_pose"], s["pose0"], opt, eo, last_pose=s["map_pose"])
    ref = er.scan_match_edges(s["map_ground"], s["scan_ground"], s["map_surf"], s["scan_surf"], s["map_edge"], s["scan_edge"], s["map_pose"], s["pose0"],
                              RES, er.edge_defaults(RES), prior, outer)
    pose = np.array(r.pose)
    print(f"pose error {np.abs(pose - ref['pose']).max():.2e}, scores {r.score_ground:.6f} / {r.score_surf:.6f} (reference {ref['score_ground']:.6f} / {ref['score_surf']:.6f})")
    assert np.all(np.abs(pose - ref["pose"]) <= 1e-6 * np.abs(ref["pose"]))
    assert r.score == ref["score"]
    assert r.surf.num_residual_blocks == ref["surf"]["num_residual_blocks"] == 400 + 150 + (1 if prior > 0 else 0)
    assert r.ground.num_residual_blocks == ref["ground"]["num_residual_blocks"]
    assert abs(r.score_surf - ref["score_surf"]) <= 1e-6 * abs(ref["score_surf"]) and abs(r.score_ground - ref["score_ground"]) <= 1e-6 * abs(ref["score_ground"])
    rel_oc = er.se3_mul(er.se3_inv(s["map_pose"]), pose)
    assert np.allclose(np.array(r.relative_o_c), rel_oc, rtol=0, atol=1e-12)
    e0, e1 = np.abs(s["pose0"][4:] - s["pose_true"][4:]).max(), np.abs(pose[4:] - s["pose_true"][4:]).max()
    assert e1 < (0.2 if prior == 0 else 1.0) * e0, (e0, e1)
    for h in (mg, sg, ms, ss, me, se):
        h.close()


# ----------------------------------------------------------------------------- edge picks inside the extraction chain
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scan_case(name):
    from tests import deskew_cases as dc
    if name == "r16x360":
        return er.scan16()
    if name == "r64x1800":
        return dc.scan_full(33), {}
    return er.edited_scan()


@pytest.mark.parametrize("host", [False, True], ids=["device_counts", "host_counts"])
@pytest.mark.parametrize("name,edge_kw", [("r16x360", {}), ("r64x1800", {}), ("r64x1800", dict(edge_threshold=0.05, n_sharp=1, n_less_sharp=3)),
                                          ("edited", {}), ("edited", dict(n_sharp=1))])
def test_extract_edges(ctx, name, edge_kw, host):
    """pick flags against edge_ref on the call's own taps; ground / surf against lvf_lidar_extract[_deskewed]; the edge clouds against
    lvf_cloud_deskew + lvf_cloud_transform of the raw picks — with and without a trajectory"""
    from lvio_fusion_amd import api, synthetic as syn
    from tests import deskew_cases as dc
    scan, kw = _scan_case(name)
    E = syn.lidar_extrinsic()
    stamps, poses = dc.drive()
    ep = api.edge_params(**edge_kw)
    prm = lambda: api.lidar_params(**kw)
    tr = api.Trajectory(ctx, stamps, poses)
    was = api.extract_host_counts(ctx, host)
    fell = api.extract_fallbacks(ctx)
    try:
        g0, s0, d0 = api.lidar_extract(ctx, scan, E, params=prm(), debug=True)
        g1, s1, d1 = api.lidar_extract_deskewed(ctx, scan, E, tr, stamps[2], poses[2], params=prm(), debug=True)
        a = api.lidar_extract_edges(ctx, scan, E, ep, params=prm(), debug=True)
        b = api.lidar_extract_edges(ctx, scan, E, ep, tr, stamps[2], poses[2], params=prm(), debug=True)
        assert api.extract_fallbacks(ctx) == fell
    finally:
        api.extract_host_counts(ctx, was)
    # ground and surf are the existing calls', bit for bit
    for (g, s, d), (ge, se, _, _, de) in (((g0, s0, d0), a), ((g1, s1, d1), b)):
        G, S, Ge, Se = g.download(), s.download(), ge.download(), se.download()
        assert G.shape == Ge.shape and np.array_equal(bits(G), bits(Ge)) and S.shape == Se.shape and np.array_equal(bits(S), bits(Se))
        for key in ("label_mat", "ground_mat", "range_mat", "ground_raw", "surf_raw"):
            assert np.array_equal(d[key], de[key], equal_nan=True) if d[key].dtype.kind == "f" else np.array_equal(d[key], de[key]), key
        assert d["n_segmented"] == de["n_segmented"] and len(G) > 20
    # the picks: integers, equal to the declared rule on the call's own taps
    da, db = a[4], b[4]
    rg, sg, rings = er.seg_layout(da["label_mat"], da["ground_mat"], da["range_mat"])
    curv = er.curvature(rg)
    assert len(curv) == da["n_segmented"] and np.array_equal(bits(da["curvature"]), bits(curv))
    fs, fl, per = er.edge_picks(curv, sg, rings, ep.edge_threshold, ep.n_sharp, ep.n_less_sharp)
    lens = [e_ - s_ + 1 for r, j, _, _ in per for s_, e_ in [er.ring_sectors(*rings[r])[j]]]
    print(f"{name} {edge_kw}: {da['n_segmented']} segmented points, sectors of {min(lens)}..{max(lens)} points, {int(fs.sum())} sharp / {int(fl.sum())} less sharp picks, "
          f"most picks in a sector {max(len(ls) for _, _, _, ls in per)}")
    assert fl.sum() > 50 and fs.sum() >= 30
    n_cand = [int(((sg[s_:e_ + 1] == 0) & (curv[s_:e_ + 1] >= np.float32(ep.edge_threshold))).sum()) for r, j, _, _ in per for s_, e_ in [er.ring_sectors(*rings[r])[j]]]
    assert any(n == 0 for n in n_cand) and (ep.n_sharp < 2 or any(0 < n < ep.n_sharp for n in n_cand))      # sectors with no candidate, with fewer than n_sharp
    for d in (da, db):
        assert np.array_equal(d["sharp_flags"], fs) and np.array_equal(d["less_sharp_flags"], fl)
        assert len(d["sharp_raw"]) == fs.sum() and len(d["less_sharp_raw"]) == fl.sum()
    assert np.array_equal(bits(da["sharp_raw"]), bits(db["sharp_raw"])) and np.array_equal(bits(da["less_sharp_raw"]), bits(db["less_sharp_raw"]))      # the taps hold the RAW picks
    # the raw picks are points of the scan, in ascending segmented index, intensity = ring + relative time; sharp is a subset; no surf pick among them
    seg_row = np.repeat(np.arange(len(rings)), np.diff(np.concatenate([[0], np.cumsum(((da["ground_mat"] == 1) | ((da["label_mat"] > 0) & (da["label_mat"] != 999999))).sum(1))])))
    assert np.array_equal(np.rint(da["less_sharp_raw"][:, 3]).astype(int), seg_row[fl == 1]) and np.array_equal(np.rint(da["sharp_raw"][:, 3]).astype(int), seg_row[fs == 1])
    key3 = lambda p: {bytes(r) for r in np.ascontiguousarray(p[:, :3])}
    less_set = key3(da["less_sharp_raw"])
    assert less_set <= key3(scan[np.isfinite(scan[:, 0])]) and key3(da["sharp_raw"]) <= less_set
    if ep.edge_threshold >= 1.0:
        assert not (less_set & key3(da["surf_raw"]))
    if name == "edited":
        ties = [ls for _, _, _, ls in per if len(ls) >= 2 and curv[ls[0]].view(np.uint32) == curv[ls[1]].view(np.uint32)]
        assert ties and all(fs[ls[0]] == 1 and fs[ls[1]] == (1 if ep.n_sharp >= 2 else 0) and ls[0] < ls[1] for ls in ties)      # n_sharp = 1: the tie decides the sharp cloud
    # the edge clouds: deskew (with a trajectory) then Sensor2Robot of the taps, through the existing calls
    for (_, _, sh, ls, d), traj in ((a, None), (b, tr)):
        for cloud, raw in ((sh, d["sharp_raw"]), (ls, d["less_sharp_raw"])):
            c0 = api.Cloud(ctx, raw)
            c1 = c0.deskew(traj, stamps[2], poses[2], prm().cycle_time, E) if traj is not None else None
            c2 = (c1 if c1 is not None else c0).transform(E)
            want, got = c2.download(), cloud.download()
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
            for h in (c0, c1, c2):
                if h is not None:
                    h.close()
    assert not np.array_equal(bits(a[2].download()), bits(b[2].download()))          # the trajectory moved the picks
    for h in (g0, s0, g1, s1, tr) + a[:4] + b[:4]:
        h.close()
