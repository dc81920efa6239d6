"""GPU parity of the LiDAR depth for visual features (lvio_fusion_amd/csrc/lidar_depth_kernels.hip) through the C-ABI against the CPU
restatement tests/lidar_depth_ref.py.  Everything is compared with `==`: the records (per cell as a set — the order inside a cell is the atomic
cursor's), the start table, and every output of the query and of the fused call, float64 included.  The kernels are compiled with contraction off
and do each float step of the restatement as one operation in the same order; float64 division and square root are correctly rounded on gfx950.
The conditions the equalities rest on (no gate comparison within 1e-9 of its threshold, no tie on d^2 but between duplicates) are asserted on the
CPU in tests/test_lidar_depth_ref.py on the same inputs: every generated cloud and feature set here comes from the generators of
tests/lidar_depth_cases.py, and lc.projection_cases() / lc.query_cases() list them all for that test.  The one gate the CPU cannot see, the
merge's far test on the device's own stereo depths, has its margin asserted in the fused test."""
import ctypes as C

import numpy as np
import pytest

from tests import lidar_depth_cases as lc, lidar_depth_ref as lr
from tests.helpers import bad_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def cloud_of(api, ctx, pts):
    return api.Cloud(ctx, pts if len(pts) else np.zeros((0, 4), np.float32))


def projected(api, ctx, case, pts, opts):
    c = cloud_of(api, ctx, pts)
    d = api.LidarDepth(ctx, c, case["cam0"], case["M"], case["width"], case["height"], api.lidar_depth_options(**opts))
    return c, d


def same_grid(d, want_rec, want_start, what):
    rec, start = d.download()
    assert len(d) == len(want_rec) == len(rec), what
    assert np.array_equal(start, want_start), what
    got = lr.by_cell(rec, start)
    assert got.tobytes() == want_rec.tobytes(), what
    return got


def same_query(got, want, what):
    for name, g, w in zip(("status", "depth", "inv_depth", "p_robot", "kps_right"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, np.nonzero(np.atleast_1d(g != w).reshape(len(w), -1).any(axis=1))[0][:8])


# ---- create ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.CLOUD_SIZES)
def test_create_bit_equal(ctx, n):
    from lvio_fusion_amd import api
    kept = 0
    for case, opts, pts in lc.create_cases(n):            # both small images x the four cell sizes
        want_rec, want_start = lr.cells(pts, case["M"], case["cam0"], case["width"], case["height"], lr.options(**opts))
        c, d = projected(api, ctx, case, pts, opts)
        got = same_grid(d, want_rec, want_start, (n, case["width"], opts))
        c2, d2 = projected(api, ctx, case, pts, opts)
        assert lr.by_cell(*d2.download()).tobytes() == got.tobytes()
        kept += len(want_rec)
        for hnd in (d, d2, c, c2):
            hnd.close()
    assert kept > 0 or n <= 3


def test_create_depth_limits_and_a_large_image(ctx):
    """other depth limits, and an image whose grid has more cells than the scan's workgroup has threads"""
    from lvio_fusion_amd import api
    for cs, opts, pts in lc.depth_limit_cases():
        want_rec, want_start = lr.cells(pts, cs["M"], cs["cam0"], cs["width"], cs["height"], lr.options(**opts))
        c, d = projected(api, ctx, cs, pts, opts)
        same_grid(d, want_rec, want_start, (opts, cs["width"]))
        assert len(want_rec) > 500
        d.close(); c.close()


# ---- query ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.FEATURE_COUNTS)
def test_query_feature_counts(ctx, n):
    from lvio_fusion_amd import api
    case, opts, pts, kps = lc.feature_count_case(n)
    w, h, o = case["width"], case["height"], lr.options(**opts)
    c, d = projected(api, ctx, case, pts, opts)
    rec, start = lr.cells(pts, case["M"], case["cam0"], w, h, o)
    want = lr.query(rec, start, case["cam0"], case["cam1"], w, h, kps, o)
    got = d.query(case["cam1"], kps)
    same_query(got, want, "n = %d" % n)
    again = d.query(case["cam1"], kps)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    if n >= 64:
        assert (got[0] == lr.ACCEPTED).sum() >= n // 8 and len(set(got[0].tolist())) >= 4
    d.close(); c.close()


@pytest.mark.parametrize("cell", lc.CELLS)
@pytest.mark.parametrize("radius", lc.RADII)
def test_query_options(ctx, cell, radius):
    """both small images, a sparse and a dense cloud each"""
    from lvio_fusion_amd import api
    for case, opts, pts, kps in lc.option_cases(cell, radius):
        w, h, o = case["width"], case["height"], lr.options(**opts)
        c, d = projected(api, ctx, case, pts, opts)
        rec, start = lr.cells(pts, case["M"], case["cam0"], w, h, o)
        same_query(d.query(case["cam1"], kps), lr.query(rec, start, case["cam0"], case["cam1"], w, h, kps, o), (w, h, cell, radius, len(pts)))
        d.close(); c.close()


def test_query_gate_options(ctx):
    from lvio_fusion_amd import api
    seen = set()
    for case, opts, pts, kps in lc.gate_cases():
        w, h, o = case["width"], case["height"], lr.options(**opts)
        c, d = projected(api, ctx, case, pts, opts)
        rec, start = lr.cells(pts, case["M"], case["cam0"], w, h, o)
        got = d.query(case["cam1"], kps)
        same_query(got, lr.query(rec, start, case["cam0"], case["cam1"], w, h, kps, o), opts)
        seen |= set(got[0].tolist())
        d.close(); c.close()
    assert seen == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("cell", lc.CELLS)
def test_query_planted(ctx, cell):
    from lvio_fusion_amd import api
    p = lc.planted()
    o = lr.options(cell=cell)
    c, d = projected(api, ctx, p, p["points"], dict(cell=cell))
    rec, start = lr.cells(p["points"], p["M"], p["cam0"], p["width"], p["height"], o)
    same_grid(d, rec, start, "planted")
    got = d.query(p["cam1"], p["kps"])
    same_query(got, lr.query(rec, start, p["cam0"], p["cam1"], p["width"], p["height"], p["kps"], o), "planted, cell %d" % cell)
    assert np.array_equal(got[0], p["expect"])
    stated = np.isfinite(p["depth"])
    assert np.array_equal(got[1][stated], p["depth"][stated])
    d.close(); c.close()


def test_query_street(ctx):
    from lvio_fusion_amd import api
    s, rec, start, want, _ = lc.street_reference()
    c, d = projected(api, ctx, s, s["points"], {})
    same_grid(d, rec, start, "street")
    got = d.query(s["cam1"], s["all_kps"])                                     # the features, then the pole-edge probes
    same_query(got, want, "street")
    assert (got[0] == lr.ACCEPTED).sum() > 700 and (got[1] > 50 * s["baseline"]).sum() >= 10
    d.close(); c.close()


# ---- the fused call -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(ctx):
    from lvio_fusion_amd import api
    f = lc.fused_case()
    il, ir = api.Image(ctx, f["left"], 3), api.Image(ctx, f["right"], 3)
    cloud = api.Cloud(ctx, f["points"])
    stereo = api.stereo_triangulate(il, ir, f["cam0"], f["cam1"], f["baseline"], f["kps"])
    yield f, il, ir, cloud, stereo
    for hnd in (il, ir, cloud):
        hnd.close()


@pytest.mark.parametrize("opts", lc.FUSED_OPTIONS)
def test_fused_equals_the_merge_of_its_parts(ctx, fused, opts):
    from lvio_fusion_amd import api
    f, il, ir, cloud, stereo = fused
    o = lr.options(**opts)
    # the merge's own gate compares a depth the DEVICE's stereo chain produced, so its margin can only be looked at here
    if o["far_factor"] > 0.0:
        z0, far_depth = lr.robot2sensor(f["cam0"], stereo[3])[stereo[1] == 1, 2], o["far_factor"] * f["baseline"]
        assert np.abs(z0 - far_depth).min() > 1e-9 * far_depth
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"], api.lidar_depth_options(**opts))
    lidar = d.query(f["cam1"], f["kps"])
    got = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], f["kps"], d)
    want = lr.merge(stereo, lidar, f["cam0"], f["baseline"], o)
    for name, g, w in zip(("kps_right", "status", "inv_depth", "p_robot", "source"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (opts, name)
    right, st, inv, pb, src = got
    keep = src != 2
    for g, s in zip((right, st, inv, pb), stereo):
        assert np.array_equal(g[keep], s[keep])
    assert np.array_equal(src[keep], (stereo[1][keep] == 1).astype(np.uint8)) and (st[~keep] == 1).all()
    if not opts:
        assert set(src.tolist()) == {0, 1, 2}
        n_lost = f["n_lost"]
        z0 = lr.robot2sensor(f["cam0"], stereo[3])[:, 2]
        far = (stereo[1] == 1) & (z0 > 50 * f["baseline"])
        print("fused: %d features, source 0 / 1 / 2 = %s, %d far by stereo, %d of the %d planted lost features have LiDAR depth" %
              (len(src), np.bincount(src, minlength=3).tolist(), int(far.sum()), int((src[-n_lost:] == 2).sum()), n_lost))
        assert far.sum() >= 10 and (src[far] == 2).sum() >= far.sum() // 2 and (src[-n_lost:] == 2).any() and (stereo[1][-n_lost:] != 1).all()
        # the replaced far features: the sweep lies on the images' own plane, so both depths agree to stereo's accuracy there
        both = far & (src == 2)
        assert np.abs(1.0 / inv[both] - 1.0 / stereo[2][both]).max() < 0.1 * (1.0 / inv[both]).max()
    d.close()


def test_fused_without_replacement_is_stereo_triangulate(ctx, fused):
    from lvio_fusion_amd import api
    f, il, ir, cloud, stereo = fused
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"], api.lidar_depth_options(far_factor=1e12, replace_lost=0))
    right, st, inv, pb, src = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], f["kps"], d)
    for g, s in zip((right, st, inv, pb), stereo):
        assert g.tobytes() == s.tobytes()
    assert np.array_equal(src, (stereo[1] == 1).astype(np.uint8))
    empty = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], np.zeros((0, 2), np.float32), d)
    assert all(len(a) == 0 for a in empty)
    d.close()


# Feature counts around the launch shapes of the chain: four features per workgroup in k_klt_flow and k_ld_query (1, 5), 256 threads per
# workgroup in k_klt_stereo_predict, k_klt_dlt and k_ld_merge (257).  Features are independent: the first n of the case are a case.
@pytest.mark.parametrize("n", [1, 5, 257])
def test_fused_feature_counts(ctx, fused, n):
    from lvio_fusion_amd import api
    f, il, ir, cloud, stereo_all = fused
    kps = f["kps"][:n]
    stereo = api.stereo_triangulate(il, ir, f["cam0"], f["cam1"], f["baseline"], kps)
    for g, s in zip(stereo, stereo_all):
        assert g.tobytes() == s[:n].tobytes()
    # no replacement: lvf_stereo_triangulate byte for byte
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"], api.lidar_depth_options(far_factor=1e12, replace_lost=0))
    right, st, inv, pb, src = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], kps, d)
    for g, s in zip((right, st, inv, pb), stereo):
        assert g.tobytes() == s.tobytes()
    assert np.array_equal(src, (stereo[1] == 1).astype(np.uint8))
    d.close()
    # the default options: the merge of its parts
    o = lr.options()
    z0, far_depth = lr.robot2sensor(f["cam0"], stereo[3])[stereo[1] == 1, 2], o["far_factor"] * f["baseline"]
    assert len(z0) == 0 or np.abs(z0 - far_depth).min() > 1e-9 * far_depth
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"])
    lidar = d.query(f["cam1"], kps)
    got = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], kps, d)
    want = lr.merge(stereo, lidar, f["cam0"], f["baseline"], o)
    for name, g, w in zip(("kps_right", "status", "inv_depth", "p_robot", "source"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (n, name)
    d.close()


def test_non_finite_cameras_are_refused(ctx, fused):
    """lvf_stereo_triangulate_lidar and lvf_lidar_depth_query: LVF_ERR_INVALID with the entry point's name, nothing written, and the same call works after"""
    from lvio_fusion_amd import api
    INVALID = 1
    f, il, ir, cloud, _ = fused
    L = ctx.L
    fp, u8, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    n = 5
    kps = np.ascontiguousarray(f["kps"][:n], np.float32)
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"])
    cams = [(w, (bad, f["cam1"])) for w, bad in bad_cameras(f["cam0"])] + [(w, (f["cam0"], bad)) for w, bad in bad_cameras(f["cam1"])]

    fo = [np.full((n, 2), 7, np.float32), np.full(n, 7, np.uint8), np.full(n, 7.0), np.full((n, 3), 7.0), np.full(n, 7, np.uint8)]

    def fused_call(cam0, cam1):
        a, b = api.make_camera(cam0), api.make_camera(cam1)
        return L.lvf_stereo_triangulate_lidar(il.h, ir.h, C.byref(a), C.byref(b), C.c_double(f["baseline"]), n, fp(kps), fp(fo[0]), u8(fo[1]), dp(fo[2]), dp(fo[3]), None, d.h,
                                              u8(fo[4]))

    qo = [np.full(n, 7, np.uint8), np.full(n, 7.0), np.full(n, 7.0), np.full((n, 3), 7.0), np.full((n, 2), 7, np.float32)]

    def query_call(cam0, cam1):
        a, b = api.make_camera(cam0), api.make_camera(cam1)
        return L.lvf_lidar_depth_query(d.h, C.byref(a), C.byref(b), n, fp(kps), u8(qo[0]), dp(qo[1]), dp(qo[2]), dp(qo[3]), fp(qo[4]))

    for call, name, outs in ((fused_call, b"lvf_stereo_triangulate_lidar:", fo), (query_call, b"lvf_lidar_depth_query:", qo)):
        for what, pair in cams:
            assert call(*pair) == INVALID, (name, what)
            assert L.lvf_last_error().startswith(name), (what, L.lvf_last_error())
        assert all((o == 7).all() for o in outs), "a refused call wrote its outputs"
        assert call(f["cam0"], f["cam1"]) == 0
    for o, w in zip(fo, api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], kps, d)):
        assert o.tobytes() == w.tobytes()
    for o, w in zip(qo, d.query(f["cam1"], kps)):
        assert o.tobytes() == w.tobytes()
    d.close()


def test_fused_landmarks_enter_the_window(ctx, fused):
    from lvio_fusion_amd import api
    f, il, ir, cloud, stereo = fused
    d = api.LidarDepth(ctx, cloud, f["cam0"], f["M"], f["width"], f["height"])
    right, st, inv, pb, src = api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], f["kps"], d)
    win = api.Window(ctx, f["cam0"], f["cam1"], baseline=f["baseline"])
    win.add_keyframe(0, np.array([0, 0, 0, 1.0, 0, 0, 0]), 46.0)
    picks = np.concatenate([np.nonzero(src == 2)[0][:20], np.nonzero(src == 1)[0][:20]])
    assert (src[picks] == 2).sum() >= 10
    for i in picks:
        win.add_landmark(int(i), 0, f["kps"][i], right[i], inv[i])
    assert win.counts()["lm_known"] == len(picks)
    for i in picks:
        assert win.inv_depth(int(i)) == inv[i]
    win.close(); d.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_returned_before_any_launch(ctx, fused):
    from lvio_fusion_amd import api
    f, il, ir, cloud, stereo = fused
    args = (f["cam0"], f["M"], f["width"], f["height"])
    for bad in (dict(cell=0), dict(cell=12), dict(cell=64), dict(radius=0.0), dict(radius=64.5), dict(radius=float("nan")), dict(min_depth=0.0), dict(min_depth=90.0),
                dict(max_depth=float("inf")), dict(max_spread=-1.0), dict(min_det=0.0), dict(max_extrapolation=-0.1), dict(far_factor=-1.0), dict(replace_lost=2)):
        with pytest.raises(ValueError):
            lr.options(**bad)
        with pytest.raises(api.LvfError):
            api.LidarDepth(ctx, cloud, *args, api.lidar_depth_options(**bad))
    for w, h in ((0, 10), (10, 0), (-1, 5), (70000, 10)):
        with pytest.raises(api.LvfError):
            api.LidarDepth(ctx, cloud, f["cam0"], f["M"], w, h)
    with pytest.raises(api.LvfError):
        api.LidarDepth(ctx, cloud, f["cam0"], np.full((3, 4), np.nan), f["width"], f["height"])
    with pytest.raises(api.LvfError):
        api.LidarDepth(ctx, cloud, dict(f["cam0"], fx=0.0), f["M"], f["width"], f["height"])
    with pytest.raises(ValueError):
        api.lidar_depth_options(nothing=1)
    other = api.Context(0)
    with pytest.raises(api.LvfError):
        api.LidarDepth(other, cloud, *args)                                    # the cloud belongs to ctx
    d = api.LidarDepth(ctx, cloud, *args)
    with pytest.raises(api.LvfError):
        d.query(dict(f["cam1"], fx=0.0), f["kps"])
    d.cam0 = dict(f["cam0"], cx=f["cam0"]["cx"] + 1.0)
    with pytest.raises(api.LvfError):
        d.query(f["cam1"], f["kps"])                                           # not the intrinsics the sweep was projected with
    d.cam0 = f["cam0"]
    img = np.zeros((f["height"], f["width"]), np.uint8)
    ol, orr = api.Image(other, img, 3), api.Image(other, img, 3)
    with pytest.raises(api.LvfError):
        api.stereo_triangulate_lidar(ol, orr, f["cam0"], f["cam1"], f["baseline"], f["kps"], d)      # images of another context
    ol.close(); orr.close(); other.close()
    with pytest.raises(api.LvfError):
        api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], -1.0, f["kps"], d)
    assert len(d) > 1000
    d.close()
    with pytest.raises(api.LvfError):
        d.query(f["cam1"], f["kps"])                                           # a closed handle
    with pytest.raises(api.LvfError):
        len(d)
    with pytest.raises(api.LvfError):
        api.stereo_triangulate_lidar(il, ir, f["cam0"], f["cam1"], f["baseline"], f["kps"], d)
