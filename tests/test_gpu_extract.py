"""GPU parity of the LiDAR feature extraction (lvf_lidar_extract = FeatureAssociation::Process) against the
literal sequential restatement in oracle/extract.h (BFS labelling, overwriting sweeps, running counters).

Every decision in this pipeline is a float comparison on atan2 / sqrt output.  sqrtf is IEEE on both sides; atan2 of floats is
cr_atan2f on both sides (correctly rounded to float, one fixed fp64 operation sequence: oracle/cr_math.h = csrc/cr_math.hpp), so
the integer / index stages — range image, ground marking, segmentation, the picks — are compared for EQUALITY.  Only the tail
(VoxelGrid centroids accumulated with atomics, RANSAC with the declared sampler) is compared by nearest-point agreement."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from lvio_fusion_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def cls(label):
    """label_mat -> class: 0 = ground/empty (-1), 1 = outlier segment, 2 = valid segment (ids differ by construction)"""
    return np.where(label < 0, 0, np.where(label == 999999, 1, 2))


def close_fraction(a, b, tol):
    if len(a) == 0 or len(b) == 0:
        return 1.0 if len(a) == len(b) else 0.0
    d, _ = cKDTree(b[:, :3].astype(np.float64)).query(a[:, :3].astype(np.float64))
    return float((d < tol).mean())


@pytest.fixture(params=["device_counts", "host_counts"])
def counts_path(request, ctx):
    """lvf_lidar_extract's two paths: counts kept on the device (one stream wait per scan, the default) / read back after every stage"""
    from lvio_fusion_amd import api
    was = api.extract_host_counts(ctx, request.param == "host_counts")
    yield request.param
    api.extract_host_counts(ctx, was)


@pytest.mark.parametrize("seed", [0x5CA9, 77])
def test_extract_stages_and_clouds(ctx, oracle, seed, counts_path):
    from lvio_fusion_amd import api
    scan = syn.raw_scan(seed=seed)
    ext = syn.lidar_extrinsic()
    ref = oracle.lidar_extract(scan, ext)
    g, s, dbg = api.lidar_extract(ctx, scan, ext, debug=True)
    # Every per-pixel decision goes through IEEE float arithmetic and cr_atan2f (one correctly-rounded definition for the oracle and the
    # device, csrc/cr_math.hpp): the integer / index outputs must be EQUAL, not close.
    assert dbg["n_filtered"] == ref["n_filtered"] and ref["n_filtered"] > 20000
    assert np.array_equal(dbg["range_mat"].view(np.uint32), ref["range_mat"].view(np.uint32)), "range image (occupancy and float bits)"
    assert np.array_equal(dbg["ground_mat"] == 1, ref["ground_mat"] == 1), "ground marking"
    assert np.array_equal(cls(dbg["label_mat"]), cls(ref["label_mat"])), "segmentation classes"
    assert (cls(ref["label_mat"]) == 2).sum() > 1000 and (cls(ref["label_mat"]) == 1).sum() > 0
    # valid segments: same partition of the pixels (label numbers are the BFS visiting order on the CPU, root pixels on the GPU)
    valid = cls(ref["label_mat"]) == 2
    pairs = np.unique(np.stack([dbg["label_mat"][valid], ref["label_mat"][valid]]), axis=1)
    assert len(np.unique(pairs[0])) == len(np.unique(pairs[1])) == pairs.shape[1], "segment partition"
    assert dbg["n_segmented"] == ref["n_segmented"]
    # ExtractFeatures' picks: identical point for point, in order, intensity (ring + relative time through cr_atan2f) included
    for k in ("ground_raw", "surf_raw"):
        assert dbg[k].shape == ref[k].shape, k
        assert np.array_equal(dbg[k].view(np.uint32), ref[k].view(np.uint32)), k
    # final clouds (VoxelGrid -> ROR / plane -> Sensor2Robot): float centroids accumulated in input order, integer-exact plane moments
    # and a bit-exact float transform — frame->feature_lidar's clouds are EQUAL, point for point
    G, S = g.download(), s.download()
    assert G.shape == ref["ground"].shape and np.array_equal(G.view(np.uint32), ref["ground"].view(np.uint32)), "points_ground"
    assert S.shape == ref["surf"].shape and np.array_equal(S.view(np.uint32), ref["surf"].view(np.uint32)), "points_surf"
    assert len(G) > 200 and len(S) > 200
    g.close(); s.close()


def test_extract_edge_cases(ctx, counts_path):
    from lvio_fusion_amd import api
    ext = syn.lidar_extrinsic()
    g, s = api.lidar_extract(ctx, np.zeros((0, 4), np.float32), ext)
    assert len(g) == 0 and len(s) == 0
    nan = np.full((100, 4), np.nan, np.float32)
    g, s = api.lidar_extract(ctx, nan, ext)
    assert len(g) == 0 and len(s) == 0
    near = np.zeros((50, 4), np.float32); near[:, 0] = 1.0          # inside min_range: all gated out
    g, s = api.lidar_extract(ctx, near, ext)
    assert len(g) == 0 and len(s) == 0
    # a handful of points: every stage sees a count of a few (or zero) — ground picks below RANSAC's three, voxel grids of one cell
    few = syn.raw_scan(seed=3)[::400]
    g, s, dbg = api.lidar_extract(ctx, few, ext, debug=True)
    assert dbg["n_filtered"] > 0 and len(g) + len(s) <= dbg["n_segmented"] + 1


def test_both_count_paths_agree_on_many_scans(ctx):
    """device-counted against host-counted path, bit for bit, on scans of different sizes and seeds (the oracle comparison above pins two of them)"""
    from lvio_fusion_amd import api
    ext = syn.lidar_extrinsic()
    for seed, step in ((11, 1), (12, 1), (13, 2), (14, 7), (15, 50), (16, 3)):
        scan = syn.raw_scan(seed=seed)[::step]
        out = {}
        for host in (False, True):
            was = api.extract_host_counts(ctx, host)
            try:
                g, s, dbg = api.lidar_extract(ctx, scan, ext, debug=True)
                out[host] = (g.download(), s.download(), dbg)
                g.close(); s.close()
            finally:
                api.extract_host_counts(ctx, was)
        for k in (0, 1):
            assert out[False][k].shape == out[True][k].shape and np.array_equal(out[False][k].view(np.uint32), out[True][k].view(np.uint32)), (seed, step, k)
        for k in ("n_filtered", "n_segmented"):
            assert out[False][2][k] == out[True][2][k]
        for k in ("ground_raw", "surf_raw", "label_mat", "range_mat"):
            assert np.array_equal(out[False][2][k].view(np.uint32), out[True][2][k].view(np.uint32)), (seed, step, k)


def test_extract_feeds_scan_matching(ctx):
    """End of the chain: two extracted scans, one as the map (ToWorld), one matched against it."""
    from lvio_fusion_amd import api
    ext = syn.lidar_extrinsic()
    a = syn.raw_scan(seed=5)
    g0, s0 = api.lidar_extract(ctx, a, ext)
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    moved = np.concatenate([syn.quat_from_ypr(np.deg2rad(0.3), 0, 0), [0.08, -0.05, 0.02]])
    opt = api.scan_match_options(0.2, outer_iterations=2, prior_weight=0.0)
    mg, ms = api.Map(ctx, g0.transform(ident), opt.thr_ground), api.Map(ctx, s0.transform(ident), opt.thr_surf)
    sg, ss = api.Scan(ctx, g0), api.Scan(ctx, s0)
    res = api.scan_match(mg, sg, ms, ss, ident, moved, opt)
    assert res.ground.num_residual_blocks > 100 and res.surf.num_residual_blocks > 100
    err0 = np.abs(moved[4:]).max(); err1 = np.abs(np.array(res.pose[:])[4:]).max()
    assert err1 < 0.5 * err0                                         # matching a scan against itself pulls the pose back to identity


def test_parameters_outside_the_device_counted_path(ctx):
    """The device-counted path sizes the voxel keys and the radius grid from max_range / resolution BEFORE it sees a point; parameters beyond
    what it can size (here: 2^26 voxels) go through the host-counted path without the caller noticing — and parameters inside it, but
    unusual (a wide range gate, a coarse resolution), still give the host-counted path's clouds bit for bit.
    The fall-back counter says which path produced a result.  It moves by exactly 1 for max_range = 400, resolution = 0.05 in device mode: the a-priori
    voxel span is (2 * 4000 + 3)^3 ~ 5e11 > 2^26, the plan is refused.  It stays for the other three: max_range = 60 gives 303^3 ~ 2.8e7 <= 2^26
    voxels, a radius grid of 151^3 <= 2^22 cells and a capacity of 38 400 <= 2^18 points, and the remaining two are smaller.  Host mode never enters
    the device-counted path: 0."""
    from lvio_fusion_amd import api
    ext = syn.lidar_extrinsic()
    scan = syn.raw_scan(seed=21)[::3]
    for kw, handed_over in ((dict(max_range=400.0, resolution=0.05), 1), (dict(max_range=60.0, min_range=1.0), 0), (dict(resolution=0.5), 0),
                            (dict(ground_rows=40, num_scans=64), 0)):
        prm = api.lidar_params(**kw)
        out = {}
        for host in (False, True):
            was = api.extract_host_counts(ctx, host)
            fell = api.extract_fallbacks(ctx)
            try:
                g, s = api.lidar_extract(ctx, scan, ext, params=prm)
                assert api.extract_fallbacks(ctx) - fell == (0 if host else handed_over), (kw, host)
                out[host] = (g.download(), s.download())
                g.close(); s.close()
            finally:
                api.extract_host_counts(ctx, was)
        for k in (0, 1):
            assert out[False][k].shape == out[True][k].shape and np.array_equal(out[False][k].view(np.uint32), out[True][k].view(np.uint32)), (kw, k)
