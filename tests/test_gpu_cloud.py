"""GPU parity of the map-cloud maintenance kernels (lvf_cloud_*: MergeScan/ToWorld, BuildMapFrame's merge, VoxelGrid,
RadiusOutlierRemoval, SegmentGround) against oracle/cloud.h, and the device-resident chain
filter -> transform -> merge -> kNN index -> association without host round trips."""
import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    c = syn.config3_icp(seed=321, n_query=20000, n_az=700)
    q = c["query"].copy()
    q[:, 3] = np.random.default_rng(0).uniform(0, 255, len(q)).astype(np.float32)
    return c, q


def test_transform_bit_exact_and_concat(ctx, oracle, scene):
    from lvio_fusion_amd import api
    c, q = scene
    cl = api.Cloud(ctx, q)
    assert len(cl) == len(q) and np.array_equal(cl.download(), q)
    tw = cl.transform(c["pose0"])
    assert np.array_equal(tw.download(), oracle.cloud_transform(q, c["pose0"]))          # bit-exact float arithmetic
    un = np.array([0.3, -0.2, 0.9, 1.7, 5.0, -3.0, 1.0])                                  # un-normalised quaternion: normalised inside
    t2 = cl.transform(un)
    assert np.array_equal(t2.download(), oracle.cloud_transform(q, un))
    merged = api.Cloud.concat(ctx, [tw, t2, cl])
    assert np.array_equal(merged.download(), np.concatenate([tw.download(), t2.download(), q]))
    empty = api.Cloud(ctx, np.zeros((0, 4), np.float32))
    assert len(empty.transform(c["pose0"])) == 0 and len(api.Cloud.concat(ctx, [empty, empty])) == 0
    for h in (cl, tw, t2, merged, empty):
        h.close()


@pytest.mark.parametrize("leaf", [0.4, 1.0])
def test_voxel_filter_parity(ctx, oracle, scene, leaf):
    from lvio_fusion_amd import api
    _, q = scene
    cl = api.Cloud(ctx, q)
    out = cl.voxel_filter(leaf).download()
    ref = oracle.voxel_filter(q, leaf)
    assert out.shape == ref.shape                               # same voxels, same (ascending index) order
    # float accumulation over each voxel's points in ascending input index, on both sides: equal bit for bit
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    # ... and independent of scheduling: a second run gives the same bits
    assert np.array_equal(cl.voxel_filter(leaf).download().view(np.uint32), out.view(np.uint32))
    assert len(api.Cloud(ctx, np.zeros((0, 4), np.float32)).voxel_filter(leaf)) == 0
    one = api.Cloud(ctx, q[:1]).voxel_filter(leaf).download()
    assert np.array_equal(one, q[:1])
    cl.close()


def test_radius_outlier_filter_parity(ctx, oracle, scene):
    from lvio_fusion_amd import api
    _, q = scene
    sub = q[:8000]
    cl = api.Cloud(ctx, sub)
    out = cl.radius_outlier_filter(0.8, 4).download()
    keep = oracle.radius_outlier_keep(sub, 0.8, 4).astype(bool)
    assert np.array_equal(out, sub[keep])                       # same points, input order preserved (integer decision: exact)
    assert 0 < keep.sum() < len(keep)
    cl.close()


def test_segment_plane_parity(ctx, oracle, scene):
    from lvio_fusion_amd import api
    c, q = scene
    g = q[c["query_ground"]]
    rng = np.random.default_rng(3)
    clutter = g[:500].copy(); clutter[:, 2] += rng.uniform(0.3, 2.0, 500).astype(np.float32)
    pts = np.concatenate([g, clutter]).astype(np.float32)
    cl = api.Cloud(ctx, pts)
    for seed in (12345, 99):
        inl, co, it = cl.segment_plane(0.05, 100, seed)
        mask, co_ref, it_ref = oracle.segment_plane(pts, 0.05, 100, seed)
        assert it == it_ref
        # the refit's moments are exact integer sums on both sides: the plane and every inlier decision are EQUAL
        assert np.array_equal(np.asarray(co, np.float64), np.asarray(co_ref, np.float64))
        got = inl.download()
        assert np.array_equal(got, pts[mask > 0])
        inl.close()
    tiny = api.Cloud(ctx, pts[:2])
    e, co, it = tiny.segment_plane(0.05)
    assert len(e) == 0 and it == 0
    cl.close()


def test_device_resident_map_pipeline(ctx, oracle, scene):
    """Sensor2Robot-style transform -> voxel filter -> ToWorld -> merge of three scans -> kNN index -> association, all
    from device clouds; must equal the same chain with every cloud taken through the host."""
    from lvio_fusion_amd import api
    c, q = scene
    poses = [c["map_pose"], c["pose0"], c["pose_true"]]
    parts_dev, parts_host = [], []
    for k, T in enumerate(poses):
        sub = q[k::3]
        cl = api.Cloud(ctx, sub)
        vf = cl.voxel_filter(0.4)
        tw = vf.transform(T)
        parts_dev.append(tw)
        parts_host.append(tw.download())
    merged = api.Cloud.concat(ctx, parts_dev)
    host_map = np.concatenate(parts_host)
    qs = api.Cloud(ctx, q[:3000])
    m1, s1 = api.Map(ctx, merged, 4.0), api.Scan(ctx, qs)
    m2, s2 = api.Map(ctx, host_map, 4.0), api.Scan(ctx, q[:3000])
    api.knn3(m1, s1, c["pose0"], 4.0); api.knn3(m2, s2, c["pose0"], 4.0)
    i1, d1, v1 = s1.download(); i2, d2, v2 = s2.download()
    assert np.array_equal(v1, v2) and np.array_equal(i1[v1 > 0], i2[v2 > 0]) and np.array_equal(d1[v1 > 0], d2[v2 > 0])
    i0, d0, v0 = oracle.knn3(host_map, q[:3000], c["pose0"], 4.0)
    assert np.array_equal(v1, v0) and np.array_equal(i1[v0 > 0], i0[v0 > 0])
    assert v0.sum() > 1000


def test_align_scan_parity(ctx, oracle, scene):
    """FeatureAssociation::AlignScan (association.cpp:39-64) on device: the slice of two consecutive raw revolutions a keyframe gets — the
    reference's double index arithmetic, truncated; False where the sweep is not covered."""
    from lvio_fusion_amd import api
    _, q = scene
    pc1, pc2 = q[:4321], q[5000:12345]
    c1, c2 = api.Cloud(ctx, pc1), api.Cloud(ctx, pc2)
    cyc = 0.1
    for t1, t2, t in ((10.0, 10.1, 10.05), (10.0, 10.1, 10.0), (10.0, 10.1, 10.1), (10.0, 10.1, 10.0333333), (3.0, 3.0999, 3.07), (10.0, 10.1, 9.99), (10.0, 10.1, 10.11),
                      (1e9, 1e9 + 0.1, 1e9 + 0.0421)):
        ref = oracle.align_scan(pc1, t1, pc2, t2, cyc, t)
        got, ok = api.Cloud.align_scan(c1, t1, c2, t2, cyc, t)
        assert ok == (ref is not None), (t1, t2, t)
        if ref is None:
            assert len(got) == 0
        else:
            assert np.array_equal(got.download(), ref), (t1, t2, t)
        got.close()
    assert oracle.align_scan(pc1, 10.0, pc2, 10.1, cyc, 10.05).shape[0] > 1000
    # the aligned sweep feeds the extraction unchanged
    g, ok = api.Cloud.align_scan(c1, 10.0, c2, 10.1, cyc, 10.02)
    assert ok and np.all(g.download()[:, 3] == 0)
    for h in (g, c1, c2):
        h.close()


@pytest.mark.parametrize("n,key_bits", [(1, 5), (4097, 13), (100000, 20), (250000, 13), (3000000, 22), (2500000, 32)])
def test_stable_pair_sort(ctx, n, key_bits):
    """The radix sort under VoxelGrid (csrc/sort_util.hip) against numpy's stable argsort: only the low key_bits bits order the pairs — stray
    bits above them must not (13 bits = digits of 7 + 6 bits: the last digit is masked to what is left) — equal keys keep their
    input order, and tables beyond 256 k (bins x tiles) entries take the multi-workgroup scan."""
    import ctypes as C
    rng = np.random.default_rng(n + key_bits)
    mask = np.uint32((1 << key_bits) - 1) if key_bits < 32 else np.uint32(0xFFFFFFFF)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if key_bits < 32:
        stray = rng.random(n) < 0.5
        keys = np.where(stray, keys, keys & mask).astype(np.uint32)      # half of the keys carry garbage above key_bits
    if n > 1000:
        keys[rng.integers(0, n, n // 3)] = keys[0]                         # long runs of one key: stability is visible
    vals = np.arange(n, dtype=np.int32)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    from lvio_fusion_amd import api
    api._chk(ctx.L.lvf_debug_sort_pairs_u32(ctx.h, vp(keys), vp(vals), n, key_bits, vp(ko), vp(vo)))
    order = np.argsort(keys & mask, kind="stable")
    assert np.array_equal(vo, vals[order])
    assert np.array_equal(ko, keys[order])


@pytest.mark.parametrize("side", [143, 162])
def test_radius_filter_on_millions_of_points(ctx, side):
    """The scan / compaction with thousands of tiles on either side of the one-launch scan's limit of 2^22 points: a cloud = a dense lattice of
    side^3 points, spacing 0.1 (every point has its 6 axis neighbours within the radius: kept), with isolated points sprinkled through the input
    (removed).  143^3 = 2 924 207 takes the one-launch scan (device_scan1) for the grid and the compaction; 162^3 = 4 251 528 > 2^22, the first
    cubic lattice beyond it, takes the grid sized on the host, its 12 M-cell start array through the three-launch scan, and the three-launch
    compaction.  The output must be the lattice points in input order, bit for bit."""
    from lvio_fusion_amd import api
    rng = np.random.default_rng(5)
    g = (np.arange(side, dtype=np.float32) * np.float32(0.1))
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    n_out = 2000                                            # a 50 x 40 sheet of points 1 m apart, 20 m above the lattice
    iy, ix = np.divmod(np.arange(n_out), 50)
    iso = np.stack([ix.astype(np.float32), iy.astype(np.float32), np.full(n_out, 20.0, np.float32)], -1)
    pts = np.zeros((len(lat) + n_out, 4), np.float32)
    where = np.sort(rng.choice(len(pts), n_out, replace=False))
    mask = np.zeros(len(pts), bool); mask[where] = True
    pts[mask, :3] = iso; pts[~mask, :3] = lat
    pts[:, 3] = np.arange(len(pts), dtype=np.float32) % 251
    cl = api.Cloud(ctx, pts)
    out = cl.radius_outlier_filter(0.15, 4)
    got = out.download()
    assert got.shape == (len(lat), 4)
    assert np.array_equal(got.view(np.uint32), pts[~mask].view(np.uint32))
    out.close(); cl.close()


@pytest.mark.parametrize("n", [50000, (1 << 22) + 1])
def test_segment_plane_on_a_sheet_in_clutter(ctx, oracle, n):
    """SegmentGround on either side of the one-launch scan's limit of 2^22 points, on one input family: a sheet of points at z = 0 (x = 0.25 i - 100,
    y = 0.25 j - 60: exact floats) with clutter 1 to 3 m above it scattered through the input.  n = 2^22 + 1 (a 1943 x 1943 sheet) compacts the
    inliers by the three-launch scan, n = 50 000 (a 211 x 211 sheet) by device_scan1.  Iterations, plane and inliers equal the oracle's, as in
    test_segment_plane_parity."""
    from lvio_fusion_amd import api
    side = 1943 if n > (1 << 22) else 211
    rng = np.random.default_rng(n)
    i, j = np.divmod(np.arange(side * side), side)
    n_clutter = n - side * side
    pts = np.zeros((n, 4), np.float32)
    mask = np.zeros(n, bool); mask[np.sort(rng.choice(n, n_clutter, replace=False))] = True
    pts[~mask, 0] = np.float32(0.25) * i.astype(np.float32) - np.float32(100.0)
    pts[~mask, 1] = np.float32(0.25) * j.astype(np.float32) - np.float32(60.0)
    pts[mask, 0] = rng.uniform(-100, 100, n_clutter); pts[mask, 1] = rng.uniform(-60, 100, n_clutter); pts[mask, 2] = rng.uniform(1, 3, n_clutter)
    pts[:, 3] = np.arange(n, dtype=np.float32) % 251
    cl = api.Cloud(ctx, pts)
    for seed in (12345, 99):
        inl, co, it = cl.segment_plane(0.05, 100, seed)
        mask_ref, co_ref, it_ref = oracle.segment_plane(pts, 0.05, 100, seed)
        assert it == it_ref
        assert np.array_equal(np.asarray(co, np.float64), np.asarray(co_ref, np.float64))
        got = inl.download()
        assert np.array_equal(got, pts[mask_ref > 0])
        assert np.array_equal(mask_ref > 0, ~mask)              # the sheet, and nothing of the clutter
        inl.close()
    cl.close()
