"""Seeded cases for the LiDAR-depth tests (tests/test_lidar_depth_ref.py on the CPU, tests/test_gpu_lidar_depth.py on the device)."""
import functools

import numpy as np

from tests import lidar_depth_ref as lr

IDENT = np.array([0.0, 0.0, 0.0, 1.0])
LIDAR_EXTRINSIC = np.array([0.004, -0.003, 0.01, 0.9999, 0.81, 0.02, 1.73])      # sensor -> robot: nearly aligned with the body, on the roof


def rig(w, h, fx, baseline=0.54, tilt=True):
    """A rectified pair mounted like the reference's (camera z = body x, camera x = -body y, camera y = -body z); with `tilt` the quaternion is
    slightly off that permutation and NOT of unit length, so that the normalisation is exercised."""
    q = np.array([0.5, -0.5, 0.5, -0.5])
    if tilt:
        q = 1.3 * (q + np.array([0.004, 0.002, -0.003, 0.001]))
    R = lr.rot(q)
    t0 = np.array([1.1, -0.3, 0.75])
    cam0 = dict(fx=fx, fy=fx * 1.01, cx=w / 2 - 0.37, cy=h / 2 - 0.21, extrinsic=np.concatenate([q, t0]))
    cam1 = dict(cam0, extrinsic=np.concatenate([q, t0 + R @ np.array([baseline, 0.0, 0.0])]))
    return cam0, cam1, baseline


def lidar_from_cam(M, pc):
    """camera-0 coordinates -> LiDAR sensor coordinates (the inverse of the 3x4 matrix M), float32"""
    R, t = M[:, :3], M[:, 3]
    return ((np.asarray(pc, np.float64) - t) @ R).astype(np.float32)


def random_cloud(seed, n, w, h, cam0, M, o=None):
    """[n, 4] float32 in the LiDAR frame: in front of the camera (depths on both sides of min_depth / max_depth), behind it, off the image, a
    run of neighbours on one image row (scan order: consecutive points share cells), and NaN / +-inf rows."""
    o = o or lr.options()
    rng = np.random.default_rng(seed)
    kind = rng.uniform(size=n)
    u, v = rng.uniform(-0.1 * w, 1.1 * w, n), rng.uniform(-0.1 * h, 1.1 * h, n)
    # four in five on a slanted surface with 0.3 m of roughness (so that triangles pass the spread gate), the rest anywhere between 0.05 m and 1.4 max_depth
    z = np.where(rng.uniform(size=n) < 0.8, 6.0 + 0.05 * u + 0.1 * v + rng.uniform(-0.3, 0.3, n), rng.uniform(0.05, 1.4 * o["max_depth"], n))
    far_off = kind > 0.9
    u[far_off] += np.where(rng.uniform(size=far_off.sum()) < 0.5, -3.0 * w, 3.0 * w)
    run = np.arange(n) >= (2 * n) // 3                                  # the last third: one ring crossing the image
    u[run] = np.linspace(-2.0, w + 2.0, int(run.sum()))
    v[run] = 0.4 * h + 0.01 * u[run]
    z[run] = 9.0 + 0.02 * u[run]
    z[(kind > 0.8) & (kind <= 0.9) & ~run] *= -1.0                     # behind the camera
    pc = np.stack([(u - cam0["cx"]) * z / cam0["fx"], (v - cam0["cy"]) * z / cam0["fy"], z], 1)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = lidar_from_cam(M, pc)
    out[:, 3] = rng.integers(0, 64, n)
    bad = np.nonzero(rng.uniform(size=n) < 0.03)[0]
    for k, i in enumerate(bad):
        out[i, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    return out


def random_features(seed, n, w, h):
    """[n, 2] float32: mostly inside the image, some on its border lines and a few outside"""
    rng = np.random.default_rng(seed)
    kps = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    edge = rng.uniform(size=n)
    kps[edge < 0.05, 0] = 0.0
    kps[(edge >= 0.05) & (edge < 0.1), 1] = h - 0.5
    kps[(edge >= 0.1) & (edge < 0.13)] += [w, 0.0]
    kps[(edge >= 0.13) & (edge < 0.15)] -= [30.0, 30.0]
    return kps.astype(np.float32)


SMALL = [(64, 48), (70, 50)]
CLOUD_SIZES = [0, 1, 2, 3, 63, 64, 65, 257, 1024, 1025, 5000]
FEATURE_COUNTS = [0, 1, 3, 4, 5, 64, 257]
CELLS = [4, 8, 16, 32]
RADII = [4.0, 12.0, 32.0]
QUERY_CLOUD, DENSE_CLOUD = 800, 5000      # points of the query tests' clouds on the SMALL images: about one record per 7 px^2 (triangles of every status), and one per px^2


GATE_OPTIONS = [dict(max_spread=0.25), dict(min_det=40.0), dict(max_extrapolation=0.0), dict(min_depth=9.0, max_depth=9.5), dict(max_spread=50.0, max_extrapolation=5.0),
                dict(min_depth=8.0, max_depth=11.0, max_extrapolation=20.0, min_det=0.5)]      # (the last: fits extrapolated out of the depth range, status 5)
DEPTH_LIMIT_OPTIONS = [dict(min_depth=2.0, max_depth=12.5), dict(cell=4), dict(cell=32, min_depth=0.125, max_depth=200.0)]
FUSED_OPTIONS = [{}, dict(far_factor=0.0), dict(replace_lost=0), dict(far_factor=30.0, cell=16, radius=20.0)]


def small_case(w, h):
    cam0, cam1, b = rig(w, h, fx=0.7 * w)
    return dict(width=w, height=h, cam0=cam0, cam1=cam1, baseline=b, M=lr.cam_from_lidar(cam0, LIDAR_EXTRINSIC))


# ---- the generated cases, one list for the device tests (which compare them with ==) and the CPU test of the conditions that rests on ---------
def create_cases(n):
    """(case, options, points) of test_create_bit_equal at cloud size n"""
    for w, h in SMALL:
        case = small_case(w, h)
        for cell in CELLS:
            opts = dict(cell=cell)
            yield case, opts, random_cloud(100 + n + cell, n, w, h, case["cam0"], case["M"], lr.options(**opts))


def depth_limit_cases():
    """(case, options, points): other depth limits, and an image whose grid has more cells than one pass of the scan takes"""
    large = dict(small_case(64, 48), width=1241, height=376)
    for opts in DEPTH_LIMIT_OPTIONS:
        pts = random_cloud(5, 3000, 64, 48, large["cam0"], large["M"], lr.options(**opts))
        for case in (small_case(70, 50), large):
            yield case, opts, pts


def feature_count_case(n):
    """(case, options, points, features) of test_query_feature_counts"""
    w, h = SMALL[1]
    case = small_case(w, h)
    return case, {}, random_cloud(48, QUERY_CLOUD, w, h, case["cam0"], case["M"]), random_features(300 + n, n, w, h)


def option_cases(cell, radius):
    opts = dict(cell=cell, radius=radius)
    for w, h in SMALL:
        case = small_case(w, h)
        for n in (QUERY_CLOUD, DENSE_CLOUD):
            yield case, opts, random_cloud(40 + cell, n, w, h, case["cam0"], case["M"], lr.options(**opts)), random_features(60 + cell, 257, w, h)


def gate_cases():
    w, h = SMALL[0]
    case = small_case(w, h)
    pts, kps = random_cloud(48, QUERY_CLOUD, w, h, case["cam0"], case["M"]), random_features(77, 257, w, h)
    for opts in GATE_OPTIONS:
        yield case, opts, pts, kps


def projection_cases():
    """every generated cloud a device test projects: (what, case, options, points)"""
    for n in CLOUD_SIZES:
        for case, opts, pts in create_cases(n):
            yield "create n = %d, %d x %d, %r" % (n, case["width"], case["height"], opts), case, opts, pts
    for case, opts, pts in depth_limit_cases():
        yield "depth limits %d x %d, %r" % (case["width"], case["height"], opts), case, opts, pts
    for what, case, opts, pts, _ in query_cases():
        yield what, case, opts, pts


def query_cases():
    """every generated (not planted) query a device test compares: (what, case, options, points, features)"""
    for n in FEATURE_COUNTS:
        yield ("feature count %d" % n,) + feature_count_case(n)
    for cell in CELLS:
        for radius in RADII:
            for case, opts, pts, kps in option_cases(cell, radius):
                yield "%d x %d, %r, %d points" % (case["width"], case["height"], opts, len(pts)), case, opts, pts, kps
    for case, opts, pts, kps in gate_cases():
        yield "gates %r" % (opts,), case, opts, pts, kps
    s = street()
    yield "street", s, {}, s["points"], s["all_kps"]
    f = fused_case()
    for opts in FUSED_OPTIONS:
        yield "fused %r" % (opts,), f, opts, f["points"], f["kps"]


# ---- planted: exactly representable pixels and depths ---------------------------------------------------------------------------------------
def planted():
    """Hand-made configurations on a 256 x 192 image.  fx = fy = 64, cx = 128, cy = 96 and the matrix is [I | 0], so a point
    ((u - cx) z / 64, (v - cy) z / 64, z) with z a power of two and u, v multiples of 1/16 projects to (u, v, z) EXACTLY.  Every configuration
    sits in a region of its own (at least 13 px from the next one's records).  `expect` [n]: the status; `depth` [n]: the exact depth where one
    is stated, else nan."""
    w, h = 256, 192
    cam0 = dict(fx=64.0, fy=64.0, cx=128.0, cy=96.0, extrinsic=np.concatenate([IDENT, [0.0, 0.0, 0.0]]))
    cam1 = dict(cam0, extrinsic=np.concatenate([IDENT, [0.5, 0.0, 0.0]]))
    M = np.hstack([np.eye(3), np.zeros((3, 1))])
    rec, kps, expect, depth = [], [], [], []

    def feature(u, v, records, status, d=np.nan):
        kps.append((u, v)); expect.append(status); depth.append(d)
        rec.extend((u + dx, v + dy, z) for dx, dy, z in records)

    ring = [(-4.0, -2.0, 4.0), (4.0, -3.0, 4.0), (-3.0, 5.0, 4.0)]                       # quadrants 0, 1, 2
    # a record exactly at the feature (quadrant 3), met twice at different depths: the tie on d2 = 0 goes to the lower source_index
    feature(40.0, 40.0, ring + [(0.0, 0.0, 4.0), (0.0, 0.0, 2.0)], lr.ACCEPTED, 4.0)
    feature(100.0, 24.0, ring + [(0.0, 0.0, 2.0), (0.0, 0.0, 4.0)], lr.ACCEPTED, 2.0)
    # a true duplicate (the same point twice) among the winners
    feature(160.0, 24.0, [(-4.0, -2.0, 8.0), (-4.0, -2.0, 8.0), (4.0, -3.0, 8.0), (-3.0, 5.0, 8.0)], lr.ACCEPTED)
    # d2 == radius^2 exactly (12^2 = 144): the third quadrant is occupied only if that record counts
    feature(100.0, 60.0, [(-3.0, -3.0, 8.0), (-2.0, 5.0, 8.0), (12.0, 0.0, 8.0)], lr.ACCEPTED)
    # ... and just beyond it: two quadrants are left
    feature(216.0, 24.0, [(-3.0, -3.0, 8.0), (-2.0, 5.0, 8.0), (12.0625, 0.0, 8.0)], lr.LOST)
    # a feature on a cell corner (160 = 20 * 8, 64 = 8 * 8; also a corner for cells of 4, 16 and 32)
    feature(160.0, 64.0, [(-4.0, -2.0, 4.0), (4.0, -3.0, 4.0), (-3.0, 5.0, 4.0), (2.0, 2.0, 4.0)], lr.ACCEPTED)
    # exactly two occupied quadrants
    feature(40.0, 100.0, [(-4.0, -2.0, 4.0), (-2.0, -5.0, 4.0), (3.0, 3.0, 4.0)], lr.LOST)
    # collinear winners on y = x / 2 - 1
    feature(100.0, 100.0, [(-4.0, -3.0, 4.0), (0.0, -1.0, 4.0), (6.0, 2.0, 4.0)], lr.DEGENERATE)
    # a triangle that straddles an occlusion edge: 4 m of spread
    feature(160.0, 100.0, [(-4.0, -2.0, 4.0), (4.0, -3.0, 4.0), (-3.0, 5.0, 8.0)], lr.SPREAD)
    # the feature far outside its triangle: wb = -4
    feature(40.0, 150.0, [(4.0, 4.0, 4.0), (10.0, -1.0, 4.0), (-1.0, 10.0, 4.0)], lr.EXTRAPOLATED)
    # a depth the fit pushes below min_depth: weights 5/3, -1/3, -1/3 pass the extrapolation gate, 1/z = 3
    feature(216.0, 100.0, [(1.0, 1.0, 0.5), (6.0, -1.0, 2.0), (-1.0, 6.0, 2.0)], lr.RANGE)
    # one cell with 300 records (lanes loop more than four times) and one with 70 (more than one pass): a block that fills quadrant 3, whose
    # nearest corner alone lies at 8 m — any other winner from the block trips the spread gate
    others = [(-4.0, -2.0, 8.0), (4.0, -3.0, 8.0), (-3.0, 5.0, 8.0)]
    dense = [(2.0 + 0.25 * a, 2.0 + 0.25 * b, 8.0 if a == b == 0 else 4.0) for b in range(15) for a in range(20)]
    feature(94.0, 158.0, others[:2] + dense + others[2:], lr.ACCEPTED)
    dense70 = [(2.0 + 0.5 * a, 2.0 + 0.5 * b, 8.0 if a == b == 0 else 4.0) for b in range(6, -1, -1) for a in range(9, -1, -1)]
    feature(158.0, 158.0, others + dense70, lr.ACCEPTED)
    # the image's corners: the window is clipped to the grid
    corner = [(1.0, 1.0, 4.0), (3.0, 0.5, 4.0), (0.5, 3.0, 4.0)]
    feature(0.0, 0.0, corner, lr.LOST)
    feature(255.5, 0.0, [(-1.0, 1.0, 4.0), (-3.0, 0.25, 4.0)], lr.LOST)
    feature(0.0, 191.5, [(1.0, -1.0, 4.0), (3.0, -0.5, 4.0)], lr.LOST)
    feature(255.5, 191.5, [(-4.0, -3.0, 4.0), (0.0, 0.0, 4.0), (0.25, -6.0, 4.0)], lr.ACCEPTED, 4.0)
    rec = np.array(rec, np.float64)
    pts = np.zeros((len(rec), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = (rec[:, 0] - 128.0) * rec[:, 2] / 64.0, (rec[:, 1] - 96.0) * rec[:, 2] / 64.0, rec[:, 2]
    return dict(points=pts, pixels=rec, M=M, cam0=cam0, cam1=cam1, width=w, height=h, kps=np.array(kps, np.float32), expect=np.array(expect, np.uint8),
                depth=np.array(depth), baseline=0.5)


# ---- a street ---------------------------------------------------------------------------------------------------------------------------------
GROUND, FAR_WALL, SIDE_WALL, POLE, NOTHING = 0, 1, 2, 3, -1
STREET_W, STREET_H = 1241, 376
SENSOR_HEIGHT, WALL_X, SIDE_Y, POLE_X, POLE_Y, POLE_TOP = 1.73, 40.0, -6.0, 12.0, (1.35, 1.65), 2.3
AZIMUTH_DECIMATION = 2


def cast(origin, d):
    """nearest hit of the rays origin + t d (robot frame: x forward, y left, z up, the LiDAR at the origin) with the ground plane, the far wall, the
    side wall and the pole (a flat board facing the sensor, so every surface is a plane): t [n] (inf: nothing) and the surface label [n]"""
    o, d = np.asarray(origin, np.float64), np.asarray(d, np.float64)
    n = len(d)
    t, label = np.full(n, np.inf), np.full(n, NOTHING)

    def take(tt, ok, lab):
        ok = ok & (tt > 0) & (tt < t)
        t[ok], label[ok] = tt[ok], lab

    with np.errstate(all="ignore"):
        take((-SENSOR_HEIGHT - o[2]) / d[:, 2], d[:, 2] < 0, GROUND)
        take((WALL_X - o[0]) / d[:, 0], d[:, 0] > 0, FAR_WALL)
        take((SIDE_Y - o[1]) / d[:, 1], d[:, 1] < 0, SIDE_WALL)
        tp = (POLE_X - o[0]) / d[:, 0]
        yp, zp = o[1] + tp * d[:, 1], o[2] + tp * d[:, 2]
        take(tp, (d[:, 0] > 0) & (yp >= POLE_Y[0]) & (yp <= POLE_Y[1]) & (zp <= POLE_TOP), POLE)
    return t, label


def street(n_features=1000, seed=7, decimation=AZIMUTH_DECIMATION):
    """An HDL-64 pattern (64 rings from +2 to -24.8 degrees, 0.2 degrees of azimuth decimated by `decimation`, the 88 degrees ahead only) over
    a street: ground, a wall at 40 m, a side wall, a pole; projected into a KITTI-like camera.  points [n, 4], label [n] per point; kps
    [n_features, 2] = the features: random pixels; edge_kps = probes beside them, a column of pixels down each edge of the pole, placed to be
    rejected; all_kps = both in that order, with the true depth and surface of every pixel's own ray."""
    w, h = STREET_W, STREET_H
    q = np.array([0.5, -0.5, 0.5, -0.5])
    t0 = np.array([0.27, 0.06, -0.08])
    cam0 = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, extrinsic=np.concatenate([q, t0]))
    R = lr.rot(q)
    baseline = 0.537
    cam1 = dict(cam0, extrinsic=np.concatenate([q, t0 + R @ np.array([baseline, 0.0, 0.0])]))
    lidar_extrinsic = np.concatenate([IDENT, np.zeros(3)])
    M = lr.cam_from_lidar(cam0, lidar_extrinsic)
    el = np.deg2rad(np.linspace(2.0, -24.8, 64))
    az = np.deg2rad(np.arange(-44.0, 44.0, 0.2 * decimation))
    E, A = np.meshgrid(el, az, indexing="ij")                           # ring-major: scan order
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    t, label = cast(np.zeros(3), d)
    hit = np.isfinite(t) & (t < 80.0)
    pts = np.zeros((int(hit.sum()), 4), np.float32)
    pts[:, :3] = (d[hit] * t[hit, None]).astype(np.float32)
    pts[:, 3] = np.repeat(np.arange(64), len(az))[hit]
    rng = np.random.default_rng(seed)
    kps = np.stack([rng.uniform(0, w, n_features), rng.uniform(0.35 * h, h, n_features)], 1)
    # the pole's edges as the camera sees them
    pole_px = [cam0["fx"] * (-(y - t0[1])) / (POLE_X - t0[0]) + cam0["cx"] for y in POLE_Y]
    edge_v = np.arange(150.0, 300.0, 6.0)
    edges = np.concatenate([np.stack([np.full(len(edge_v), px + s), edge_v], 1) for px in pole_px for s in (-2.0, 2.0)])
    all_kps = np.concatenate([kps, edges]).astype(np.float32)
    k64 = all_kps.astype(np.float64)
    ray = np.stack([(k64[:, 0] - cam0["cx"]) / cam0["fx"], (k64[:, 1] - cam0["cy"]) / cam0["fy"], np.ones(len(k64))], 1) @ R.T
    true_depth, true_label = cast(t0, ray)                               # (the ray has camera depth 1 per unit of t)
    return dict(points=pts, label=label[hit], M=M, cam0=cam0, cam1=cam1, baseline=baseline, width=w, height=h, kps=all_kps[:n_features],
                edge_kps=all_kps[n_features:], all_kps=all_kps, true_depth=true_depth, true_label=true_label)


@functools.lru_cache(maxsize=None)
def street_reference():
    """street() with the restatement's records, and its results and per-pixel details over all_kps: computed once, shared by the tests, not to
    be modified"""
    s = street()
    rec, start = lr.cells(s["points"], s["M"], s["cam0"], s["width"], s["height"])
    det = []
    out = lr.query(rec, start, s["cam0"], s["cam1"], s["width"], s["height"], s["all_kps"], details=det)
    return s, rec, start, out, det


# ---- a sweep on stereo_case's own plane ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_case(seed=3, n=300):
    """(computed once and shared: not to be modified)  klt_cases.stereo_case and a cloud laid on its disparity plane (depth fx b / d(row)) like rings: every 4th pixel along a row, every 3rd
    row (closer than that the triangles fall below min_det; at 6 px of disparity the plane's depth changes by 0.55 m per row, so wider rows
    fail the 2 m spread gate), the whole width above the middle row and x >= 100 below it.  Extra features in the columns 0 .. 5 have their right
    pixel outside the right image: the flow cannot accept them."""
    from tests import klt_cases as kc
    c = kc.stereo_case(seed, n=n)
    w, h = kc.W, kc.H
    rng = np.random.default_rng(seed + 50)
    lost = np.stack([rng.uniform(0.0, 5.0, 24), rng.uniform(20.0, h - 20.0, 24)], 1).astype(np.float32)
    kps = np.concatenate([c["kps"], lost])
    x, y = np.meshgrid(np.arange(0.5, w, 4.0), np.arange(0.5, h, 3.0))
    x, y = x.ravel() + rng.uniform(-0.4, 0.4, x.size), y.ravel() + rng.uniform(-0.4, 0.4, x.size)
    keep = (y < h / 2) | (x >= 100.0)
    x, y = x[keep], y[keep]
    cam0 = c["cam0"]
    z = cam0["fx"] * c["baseline"] / kc.disparity(y, h)
    pc = np.stack([(x - cam0["cx"]) * z / cam0["fx"], (y - cam0["cy"]) * z / cam0["fy"], z], 1)
    lidar_extrinsic = np.concatenate([IDENT, [0.9, 0.0, 1.6]])
    M = lr.cam_from_lidar(cam0, lidar_extrinsic)
    pts = np.zeros((len(pc), 4), np.float32)
    pts[:, :3] = lidar_from_cam(M, pc)
    return dict(c, kps=kps, points=pts, M=M, width=w, height=h, n_lost=len(lost))
