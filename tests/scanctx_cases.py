"""Seeded inputs of the place-recognition tests (tests/test_scanctx_ref.py on the CPU, tests/test_gpu_scanctx.py on the GPU): a synthetic
world of poles, wall segments and a noisy ground plane, sensor-frame views of it along a curved trajectory, points on the bin edges, and random
descriptor databases with planted rotations, duplicates and an empty entry.  Nothing here is read from a file."""
import numpy as np

from tests import scanctx_ref as sr

F = np.float32
SENSOR_Z = 2.0                      # the sensor rides this far above the ground plane (scanctx option sensor_height)
VIEW_RANGE = 85.0

# the search cases of the GPU test: (seed, entries, empty columns); tests/test_scanctx_ref.py asserts the distance gaps on exactly these
SEARCH_CASES = {0: (500, 0, 3), 1: (501, 1, 0), 3: (503, 3, 5), 4: (504, 4, 0), 5: (505, 5, 7), 130: (630, 130, 4)}
SEARCH_KS = (1, 5, 16)
SEARCH_PREFIXES = (130, 65, 13, 1, 0)             # the prefix lengths the max_stamp cases of the 130-entry database select
OTHER_OPTIONS = (dict(num_rings=16, num_sectors=64), dict(num_rings=32, num_sectors=40, max_range=50.0, min_range=1.0, sensor_height=1.5, inv_height_step=4.0))
OTHER_SHAPE_SEEDS = (41, 42)                      # a 9-entry database, 2 empty columns, for each of OTHER_OPTIONS
ROTATIONS = {1: 31, 3: 0, 40: 1, 90: 59}          # entry index -> the shift at which the query matches it exactly
DUPLICATES = {4: 3, 100: 5}                       # entry index -> the entry it copies
EMPTY_ENTRY = 7

# the drift scenario
N_KEYFRAMES, REVISITED, KF_PERIOD, QUERY_STAMP = 40, 5, 2.0, 200.0
REVISIT_OFFSET, REVISIT_YAW = (1.5, -0.75), 3.0
DRIFT_M, POSITION_THRESHOLD = 25.0, 20.0
WORLD_SEED = 11


def world(seed):
    """[n, 3] float64 world points: poles and wall segments of random height, a noisy ground plane, over +-300 m"""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(400):                                                       # poles: a vertical line of points every 0.25 m
        x, y, h = rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(2.0, 12.0)
        z = np.arange(0.1, h, 0.25)
        parts.append(np.stack([np.full_like(z, x), np.full_like(z, y), z], 1))
    for _ in range(300):                                                       # walls: a 0.5 m grid over length x height
        x, y, a = rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(0, np.pi)
        ln, h = rng.uniform(5.0, 30.0), rng.uniform(2.0, 10.0)
        s, z = np.meshgrid(np.arange(0.0, ln, 0.5), np.arange(0.1, h, 0.5))
        parts.append(np.stack([x + s.ravel() * np.cos(a), y + s.ravel() * np.sin(a), z.ravel()], 1))
    g = np.stack([rng.uniform(-300, 300, 150000), rng.uniform(-300, 300, 150000), rng.normal(0.0, 0.03, 150000)], 1)
    parts.append(g)
    return np.concatenate(parts)


def view(wpts, xy, yaw, seed, noise=0.02, keep=0.8):
    """The world points within 85 m of the sensor at (xy, SENSOR_Z) heading `yaw`, in the sensor frame, with Gaussian noise and dropout:
    [n, 4] float32 (x, y, z, intensity 0)."""
    rng = np.random.default_rng(seed)
    d = wpts[:, :2] - np.asarray(xy, np.float64)[None]
    near = (d * d).sum(1) < VIEW_RANGE ** 2
    d, z = d[near], wpts[near, 2] - SENSOR_Z
    c, s = np.cos(yaw), np.sin(yaw)
    p = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], z], 1)
    sel = rng.uniform(size=len(p)) < keep
    p = p[sel] + rng.normal(0.0, noise, (int(sel.sum()), 3))
    out = np.zeros((len(p), 4), F)
    out[:, :3] = p
    return out


def trajectory():
    """N_KEYFRAMES keyframes 8 m apart on an arc of radius 120 m: xy [n, 2], yaw [n], stamps [n]"""
    a = np.arange(N_KEYFRAMES) * (8.0 / 120.0)
    return np.stack([120.0 * np.sin(a), -100.0 + 120.0 * (1.0 - np.cos(a))], 1), a, np.arange(N_KEYFRAMES) * KF_PERIOD


_scenario = {}


def scenario():
    """The drift scenario, built once: keyframe clouds along the trajectory and the query that revisits keyframe REVISITED"""
    if not _scenario:
        w = world(WORLD_SEED)
        xy, yaw, stamps = trajectory()
        clouds = [view(w, xy[i], yaw[i], 1000 + i) for i in range(N_KEYFRAMES)]
        c, s = np.cos(yaw[REVISITED]), np.sin(yaw[REVISITED])
        off = np.array([c * REVISIT_OFFSET[0] - s * REVISIT_OFFSET[1], s * REVISIT_OFFSET[0] + c * REVISIT_OFFSET[1]])      # (offset in the old sensor frame)
        q_xy, q_yaw = xy[REVISITED] + off, yaw[REVISITED] + REVISIT_YAW
        radial = (xy[REVISITED] - np.array([0.0, 20.0])) / np.linalg.norm(xy[REVISITED] - np.array([0.0, 20.0]))               # away from the arc's centre
        _scenario.update(world=w, xy=xy, yaw=yaw, stamps=stamps, clouds=clouds, query=view(w, q_xy, q_yaw, 2000), query_xy=q_xy, query_yaw=q_yaw,
                         estimated_xy=q_xy + DRIFT_M * radial)
    return _scenario


def pose_of(xy, yaw, z=0.0):
    """[qx, qy, qz, qw, tx, ty, tz] of a planar pose"""
    return np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), xy[0], xy[1], z])


def boundary_points():
    """Points ON the bin edges of the default options (ring_scale = 0.25 exactly): [n, 4] float32"""
    rows = []
    for k in range(1, 20):
        rows.append((4.0 * k, 0.0, 0.5))                                       # r exactly on a ring edge
        rows.append((0.0, -4.0 * k, 1.0))
    rows += [(2.4, 3.2, 0.0), (-7.2, 9.6, 0.3), (48.0, -64.0, 2.0)]             # 3-4-5 triples: r = 4, 12, 80 (the last one is out of range)
    rows += [(0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.3, 0.4, 0.0), (0.49999997, 0.0, 0.0)]                       # r = min_range, and just below it
    rows += [(80.0, 0.0, 0.0), (0.0, -80.0, 0.0), (float(np.nextafter(F(80.0), F(0.0))), 0.0, 0.0)]           # r = max_range, and just below it
    rows += [(-5.0, 0.0, 1.0), (-5.0, -0.0, 1.0), (-30.0, 0.0, 0.2), (-30.0, -0.0, 0.2)]                      # y = +-0 with x < 0: th = +-pi
    rows += [(5.0, 0.0, 1.0), (5.0, -0.0, 1.0), (0.0, 6.0, 0.0), (0.0, -6.0, 0.0), (7.0, 7.0, 0.0), (-7.0, 7.0, 0.0)]      # th = 0, +-pi/2, pi/4, 3pi/4
    rows += [(10.0, 1.0, -2.0), (10.0, 2.0, -3.0), (10.0, 3.0, float(np.nextafter(F(-2.0), F(0.0))))]         # h = 0, h < 0, the first h > 0
    rows += [(20.0, 1.0, 100.0), (20.0, 5.0, 23.4), (20.0, 9.0, 23.3), (20.0, 13.0, 3.0e38)]                  # beyond the cap, at it, below it
    rows += [(np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (3.0, 1.0, np.nan), (np.inf, 1.0, 1.0), (3.0, -np.inf, 1.0), (3.0, 2.0, np.inf), (3.0e38, 3.0e38, 1.0)]
    out = np.zeros((len(rows), 4), F)
    out[:, :3] = np.array(rows, np.float64).astype(F)
    return out


def random_cloud(seed, n):
    """n sensor-frame points over +-90 m (some out of range), heights -3 .. 25 m"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4), F)
    out[:, 0], out[:, 1], out[:, 2] = rng.uniform(-90, 90, n), rng.uniform(-90, 90, n), rng.uniform(-3, 25, n)
    return out


def random_descriptors(seed, n, empty_columns, o=None):
    """(entries [n, S, R] uint8, query [S, R] uint8): random descriptors with `empty_columns` empty columns each; where the index exists, entry
    i in ROTATIONS is the query rolled so that it matches at that shift, entry i in DUPLICATES copies another entry, entry EMPTY_ENTRY is empty."""
    o = o if o is not None else sr.options()
    S, R = int(o["num_sectors"]), int(o["num_rings"])
    rng = np.random.default_rng(seed)

    def one():
        d = rng.integers(0, 256, (S, R)).astype(np.uint8)
        d[rng.uniform(size=(S, R)) < 0.3] = 0
        d[rng.choice(S, empty_columns, replace=False)] = 0
        return d
    query = one()
    entries = np.stack([one() for _ in range(n)]) if n else np.zeros((0, S, R), np.uint8)
    for i in range(n):
        if i in ROTATIONS:
            entries[i] = np.roll(query, ROTATIONS[i], axis=0)
        if i in DUPLICATES:
            entries[i] = entries[DUPLICATES[i]]
        if i == EMPTY_ENTRY:
            entries[i] = 0
    return entries, query


_search = {}


def search_case(n):
    """(entries, query, every entry's d(s) [n, S]) of SEARCH_CASES[n], the restatement's distances computed once"""
    if n not in _search:
        seed, cnt, empty = SEARCH_CASES[n]
        entries, query = random_descriptors(seed, cnt, empty)
        _search[n] = (entries, query, sr.search(entries, query, cnt, 1)[3])
    return _search[n]
