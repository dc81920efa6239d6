"""CPU checks of the place recognition's declared semantics (tests/scanctx_ref.py): the restatement against plain Python loops, the
sign convention of the shift, ties, the host helpers of relocalize.py, the interface pins, and the two conditions the GPU test's equalities rest
on — asserted here, on the committed seeds, with the restatement alone.

Boundary margins, recorded: of the 531 424 points of the drift scenario's 41 clouds that count, 4 lie within 4 float32 ulp of a bin edge in
r * ring_scale and 9 in (th + PI_F) * sector_scale.  Both sides run the same float operations, so this is
informational; the test only asserts that the fraction stays of the order the float spacing predicts."""
import math
import re

import numpy as np
import pytest

from lvio_fusion_amd import _lib, relocalize as rl
from tests import scanctx_cases as sc, scanctx_ref as sr

F = np.float32
GAP = 1e-9


# ---- the restatement against plain loops ----------------------------------------------------------------------------------------------------
def describe_loop(points, o):
    """one point at a time, every float32 step spelled out"""
    R, S = o["num_rings"], o["num_sectors"]
    ring_scale, sector_scale = sr.scales(o)
    desc = np.zeros((S, R), np.uint8)
    for x, y, z, _ in np.asarray(points, F):
        with np.errstate(all="ignore"):
            r = np.sqrt(F(F(x * x) + F(y * y)))
            if not (np.isfinite(r) and np.isfinite(z) and F(o["min_range"]) <= r < F(o["max_range"])):
                continue
            th = sr.pyoracle.cr_atan2f(np.array([y], F), np.array([x], F))[0]
            ring = min(R - 1, int(math.floor(F(r * ring_scale))))
            sector = min(max(int(math.floor(F(F(th + sr.PI_F) * sector_scale))), 0), S - 1)
            h = F(z + F(o["sensor_height"]))
            cell = 0
            if h > 0:
                hq = F(h * F(o["inv_height_step"]))
                cell = 255 if hq >= 254 else min(255, 1 + int(math.floor(hq)))
        desc[sector, ring] = max(desc[sector, ring], cell)
    return desc


def distance_loop(q, d):
    """the triple loop's inner two: (shift, column), integer dot products by hand"""
    S, R = q.shape
    n2 = lambda a, j: sum(int(v) * int(v) for v in a[j])
    best, arg = None, -1
    for s in range(S):
        total, count = 0.0, 0
        for j in range(S):
            c = (j + s) % S
            a, b = n2(q, j), n2(d, c)
            if a == 0 or b == 0:
                continue
            dot = sum(int(q[j, k]) * int(d[c, k]) for k in range(R))
            total += float(dot) / math.sqrt(float(a * b))
            count += 1
        ds = 1.0 - total / float(count) if count else 1.0
        if best is None or ds < best:
            best, arg = ds, s
    return best, arg


@pytest.mark.parametrize("opts", [{}, dict(num_rings=16, num_sectors=64), dict(num_rings=32, num_sectors=40, max_range=50.0, min_range=1.0, sensor_height=1.5,
                                                                                  inv_height_step=4.0)])
def test_describe_equals_the_point_loop(oracle, opts):
    o = sr.options(**opts)
    for pts in (sc.random_cloud(3, 700), sc.boundary_points(), np.zeros((0, 4), F)):
        desc, norm = sr.describe(pts, o)
        assert np.array_equal(desc, describe_loop(pts, o))
        assert np.array_equal(norm, (desc.astype(np.int64) ** 2).sum(1)) and desc.shape == (o["num_sectors"], o["num_rings"])


def test_boundary_points_land_where_declared(oracle):
    b, o = sc.boundary_points(), sr.options()
    counts, ring, sector, cell, _, _ = sr.bins(b, o)
    at = lambda x, y: int(np.flatnonzero((b[:, 0] == F(x)) & (b[:, 1] == F(y)))[0])
    for k in range(1, 20):
        assert ring[at(4.0 * k, 0.0)] == k                                     # an edge belongs to the outer ring
    assert counts[at(0.5, 0.0)] and not counts[at(0.49999997, 0.0)] and not counts[at(80.0, 0.0)] and counts[at(np.nextafter(F(80.0), F(0.0)), 0.0)]
    neg = np.flatnonzero((b[:, 0] == F(-5.0)) & (b[:, 1] == 0))
    assert sorted(sector[neg]) == [0, 59] and sector[neg[np.signbit(b[neg, 1])][0]] == 0          # y = -0: th = -pi, the first sector
    assert sector[at(5.0, 0.0)] == 30
    assert cell[at(10.0, 1.0)] == 0 and cell[at(10.0, 2.0)] == 0 and cell[at(10.0, 3.0)] == 1
    assert cell[at(20.0, 1.0)] == 255 and cell[at(20.0, 5.0)] == 255 and cell[at(20.0, 9.0)] == 254 and cell[at(20.0, 13.0)] == 255
    assert not counts[~np.isfinite(b[:, :3]).all(1)].any() and not counts[at(3.0e38, 3.0e38)]


def test_search_equals_the_triple_loop():
    for n in (3, 5):
        entries, query, alls = sc.search_case(n)
        idx, sh, dist, _ = sr.search(entries, query, n, 16, alls)
        loop = [distance_loop(query, entries[i]) + (i,) for i in range(n)]
        order = sorted(range(n), key=lambda i: (loop[i][0], i))
        assert list(idx[:n]) == order and list(sh[:n]) == [loop[i][1] for i in order] and list(dist[:n]) == [loop[i][0] for i in order]
        assert (idx[n:] == -1).all() and (sh[n:] == -1).all() and np.isinf(dist[n:]).all()


def test_rotation_fixes_the_sign_of_the_shift():
    entries, query, alls = sc.search_case(130)
    for i, s in sc.ROTATIONS.items():
        assert sr.distance(query, entries[i]) == (0.0, s)
        assert np.array_equal(entries[i][(np.arange(60) + s) % 60], query)     # column j of the query IS column (j + s) % S of the entry
    # the same through the geometry: a sweep taken at yaw psi_old + s * 2 pi / S matches at shift s
    pts = sc.random_cloud(9, 3000)
    for s in (0, 7, 59):
        a = s * 2.0 * np.pi / 60 + 1e-3                                        # (+1 mrad: off the sector edges)
        rot = pts.copy()
        rot[:, 0], rot[:, 1] = (np.cos(a) * pts[:, 0].astype(np.float64) + np.sin(a) * pts[:, 1]), (-np.sin(a) * pts[:, 0].astype(np.float64) + np.cos(a) * pts[:, 1])
        d, got = sr.distance(sr.describe(rot)[0], sr.describe(pts)[0])
        assert got == s and d < 0.1


def test_duplicates_tie_and_the_lower_index_comes_first():
    entries, query, alls = sc.search_case(130)
    idx, sh, dist, _ = sr.search(entries, query, 130, 16, alls)
    assert list(idx[:5]) == [1, 3, 4, 40, 90] and list(sh[:5]) == [31, 0, 0, 1, 59] and (dist[:5] == 0.0).all()
    pos = {int(i): k for k, i in enumerate(np.lexsort((np.arange(130), alls.min(1))))}
    assert alls[100].min() == alls[5].min() and pos[100] == pos[5] + 1          # a duplicated random entry: equal distance, adjacent, lower index first
    assert (alls[sc.EMPTY_ENTRY] == 1.0).all() and sr.distance(query, entries[sc.EMPTY_ENTRY]) == (1.0, 0)


def test_an_empty_query_is_at_distance_one_from_everything():
    entries, _, _ = sc.search_case(5)
    idx, sh, dist, alls = sr.search(entries, np.zeros_like(entries[0]), 5, 5)
    assert (alls == 1.0).all() and list(idx) == [0, 1, 2, 3, 4] and (sh == 0).all() and (dist == 1.0).all()


def test_prefix_is_the_longest_run_of_stamps_not_after_max_stamp():
    st = [0.0, 1.0, 1.0, 2.0, 5.0]
    assert [sr.prefix(st, t) for t in (-1.0, 0.0, 1.0, 1.5, 5.0, np.inf)] == [0, 1, 3, 3, 5, 5]


# ---- relocalize.py's host helpers on hand-computed inputs -----------------------------------------------------------------------------------
def test_detect_loop_by_position_by_hand():
    p = np.array([[0.0, 0.0], [3.0, 4.0], [10.0, 0.0], [0.0, 6.0], [100.0, 100.0]])
    ids = [10, 11, 12, 13, 14]
    assert rl.detect_loop_by_position(p, ids, (0.0, 1.0), 5.5) == 10           # distances 1, sqrt(18), sqrt(101), 5, ...: the three nearest are 1, 4.24, 5
    assert rl.detect_loop_by_position(p, ids, (0.0, 1.0), 5.0) is None         # `<`, not `<=`
    assert rl.detect_loop_by_position(p, ids, (3.0, 3.0), 6.0) == 11           # 1, sqrt(18), sqrt(18) with (0,0) and (0,6): all below 6
    assert rl.detect_loop_by_position(p[:2], ids[:2], (0.0, 0.0), 100.0) is None
    assert rl.detect_loop_by_position(p, ids, (60.0, 60.0), 50.0) is None


def test_seed_relative_o_c_by_hand():
    # planar poses: old at (10, 20, z 1) heading 90 deg; the frame's estimate at (13, 24, z 5) with some other yaw; shift 15 of 60 = +90 deg
    old = sc.pose_of((10.0, 20.0), np.pi / 2, 1.0)
    frame = sc.pose_of((13.0, 24.0), 0.3, 5.0)
    rel = rl.seed_relative_o_c(old, frame, 15, 60)
    # relative yaw 90 deg: q = (0, 0, sin 45, cos 45); translation R_old^T (3, 4, 0) = (4, -3, 0): z is the old frame's, so 0
    assert np.allclose(rel, [0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5), 4.0, -3.0, 0.0], atol=1e-15)
    # roll and pitch of the frame survive, its yaw does not: the seed's absolute rotation is Rz(old yaw + shift) Ry(pitch) Rx(roll)
    rpy = np.array([1.1, 0.2, -0.1])
    frame2 = np.concatenate([rl._quat_of(rpy), [13.0, 24.0, 5.0]])
    old2 = np.concatenate([rl._quat_of(np.array([0.5, 0.0, 0.0])), [10.0, 20.0, 1.0]])
    rel2 = rl.seed_relative_o_c(old2, frame2, 6, 60)
    want = rl._rotmat(rl._quat_of(np.array([0.5, 0.0, 0.0]))).T @ rl._rotmat(rl._quat_of(np.array([0.5 + 6 * 2 * np.pi / 60, 0.2, -0.1])))
    assert np.allclose(rl._rotmat(rel2[:4]), want, atol=1e-14)
    assert np.allclose(rl._rpy_of(rl._quat_of(rpy)), rpy, atol=1e-14)


# ---- interface pins (these fail on the parent commit) ---------------------------------------------------------------------------------------
NAMES = ("lvf_scanctx_options_default", "lvf_scanctx_describe", "lvf_scanctx_db_create", "lvf_scanctx_db_destroy", "lvf_scanctx_db_size", "lvf_scanctx_db_append",
         "lvf_scanctx_db_append_descriptor", "lvf_scanctx_db_download", "lvf_scanctx_search", "lvf_scanctx_detect")


def test_the_new_names_are_declared_and_have_signatures():
    declared = _lib.declared_symbols()
    for n in NAMES:
        assert n in declared and n in _lib._SIGS, n


def test_options_struct_matches_the_header():
    import ctypes as C
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef struct lvf_scanctx_options \{(.*?)\} lvf_scanctx_options;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(int|float)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in _lib.ScanCtxOptions._fields_]
    assert C.sizeof(_lib.ScanCtxOptions) == 4 * len(fields) == 24
    for (ctype, name), (_, pytype) in zip(fields, _lib.ScanCtxOptions._fields_):
        assert pytype is (C.c_int if ctype == "int" else C.c_float), name
    assert sr.DEFAULTS == dict(num_rings=20, num_sectors=60, max_range=80.0, min_range=0.5, sensor_height=2.0, inv_height_step=10.0)


# ---- the conditions the GPU equalities rest on ----------------------------------------------------------------------------------------------
def gap_violations(alls, n_search, k):
    """pairs of keys a top-k selection over the first n_search entries compares that lie within GAP without being equal: neighbours in the sorted
    order up to the k-th against the (k + 1)-th, and the best two shifts of each returned entry"""
    a = np.asarray(alls)[:n_search]
    if n_search == 0:
        return []
    best = np.sort(a.min(1))[:k + 1]
    bad = [("entries", float(x), float(y)) for x, y in zip(best[:-1], best[1:]) if x != y and y - x <= GAP]
    for i in np.lexsort((np.arange(n_search), a.min(1)))[:k]:
        two = np.sort(a[i])[:2]
        if len(two) == 2 and two[0] != two[1] and two[1] - two[0] <= GAP:
            bad.append(("shifts of %d" % i, float(two[0]), float(two[1])))
    return bad


def test_distance_gaps_on_the_committed_seeds(oracle):
    for n in sc.SEARCH_CASES:
        _, _, alls = sc.search_case(n)
        for k in sc.SEARCH_KS:
            for n_search in {n} | {p for p in sc.SEARCH_PREFIXES if p <= n}:
                assert gap_violations(alls, n_search, k) == [], (n, k, n_search)
    for opts, seed in zip(sc.OTHER_OPTIONS, sc.OTHER_SHAPE_SEEDS):
        entries, query = sc.random_descriptors(seed, 9, 2, sr.options(**opts))
        assert gap_violations(sr.search(entries, query, 9, 16)[3], 9, 16) == []
    s = sc.scenario()
    o = sr.options()
    descs = [sr.describe(c, o)[0] for c in s["clouds"]]
    _, _, _, alls = sr.search(descs, sr.describe(s["query"], o)[0], len(descs), 1)
    for k in (1, 5, 16):
        assert gap_violations(alls, len(descs), k) == []


def test_boundary_margins_in_the_random_scenes(oracle):
    s = sc.scenario()
    o = sr.options()
    near_r = near_th = total = 0
    for c in s["clouds"] + [s["query"]]:
        counts, _, _, _, rq, sq = sr.bins(c, o)
        for v, which in ((rq[counts], "r"), (sq[counts], "th")):
            edge = np.rint(v)
            close = np.abs(v.astype(np.float64) - edge) <= 4.0 * np.spacing(np.maximum(np.abs(edge), F(1.0)).astype(F)).astype(np.float64)
            if which == "r":
                near_r += int(close.sum())
            else:
                near_th += int(close.sum())
        total += int(counts.sum())
    print("points within 4 ulp of a bin edge: %d in r, %d in th, of %d" % (near_r, near_th, total))
    # a value v near an integer has spacing 2^-23 v (up to a factor 2), so the window is about 8 * 2^-23 * v wide per unit: below 1e-4 for v <= 64
    assert total > 400000 and near_r <= 1e-4 * total and near_th <= 1e-4 * total
