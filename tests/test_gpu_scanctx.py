"""GPU parity of the LiDAR place recognition (lvio_fusion_amd/csrc/scanctx_kernels.hip) through the C-ABI against the CPU restatement
tests/scanctx_ref.py.  Descriptors, norms, indices and shifts are bit-equal, and so are the distances: the bound that holds whatever the device's
float64 square root and division do is 1e-12 (at most 64 terms, each carrying a few roundings of 1.1e-16 on values <= 1, stay below 1e-13), but on
gfx950 both are correctly rounded and the sum runs in the declared order, every case here measured a difference of exactly 0, and so the test
asserts `==`.  The conditions the integer equalities rest on (no two compared distances within 1e-9 unless equal) are asserted on the CPU in
tests/test_scanctx_ref.py, on the same seeds."""
import numpy as np
import pytest

from tests import scanctx_cases as sc, scanctx_ref as sr

pytestmark = pytest.mark.gpu

OPTS = [{}] + list(sc.OTHER_OPTIONS)


@pytest.fixture(scope="module")
def ctx():
    from lvio_fusion_amd import api
    c = api.Context(0)
    yield c
    c.close()


def same_records(got, want, what=""):
    gi, gs, gd = got
    wi, ws, wd = want[:3]
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (what, gi, wi, gs, ws)
    used = wi >= 0
    assert np.isposinf(gd[~used]).all()
    diff = float(np.abs(gd[used] - wd[used]).max()) if used.any() else 0.0
    print("%s: max |distance - restatement| = %.3e over %d records" % (what, diff, int(used.sum())))
    assert np.array_equal(gd[used], wd[used]), what


def filled_db(api, ctx, entries, stamps=None, capacity=None, opt=None):
    db = api.ScanContextDb(ctx, capacity or max(len(entries), 1), opt)
    for i, e in enumerate(entries):
        db.append_descriptor(e, float(i) if stamps is None else stamps[i])
    return db


# ---- describe -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1024, 1025, 5000])
def test_describe_bit_equal(ctx, n):
    from lvio_fusion_amd import api
    pts = sc.random_cloud(20 + n, n)
    c = api.Cloud(ctx, pts) if n else api.Cloud(ctx, np.zeros((0, 4), np.float32))
    desc, norm = c.scan_context()
    want = sr.describe(pts)
    assert np.array_equal(desc, want[0]) and np.array_equal(norm, want[1])
    assert (desc.any() or n <= 1) and (n > 0 or not desc.any())
    again = c.scan_context()
    assert np.array_equal(again[0], desc) and np.array_equal(again[1], norm)
    c.close()


@pytest.mark.parametrize("opts", OPTS)
def test_describe_boundaries_and_options(ctx, opts):
    from lvio_fusion_amd import api
    o = sr.options(**opts)
    for pts in (sc.boundary_points(), sc.random_cloud(5, 3000)):
        c = api.Cloud(ctx, pts)
        desc, norm = c.scan_context(api.scanctx_options(**opts))
        want = sr.describe(pts, o)
        assert desc.shape == want[0].shape and np.array_equal(desc, want[0]) and np.array_equal(norm, want[1])
        c.close()


def test_describe_a_scene_view(ctx):
    from lvio_fusion_amd import api
    pts = sc.scenario()["clouds"][0]
    c = api.Cloud(ctx, pts)
    desc, norm = c.scan_context()
    want = sr.describe(pts)
    assert len(pts) > 10000 and np.array_equal(desc, want[0]) and np.array_equal(norm, want[1])
    c.close()


def test_options_are_checked(ctx):
    from lvio_fusion_amd import api
    c = api.Cloud(ctx, sc.random_cloud(1, 10))
    for bad in (dict(num_rings=18), dict(num_rings=36), dict(num_rings=0), dict(num_sectors=65), dict(num_sectors=0), dict(min_range=0.0), dict(max_range=0.25),
                dict(inv_height_step=0.0), dict(max_range=-1.0)):
        with pytest.raises(api.LvfError):
            c.scan_context(api.scanctx_options(**bad))
        with pytest.raises(api.LvfError):
            api.ScanContextDb(ctx, 4, api.scanctx_options(**bad))
    with pytest.raises(api.LvfError):
        api.ScanContextDb(ctx, 0)
    c.close()


# ---- database -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTS)
def test_database_append_download(ctx, opts):
    from lvio_fusion_amd import api
    o = api.scanctx_options(**opts)
    db = api.ScanContextDb(ctx, 3, o)
    clouds = [api.Cloud(ctx, sc.random_cloud(70 + i, 2000 + 100 * i)) for i in range(2)]
    for i, c in enumerate(clouds):
        db.append(c, 10.0 + i)
    assert len(db) == 2
    for i, c in enumerate(clouds):
        d, n = db.download(i)
        w = c.scan_context(o)
        assert np.array_equal(d, w[0]) and np.array_equal(n, w[1]) and d.any()
    # a descriptor made elsewhere: the norms are the library's
    made = sr.describe(sc.random_cloud(90, 500), sr.options(**opts))
    db.append_descriptor(made[0], 11.0)                                        # (an equal stamp is allowed)
    d, n = db.download(2)
    assert np.array_equal(d, made[0]) and np.array_equal(n, made[1])
    with pytest.raises(api.LvfError):
        db.append(clouds[0], 12.0)                                             # full
    with pytest.raises(api.LvfError):
        db.append_descriptor(made[0], 12.0)
    with pytest.raises(api.LvfError):
        db.download(3)
    assert len(db) == 3
    for h in clouds + [db]:
        h.close()


def test_database_refuses_decreasing_stamps(ctx):
    from lvio_fusion_amd import api
    db = api.ScanContextDb(ctx, 8)
    c = api.Cloud(ctx, sc.random_cloud(1, 100))
    db.append(c, 5.0)
    with pytest.raises(api.LvfError):
        db.append(c, 4.5)
    with pytest.raises(api.LvfError):
        db.append_descriptor(np.zeros((60, 20), np.uint8), 4.5)
    with pytest.raises(api.LvfError):
        db.append(c, np.nan)
    with pytest.raises(api.LvfError):
        db.detect(c, 4.0, k=1, append=True)
    with pytest.raises(ValueError):
        db.append_descriptor(np.zeros((20, 60), np.uint8), 6.0)
    assert len(db) == 1
    db.append(c, 5.0)
    assert len(db) == 2
    c.close(); db.close()


# ---- search ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(sc.SEARCH_CASES))
def test_search_bit_equal(ctx, n):
    from lvio_fusion_amd import api
    entries, query, alls = sc.search_case(n)
    db = filled_db(api, ctx, entries)
    assert len(db) == n
    for k in sc.SEARCH_KS:
        got = db.search(query, k=k)
        same_records(got, sr.search(entries, query, n, k, alls), "n = %d, k = %d" % (n, k))
        again = db.search(query, k=k)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    for k in (0, 17):
        with pytest.raises(api.LvfError):
            db.search(query, k=k)
    db.close()


def test_search_rotations_duplicates_and_the_empty_entry(ctx):
    from lvio_fusion_amd import api
    entries, query, alls = sc.search_case(130)
    db = filled_db(api, ctx, entries)
    idx, sh, dist = db.search(query, k=16)
    assert list(idx[:5]) == [1, 3, 4, 40, 90] and list(sh[:5]) == [31, 0, 0, 1, 59] and (dist[:5] == 0.0).all()
    where = {int(i): k for k, i in enumerate(idx)}
    if 5 in where and where[5] < 15:
        assert where[100] == where[5] + 1 and dist[where[100]] == dist[where[5]]
    # the empty entry alone: distance exactly 1 at shift 0; an empty query: the same against everything
    e = filled_db(api, ctx, entries[sc.EMPTY_ENTRY:sc.EMPTY_ENTRY + 1])
    i1, s1, d1 = e.search(query, k=2)
    assert list(i1) == [0, -1] and list(s1) == [0, -1] and d1[0] == 1.0 and np.isposinf(d1[1])
    i2, s2, d2 = db.search(np.zeros_like(query), k=16)
    assert list(i2) == list(range(16)) and (s2 == 0).all() and (d2 == 1.0).all()
    db.close(); e.close()


def test_search_prefix_by_stamp(ctx):
    from lvio_fusion_amd import api
    entries, query, alls = sc.search_case(130)
    stamps = np.arange(130) * 0.5
    stamps[10:13] = stamps[10]                                                 # equal stamps: all of them belong to the prefix
    db = filled_db(api, ctx, entries, stamps)
    for max_stamp, n_search in ((np.inf, 130), (1e9, 130), (-1.0, 0), (-np.inf, 0), (stamps[10], 13), (32.25, 65), (0.0, 1)):
        assert sr.prefix(stamps, max_stamp) == n_search
        for k in (1, 16):
            same_records(db.search(query, max_stamp=max_stamp, k=k), sr.search(entries, query, n_search, k, alls), "max_stamp = %g, k = %d" % (max_stamp, k))
    with pytest.raises(api.LvfError):
        db.search(query, max_stamp=np.nan, k=1)
    db.close()


def test_search_other_shapes(ctx):
    from lvio_fusion_amd import api
    for opts, seed in zip(sc.OTHER_OPTIONS, sc.OTHER_SHAPE_SEEDS):
        o = sr.options(**opts)
        entries, query = sc.random_descriptors(seed, 9, 2, o)
        db = filled_db(api, ctx, entries, opt=api.scanctx_options(**opts))
        same_records(db.search(query, k=16), sr.search(entries, query, 9, 16), "%d x %d" % (o["num_rings"], o["num_sectors"]))
        db.close()


# ---- detect ---------------------------------------------------------------------------------------------------------------------------------
def test_detect_equals_its_parts(ctx):
    from lvio_fusion_amd import api
    s = sc.scenario()
    clouds = [api.Cloud(ctx, c) for c in s["clouds"][:12]]
    a, b = api.ScanContextDb(ctx, 16), api.ScanContextDb(ctx, 16)
    for i, c in enumerate(clouds[:8]):
        a.append(c, float(i)); b.append(c, float(i))
    for step, c in enumerate(clouds[8:]):
        append = step % 2 == 0
        stamp, max_stamp = 8.0 + step, 5.5 + step
        before = len(a)
        got = a.detect(c, stamp, max_stamp=max_stamp, k=5, append=append)
        assert len(a) == before + (1 if append else 0)
        desc, norm = c.scan_context()
        want = b.search(desc, max_stamp=max_stamp, k=5)
        if append:
            b.append(c, stamp)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and (got[0] >= 0).all()
        if append:
            d, n = a.download(before)
            assert np.array_equal(d, desc) and np.array_equal(n, norm)
    assert len(a) == len(b) == 10
    # an empty database: K empty slots, and the sweep still joins it
    e = api.ScanContextDb(ctx, 2)
    i0, s0, d0 = e.detect(clouds[0], 0.0, k=3, append=True)
    assert (i0 == -1).all() and (s0 == -1).all() and np.isposinf(d0).all() and len(e) == 1
    for h in clouds + [a, b, e]:
        h.close()


# ---- drift, end to end ----------------------------------------------------------------------------------------------------------------------
def test_a_revisit_under_drift_is_found_by_appearance(ctx):
    from lvio_fusion_amd import api, relocalize as rl
    s = sc.scenario()
    db = api.ScanContextDb(ctx, sc.N_KEYFRAMES + 1)
    for pts, t in zip(s["clouds"], s["stamps"]):
        c = api.Cloud(ctx, pts)
        db.append(c, t)
        c.close()
    ids = list(range(sc.N_KEYFRAMES))
    # the position gate: with the true position it proposes the revisited keyframe, with 25 m of drift nothing
    assert rl.detect_loop_by_position(s["xy"], ids, s["query_xy"], sc.POSITION_THRESHOLD) == sc.REVISITED
    assert rl.detect_loop_by_position(s["xy"], ids, s["estimated_xy"], sc.POSITION_THRESHOLD) is None
    q = api.Cloud(ctx, s["query"])
    found = rl.detect_loop_by_scan(db, q, sc.QUERY_STAMP, k=5)
    assert found and found[0][0] == sc.REVISITED and len(db) == sc.N_KEYFRAMES
    index, shift, dist = found[0]
    sector = 2.0 * np.pi / 60
    wrap = lambda a: (a + np.pi) % (2.0 * np.pi) - np.pi
    assert abs(wrap(shift * sector - sc.REVISIT_YAW)) <= sector
    # the same through the restatement
    descs = [sr.describe(c)[0] for c in s["clouds"]]
    want = sr.search(descs, sr.describe(s["query"])[0], sc.N_KEYFRAMES, 5)
    same_records(db.detect(q, sc.QUERY_STAMP, max_stamp=sc.QUERY_STAMP - 30.0, k=5, append=False), want, "drift scenario")
    # nothing is old enough: no candidate
    assert rl.detect_loop_by_scan(db, q, 20.0, k=5) == []
    # the seed for the scan match: the old frame's yaw plus the shift, whatever heading the drifted estimate has
    old = sc.pose_of(s["xy"][index], s["yaw"][index], 0.4)
    frame = sc.pose_of(s["estimated_xy"], s["query_yaw"] + 0.7, 1.3)
    rel = rl.seed_relative_o_c(old, frame, shift, 60)
    assert abs(wrap(2.0 * np.arctan2(rel[2], rel[3]) - sc.REVISIT_YAW)) <= sector and rel[6] == 0.0
    q.close(); db.close()
