"""The DECLARED semantics of the LiDAR place recognition (lvio_fusion_amd/csrc/scanctx_kernels.hip): Scan Context (Kim & Kim, IROS 2018)
descriptors, their column-shifted cosine distance and the search, in numpy.  The reference proposes loop candidates by estimated position only
(Relocator::DetectLoop, relocator.cpp:87-133), so there is no reference text to pin these to; this file is the statement of record, checked
against plain Python loops in tests/test_scanctx_ref.py.

Two named deviations from the paper: heights are quantised to 8 bits, and the search is exhaustive (no ring key).

Every float32 step is ONE operation, so the device (contraction off) rounds identically and every integer result is bit-equal.  A descriptor is
an array [num_sectors, num_rings] uint8 — row j is column j of the polar image — with its column norms [num_sectors] uint32."""
import numpy as np

from oracle import pyoracle

F = np.float32
PI_F = F(np.pi)
DEFAULTS = dict(num_rings=20, num_sectors=60, max_range=80.0, min_range=0.5, sensor_height=2.0, inv_height_step=10.0)
MAX_K = 16


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise ValueError(f"scanctx options: no field {k}")
        o[k] = v
    R, S = int(o["num_rings"]), int(o["num_sectors"])
    if not (4 <= R <= 32 and R % 4 == 0 and 1 <= S <= 64):
        raise ValueError("scanctx options: num_rings must be a multiple of 4 up to 32, num_sectors at most 64")
    if not (0 < o["min_range"] < o["max_range"] and o["inv_height_step"] > 0):
        raise ValueError("scanctx options: ranges and step must be positive, min_range < max_range")
    return o


def scales(o):
    """(ring_scale, sector_scale): formed once in double, rounded to float"""
    return F(np.float64(o["num_rings"]) / np.float64(F(o["max_range"]))), F(np.float64(o["num_sectors"]) / (2.0 * np.pi))


def bins(points, o):
    """Per point: counts (bool), ring, sector, cell (ints; meaningful where counts) and the two pre-floor products (float32)."""
    p = np.asarray(points, F).reshape(-1, 4) if np.asarray(points).size else np.zeros((0, 4), F)
    R, S = int(o["num_rings"]), int(o["num_sectors"])
    ring_scale, sector_scale = scales(o)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        xx, yy = x * x, y * y
        r = np.sqrt(xx + yy)
        counts = np.isfinite(r) & np.isfinite(z) & (r >= F(o["min_range"])) & (r < F(o["max_range"]))
        rq = r * ring_scale
        th = pyoracle.cr_atan2f(y, x) if len(p) else np.zeros(0, F)
        sq = (th + PI_F) * sector_scale
        h = z + F(o["sensor_height"])
        hq = np.floor(h * F(o["inv_height_step"]))
    ok = lambda a: np.where(counts, a, F(0))                                  # (what does not count is never binned: keep the casts defined)
    ring = np.minimum(R - 1, np.floor(ok(rq)).astype(np.int64))
    sector = np.clip(np.floor(ok(sq)).astype(np.int64), 0, S - 1)
    hq = np.where(counts & (h > 0), hq, F(0))
    cell = np.where(counts & (h > 0), np.where(hq >= F(254.0), 255, 1 + np.minimum(hq, F(254.0)).astype(np.int64)), 0)
    return counts, ring, sector, cell, rq, sq


def norms(desc):
    d = np.asarray(desc, np.uint8).astype(np.uint64)
    return (d * d).sum(1).astype(np.uint32)


def describe(points, o=None):
    """desc [S, R] uint8 (the per-cell maximum; 0 = empty), norm [S] uint32"""
    o = o if o is not None else options()
    counts, ring, sector, cell, _, _ = bins(points, o)
    desc = np.zeros((int(o["num_sectors"]), int(o["num_rings"])), np.uint8)
    np.maximum.at(desc, (sector[counts], ring[counts]), cell[counts].astype(np.uint8))
    return desc, norms(desc)


def shift_distances(q, d):
    """d(s) for every shift s in [0, S): column j of q pairs with column (j + s) % S of d; float64 terms added in ascending j"""
    q, d = np.asarray(q, np.uint8), np.asarray(d, np.uint8)
    S = q.shape[0]
    nq, nd = norms(q).astype(np.uint64), norms(d).astype(np.uint64)
    qi, di = q.astype(np.int64), d.astype(np.int64)
    out = np.ones(S)
    for s in range(S):
        c = (np.arange(S) + s) % S
        valid = (nq != 0) & (nd[c] != 0)
        if not valid.any():
            continue
        dot = (qi[valid] * di[c][valid]).sum(1)
        term = dot.astype(np.float64) / np.sqrt((nq[valid] * nd[c][valid]).astype(np.float64))
        total = 0.0
        for t in term:                                                        # (sequential, as declared; np.sum adds pairwise)
            total = total + t
        out[s] = 1.0 - total / np.float64(valid.sum())
    return out


def distance(q, d):
    """(min over s of d(s), the lowest such s)"""
    ds = shift_distances(q, d)
    s = int(np.argmin(ds))                                                    # (argmin returns the first minimum)
    return float(ds[s]), s


def search(entries, query, n_search, k, alls=None):
    """The k smallest (distance, index, shift) over the first n_search entries, ordered by (distance, index); unused slots: index -1, shift -1,
    distance +inf.  Returns index [k] int32, shift [k] int32, distance [k] float64 and, for the margin checks, every entry's d(s) [n_search, S]
    (`alls`: those of an earlier call on at least n_search entries of the same database and query, to be re-used)."""
    assert 1 <= k <= MAX_K
    alls = np.array([shift_distances(query, entries[i]) for i in range(n_search)]).reshape(n_search, np.asarray(query).shape[0]) if alls is None else np.asarray(alls)[:n_search]
    idx, sh, dist = np.full(k, -1, np.int32), np.full(k, -1, np.int32), np.full(k, np.inf)
    if n_search:
        best, arg = alls.min(1), alls.argmin(1)
        order = np.lexsort((np.arange(n_search), best))[:k]
        idx[:len(order)], sh[:len(order)], dist[:len(order)] = order, arg[order], best[order]
    return idx, sh, dist, alls


def prefix(stamps, max_stamp):
    """length of the longest prefix of the (non-decreasing) stamps that are <= max_stamp"""
    return int(np.searchsorted(np.asarray(stamps, np.float64), max_stamp, side="right"))
