"""CPU checks of the ORB restatement tests/orb_ref.py against independent statements, and of the C-ABI surface that carries it.  The device is
compared with the restatement in tests/test_gpu_orb.py; nothing here needs a GPU."""
import ctypes as C
import re
import zlib

import numpy as np
import pytest

from tests import klt_ref as kr
from tests import orb_cases as oc
from tests import orb_ref as R

IMAGES = {"texture": lambda w, h: oc.texture(3, w, h), "rectangles": lambda w, h: oc.rectangles(4, w, h),
          "noise": lambda w, h: np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)}


def test_header_declares_orb_entry_points():
    from lvio_fusion_amd import _lib
    names = set(_lib.declared_symbols())
    want = {"lvf_orb_options_default", "lvf_orb_create", "lvf_orb_destroy", "lvf_orb_pattern", "lvf_orb_level_info", "lvf_orb_capacity", "lvf_orb_set_image",
            "lvf_orb_detect", "lvf_orb_orientation", "lvf_orb_compute", "lvf_orb_download_level", "lvf_orb_search"}
    assert want <= names and want <= set(_lib._SIGS)
    body = re.search(r"typedef struct lvf_orb_options \{(.*?)\} lvf_orb_options;", re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S), re.S).group(1)
    fields = [(t, n.strip()) for t, names_ in re.findall(r"\b(int|float)\s+([^;]+);", body) for n in names_.split(",")]
    assert [n for _, n in fields] == [n for n, _ in _lib.OrbOptions._fields_]
    assert all({"int": C.c_int, "float": C.c_float}[t] is ct for (t, _), (_, ct) in zip(fields, _lib.OrbOptions._fields_))
    assert C.sizeof(_lib.OrbOptions) == 4 * len(fields) == 32


def test_options_follow_the_reference():
    o = R.Options()
    assert o.num_desired == [161, 134, 112, 93] and sum(o.num_desired) == 500                    # extractor.cpp:34-45 with the defaults
    assert o.umax == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert [float(s) for s in o.scale] == [1.0, float(np.float32(1.2)), float(np.float32(1.2) * np.float32(1.2)), float(np.float32(np.float32(1.2) * np.float32(1.2)) * np.float32(1.2))]
    assert o.level_size(1241, 376, 1) == (1034, 313) and o.level_size(640, 376, 3) == (370, 218)
    # the disc of umax is symmetric: row v is as wide as column v is tall
    disc = np.array([[abs(u) <= o.umax[abs(v)] for u in range(-15, 16)] for v in range(-15, 16)])
    assert np.array_equal(disc, disc.T)


def test_level_coordinates_invert_exactly():
    """rint(float32(c) * scale / scale) == c for every coordinate up to 4096 on every level: compute reads where detect found"""
    o = R.Options(num_levels=8)
    c = np.arange(4097, dtype=np.float32)
    for L in range(8):
        assert np.array_equal(np.rint((c * o.scale[L]) / o.scale[L]), c), f"level {L}"


@pytest.mark.parametrize("kind", list(IMAGES))
@pytest.mark.parametrize("w,h", [(1241, 376), (640, 376)])
def test_resize_against_float64_bilinear(kind, w, h):
    """the fixed-point resize stays within 1 grey level of bilinear interpolation in float64 (measured: at most 0.80)"""
    o = R.Options()
    levels = R.pyramid(o, IMAGES[kind](w, h))
    worst = 0.0
    for L in range(1, 4):
        S = levels[L - 1].astype(np.float64)
        sh, sw = S.shape
        dh, dw = levels[L].shape
        assert (dw, dh) == o.level_size(w, h, L)
        fx = np.clip((np.arange(dw) + 0.5) * sw / dw - 0.5, 0, sw - 1)
        fy = np.clip((np.arange(dh) + 0.5) * sh / dh - 0.5, 0, sh - 1)
        x0, y0 = np.minimum(np.floor(fx).astype(int), sw - 2), np.minimum(np.floor(fy).astype(int), sh - 2)
        ax, ay = fx - x0, (fy - y0)[:, None]
        top = S[y0][:, x0] * (1 - ax) + S[y0][:, x0 + 1] * ax
        bot = S[y0 + 1][:, x0] * (1 - ax) + S[y0 + 1][:, x0 + 1] * ax
        worst = max(worst, np.abs(top * (1 - ay) + bot * ay - levels[L]).max())
    print(f"resize {kind} {w} x {h}: max |fixed point - float64 bilinear| = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("kind", list(IMAGES))
def test_blur_against_float64_gaussian(kind):
    """the integer blur against the float64 7 x 7 Gaussian of sigma 2 (normalised weights, reflect-101).  Measured on the three 640 x 376 test
    images: at most 0.629 grey levels (rounding to uint8 alone is 0.5); the bound is 1.5 times that."""
    img = IMAGES[kind](640, 376)
    g = np.exp(-np.arange(-3, 4) ** 2 / 8.0)
    g /= g.sum()
    h, w = img.shape
    P = img.astype(np.float64)[:, kr.reflect101(np.arange(-3, w + 3), w)]
    Hs = sum(g[k] * P[:, k:k + w] for k in range(7))[kr.reflect101(np.arange(-3, h + 3), h)]
    want = sum(g[k] * Hs[k:k + h] for k in range(7))
    err = np.abs(R.blur(img) - want).max()
    print(f"blur {kind}: max |integer - float64| = {err:.4f}")
    assert err <= 1.5 * 0.629
    assert sum(R.BLUR_W) == 1024 and R.BLUR_W == tuple(int(x) for x in np.rint(1024 * g) + np.array([0, 0, 0, 1024 - np.rint(1024 * g).sum(), 0, 0, 0]))


def _is_corner(img, x, y, t):
    """the literal arc scan: 9 contiguous ring pixels all brighter than v + t or all darker than v - t"""
    v = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in R.RING]
    for s in range(16):
        arc = [ring[(s + k) % 16] for k in range(9)]
        if all(p > v + t for p in arc) or all(p < v - t for p in arc):
            return True
    return False


def test_fast_score_against_the_arc_scan():
    img = oc.rectangles(8, 64, 48, 30)                                 # 64 x 48, corners of many contrasts
    for t in (7, 14):
        score = R.fast_score(img, t, edge=3)
        n = 0
        for y in range(3, 45):
            for x in range(3, 61):
                s = int(score[y, x])
                assert (s > 0) == _is_corner(img, x, y, t), (x, y, t)
                if s:                                                  # the score is the LARGEST threshold at which it is a corner
                    assert s >= t and _is_corner(img, x, y, s) and not _is_corner(img, x, y, s + 1), (x, y, s)
                    n += 1
        assert n > 20, "the crop holds too few corners to tell anything"
    assert np.array_equal(R.fast_score(img, 7, edge=3) >= 14, R.fast_score(img, 14, edge=3) > 0)      # one map serves both thresholds
    full = R.fast_score(oc.rectangles(4, 200, 150), 7)
    assert full[:31].max() == 0 and full[:, :31].max() == 0 and full[-31:].max() == 0 and full[:, -31:].max() == 0 and full.max() > 0


def test_cell_nms_and_threshold_fallback():
    rng = (31, 61, 31, 61)
    s = np.zeros((100, 100), np.uint8)
    assert R.cell_corners(s, rng, 14) == []                                                          # an empty cell
    s[40, 40], s[50, 52] = 9, 12
    assert sorted(R.cell_corners(s, rng, 14)) == [(40, 40, 9), (52, 50, 12)]                         # corners only below ini: the min list
    s[45, 45] = 20
    assert R.cell_corners(s, rng, 14) == [(45, 45, 20)]                                              # one at ini: the weak ones are not reported
    s[45, 46] = 20
    assert R.cell_corners(s, rng, 14) == [(40, 40, 9), (52, 50, 12)]        # equal neighbours suppress each other; the list after NMS is empty at ini
    s[:] = 0
    s[40, 60], s[40, 61] = 20, 30                                                                    # a maximum on the cell edge: its stronger
    assert R.cell_corners(s, rng, 14) == [(60, 40, 20)]                                              # neighbour lies in the next cell and counts as 0
    assert R.cell_corners(s, (61, 91, 31, 61), 14) == [(61, 40, 30)]                                 # ... where it survives too
    g = R.cell_grid(200, 150)
    assert (g["ncols"], g["nrows"], g["cw"], g["ch"]) == (4, 3, 36, 32)
    covered = np.zeros((150, 200), int)
    for x0, x1, y0, y1 in g["cells"]:
        covered[y0:y1, x0:x1] += 1
    assert covered.max() == 1 and covered[31:150 - 31, 31:200 - 31].min() == 1 and covered.sum() == (150 - 62) * (200 - 62)      # the ranges tile the area
    assert R.cell_grid(146, 76) is None and R.cell_grid(86, 86) is not None and R.cell_grid(85, 86) is None


def _point_sets():
    rng = np.random.default_rng(9)
    for k in range(24):
        cols, rows = int(rng.integers(90, 500)), int(rng.integers(90, 300))
        W, H = cols - 56, rows - 56
        n = int(rng.integers(1, 600))
        xy = np.unique(np.stack([rng.integers(3, W - 3, n), rng.integers(3, H - 3, n)], 1), axis=0)
        if k % 3 == 0:                                                 # clusters: deep trees, many equal counts
            xy = np.unique(np.clip(xy // 8 * 8 + rng.integers(0, 3, xy.shape), 3, [W - 4, H - 4]), axis=0)
        resp = rng.integers(7, 12 if k % 2 else 200, len(xy))          # every other set: few distinct responses, so ties
        yield cols, rows, np.concatenate([xy, resp[:, None]], 1), int(rng.integers(1, 120))
    grid = np.array([(x, y, 10) for x in range(4, 120, 8) for y in range(4, 120, 8)])       # a regular grid: count ties at the stop index
    for num in (5, 17, 40, 64, 100):
        yield 180, 180, grid, num


def test_quadtree_set_form_equals_list_form():
    n_sets = ties = 0
    for cols, rows, pts, num in _point_sets():
        a, b = R.quadtree_sets(pts, cols, rows, num), R.quadtree_list(pts, cols, rows, num)
        assert a == b, (cols, rows, len(pts), num)
        assert len(a) <= max(num + 2, 4 * R.init_nodes(cols, rows)[0]) and len(a) <= len(pts)
        assert len(set(a)) == len(a) and set(a) <= set(map(tuple, pts.tolist()))
        n_sets += 1
        ties += len(set(pts[:, 2].tolist())) < len(pts)
    assert n_sets >= 20 and ties >= 10


@pytest.mark.parametrize("case", [("rectangles", 200, 150, 60), ("rectangles", 116, 87, 60), ("texture", 320, 200, 500), ("rectangles", 253, 131, 60)])
def test_detect_stays_within_capacity(case):
    kind, w, h, nf = case
    o = R.Options(num_features=nf)
    img = oc.rectangles(1, w, h) if kind == "rectangles" else oc.texture(3, w, h)
    d = R.detect(o, img)
    d2 = R.detect(o, img, R.quadtree_list)
    assert all(np.array_equal(d[k], d2[k]) for k in ("pt", "octave", "response", "level_count"))
    assert len(d["pt"]) <= R.capacity(o, w, h)
    for L in range(o.num_levels):
        lw, lh = o.level_size(w, h, L)
        assert d["level_count"][L] <= R.level_capacity(o, lw, lh, L)
        lc = R.level_coords(o, d["pt"][d["octave"] == L], d["octave"][d["octave"] == L])
        assert len(lc) == 0 or (lc.min(0) >= 31).all() and (lc[:, 0].max() <= lw - 32 and lc[:, 1].max() <= lh - 32)
    print(f"{kind} {w} x {h}: {d['level_count']} of {o.num_desired}, capacity {R.capacity(o, w, h)}")
    assert d["level_count"][0] >= min(o.num_desired[0], 15)


def test_ic_angle_of_a_ramp():
    """a linear ramp rising along theta has its intensity centroid along theta.  Measured deviation of the uint8-quantised ramp (slope 3 grey
    levels per pixel, the disc of umax is not perfectly round) at the five angles: at most 0.129 degrees; the bound is 1.5 times that."""
    o = R.Options()
    yy, xx = np.mgrid[0:63, 0:63].astype(np.float64) - 31
    worst = 0.0
    for theta in (0, 37, 90, 200, 315):
        t = np.deg2rad(theta)
        img = np.rint(128 + 3.0 * (xx * np.cos(t) + yy * np.sin(t))).astype(np.uint8)
        a = float(R.angle_of(*R.ic_moments(img, 31, 31, o.umax)))
        dev = abs((a - theta + 180) % 360 - 180)
        worst = max(worst, dev)
    print(f"ramp: max deviation {worst:.5f} degrees")
    assert worst <= 1.5 * 0.129
    assert R.angle_of(0, 0) == 0 and R.angle_of(0, 5) == 0 and R.angle_of(5, 0) == 90 and R.angle_of(-5, 0) == 270 and 0 <= R.angle_of(-1, 10 ** 9) < 360


def test_descriptor_follows_a_quarter_turn():
    """np.rot90 turns the image a quarter turn: the pixel (x, y) goes to (y, W - 1 - x) and an offset (dx, dy) to (dy, -dx), which in the image's
    y-down axes is a rotation by -90 degrees.  The blur commutes with it, so the descriptor at the turned position with angle - 90 is bit equal."""
    img = np.random.default_rng(12).integers(0, 256, (70, 90), dtype=np.uint8)
    pattern = R.builtin_pattern()
    h, w = img.shape
    b0, b1 = R.blur(img), R.blur(np.rot90(img))
    assert np.array_equal(np.rot90(b0), b1)
    for x, y, angle in ((40, 30, 37.0), (25, 44, 123.5), (60, 22, 291.25), (33, 33, 0.0)):
        turned = np.float32((angle - 90) % 360)
        assert R.half_integer_margin(pattern, [np.float32(angle), turned]) > 1e-6
        assert np.array_equal(R.brief(b0, x, y, np.float32(angle), pattern), R.brief(b1, y, w - 1 - x, turned, pattern)), (x, y, angle)
    assert not np.array_equal(R.brief(b0, 40, 30, np.float32(37), pattern), R.brief(b0, 40, 30, np.float32(127), pattern))


PATTERN_CRC = 0xE2DD3F5C          # of the table as generated when it was introduced: the generator must never drift


def test_builtin_pattern():
    p = R.builtin_pattern()
    assert p.shape == (256, 4) and p.dtype == np.int8 and np.abs(p).max() <= 13
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()
    assert 5.0 < p.astype(np.float64).std() < 7.0 and abs(p.astype(np.float64).mean()) < 0.5           # about 31 / 5
    assert zlib.crc32(p.tobytes()) == PATTERN_CRC
    assert not np.array_equal(R.builtin_pattern(12345), p)




def test_search_against_plain_loops():
    from tests import klt_cases as kc
    rng = np.random.default_rng(3)
    o = R.Options()
    cam0, _, _ = kc.rig()
    pose = np.array([0.02, -0.01, 0.05, 1.0, 0.3, -0.2, 0.1])
    n_last, n_cur = 300, 120
    last_pt = np.stack([rng.uniform(0, 640, n_last), rng.uniform(0, 376, n_last)], 1).astype(np.float32)
    last_oct, cur_oct = rng.integers(0, 4, n_last), rng.integers(0, 4, n_cur)
    last_ang, cur_ang = rng.uniform(0, 60, n_last).astype(np.float32), rng.uniform(0, 60, n_cur).astype(np.float32)
    base = rng.integers(0, 256, (8, 32), dtype=np.uint8)                                              # a few families: close descriptors, ties
    noise = lambda n: (rng.uniform(size=(n, 32, 8)) < 0.06).astype(np.uint8)
    last_desc = base[rng.integers(0, 8, n_last)] ^ np.packbits(noise(n_last), axis=-1).reshape(n_last, 32)
    cur_desc = base[rng.integers(0, 8, n_cur)] ^ np.packbits(noise(n_cur), axis=-1).reshape(n_cur, 32)
    px = np.stack([rng.uniform(0, 640, n_cur), rng.uniform(0, 376, n_cur)], 1)
    depth = np.where(rng.uniform(size=n_cur) < 0.1, -5.0, rng.uniform(2, 30, n_cur))                  # a tenth behind the camera
    pw = kr.se3_apply(pose, kr.se3_apply(cam0["extrinsic"], kr.pixel2sensor(cam0, px, 1.0) * depth[:, None]))
    args = (o, cam0, pose, last_pt, last_oct, last_ang, last_desc, pw, cur_oct, cur_ang, cur_desc)
    m, b, s, marg = R.search(*args)
    loops = R.search_loops(*args)
    assert [tuple(int(v) for v in r) for r in zip(m, b, s)] == [tuple(int(v) for v in r) for r in loops]
    assert (m >= 0).sum() >= 10 and (m[depth < 0] == -1).all() and (b[depth < 0] == -1).all() and ((b >= 0) & (s < 0)).any()
    skip = np.arange(n_cur) % 2
    ms, bs, _, _ = R.search(*args, skip=skip)
    assert (ms[skip > 0] == -1).all() and (bs[skip > 0] == -1).all() and np.array_equal(ms[skip == 0], m[skip == 0])
