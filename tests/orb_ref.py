"""The declared semantics of the ORB part of the front-end, restated in numpy: Extractor's options and scale pyramid
(extractor.cpp:9-64, :455-477), the FAST-9/16 corner score, ICAngle (:66-93), the blurred level and rBRIEF (:504-530 as ORB-SLAM2's
computeDescriptors has it) and the numeric part of LocalMap::Search (local_map.cpp:313-368).  OpenCV is not reproduced bit for bit; what is
integer arithmetic here is bit equal on the device (tests/test_gpu_orb.py), and this file is checked against independent statements in
tests/test_orb_ref.py."""
import numpy as np

from tests import klt_ref as kr

PATCH, HALF, EDGE = 31, 15, 31
BORDER = 19                 # a keypoint's level coordinates lie at least this far inside the level: the rotated pattern reaches rint(13 * sqrt 2) = 18
BLUR_W = (72, 134, 195, 222, 195, 134, 72)          # rint(1024 g), sigma 2, the centre absorbing the remainder; the sum is 1024
# the radius-3 ring, in circular order (dx, dy)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


class Options:
    def __init__(self, num_features=500, scale_factor=1.2, num_levels=4, ini_th_fast=14, min_th_fast=7):
        self.num_features, self.scale_factor, self.num_levels = int(num_features), np.float32(scale_factor), int(num_levels)
        self.ini_th_fast, self.min_th_fast = int(ini_th_fast), int(min_th_fast)
        f32 = np.float32
        self.scale = [f32(1)]
        for _ in range(1, self.num_levels):
            self.scale.append(f32(self.scale[-1] * self.scale_factor))                     # extractor.cpp:14-22, float products
        self.inv_scale = [f32(f32(1) / s) for s in self.scale]
        inv = f32(f32(1) / self.scale_factor)
        nd = f32(f32(f32(self.num_features) * f32(f32(1) - inv)) / f32(f32(1) - f32(pow(float(inv), float(self.num_levels)))))      # :36
        self.num_desired, total = [], 0
        for _ in range(self.num_levels - 1):
            self.num_desired.append(int(np.rint(nd)))                                      # cvRound: half to even
            total += self.num_desired[-1]
            nd = f32(nd * inv)
        self.num_desired.append(max(self.num_features - total, 0))
        self.umax = umax()
        self.scale64 = [1.0]                                                               # local_map.h:26-31: double products of the float factor
        for _ in range(1, self.num_levels):
            self.scale64.append(self.scale64[-1] * float(self.scale_factor))

    def level_size(self, w, h, level):
        """(cvRound(float(cols) * inv_scale), cvRound(float(rows) * inv_scale)), extractor.cpp:459-460"""
        s = self.inv_scale[level]
        return int(np.rint(np.float32(np.float32(w) * s))), int(np.rint(np.float32(np.float32(h) * s)))


def umax():
    """extractor.cpp:49-63: the end of each row of the circular patch"""
    u = [0] * (HALF + 1)
    half = np.float32(HALF) * np.sqrt(np.float32(2)) / np.float32(2)
    vmax, vmin = int(np.floor(half + np.float32(1))), int(np.ceil(half))
    for v in range(vmax + 1):
        u[v] = int(np.rint(np.sqrt(float(HALF * HALF - v * v))))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------------------
def resize_table(src, dst):
    """per output index: the left source index and the 11-bit weight pair (a0, a1) of cv::resize INTER_LINEAR's fixed-point path"""
    d = np.arange(dst, dtype=np.float64)
    f = (d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5
    i = np.floor(f).astype(np.int64)
    f = f - i
    lo, hi = i < 0, i >= src - 1
    i[lo], f[lo] = 0, 0.0
    i[hi], f[hi] = src - 1, 0.0
    a1 = np.rint(2048.0 * f).astype(np.int32)
    return i, 2048 - a1, a1


def resize(S, dw, dh):
    h, w = S.shape
    ix, a0, a1 = resize_table(w, dw)
    iy, b0, b1 = resize_table(h, dh)
    S32 = S.astype(np.int32)
    H = a0[None, :] * S32[:, ix] + a1[None, :] * S32[:, np.minimum(ix + 1, w - 1)]
    H0, H1 = H[iy] >> 4, H[np.minimum(iy + 1, h - 1)] >> 4
    return ((((b0[:, None] * H0) >> 16) + ((b1[:, None] * H1) >> 16) + 2) >> 2).astype(np.uint8)


def pyramid(opt, img):
    """level L is the resize of level L - 1 (extractor.cpp:468)"""
    h, w = img.shape
    levels = [np.ascontiguousarray(img)]
    for L in range(1, opt.num_levels):
        lw, lh = opt.level_size(w, h, L)
        levels.append(resize(levels[-1], lw, lh))
    return levels


# ---- FAST-9/16 -------------------------------------------------------------------------------------------------------------------------------
def fast_score(img, min_th, edge=EDGE):
    """uint8 map: the largest t at which the pixel is a FAST-9/16 corner (9 contiguous ring pixels all > v + t or all < v - t), 0 where that
    is below min_th or the pixel is closer than 31 (`edge`) to an edge."""
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    if w <= 2 * edge or h <= 2 * edge:
        return out
    I = img.astype(np.int16)
    v = I[edge:h - edge, edge:w - edge]
    d = np.stack([I[edge + dy:h - edge + dy, edge + dx:w - edge + dx] - v for dx, dy in RING])
    d = np.concatenate([d, d[:8]])
    best = np.full(v.shape, -256, np.int16)
    for e in (d, -d):
        for s in range(16):
            best = np.maximum(best, e[s:s + 9].min(0))
    score = best - 1
    score[score < min_th] = 0
    out[edge:h - edge, edge:w - edge] = score.astype(np.uint8)
    return out


# ---- blur ------------------------------------------------------------------------------------------------------------------------------------
def blur(img):
    """7 x 7, sigma 2, separable and integer: (sum_v w_v (sum_u w_u p) + 2^19) >> 20, reflect-101"""
    h, w = img.shape
    P = img.astype(np.int64)[:, kr.reflect101(np.arange(-3, w + 3), w)]
    Hs = sum(BLUR_W[k] * P[:, k:k + w] for k in range(7))
    Hs = Hs[kr.reflect101(np.arange(-3, h + 3), h)]
    V = sum(BLUR_W[k] * Hs[k:k + h] for k in range(7))
    return ((V + (1 << 19)) >> 20).astype(np.uint8)


# ---- pattern ---------------------------------------------------------------------------------------------------------------------------------
def builtin_pattern(seed=0x9E3779B97F4A7C15):
    """int8 [256, 4] = (x1, y1, x2, y2) per descriptor bit.  Integer only: a 64-bit LCG (Knuth's MMIX constants); a coordinate is the sum of four
    draws of (state >> 33) % 11 minus 20 (variance 40: sigma 6.3, about 31 / 5), redrawn while it exceeds 13 in magnitude; a pair whose two
    points coincide is redrawn.  NOT OpenCV's learned bit_pattern_31_."""
    s = seed
    mask = (1 << 64) - 1

    def draw():
        nonlocal s
        while True:
            t = 0
            for _ in range(4):
                s = (s * 6364136223846793005 + 1442695040888963407) & mask
                t += (s >> 33) % 11
            if abs(t - 20) <= 13:
                return t - 20

    rows = []
    while len(rows) < 256:
        r = [draw() for _ in range(4)]
        if r[0] == r[2] and r[1] == r[3]:
            continue
        rows.append(r)
    return np.array(rows, np.int8)


# ---- keypoints -------------------------------------------------------------------------------------------------------------------------------
def level_coords(opt, pt, octave):
    """rint(pt / scale_L) in float32: inverts Detect's `pt *= scale` (extractor.cpp:489-501)"""
    pt = np.asarray(pt, np.float32).reshape(-1, 2)
    s = np.array(opt.scale, np.float32)[np.asarray(octave)]
    return np.rint(pt / s[:, None]).astype(np.int64)


def ic_moments(img, x, y, um):
    m10 = m01 = 0
    for v in range(-HALF, HALF + 1):
        d = um[abs(v)]
        row = img[y + v, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m01, m10


def angle_of(m01, m10):
    """atan2 in degrees in [0, 360), evaluated in float64 and rounded to float32"""
    if m01 == 0 and m10 == 0:
        return np.float32(0)
    deg = np.arctan2(np.float64(m01), np.float64(m10)) * (180.0 / np.pi)
    if deg < 0:
        deg += 360.0
    a = np.float32(deg)
    return np.float32(0) if a >= np.float32(360) else a


def orientation(opt, levels, pt, octave):
    lc = level_coords(opt, pt, octave)
    return np.array([angle_of(*ic_moments(levels[o], x, y, opt.umax)) for (x, y), o in zip(lc, octave)], np.float32).reshape(-1)


def rotated_pattern(pattern, angle):
    """(fx, fy) [512] in float64 before rounding: x a - y b, x b + y a"""
    th = np.float64(np.float32(angle)) * (np.pi / 180.0)
    a, b = np.cos(th), np.sin(th)
    P = np.asarray(pattern, np.int8).astype(np.float64).reshape(512, 2)
    return P[:, 0] * a - P[:, 1] * b, P[:, 0] * b + P[:, 1] * a


def brief(blurred, x, y, angle, pattern):
    fx, fy = rotated_pattern(pattern, angle)
    vals = blurred[y + np.rint(fy).astype(np.int64), x + np.rint(fx).astype(np.int64)]
    return np.packbits(vals[0::2] < vals[1::2], bitorder="little")


def half_integer_margin(pattern, angles):
    """the smallest distance of any rotated pattern coordinate from a half-integer (where rint would depend on the last bit of cos / sin)"""
    m = np.inf
    for a in angles:
        for f in rotated_pattern(pattern, a):
            m = min(m, np.abs(np.abs(f - np.floor(f)) - 0.5).min())
    return m


def compute(opt, levels, pt, octave, angle, pattern, blurred=None):
    lc = level_coords(opt, pt, octave)
    blurred = blurred if blurred is not None else {}
    out = np.zeros((len(lc), 32), np.uint8)
    for i, ((x, y), o) in enumerate(zip(lc, octave)):
        if int(o) not in blurred:
            blurred[int(o)] = blur(levels[int(o)])                                    # only levels that have keypoints are blurred
        out[i] = brief(blurred[int(o)], x, y, angle[i], pattern)
    return out


# ---- search ----------------------------------------------------------------------------------------------------------------------------------
def hamming(a, b):
    return np.unpackbits(np.bitwise_xor(a, b), axis=-1).sum(-1).astype(np.int64)


def search(opt, cam0, last_pose, last_pt, last_octave, last_angle, last_desc, cur_pw, cur_octave, cur_angle, cur_desc, skip=None):
    """returns match, best, second [n_cur] int32 and the mask of marginal features (a candidate test within 1e-3 of its threshold or |pc.z| < 1e-9)"""
    n = len(cur_octave)
    last_pt, last_angle = np.asarray(last_pt, np.float32).reshape(-1, 2), np.asarray(last_angle, np.float32)
    last_octave, cur_angle = np.asarray(last_octave, np.int64), np.asarray(cur_angle, np.float32)
    match, best, second, marg = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, bool)
    if n == 0:
        return match, best, second, marg
    pc = kr.world2sensor(cam0, np.asarray(cur_pw, np.float64).reshape(-1, 3), last_pose)
    with np.errstate(all="ignore"):
        p = kr.sensor2pixel(cam0, pc).astype(np.float32)
    order = np.lexsort((np.arange(len(last_octave)), last_octave))                    # (level, index)
    radius = PATCH * np.array(opt.scale64)
    for i in range(n):
        if skip is not None and skip[i]:
            continue
        marg[i] = abs(pc[i, 2]) < 1e-9
        if pc[i, 2] < 0 or len(order) == 0:
            continue
        o = int(cur_octave[i])
        rot = np.abs(last_angle - cur_angle[i]).astype(np.float64)                    # a float difference, as the reference forms it
        dist = np.sqrt(((p[i].astype(np.float64) - last_pt.astype(np.float64)) ** 2).sum(1))
        lvl = (last_octave == o) | (last_octave == o + 1)
        r = radius[np.minimum(last_octave, opt.num_levels - 1)]
        marg[i] |= bool((lvl & ((np.abs(rot - 15.0) < 1e-3) | (np.abs(dist - r) < 1e-3))).any())
        cand = order[(lvl & (rot < 15.0) & (dist < r))[order]]
        if len(cand) == 0:
            continue
        d = hamming(last_desc[cand], cur_desc[i][None, :])
        k = np.argsort(d, kind="stable")
        best[i] = d[k[0]]
        if len(cand) < 2:
            continue
        second[i] = d[k[1]]
        if d[k[0]] < 50 and np.float32(d[k[0]]) < np.float32(0.8) * np.float32(d[k[1]]):
            match[i] = cand[k[0]]
    return match, best, second, marg


def search_loops(opt, cam0, last_pose, last_pt, last_octave, last_angle, last_desc, cur_pw, cur_octave, cur_angle, cur_desc):
    """the same in plain loops, as local_map.cpp:313-368 reads (tests/test_orb_ref.py compares the two)"""
    out = []
    for i in range(len(cur_octave)):
        pc = kr.world2sensor(cam0, np.asarray(cur_pw[i], np.float64), last_pose)
        if pc[2] < 0:
            out.append((-1, -1, -1))
            continue
        p = kr.sensor2pixel(cam0, pc).astype(np.float32)
        cands = []
        for lv in range(int(cur_octave[i]), min(int(cur_octave[i]) + 2, opt.num_levels)):
            radius = PATCH * opt.scale64[lv]
            for j in range(len(last_octave)):
                if int(last_octave[j]) != lv:
                    continue
                if float(abs(np.float32(last_angle[j]) - np.float32(cur_angle[i]))) < 15:
                    dx, dy = float(p[0]) - float(last_pt[j][0]), float(p[1]) - float(last_pt[j][1])
                    if np.sqrt(dx * dx + dy * dy) < radius:
                        cands.append(j)
        b1 = b2 = (1 << 30, -1)
        for c, j in enumerate(cands):
            d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(last_desc[j], cur_desc[i]))
            if d < b1[0]:
                b1, b2 = (d, j), b1
            elif d < b2[0]:
                b2 = (d, j)
        m = -1
        if len(cands) >= 2 and b1[0] < 50 and np.float32(b1[0]) < np.float32(0.8) * np.float32(b2[0]):
            m = b1[1]
        out.append((m, b1[0] if cands else -1, b2[0] if len(cands) >= 2 else -1))
    return out


# ---- detection -------------------------------------------------------------------------------------------------------------------------------
MIN_BORDER = EDGE - 3          # extractor.cpp:375
CELL = 30                      # W, :372


def cell_grid(cols, rows):
    """the cells of ComputeKeyPointsQuadTree (:383-407) as candidate ranges (x0, x1, y0, y1), x1 / y1 exclusive, in level pixels: a cell's FAST
    sub-image [init, max) loses 3 pixels on every side.  None where the level has no cell (the reference divides by zero there)."""
    f32 = np.float32
    max_bx, max_by = cols - EDGE + 3, rows - EDGE + 3
    width, height = f32(max_bx - MIN_BORDER), f32(max_by - MIN_BORDER)
    if width <= 0 or height <= 0:
        return None
    ncols, nrows = int(width / f32(CELL)), int(height / f32(CELL))
    if ncols == 0 or nrows == 0:
        return None
    cw, ch = int(np.ceil(width / f32(ncols))), int(np.ceil(height / f32(nrows)))
    cells = []
    for i in range(nrows):
        iy = MIN_BORDER + i * ch
        my = min(iy + ch + 6, max_by)
        if iy >= max_by - 3:
            continue
        for j in range(ncols):
            ix = MIN_BORDER + j * cw
            mx = min(ix + cw + 6, max_bx)
            if ix >= max_bx - 6:
                continue
            cells.append((ix + 3, mx - 3, iy + 3, my - 3))
    return dict(ncols=ncols, nrows=nrows, cw=cw, ch=ch, cells=cells)


def cell_corners(score, rng, ini_th):
    """cv::FAST(cell, ini, nonmax) and, if that list is empty, cv::FAST(cell, min, nonmax), from the one score map: a corner is kept if its score
    is >= t and strictly greater than its 8 neighbours' (a neighbour outside the cell's candidate range counts as 0).  [(x, y, score)]"""
    x0, x1, y0, y1 = rng
    if x1 <= x0 or y1 <= y0:
        return []
    s = np.zeros((y1 - y0 + 2, x1 - x0 + 2), np.int32)
    s[1:-1, 1:-1] = score[y0:y1, x0:x1]
    c = s[1:-1, 1:-1]
    nb = np.max([s[1 + dy:s.shape[0] - 1 + dy, 1 + dx:s.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
    keep = (c > 0) & (c > nb)
    if (keep & (c >= ini_th)).any():
        keep &= c >= ini_th
    ys, xs = np.nonzero(keep)
    return [(int(x) + x0, int(y) + y0, int(c[y, x])) for y, x in zip(ys, xs)]


def level_candidates(opt, score):
    """distribute_kps of one level, relative to (MIN_BORDER, MIN_BORDER) as the reference holds them: int array [n, 3] = (x, y, score)"""
    rows, cols = score.shape
    g = cell_grid(cols, rows)
    pts = []
    if g is not None:
        for rng in g["cells"]:
            pts += [(x - MIN_BORDER, y - MIN_BORDER, s) for x, y, s in cell_corners(score, rng, opt.ini_th_fast)]
    return np.array(pts, np.int64).reshape(-1, 3)


def init_nodes(cols, rows):
    """DistributeQuadTree :165-181: (n_init, hx float32, [(ulx, uly, brx, bry)]).  n_init = 0 (the reference divides by zero) is declared 1."""
    f32 = np.float32
    W, H = cols - 2 * MIN_BORDER, rows - 2 * MIN_BORDER
    r = f32(W) / f32(H)
    n_init = max(int(np.floor(r + f32(0.5))), 1)                  # C round(): half away from zero, r > 0
    hx = f32(W) / f32(n_init)
    return n_init, hx, [(int(hx * f32(i)), 0, int(hx * f32(i + 1)), H) for i in range(n_init)]


def _children(node):
    ulx, uly, brx, bry = node
    hx, hy = (brx - ulx + 1) >> 1, (bry - uly + 1) >> 1           # ceil(float(d) / 2), :105-106
    return [(ulx, uly, ulx + hx, uly + hy), (ulx + hx, uly, brx, uly + hy), (ulx, uly + hy, ulx + hx, bry), (ulx + hx, uly + hy, brx, bry)]


def _child_of(node, x, y):
    ulx, uly, brx, bry = node
    hx, hy = (brx - ulx + 1) >> 1, (bry - uly + 1) >> 1
    return (0 if x < ulx + hx else 1) + (0 if y < uly + hy else 2)   # n1, n2, n3, n4 of :137-147


def _best(pts):
    """maximum response, ties to the smallest (y, x)"""
    return min(pts, key=lambda p: (-p[2], p[1], p[0]))


def quadtree_sets(pts, cols, rows, num):
    """DistributeQuadTree stated on sets: at any time the nodes that may still split are exactly those with more than one point, so a round is
    'child counts of every such node, choose which split, rebuild'.  Returns the sorted list of (x, y, score)."""
    f32 = np.float32
    n_init, hx, boxes = init_nodes(cols, rows)
    nodes = {}
    for p in map(tuple, pts):
        nodes.setdefault(int(f32(p[0]) / hx), []).append(p)
    nodes = [(boxes[i], v) for i, v in sorted(nodes.items())]
    careful = False
    while True:
        prev = len(nodes)
        cand = [k for k, (_, v) in enumerate(nodes) if len(v) > 1]
        split = {}
        for k in cand:
            box, v = nodes[k]
            ch = [[], [], [], []]
            for p in v:
                ch[_child_of(box, p[0], p[1])].append(p)
            split[k] = [(b, c) for b, c in zip(_children(box), ch) if c]
        if careful:
            cand.sort(key=lambda k: (-len(nodes[k][1]), nodes[k][0][1], nodes[k][0][0]))
            size, chosen = len(nodes), []
            for k in cand:
                chosen.append(k)
                size += len(split[k]) - 1
                if size >= num:
                    break
        else:
            chosen = cand
        chosen = set(chosen)
        new = [nd for k, nd in enumerate(nodes) if k not in chosen]
        expand = 0
        for k in sorted(chosen):
            new += split[k]
            expand += sum(len(c) > 1 for _, c in split[k])
        nodes = new
        if len(nodes) >= num or len(nodes) == prev:
            break
        if not careful and len(nodes) + 3 * expand > num:
            careful = True
    return sorted((_best(v) for _, v in nodes), key=lambda p: (p[1], p[0]))


def quadtree_list(pts, cols, rows, num):
    """DistributeQuadTree as extractor.cpp:160-366 reads, list and all; the pointer tie of the sort (:290) replaced by the declared one."""
    f32 = np.float32
    n_init, hx, boxes = init_nodes(cols, rows)
    lst = [dict(box=b, kps=[], no_more=False) for b in boxes]
    for p in map(tuple, pts):
        lst[int(f32(p[0]) / hx)]["kps"].append(p)
    lst = [n for n in lst if n["kps"]]
    for n in lst:
        n["no_more"] = len(n["kps"]) == 1

    def divide(n):
        ch = [dict(box=b, kps=[], no_more=False) for b in _children(n["box"])]
        for p in n["kps"]:
            ch[_child_of(n["box"], p[0], p[1])]["kps"].append(p)
        for c in ch:
            c["no_more"] = len(c["kps"]) == 1
        return ch

    finished = False
    while not finished:
        prev_size = len(lst)
        num_expand, size_and_nodes = 0, []
        for n in list(lst):                                       # the nodes pushed to the front during the walk are not visited by it
            if n["no_more"]:
                continue
            for c in divide(n):
                if c["kps"]:
                    lst.insert(0, c)
                    if len(c["kps"]) > 1:
                        num_expand += 1
                        size_and_nodes.append(c)
            lst.remove(n)
        if len(lst) >= num or len(lst) == prev_size:
            finished = True
        elif len(lst) + 3 * num_expand > num:
            while not finished:
                prev_size = len(lst)
                prev_nodes, size_and_nodes = size_and_nodes, []
                prev_nodes.sort(key=lambda n: (-len(n["kps"]), n["box"][1], n["box"][0]))
                for n in prev_nodes:
                    for c in divide(n):
                        if c["kps"]:
                            lst.insert(0, c)
                            if len(c["kps"]) > 1:
                                size_and_nodes.append(c)
                    lst.remove(n)
                    if len(lst) >= num:
                        break
                if len(lst) >= num or len(lst) == prev_size:
                    finished = True
    return sorted((_best(n["kps"]) for n in lst), key=lambda p: (p[1], p[0]))


def level_capacity(opt, cols, rows, level):
    """the most keypoints a level can return: a split adds at most 3 nodes and the careful passes stop at the first size >= num (so <= num + 2);
    a full round is only entered with size + 3 * (nodes that split) <= num, except the first, which ends with at most 4 * n_init nodes"""
    if cell_grid(cols, rows) is None:
        return 0
    return max(opt.num_desired[level] + 2, 4 * init_nodes(cols, rows)[0])


def capacity(opt, w, h):
    return sum(level_capacity(opt, *opt.level_size(w, h, L), L) for L in range(opt.num_levels))


def detect(opt, img, quadtree=quadtree_sets):
    """Extractor::Detect: dict(levels, scores, level_count, pt [n, 2] f32, octave, angle, response, size), level-major, each level by (y, x)"""
    f32 = np.float32
    levels = pyramid(opt, img)
    scores = [fast_score(g, opt.min_th_fast) for g in levels]
    pt, octave, resp, size, count = [], [], [], [], []
    for L, (g, s) in enumerate(zip(levels, scores)):
        rows, cols = g.shape
        kps = quadtree(level_candidates(opt, s), cols, rows, opt.num_desired[L]) if cell_grid(cols, rows) is not None else []
        assert len(kps) <= level_capacity(opt, cols, rows, L)
        count.append(len(kps))
        for x, y, r in kps:
            pt.append((f32(x + MIN_BORDER) * opt.scale[L], f32(y + MIN_BORDER) * opt.scale[L]))
            octave.append(L); resp.append(f32(r)); size.append(f32(int(f32(PATCH) * opt.scale[L])))
    pt, octave = np.array(pt, f32).reshape(-1, 2), np.array(octave, np.int32)
    return dict(levels=levels, scores=scores, level_count=np.array(count, np.int32), pt=pt, octave=octave, angle=orientation(opt, levels, pt, octave),
                response=np.array(resp, f32), size=np.array(size, f32))
