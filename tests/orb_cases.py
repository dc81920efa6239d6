"""Seeded images for the ORB tests (tests/test_orb_ref.py on the CPU, tests/test_gpu_orb.py on the device)."""
import functools

import numpy as np

from tests import klt_ref as kr


@functools.lru_cache(maxsize=None)
def texture(seed, w, h):
    """klt_ref.Texture: smooth, about 4 800 corners after NMS at threshold 14 at 640 x 376"""
    return kr.Texture(seed).image(w, h)


@functools.lru_cache(maxsize=None)
def rectangles(seed, w, h, n=None):
    """random grey rectangles painted over each other plus sigma = 2 noise: sharp corners of every contrast (about 210 at 200 x 150)"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128.0)
    for _ in range(n if n is not None else max(w * h // 250, 8)):
        x0, y0 = rng.integers(0, w), rng.integers(0, h)
        rw, rh = rng.integers(4, max(w // 4, 6)), rng.integers(4, max(h // 4, 6))
        img[y0:y0 + rh, x0:x0 + rw] = rng.uniform(20, 235)
    return np.clip(np.rint(img + rng.normal(0, 2, (h, w))), 0, 255).astype(np.uint8)


def random_keypoints(opt, w, h, n, seed):
    """n keypoints spread over the levels, as Detect would scale them: (pt [n, 2] float32, octave [n] int32)"""
    rng = np.random.default_rng(seed)
    octave = rng.integers(0, opt.num_levels, n).astype(np.int32)
    pt = np.zeros((n, 2), np.float32)
    for i, o in enumerate(octave):
        lw, lh = opt.level_size(w, h, int(o))
        pt[i] = np.float32(rng.integers(31, lw - 31)) * opt.scale[o], np.float32(rng.integers(31, lh - 31)) * opt.scale[o]
    return pt, octave
