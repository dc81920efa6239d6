#!/usr/bin/env python3
"""Times the LiDAR place recognition:

    describe    Cloud.scan_context on a 115 200-point sweep (64 rings x 1 800 columns), download included
    search      ScanContextDb.search with K = 5 against 1 000 and 10 000 entries
    detect      ScanContextDb.detect (describe + search + select, one wait, no append) against the same databases

The sweep is a synthetic sensor-frame cloud (ranges 1 .. 90 m, heights -2.5 .. 12 m); the database holds random descriptors with 30 % empty
cells, so every column pair is valid and the search does its full work.  Each timed call is bracketed by device events AND by the host clock.
Prints one JSON line: medians with p10 / p90.

    python tools/scanctx_bench.py [--warmup 20] [--reps 100]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lvio_fusion_amd import api  # noqa: E402
from tools.klt_bench import timed  # noqa: E402


def sweep(seed, n):
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(1.0, 90.0, n), np.sort(rng.uniform(-np.pi, np.pi, n))      # (scan order: consecutive points share sectors)
    out = np.zeros((n, 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = r * np.cos(a), r * np.sin(a), rng.uniform(-2.5, 12.0, n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--points", type=int, default=115200)
    ap.add_argument("--entries", default="1000,10000")
    ap.add_argument("--k", type=int, default=5)
    a = ap.parse_args()
    ctx = api.Context(0)
    cloud = api.Cloud(ctx, sweep(1, a.points))
    desc, _ = cloud.scan_context()
    out = {"points": a.points, "k": a.k, "occupied_cells": int((desc > 0).sum()),
           "box_calibration": api.box_calibration(ctx) if hasattr(api, "box_calibration") else None}
    out["describe"] = timed(ctx, lambda: cloud.scan_context(), a.warmup, a.reps)
    rng = np.random.default_rng(2)
    for n in [int(v) for v in a.entries.split(",")]:
        db = api.ScanContextDb(ctx, n)
        for i in range(n):
            d = rng.integers(1, 256, (60, 20)).astype(np.uint8)
            d[rng.uniform(size=d.shape) < 0.3] = 0
            db.append_descriptor(d, float(i))
        out["search_%d" % n] = timed(ctx, lambda: db.search(desc, k=a.k), a.warmup, a.reps)
        out["detect_%d" % n] = timed(ctx, lambda: db.detect(cloud, float(n), k=a.k, append=False), a.warmup, a.reps)
        db.close()
    print(json.dumps(out))
    cloud.close()
    ctx.close()


if __name__ == "__main__":
    main()
