#!/usr/bin/env python3
"""Times the LiDAR depth for visual features:

    create      LidarDepth on a 115 200-point sweep (64 rings x 1 800 columns over a street), projected into a 1241 x 376 camera; the call
                queues its launches and returns, so the timed region ends with len(), the 4-byte read-back that waits for the chain
    query       LidarDepth.query at 500 and 2 000 features (upload, one launch, five arrays down)
    stereo      stereo_triangulate alone on 1241 x 376 images at the same feature counts
    fused       stereo_triangulate_lidar at the same feature counts, in the same run: the figure to judge is fused - stereo

The sweep is tests/lidar_depth_cases.street's scene at full azimuth resolution and all around; the images are a klt_ref.Texture pair with the
disparity of tests/klt_cases.  Each timed call is bracketed by device events AND by the host clock.  Prints one JSON line: medians with p10 / p90.

    python tools/lidar_depth_bench.py [--warmup 20] [--reps 100]
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

W, H = 1241, 376


def sweep(n_rings=64, n_columns=1800):
    """the street of the tests, all around: ground, a wall 40 m ahead, a side wall, nothing behind beyond the ground (ring-major scan order)"""
    from tests import lidar_depth_cases as lc
    el = np.deg2rad(np.linspace(2.0, -24.8, n_rings))
    az = np.deg2rad(np.arange(n_columns) * (360.0 / n_columns) - 180.0)
    E, A = np.meshgrid(el, az, indexing="ij")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    t, _ = lc.cast(np.zeros(3), d)
    t = np.where(np.isfinite(t) & (t < 80.0), t, 0.0)                    # (no return: the driver's zero point, dropped by min_depth)
    out = np.zeros((len(d), 4), np.float32)
    out[:, :3] = d * t[:, None]
    out[:, 3] = np.repeat(np.arange(n_rings), n_columns)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--features", default="500,2000")
    a = ap.parse_args()
    from tests import klt_cases as kc, klt_ref as kr, lidar_depth_cases as lc
    s = lc.street(n_features=10)
    cam0, cam1, baseline, M = s["cam0"], s["cam1"], s["baseline"], s["M"]
    ctx = api.Context(0)
    pts = sweep()
    cloud = api.Cloud(ctx, pts)
    depth = api.LidarDepth(ctx, cloud, cam0, M, W, H)
    out = {"points": len(pts), "kept": len(depth), "width": W, "height": H, "box_calibration": api.box_calibration(ctx) if hasattr(api, "box_calibration") else None}

    def create():
        d = api.LidarDepth(ctx, cloud, cam0, M, W, H)
        n = len(d)
        d.close()
        return n

    out["create"] = timed(ctx, create, a.warmup, a.reps)
    tex = kr.Texture(5)
    left = tex.image(W, H)
    right = tex.image(W, H, lambda x, y: (x + kc.disparity(y, H), y))
    il, ir = api.Image(ctx, left, 3), api.Image(ctx, right, 3)
    rng = np.random.default_rng(3)
    for n in [int(v) for v in a.features.split(",")]:
        kps = np.stack([rng.uniform(40.0, W - 4.0, n), rng.uniform(0.4 * H, H - 4.0, n)], 1).astype(np.float32)
        st = depth.query(cam1, kps)[0]
        src = api.stereo_triangulate_lidar(il, ir, cam0, cam1, baseline, kps, depth)[4]
        out["accepted_%d" % n] = int((st == 1).sum())
        out["source_%d" % n] = np.bincount(src, minlength=3).tolist()
        out["query_%d" % n] = timed(ctx, lambda: depth.query(cam1, kps), a.warmup, a.reps)
        out["stereo_%d" % n] = timed(ctx, lambda: api.stereo_triangulate(il, ir, cam0, cam1, baseline, kps), a.warmup, a.reps)
        out["fused_%d" % n] = timed(ctx, lambda: api.stereo_triangulate_lidar(il, ir, cam0, cam1, baseline, kps, depth), a.warmup, a.reps)
        out["fused_minus_stereo_%d" % n] = {k: {"median_us": out["fused_%d" % n][k]["median_us"] - out["stereo_%d" % n][k]["median_us"]} for k in ("device_events", "host_clock")}
    print(json.dumps(out))
    for h in (il, ir, depth, cloud):
        h.close()
    ctx.close()


if __name__ == "__main__":
    main()
