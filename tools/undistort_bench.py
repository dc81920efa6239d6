#!/usr/bin/env python3
"""Times the image undistortion at KITTI size (1241 x 376) against the call it extends: lvf_image_create on the same pixels (upload,
3 decimations, 4 Scharr passes — what a caller without lens distortion pays), lvf_image_create_undistorted (the same plus the staging upload
and the remap) and lvf_image_pair_create_undistorted (Estimator::InputImage: two frames, one wait).  Each timed call is bracketed by device
events AND by the host clock; the C calls wait for their own results.  Prints one JSON line with the three medians and the differences
(undistorted - plain, and pair - 2 x plain).

    python tools/undistort_bench.py [--warmup 20] [--reps 100]
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
from tools.klt_bench import W, H, texture, timed  # noqa: E402

DIST = (-0.28, 0.07, 2e-3, -1.5e-3)          # EuRoC-like


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    ctx = api.Context(0)
    image = texture(7)
    px0, px1 = image(0.0, 0.0), image(-12.0, 0.0)
    cam0 = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
    cam1 = dict(cam0, cx=604.0814, cy=183.1104)
    u0, u1 = api.Undistort(ctx, cam0, DIST, W, H), api.Undistort(ctx, cam1, DIST, W, H)
    out = {"image": [W, H], "distortion": list(DIST), "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}
    made = []

    def keep(*imgs):
        made.extend(imgs)
        while len(made) > 8:
            made.pop(0).close()

    out["image_create"] = timed(ctx, lambda: keep(api.Image(ctx, px0, 3)), a.warmup, a.reps)
    out["image_create_undistorted"] = timed(ctx, lambda: keep(u0.image(px0, 3)), a.warmup, a.reps)
    out["image_pair_create_undistorted"] = timed(ctx, lambda: keep(*u0.pair(u1, px0, px1, 3)), a.warmup, a.reps)
    for clock in ("device_events", "host_clock"):
        plain, one, pair = (out[k][clock]["median_us"] for k in ("image_create", "image_create_undistorted", "image_pair_create_undistorted"))
        out["difference_" + clock] = {"undistorted_minus_plain_us": one - plain, "pair_minus_two_plain_us": pair - 2 * plain}
    for im in made:
        im.close()
    u0.close(); u1.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
