#!/usr/bin/env python3
"""Times the ORB front-end at KITTI size (1241 x 376): the scale pyramid with the FAST score maps (lvf_orb_set_image), one lvf_orb_detect
(pyramid, score, cells, quadtree, orientation and its one download), lvf_orb_compute of 500 keypoints (blur of the levels they lie on and
rBRIEF) and lvf_orb_search of 500 current against 500 last features.  Each timed call is bracketed by device events AND by the host clock;
the C calls wait for their own results, so both include the copies up and down.  The image is an analytic texture; the second view of the
search is the first displaced by a few pixels.  Prints one JSON line.

    python tools/orb_bench.py [--warmup 20] [--reps 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lvio_fusion_amd import api  # noqa: E402
from tools.klt_bench import W, H, stats, texture, timed  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    ctx = api.Context(0)
    image = texture(7)
    shift = (3.7, -2.2)                                  # B(x) = A(x - shift): a point of A at p is at p + shift in B
    ia, ib = api.Image(ctx, image(0.0, 0.0), 3), api.Image(ctx, image(-shift[0], -shift[1]), 3)
    orb_a, orb_b = api.Orb(ctx), api.Orb(ctx)
    out = {"image": [W, H], "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}
    out["pyramid_and_score"] = timed(ctx, lambda: orb_a.set_image(ia) or ctx.synchronize(), a.warmup, a.reps)
    out["detect"] = timed(ctx, lambda: orb_a.detect(ia), a.warmup, a.reps)
    da, db = orb_a.detect(ia), orb_b.detect(ib)
    out["detect"].update(keypoints=int(len(da["pt"])), level_count=da["level_count"].tolist())

    def compute():
        orb_a.set_image(ia)                              # (a new frame: the blurred levels are made again)
        return orb_a.compute(da["pt"], da["octave"], da["angle"])

    out["compute"] = timed(ctx, compute, a.warmup, a.reps)
    out["compute"]["keypoints"] = int(len(da["pt"]))
    desc_a, desc_b = compute(), orb_b.compute(db["pt"], db["octave"], db["angle"])
    # landmarks of the current (B) features, 10 m in front of the last camera where they were in A
    cam0 = dict(fx=718.856, fy=718.856, cx=607.19, cy=185.2, extrinsic=np.array([0, 0, 0, 1.0, 0, 0, 0]))
    pose = np.array([0, 0, 0, 1.0, 0, 0, 0])
    in_a = db["pt"].astype(np.float64) - np.array(shift)
    pw = np.stack([(in_a[:, 0] - cam0["cx"]) * 10.0 / cam0["fx"], (in_a[:, 1] - cam0["cy"]) * 10.0 / cam0["fy"], np.full(len(in_a), 10.0)], 1)
    args = (cam0, pose, da["pt"], da["octave"], da["angle"], desc_a, pw, db["octave"], db["angle"], desc_b)
    out["search"] = timed(ctx, lambda: api.orb_search(ctx, *args), a.warmup, a.reps)
    m, _, _ = api.orb_search(ctx, *args)
    out["search"].update(last=int(len(da["pt"])), current=int(len(db["pt"])), matched=int((m >= 0).sum()))
    for x in (orb_a, orb_b, ia, ib):
        x.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
