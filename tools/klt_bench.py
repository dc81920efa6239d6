#!/usr/bin/env python3
"""Times the feature tracker at KITTI size (1241 x 376): the image object's build (upload, 3 decimations, 4 Scharr passes) and one
lvf_optical_flow call (21 x 21 / 4 levels forward, 3 x 3 / 2 levels backward, gate) at N = 500 / 1500 / 5000 points.  Each timed call is
bracketed by device events AND by the host clock; the C calls wait for their own results, so both include the copies of the points up and
the results down.  The second image is the first one displaced by a few pixels (an analytic texture sampled at shifted coordinates) and
the initial flow is off by N(0, 3 px), so the iteration counts are those of a real frame pair.  Prints one JSON line.

    python tools/klt_bench.py [--sizes 500,1500,5000] [--warmup 20] [--reps 100]
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

W, H = 1241, 376


def texture(seed, n_waves=60, sigma=45.0):
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(8.0), np.log(80.0), n_waves))
    th = rng.uniform(0, 2 * np.pi, n_waves)
    u, v, ph = np.cos(th) / lam, np.sin(th) / lam, rng.uniform(0, 2 * np.pi, n_waves)
    amp = rng.uniform(0.5, 1.0, n_waves)
    amp *= sigma / np.sqrt(0.5 * np.sum(amp ** 2))

    def image(dx, dy):
        x, y = np.meshgrid(np.arange(W, dtype=np.float64) + dx, np.arange(H, dtype=np.float64) + dy)
        acc = np.zeros((H, W))
        for k in range(n_waves):
            acc += amp[k] * np.sin(2 * np.pi * (u[k] * x + v[k] * y) + ph[k])
        return np.clip(np.rint(128 + acc), 0, 255).astype(np.uint8)

    return image


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median_us": float(np.median(v)), "p10_us": float(v[len(v) // 10]), "p90_us": float(v[(9 * len(v)) // 10]), "n": int(len(v))}


def timed(ctx, fn, warmup, reps):
    dev, host = [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        ctx.timer_begin()
        fn()
        ctx.timer_end()
        ms = ctx.timer_ms()
        t1 = time.perf_counter()
        if i >= warmup:
            dev.append(1e3 * ms); host.append(1e6 * (t1 - t0))
    return {"device_events": stats(dev), "host_clock": stats(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,1500,5000")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    ctx = api.Context(0)
    image = texture(7)
    shift = (3.7, -2.2)                                  # B(x) = A(x - shift): a point of A at p is at p + shift in B
    a_px, b_px = image(0.0, 0.0), image(-shift[0], -shift[1])
    out = {"image": [W, H], "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}
    made = []

    def build():
        made.append(api.Image(ctx, a_px, 3))
        if len(made) > 4:
            made.pop(0).close()

    out["image_create"] = timed(ctx, build, a.warmup, a.reps)
    for im in made:
        im.close()
    ia, ib = api.Image(ctx, a_px, 3), api.Image(ctx, b_px, 3)
    out["sizes"] = {}
    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        prev = np.stack([rng.uniform(12, W - 12, n), rng.uniform(12, H - 12, n)], 1).astype(np.float32)
        init = (prev + np.array(shift) + rng.normal(0, 3, (n, 2))).astype(np.float32)
        res = timed(ctx, lambda: api.optical_flow(ia, ib, prev, init), a.warmup, a.reps)
        nxt, st, _ = api.optical_flow(ia, ib, prev, init)
        err = np.linalg.norm(nxt[st > 0] - (prev[st > 0] + np.array(shift, np.float32)), axis=1)
        res.update(accepted=int(st.sum()), median_error_px=float(np.median(err)) if len(err) else None)
        out["sizes"][str(n)] = res
    ia.close(); ib.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
