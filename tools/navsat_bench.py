#!/usr/bin/env python3
"""Times the per-keyframe GNSS fix of a section (the loop of Navsat::Optimize / QuickFix, navsat.cpp:150-155) two ways, in ONE process and
alternating: (a) lvf_navsat_fix_chain — the whole loop as one launch — and (b) the same work as n - 1 lvf_navsat_optimize_bc(mode 0b110111)
calls, the straightforward port that (a) exists to avoid.  Each timed call is bracketed by device events and ends in a synchronise (the
C calls wait for their own results).  Prints one JSON line: medians, spreads, launches per call, bytes over PCIe, the box calibration.

    python tools/navsat_bench.py [--sizes 64,256,1024] [--warmup 20] [--reps 200]
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


def section(n, seed):
    """n keyframes after B (C last) on a winding road, fixes with 0.15 m noise and an outlier every 7th, one keyframe in five without a fix."""
    rng = np.random.default_rng(seed)
    yaw = 0.3 + np.cumsum(rng.normal(0.0, 0.03, n))
    h = yaw / 2
    poses = np.zeros((n, 7))
    poses[:, 2], poses[:, 3] = np.sin(h), np.cos(h)
    fwd = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(n)], axis=1)
    poses[1:, 4:] = np.cumsum(fwd[:-1], axis=0)
    fix = poses[:-1, 4:] + rng.normal(0.0, 0.15, (n - 1, 3))
    fix[::7] += rng.normal(0.0, 1.5, fix[::7].shape)
    has = (rng.uniform(size=n - 1) >= 0.2).astype(np.int32)
    cov = rng.uniform(0.02, 0.2, (n - 1, 3))
    return poses, has, fix, cov


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median_us": float(np.median(v)), "p10_us": float(v[len(v) // 10]), "p90_us": float(v[(9 * len(v)) // 10]), "n": int(len(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    ctx = api.Context(0)
    opt = api.navsat_bc_options(mode=0b110111)
    out = {"box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx), "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        poses, has, fix, cov = section(n, n)

        def chain():
            P = poses.copy()
            ctx.timer_begin()
            x, it, _ = api.navsat_fix_chain(ctx, P, has, fix, cov)
            ctx.timer_end()
            return 1e3 * ctx.timer_ms(), P, int(it.sum())

        def separate():
            Q = poses.copy()
            ctx.timer_begin()
            for k in range(n - 1):
                api.navsat_optimize_bc(ctx, Q[k:], 1, has[k:k + 1], fix[k:k + 1], cov[k:k + 1], opt)
            ctx.timer_end()
            return 1e3 * ctx.timer_ms(), Q

        ta, tb = [], []
        for rep in range(a.warmup + a.reps):
            us_a, P, iters = chain()
            us_b, Q = separate()
            if rep >= a.warmup:
                ta.append(us_a); tb.append(us_b)
        steps = n - 1
        # bytes over PCIe per call: (a) poses up and down, has_fix / fix / cov up, x / iterations / one record down;
        # (b) step k moves the n - k poses behind it up and down, one block's inputs up and one record down
        bytes_a = 2 * 56 * n + steps * (4 + 24 + 24) + steps * (8 + 4) + 32
        bytes_b = sum(2 * 56 * (n - k) + (4 + 24 + 24) + 176 for k in range(steps))
        out["sizes"][str(n)] = {
            "fix_chain_one_launch": dict(stats(ta), launches_per_call=1, pcie_bytes_per_call=bytes_a),
            "separate_optimize_bc_calls": dict(stats(tb), launches_per_call=steps, pcie_bytes_per_call=bytes_b),
            "speedup_of_medians": float(np.median(tb) / np.median(ta)),
            "lm_iterations_in_chain": iters,
            "us_per_chain_step": float(np.median(ta) / steps),
            "max_abs_pose_difference": float(np.abs(P - Q).max()),
        }
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
