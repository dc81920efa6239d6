#!/usr/bin/env python3
"""Times the LiDAR sweep deskew on a 115 200-point syn.raw_scan against the call it extends: lvf_lidar_extract (the baseline),
lvf_lidar_extract_deskewed on the same scan with a 3-keyframe trajectory (two more launches inside the same one-wait chain) and
lvf_cloud_deskew alone on the plain call's surf picks (one launch, then the context is waited for).  Each timed call is bracketed by device
events AND by the host clock.  The two extraction calls ALTERNATE, one of each per repetition with the order swapped every repetition, so
that whatever else the machine is doing falls on both alike; the difference is taken pair by pair.  Prints one JSON line with the three
medians (p10 / p90 alongside) and the median of the paired differences deskewed - plain.

    python tools/deskew_bench.py [--warmup 20] [--reps 100]
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

from lvio_fusion_amd import api, synthetic as syn  # noqa: E402
from tools.klt_bench import stats, timed  # noqa: E402


def timed_alternating(ctx, fa, fb, warmup, reps):
    """one call of each per repetition, the order swapped every repetition: (a, b, b - a pair by pair), each as timed() reports"""
    rec = {k: {"dev": [], "host": []} for k in "ab"}
    for i in range(warmup + reps):
        for k in ("ab" if i % 2 == 0 else "ba"):
            t0 = time.perf_counter()
            ctx.timer_begin()
            (fa if k == "a" else fb)()
            ctx.timer_end()
            ms = ctx.timer_ms()
            t1 = time.perf_counter()
            if i >= warmup:
                rec[k]["dev"].append(1e3 * ms); rec[k]["host"].append(1e6 * (t1 - t0))
    res = {k: {"device_events": stats(rec[k]["dev"]), "host_clock": stats(rec[k]["host"])} for k in "ab"}
    diff = {"device_events": stats(np.array(rec["b"]["dev"]) - np.array(rec["a"]["dev"])), "host_clock": stats(np.array(rec["b"]["host"]) - np.array(rec["a"]["host"]))}
    return res["a"], res["b"], diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    ctx = api.Context(0)
    scan = syn.raw_scan(seed=0x5CA9)
    ext = syn.lidar_extrinsic()
    prm = api.lidar_params()
    # 3 keyframes 0.1 s apart at 15 m/s and 0.3 rad/s; the scan belongs to the newest one
    stamps = 0.1 * np.arange(3)
    yaw = 0.3 * stamps
    poses = np.concatenate([syn.quat_from_ypr(yaw, 0 * yaw, 0 * yaw).reshape(3, 4), np.stack([15.0 * stamps * np.cos(yaw), 15.0 * stamps * np.sin(yaw), 0 * yaw], 1)], 1)
    traj = api.Trajectory(ctx, stamps, poses)
    g, s, dbg = api.lidar_extract(ctx, scan, ext, params=prm, debug=True)
    picks = api.Cloud(ctx, dbg["surf_raw"])
    out = {"scan_points": int(scan.shape[0]), "ground_picks": int(len(dbg["ground_raw"])), "surf_picks": int(len(dbg["surf_raw"])), "ground": len(g), "surf": len(s),
           "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}
    g.close(); s.close()

    def plain():
        for c in api.lidar_extract(ctx, scan, ext, params=prm):
            c.close()

    def deskewed():
        for c in api.lidar_extract_deskewed(ctx, scan, ext, traj, stamps[2], poses[2], params=prm):
            c.close()

    def alone():
        d = picks.deskew(traj, stamps[2], poses[2], prm.cycle_time, ext)
        ctx.synchronize()
        d.close()

    out["lidar_extract"], out["lidar_extract_deskewed"], out["deskewed_minus_plain"] = timed_alternating(ctx, plain, deskewed, a.warmup, a.reps)
    out["cloud_deskew"] = timed(ctx, alone, a.warmup, a.reps)
    out["extract_fallbacks"] = api.extract_fallbacks(ctx)      # 0: every timed extraction finished on the device-counted path
    picks.close(); traj.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
