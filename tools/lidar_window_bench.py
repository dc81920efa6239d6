#!/usr/bin/env python3
"""Times one LM iteration of the 50-keyframe / 10 000-landmark bench window (bench.py's) in three set-ups:

    fused        the window as bench.py solves it (the fused chain: the candidate pass linearises)
    plain        the same window on the non-fused chain — what a window with lidar planes runs — forced by ONE pose-prior block of weight 0
                 (zero residual, zero Jacobian: an empty batch would not count as priors); the fair parent of the third set-up
    lidar        `plain` without the prior block, with 50 x 2 000 LiDAR plane blocks on the keyframe poses

The three ALTERNATE, their order rotated every repetition; a repetition of a set-up is one lvf_problem_solve of --iterations iterations from the
same start, bracketed by device events and by the host clock; figures are per iteration.  The two new launches alone come from
lvf_problem_stage_times: k_lidar_lin closes the linearisation right ahead of k_prepare and k_lidar_cost runs ahead of k_cost_decide, so they
are the growth of those two stages' spans from `plain` to `lidar`.  Prints one JSON line: medians with p10 / p90.

    python tools/lidar_window_bench.py [--warmup 5] [--reps 30] [--iterations 10] [--per-kf 2000]
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

import bench  # noqa: E402
from lvio_fusion_amd import api, synthetic as syn  # noqa: E402
from tests.lidar_window_cases import plane_blocks  # noqa: E402  (the tests' scene: three mutually non-parallel planes, 1 cm of range noise)
from tools.klt_bench import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--per-kf", type=int, default=2000)
    a = ap.parse_args()
    ctx = api.Context(0)
    out = {"box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx), "iterations_per_solve": a.iterations}
    opt = bench.fixed_iterations(api, a.iterations)
    setups, keep = {}, []
    for name in ("fused", "plain", "lidar"):
        cfg, prob, handles = bench.build_window(api, syn, ctx)
        keep += [prob] + [h for h in handles if h is not None]
        if name == "plain":
            b = api.pose_prior_batch(ctx, [-1], [0], cfg["poses"][:1], [0.0], [0.0])
            prob.set_pose_priors(b); keep.append(b)
        if name == "lidar":
            blocks = plane_blocks(cfg["poses_true"], a.per_kf, np.random.default_rng(1))
            b = api.lidar_pose_batch(ctx, *blocks, weight=100.0, huber_a=0.0)
            prob.set_lidar_planes(b); keep.append(b)
            out["lidar_blocks"] = b.n
        setups[name] = (cfg, prob, handles[-1])
    out["n_kf"], out["n_lm"] = setups["fused"][0]["n_kf"], setups["fused"][0]["n_lm"]
    names = list(setups)
    rec = {n: {"dev": [], "host": []} for n in names}
    summaries = {}
    for i in range(a.warmup + a.reps):
        for n in names[i % 3:] + names[:i % 3]:
            cfg, prob, st = setups[n]
            bench.reset_state(api, st, cfg)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.timer_begin()
            summaries[n] = prob.solve(opt)
            ctx.timer_end()
            ms = ctx.timer_ms()
            t1 = time.perf_counter()
            if i >= a.warmup:
                rec[n]["dev"].append(1e3 * ms / a.iterations); rec[n]["host"].append(1e6 * (t1 - t0) / a.iterations)
    for n in names:
        s = summaries[n]
        out[n] = {"per_iteration_device_events": stats(rec[n]["dev"]), "per_iteration_host_clock": stats(rec[n]["host"]), "iterations": s.num_iterations,
                  "accepted": s.num_successful_steps, "final_cost": s.final_cost, "residual_blocks": s.num_residual_blocks}
    out["lidar_minus_plain"] = {"per_iteration_device_events": stats(np.array(rec["lidar"]["dev"]) - np.array(rec["plain"]["dev"]))}
    out["plain_minus_fused"] = {"per_iteration_device_events": stats(np.array(rec["plain"]["dev"]) - np.array(rec["fused"]["dev"]))}
    # the stages of one iteration (kernel durations where every launch of the stage carries its own events, the stage's span otherwise)
    stages = {}
    for n in names:
        cfg, prob, st = setups[n]
        bench.reset_state(api, st, cfg)
        stages[n] = prob.stage_times(api.default_solver_options(), radius=1e4, reps=10, spans=True)
        out[n]["stages"] = [{"stage": name.split(" ")[0], "us": us, "launches": la, "span_us": sp} for name, us, la, sp in stages[n] if la]
        out[n]["launches_per_iteration"] = int(sum(la for _, _, la, _ in stages[n]))
    span = lambda n, key: next(sp for name, _, _, sp in stages[n] if name.startswith(key))
    out["k_lidar_lin_us"] = span("lidar", "k_prepare") - span("plain", "k_prepare")
    out["k_lidar_cost_us"] = span("lidar", "k_cost_decide") - span("plain", "k_cost_decide")
    for h in keep:
        h.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
