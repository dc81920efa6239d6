#!/usr/bin/env python3
"""Times one LM iteration of the 50-keyframe / 10 000-landmark bench window (bench.py's) in four set-ups, and the marginalising slide
beside the plain one:

    fused        the window as bench.py solves it (the fused chain: the candidate pass linearises)
    plain        the same window on the non-fused chain — what a window with pose priors runs — forced by ONE pose-prior block of weight 0
    dense1       `plain` plus a dense prior on keyframe 0
    dense8       `plain` plus a dense prior on keyframes 0 .. 7

The four ALTERNATE, their order rotated every repetition; a repetition of a set-up is one lvf_problem_solve of --iterations iterations from
the same start, bracketed by device events; figures are per iteration.  A window that has taken its first marginalising slide pays
dense1 - fused per iteration from then on (less the two pose-prior launches when it has no weak-constraint prior).  The two new launches
alone are the growth of the k_prepare and k_cost_decide stages' spans from `plain` to `dense1` / `dense8` (lvf_problem_stage_times).

The slides: a persistent window over the same scene, --slide-reps times from scratch: Window.slide past one keyframe against
Window.slide_marginalize past one keyframe, host clock around the call (the marginalising slide waits for its result; the plain one
touches no device).  Prints one JSON line: medians with p10 / p90.

    python tools/dense_prior_bench.py [--warmup 5] [--reps 30] [--iterations 10] [--slide-reps 5]
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
from tools.klt_bench import stats  # noqa: E402


def prior_on(ctx, cfg, kfs, rng):
    """a full-rank prior at the window's own state (e = 0 at the start), weights of the order of the visual blocks'"""
    m = 15 * len(kfs)
    A = 30.0 * rng.normal(size=(m + 5, m))
    x0 = np.array([np.concatenate([cfg["poses"][k], cfg["vel"][k], cfg["ba"][k], cfg["bg"][k]]) for k in kfs])
    return api.DensePrior(ctx, kfs, x0, A.T @ A, None, 0.0)


def fill_window(win, cfg, pre):
    tc, tf = cfg["tc"], cfg["tf"]
    by_kf_tc = [np.nonzero(tc["kf_idx"] == t)[0] for t in range(cfg["n_kf"])]
    by_kf_tf = [np.nonzero(tf["kf2_idx"] == t)[0] for t in range(cfg["n_kf"])]
    for t in range(cfg["n_kf"]):
        win.add_keyframe(100 + t, cfg["poses"][t], cfg["w_kf"][t])
        win.set_imu(100 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], pre[t - 1] if t > 0 else None)
        for i in by_kf_tc[t]:
            win.add_landmark(5000 + int(tc["lm_idx"][i]), 100 + t, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][int(tc["lm_idx"][i])])
        for i in by_kf_tf[t]:
            win.add_observation(5000 + int(tf["lm_idx"][i]), 100 + t, tf["ob"][i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--slide-reps", type=int, default=5)
    a = ap.parse_args()
    ctx = api.Context(0)
    out = {"box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx), "iterations_per_solve": a.iterations}
    opt = bench.fixed_iterations(api, a.iterations)
    rng = np.random.default_rng(1)
    setups, keep = {}, []
    for name in ("fused", "plain", "dense1", "dense8"):
        cfg, prob, handles = bench.build_window(api, syn, ctx)
        keep += [prob] + [h for h in handles if h is not None]
        if name != "fused":                  # (dense1 / dense8 are `plain` PLUS a dense prior: they keep its pose-prior block)
            b = api.pose_prior_batch(ctx, [-1], [0], cfg["poses"][:1], [0.0], [0.0])
            prob.set_pose_priors(b); keep.append(b)
        if name.startswith("dense"):
            d = prior_on(ctx, cfg, list(range(int(name[5:]))), rng)
            prob.set_dense_prior(d); keep.append(d)
        setups[name] = (cfg, prob, handles[-1])
    out["n_kf"], out["n_lm"] = setups["fused"][0]["n_kf"], setups["fused"][0]["n_lm"]
    names = list(setups)
    rec = {n: [] for n in names}
    summaries = {}
    for i in range(a.warmup + a.reps):
        r = i % len(names)
        for n in names[r:] + names[:r]:
            cfg, prob, st = setups[n]
            bench.reset_state(api, st, cfg)
            ctx.synchronize()
            ctx.timer_begin()
            summaries[n] = prob.solve(opt)
            ctx.timer_end()
            if i >= a.warmup:
                rec[n].append(1e3 * ctx.timer_ms() / a.iterations)
    for n in names:
        s = summaries[n]
        out[n] = {"per_iteration_device_events": stats(rec[n]), "iterations": s.num_iterations, "accepted": s.num_successful_steps, "final_cost": s.final_cost,
                  "residual_blocks": s.num_residual_blocks}
    for x, y in (("plain", "fused"), ("dense1", "plain"), ("dense8", "plain"), ("dense1", "fused")):
        out[f"{x}_minus_{y}"] = {"per_iteration_device_events": stats(np.array(rec[x]) - np.array(rec[y]))}
    stages = {}
    for n in names:
        cfg, prob, st = setups[n]
        bench.reset_state(api, st, cfg)
        stages[n] = prob.stage_times(api.default_solver_options(), radius=1e4, reps=10, spans=True)
        out[n]["launches_per_iteration"] = int(sum(la for _, _, la, _ in stages[n]))
    span = lambda n, key: next(sp for name, _, _, sp in stages[n] if name.startswith(key))
    for n in ("dense1", "dense8"):
        out[f"k_dense_prior_lin_us_{n}"] = span(n, "k_prepare") - span("plain", "k_prepare")
        out[f"k_dense_prior_cost_us_{n}"] = span(n, "k_cost_decide") - span("plain", "k_cost_decide")
    # the slides
    cfg = setups["fused"][0]
    from oracle import pyoracle as po
    pre = [po.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]]
    o0 = api.default_solver_options(); o0.max_num_iterations = 0
    t_plain, t_marg, last = [], [], None
    for i in range(a.slide_reps + 1):
        for kind in ("plain", "marginalize"):
            win = api.Window(ctx, cfg["cam0"], cfg["cam1"], baseline=syn.baseline())
            fill_window(win, cfg, pre)
            win.solve(o0)
            if kind == "marginalize" and i == 0:
                win.slide_marginalize(100, api.default_solver_options())      # (no departing keyframe: nothing happens)
            ctx.synchronize()
            t0 = time.perf_counter()
            if kind == "plain":
                win.slide(101)
            else:
                last = win.slide_marginalize(101, api.default_solver_options())
            t1 = time.perf_counter()
            if kind == "marginalize":
                # the second marginalising slide of the same window: the sub-problem's buffers are warm
                t2 = time.perf_counter()
                last = win.slide_marginalize(102, api.default_solver_options())
                t3 = time.perf_counter()
                if i > 0:
                    t_marg.append(1e3 * (t3 - t2))
            elif i > 0:
                t_plain.append(1e3 * (t1 - t0))
            win.close()
    out["slide_ms"] = stats(t_plain)
    out["slide_marginalize_ms_warm"] = stats(t_marg)
    out["slide_marginalize_stats"] = last
    for h in keep:
        h.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
