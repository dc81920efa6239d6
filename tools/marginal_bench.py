#!/usr/bin/env python3
"""Times the marginal covariance of keyframes on the 50-keyframe / 10 000-landmark window, beside one LM iteration of the same window:

    marginal_1 / marginal_8   Problem.marginal for the newest keyframe / the newest eight (linearisation, undamped reduced system, gather,
                              elimination of the rest, the selected block's factor and inverse, one download), device events and host clock
    lm_iteration              the stages of one LM iteration (lvf_problem_stage_times: the kernels' own durations) and their sum

Prints one JSON line: medians with p10 / p90.

    python tools/marginal_bench.py [--warmup 5] [--reps 30]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lvio_fusion_amd import api, synthetic as syn  # noqa: E402
from oracle import pyoracle as po  # noqa: E402  (the IMU pre-integrations of the synthetic window)
from tools.klt_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    po.build()
    ctx = api.Context(0)
    cfg = syn.config4_window()
    pre = api.preintegrate_or_none(ctx, cfg)
    st = api.State(ctx, cfg["n_kf"], cfg["n_lm"])
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
        st.set(field, cfg[key])
    tc, tf, pob = cfg["tc"], cfg["tf"], cfg["po"]
    hs = [api.two_camera_batch(ctx, cfg["cam0"], cfg["cam1"], tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"]),
          api.two_frame_batch(ctx, cfg["cam0"], cfg["cam1"], tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"]),
          api.pose_only_batch(ctx, cfg["cam0"], pob["ob"], pob["kf_idx"], pob["pw_idx"], pob["pw"]),
          api.imu_batch(ctx, pre, [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]])]
    prob = api.Problem(ctx, st, *hs)
    opt = api.default_solver_options()
    n_kf = cfg["n_kf"]
    out = {"n_kf": n_kf, "n_lm": cfg["n_lm"], "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}
    for n_sel in (1, 8):
        kfs = list(range(n_kf - 1, n_kf - 1 - n_sel, -1))
        stats = {}

        def call():
            stats.update(prob.marginal(opt, kfs)[2])
        out[f"marginal_{n_sel}"] = timed(ctx, call, a.warmup, a.reps)
        out[f"marginal_{n_sel}"]["stats"] = dict(stats)
    stages = prob.stage_times(opt, 1e4, reps=10)
    out["lm_iteration"] = {"stages_us": {n.split(" ")[0]: [round(us, 2), la] for n, us, la in stages if la}, "sum_us": round(sum(us for _, us, la in stages if la), 2)}
    print(json.dumps(out))
    prob.close()
    for h in hs + [st]:
        h.close()
    ctx.close()


if __name__ == "__main__":
    main()
