#!/usr/bin/env python3
"""Times the device pose-chain solve:

    chain_M          lvf_pose_chain_solve on a pose-graph chain of M free poses (PoseGraphError edges, RError unaries, both ends constant, the
                     last pose relocated by a loop closure as in tests/test_gpu_posegraph.py), upload and download included
    window_route_48  the same 48-pose chain through lvf_problem_* with a pose-prior batch (15 unknowns per keyframe, dense reduced system):
                     poses set, lvf_problem_solve, poses read back

Every call starts from the same poses and runs ceres::Solve's defaults to its own termination; the iteration counts are printed beside the
times.  Each timed call is bracketed by device events AND by the host clock.  Prints one JSON line: medians with p10 / p90.

    python tools/pose_chain_bench.py [--warmup 5] [--reps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lvio_fusion_amd import api, synthetic as syn  # noqa: E402
from oracle import pyoracle as po  # noqa: E402  (the edge targets: PoseGraphError's constructor)
from tools.klt_bench import timed  # noqa: E402


def chain(m, seed):
    """poses [m + 2][7] with the last one relocated, the prior batch of the window route and the same blocks as chain arrays"""
    n = m + 2
    rng = np.random.default_rng(seed)
    P = syn.drive_poses(n, rng, step=6.0)
    before = P[-1].copy()
    corr = np.concatenate([syn.quat_from_ypr(np.deg2rad(3.0), np.deg2rad(0.4), np.deg2rad(-0.3)), [1.5, -0.8, 0.2]])
    P[-1] = po.se3_mul(corr, P[-1])
    tg = np.array([po.pose_graph_target(P[k], P[k + 1] if k + 2 < n else before) for k in range(n - 1)])
    kind = np.zeros(n, np.int32); kind[1:n - 1] = api.CHAIN_R
    kf_a, kf_b, target, w, v = [], [], [], [], []
    for k in range(n - 1):
        kf_a.append(k); kf_b.append(k + 1); target.append(np.concatenate([tg[k], [0.0]])); w.append(1.0); v.append(1.0)
        if k + 2 < n:
            kf_a.append(-2); kf_b.append(k + 1); target.append(P[k + 1].copy()); w.append(1.0); v.append(0.0)
    pr = dict(kf_a=np.array(kf_a, np.int32), kf_b=np.array(kf_b, np.int32), target=np.array(target), weight=np.array(w), v=np.array(v))
    return P, dict(tg=tg, ew=np.ones(n - 1), ev=np.ones(n - 1), kind=kind, ut=P[:, :4].copy(), uw=np.ones(n)), pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="8,48,256,1022")
    a = ap.parse_args()
    po.build()
    ctx = api.Context(0)
    opt = api.default_solver_options()
    out = {"capacity": api.pose_chain_capacity(), "box_calibration": api.box_calibration(ctx) if hasattr(api, "box_calibration") else None}
    for m in [int(v) for v in a.sizes.split(",")]:
        P, c, pr = chain(m, 5)

        def run_chain():
            Q = P.copy()
            return Q, api.pose_chain_solve(ctx, Q, c["tg"], c["ew"], c["ev"], c["kind"], c["ut"], c["uw"], 0.0, opt)

        Q, s = run_chain()
        out["chain_%d" % m] = dict(timed(ctx, run_chain, a.warmup, a.reps), iterations=s.num_iterations, termination=s.termination,
                                   initial_cost=s.initial_cost, final_cost=s.final_cost)
        if m == 48:
            n = m + 2
            st = api.State(ctx, n, 0)
            b = api.pose_prior_batch(ctx, pr["kf_a"], pr["kf_b"], pr["target"], pr["weight"], pr["v"])
            prob = api.Problem(ctx, st, None, None, None, None)
            prob.set_pose_priors(b)
            prob.set_pose_constant(0, True); prob.set_pose_constant(n - 1, True)

            def run_window():
                st.set(api.POSES, P)
                sw = prob.solve(opt)
                return st.get(api.POSES), sw

            W, sw = run_window()
            out["window_route_%d" % m] = dict(timed(ctx, run_window, a.warmup, a.reps), iterations=sw.num_iterations, termination=sw.termination,
                                              initial_cost=sw.initial_cost, final_cost=sw.final_cost,
                                              max_pose_difference=float(np.abs(np.asarray(W).reshape(-1, 7) - Q).max()))
            prob.close(); b.close(); st.close()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
