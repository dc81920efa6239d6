#!/usr/bin/env python3
"""Times the LiDAR edge features on the 115 200-point syn.raw_scan against the calls they extend:

    lvf_lidar_extract  vs  lvf_lidar_extract_edges      the two ALTERNATE (tools/deskew_bench.py's scheme), the difference taken pair by pair
    lvf_edge_associate                                  the scan's own less-sharp cloud against a map of three jittered copies of it
    lvf_icp_solve      vs  lvf_icp_solve_edges          the (yaw, x, y) sub-problem on the scan's surf cloud, without and with the lines

Each timed call is bracketed by device events AND by the host clock.  Prints one JSON line: medians with p10 / p90.

    python tools/edge_bench.py [--warmup 20] [--reps 100]
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
from tools.deskew_bench import timed_alternating  # noqa: E402
from tools.klt_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    ctx = api.Context(0)
    scan = syn.raw_scan(seed=0x5CA9)
    ext = syn.lidar_extrinsic()
    prm, ep = api.lidar_params(), api.edge_params()
    g, s, sh, ls, dbg = api.lidar_extract_edges(ctx, scan, ext, ep, params=prm, debug=True)
    out = {"scan_points": int(scan.shape[0]), "segmented": int(dbg["n_segmented"]), "ground": len(g), "surf": len(s), "sharp": len(sh), "less_sharp": len(ls),
           "box_calibration": api.box_calibration(ctx), "event_pair_us": api.event_pair_us(ctx)}

    def plain():
        for c in api.lidar_extract(ctx, scan, ext, params=prm):
            c.close()

    def edges():
        for c in api.lidar_extract_edges(ctx, scan, ext, ep, params=prm):
            c.close()

    out["lidar_extract"], out["lidar_extract_edges"], out["edges_minus_plain"] = timed_alternating(ctx, plain, edges, a.warmup, a.reps)
    out["extract_fallbacks"] = api.extract_fallbacks(ctx)      # 0: every timed extraction finished on the device-counted path

    # the map: the frame's own clouds, three copies jittered by 2 cm (three merged keyframes); the frame is displaced by 10 cm and 0.3 deg
    rng = np.random.default_rng(1)
    res = prm.resolution
    eo = api.edge_icp_options(res)
    thr_surf = float(np.float32(res * res * 25.0))

    def merged(cloud):
        p = cloud.download()
        m = np.concatenate([p] * 3)
        m[:, :3] += rng.normal(0, 0.02, (len(m), 3)).astype(np.float32)
        return m

    map_pose = np.array([0, 0, 0, 1.0, 0, 0, 0])
    pose0 = np.concatenate([syn.quat_from_ypr(np.deg2rad(0.3), 0.0, 0.0).reshape(4), [0.10, -0.05, 0.0]])
    rp0 = np.array([np.deg2rad(0.3), 0.0, 0.0, 0.10, -0.05, 0.0])
    m_surf, m_edge = api.Map(ctx, merged(s), thr_surf), api.Map(ctx, merged(ls), eo.thr)
    q_surf, q_edge = api.Scan(ctx, s), api.Scan(ctx, ls)
    out["map_surf"], out["map_edge"] = m_surf.M, m_edge.M

    def assoc():
        api.edge_associate(m_edge, q_edge, pose0, eo.thr, eo.min_eigen_ratio)
        ctx.synchronize()

    out["edge_associate"] = timed(ctx, assoc, a.warmup, a.reps)
    out["lines_valid"] = int(q_edge.download_edges()[2].sum())
    summ = {}

    def solve_planes():
        summ["planes"] = api.icp_solve(m_surf, q_surf, map_pose, pose0, rp0.copy(), 1, thr_surf, float(np.float32(0.01)), 0.1)

    def solve_both():
        summ["both"] = api.icp_solve_edges(m_surf, q_surf, m_edge, q_edge, map_pose, pose0, rp0.copy(), thr_surf, float(np.float32(0.01)), 0.1, eo)

    out["icp_solve"], out["icp_solve_edges"], out["solve_edges_minus_planes"] = timed_alternating(ctx, solve_planes, solve_both, a.warmup, a.reps)
    out["blocks_planes"], out["blocks_planes_and_lines"] = summ["planes"].num_residual_blocks, summ["both"].num_residual_blocks
    for h in (g, s, sh, ls, m_surf, m_edge, q_surf, q_edge):
        h.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
