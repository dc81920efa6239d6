#!/usr/bin/env python3
"""Times the visual relocalisation at 2 000 x 2 000 descriptors with 512 hypotheses:

    lvf_orb_match            2 000 current against 2 000 old descriptors, cross-check on
    lvf_pnp_ransac           the matched pairs, 512 hypotheses, 2 refinement rounds
    lvf_relocate_by_image    both, one wait

The old frame holds 2 000 landmarks; 700 of the 2 000 current features re-observe one (up to 8 flipped descriptor bits, 0.3 px noise), the rest
are independent draws.  Each timed call is bracketed by device events AND by the host clock.  Prints one JSON line: medians with p10 / p90.

    python tools/reloc_image_bench.py [--warmup 20] [--reps 100]
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
from tests import reloc_cases as rc  # noqa: E402
from tools.klt_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--common", type=int, default=700)
    ap.add_argument("--hypotheses", type=int, default=512)
    a = ap.parse_args()
    ctx = api.Context(0)
    c = rc.image_pair(77, n_old=a.features, n_cur=a.features, n_common=a.common)
    po = api.pnp_options(num_hypotheses=a.hypotheses, seed=rc.PNP_SEED)
    m, _, _ = api.orb_match(ctx, c["cur_desc"], c["old_desc"])
    q = np.flatnonzero(m >= 0)
    pw, pt = np.ascontiguousarray(c["old_pw"][m[q]]), np.ascontiguousarray(c["cur_pt"][q])
    init = api.forward_update(ctx, c["old_pose"], c["relative_o_c"].reshape(1, 7))[0][0]
    res = api.relocate_by_image(ctx, c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, po)
    out = {"features": a.features, "true_pairs": a.common, "hypotheses": a.hypotheses, "pairs": int(len(q)), "score": int(res["score"]),
           "box_calibration": api.box_calibration(ctx) if hasattr(api, "box_calibration") else None}
    out["orb_match"] = timed(ctx, lambda: api.orb_match(ctx, c["cur_desc"], c["old_desc"]), a.warmup, a.reps)
    out["pnp_ransac"] = timed(ctx, lambda: api.pnp_ransac(ctx, c["cam0"], pw, pt, init, po), a.warmup, a.reps)
    out["relocate_by_image"] = timed(
        ctx, lambda: api.relocate_by_image(ctx, c["cam0"], c["old_pose"], c["old_pw"], c["old_desc"], c["cur_pt"], c["cur_desc"], c["relative_o_c"], None, po),
        a.warmup, a.reps)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
