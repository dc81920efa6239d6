"""tests/window_ref.py (the numpy restatement of a window tick's assembly) against the lists the REFERENCE's own Backend::BuildProblem
produced for tests/window_replay.Drive's 12 ticks (tests/golden/ref_v4.npz), compared exactly as test_gpu_window.py's
test_block_lists_equal_the_references_build_problem compares the device's; and every drive of tests/window_cases.py constructed, which
asserts each case's conditions from its mirror.  No GPU."""
import os

import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import window_cases as wc
from tests import window_ref as ref
from tests import window_replay as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_v4.npz")


@pytest.mark.parametrize("with_imu", [True, False])
def test_reference_reproduces_the_references_build_problem(with_imu):
    R4 = np.load(GOLDEN)
    tag = f"imu{int(with_imu)}"
    drive = wr.Drive(with_imu)
    cfg = drive.cfg
    m = wc.Mirror(cfg["cam0"], cfg["cam1"], syn.baseline(), 20, wr.N_LM)
    seen = {k: 0 for k in wr.KINDS}
    for t in range(wr.N_KF):
        ev, first = drive.tick(t)
        for e in ev:
            if e[0] == "kf":
                m.add_keyframe(wr.KF_ID0 + t, cfg["poses"][t], drive.w_kf[t])
                if with_imu:
                    m.set_imu(wr.KF_ID0 + t, cfg["vel"][t], cfg["ba"][t], cfg["bg"][t], t - 1 if t > 0 else None)
            elif e[0] == "lm":
                l = e[1]
                m.add_landmarks(wr.KF_ID0 + t, [drive.lm_id[l]], drive.left_ob[l], drive.right_ob[l], [drive.inv_depth[l]])
            elif e[0] == "ob":
                m.add_observations(wr.KF_ID0 + t, [drive.lm_id[e[1]]], e[3])
            else:
                m.remove_observations(wr.KF_ID0 + e[2], [drive.lm_id[e[1]]])
        m.slide(wr.KF_ID0 + first)
        got = m.assemble()
        want = {kind: dict(ids=R4[f"{tag}_t{t}_{kind}_ids"], vals=R4[f"{tag}_t{t}_{kind}_vals"]) for kind in wr.KINDS}
        ref.compare_lists(got["lists"], want, f"{tag} tick {t}", pw_bound=1e-12)
        meta = R4[f"{tag}_meta"][t]
        c = got["counts"]
        assert c["kf"] == meta[0] and c["tc"] + c["tf"] + c["po"] + c["imu"] + c["prior"] == meta[3]
        for kind in wr.KINDS:
            seen[kind] += len(want[kind]["ids"])
    assert seen["PoseOnly"] > 0 and seen["TwoFrame"] > 0 and (with_imu or (seen["PoseGraphError"] > 0 and seen["PoseError"] > 0))


@pytest.mark.parametrize("name", wc.NAMES)
def test_case_conditions(name):
    """the constructor dry-runs the drive over its mirror and asserts what the case is for (window_cases.py: `conditions`)"""
    case = wc.make(name)
    assert len(case.stats) > 0
