"""The persistent window's device-side assembly (k_da_classify, k_da_scan, k_da_emit, k_da_scatter_invd, k_window_unpack and their host
side, assemble_device) past one tile and over a long drive: the drives of tests/window_cases.py fed to a device_assembly=True window
and to a device_assembly=False twin (the host walk), tick by tick, against tests/window_ref.py's restatement of the tick.

Every tick: the census and all six block lists of the device window against the reference's — ids, order and indices exact, weights and
observations exact, frozen world points to 1e-12 of the largest coordinate (test_block_lists_equal_the_references_build_problem's
bounds) — and against the twin's with the same checks (3e-6 on the frozen points once a solved tick has let the twins' states drift
apart, as in test_window_crosses_the_device_assembly_limit_and_back).  Where the step asks for it, initial_cost against the same tick
solved through the flat batch API with the REFERENCE's block lists and slots (1e-8, test_ticks_match_from_scratch_assembly's bound), and
on such a tick without iterations every live landmark's inverse depth and every pose read back unchanged (k_da_scatter_invd and the
read-back by landmark index put each value back where it came from).  Solved ticks (two iterations): assert_parity on every pose and
velocity and 1e-6 on EVERY live landmark's inverse depth between the twins; the mirror then takes the device window's state forward.
The outlier gate: both windows remove the same (landmark, keyframe) set.  At the end: lm_known is the mirror's live count and a departed
pose is queryable exactly while a live landmark anchors it.

Measured on an MI355X (whole test: the case's dry run, the per-item python feeding of both windows, every check): test_tiles[tiles_imu]
1.8 s, test_tiles[tiles_no_imu] 1.3 s, test_big 1.3 s (with its twin), test_long 0.2 s, test_empty 0.1 s."""
import time

import numpy as np
import pytest

from lvio_fusion_amd import synthetic as syn
from tests import window_cases as wc
from tests import window_ref as ref
from tests import window_replay as wr
from tests.helpers import assert_parity

pytestmark = pytest.mark.gpu

CENSUS = ("kf", "lm", "tc", "tf", "po", "imu", "prior")


class Actor:
    def __init__(self, api, oracle, ctx, case, mirror):
        self.api, self.oracle, self.ctx, self.case, self.m = api, oracle, ctx, case, mirror
        self.wins = [api.Window(ctx, case.left, case.right, baseline=syn.baseline(), weak_visual_threshold=case.weak_thr, device_assembly=d)
                     for d in (True, False)]          # the device assembly, and its twin on the host walk
        self.pre_cache = {}
        self.solved = False          # a solved tick has happened: the twins' states agree to assert_parity's bounds, no longer bit for bit
        self.seen = dict(cost=0, rejected=0, ticks=0)

    def pre(self, i):
        if i not in self.pre_cache:
            f = self.case.imu_frame(i)
            self.pre_cache[i] = self.oracle.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE)
        return self.pre_cache[i]

    def feed(self, events):
        for win in self.wins:
            for e in events:
                if e[0] == "kf":
                    win.add_keyframe(e[1], e[2], e[3])
                elif e[0] == "imu":
                    win.set_imu(e[1], e[2], e[3], e[4], self.pre(e[5]) if e[5] is not None else None)
                elif e[0] == "lm":
                    for k, i, l, r, d in zip(e[1].tolist(), e[2].tolist(), e[3], e[4], e[5].tolist()):
                        win.add_landmark(i, k, l, r, d)
                elif e[0] == "ob":
                    for i, xy in zip(e[2].tolist(), e[3]):
                        win.add_observation(i, e[1], xy)
                elif e[0] == "rm":
                    for i in e[2].tolist():
                        win.remove_observation(i, e[1])
                else:
                    win.slide(e[1])

    def flat_cost(self, asm):
        """the tick's initial cost through the flat batch API, from the REFERENCE's block lists"""
        api, ctx, m, f = self.api, self.ctx, self.m, asm["flat"]
        left, right = self.case.left, self.case.right
        n_kf, n_lm = len(m.kf), asm["counts"]["lm"]
        st = api.State(ctx, n_kf, max(n_lm, 1))
        poses = np.array([m.pose[k] for k in m.kf])
        st.set(api.POSES, poses); st.set(api.W_VISUAL, np.array([m.w[k] for k in m.kf]))
        if all(m.good[k] for k in m.kf):
            st.set(api.VEL, np.array([m.vel[k] for k in m.kf])); st.set(api.BA, np.array([m.ba[k] for k in m.kf])); st.set(api.BG, np.array([m.bg[k] for k in m.kf]))
        st.set(api.INV_DEPTH, f["inv_depth"] if n_lm else np.ones(1))
        tc, tf, po = f["tc"], f["tf"], f["po"]
        btc = api.two_camera_batch(ctx, left, right, tc["left_ob"], tc["right_ob"], tc["lm"], tc["kf"])
        if len(tc["kf"]):
            btc.set_block_weights(tc["weight"])
        btf = api.two_frame_batch(ctx, left, right, tf["first_ob"], tf["ob"], tf["lm"], tf["kf1"], tf["kf2"])
        npo = len(po["kf"])
        bpo = api.pose_only_batch(ctx, left, po["ob"], po["kf"], np.arange(npo, dtype=np.int32), po["pw"] if npo else np.zeros((1, 3)))
        bim = None
        if len(f["imu_j"]):
            bim = api.imu_batch(ctx, np.array([self.pre(m.pre[m.kf[j]]) for j in f["imu_j"]]), f["imu_i"], f["imu_j"])
        prob = api.Problem(ctx, st, btc, btf, bpo, bim)
        bpr = None
        if len(f["prior_b"]):
            target = [np.concatenate([self.oracle.pose_graph_target(poses[a], poses[b]), [0.0]]) if a >= 0 else poses[b] for a, b in zip(f["prior_a"], f["prior_b"])]
            bpr = api.pose_prior_batch(ctx, f["prior_a"], f["prior_b"], np.array(target), np.full(len(target), 100.0), np.zeros(len(target)))
            prob.set_pose_priors(bpr)
        opt = api.default_solver_options(); opt.max_num_iterations = 0
        s = prob.solve(opt)
        for h in (prob, bim, bpr, bpo, btf, btc, st):
            if h is not None:
                h.close()
        return s.initial_cost

    def solve(self, step, events, asm):
        api, m, what = self.api, self.m, step["label"]
        self.feed(events)
        opt = api.default_solver_options(); opt.max_num_iterations = step["iters"]
        summ = [win.solve(opt) for win in self.wins]
        dev, host = self.wins
        cnt = dev.counts()
        assert tuple(cnt[k] for k in CENSUS) == tuple(asm["counts"][k] for k in CENSUS), f"{what}: census {cnt} vs the reference's {asm['counts']}"
        assert cnt["lm_known"] == len(m.index), f"{what}: known landmarks"
        ld = wr.window_lists(dev)
        ref.compare_lists(ld, asm["lists"], f"{what} (device window vs window_ref)", pw_bound=1e-12)
        assert host.counts() == cnt, f"{what}: census {cnt} vs the twin's {host.counts()}"
        ref.compare_lists(ld, wr.window_lists(host), f"{what} (device window vs host twin)", pw_bound=3e-6 if self.solved else 1e-12)
        if step["check_cost"]:
            c = self.flat_cost(asm)
            print(f"{what}: initial cost {summ[0].initial_cost:.12e} vs flat {c:.12e} (rel {abs(summ[0].initial_cost - c) / max(abs(c), 1e-300):.2e})")
            assert abs(summ[0].initial_cost - c) <= 1e-8 * abs(c) + 1e-12, f"{what}: initial cost {summ[0].initial_cost!r} vs {c!r} through the flat API"
            self.seen["cost"] += 1
        if step["iters"] > 0:
            for k in m.kf:
                assert_parity(dev.pose(k), host.pose(k), f"{what} pose {k}")
                if m.good[k]:
                    assert_parity(dev.imu(k)[0], host.imu(k)[0], f"{what} vel {k}")
            a = np.array([dev.inv_depth(i) for i in m.index]); b = np.array([host.inv_depth(i) for i in m.index])
            worst = np.abs(a - b) / np.abs(b)
            print(f"{what}: {len(a)} live landmarks, worst inverse-depth difference of the twins {worst.max():.2e}")
            assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b)), f"{what}: inverse depth of landmark {list(m.index)[int(worst.argmax())]}: {worst.max():.3e}"
            m.take_state(dev.pose, dev.imu, dev.inv_depth)
            self.solved = True
        else:
            for k in m.kf:
                assert np.array_equal(dev.pose(k), m.pose[k]), f"{what}: pose {k} changed over a tick without iterations"
            for i, at in m.index.items():
                assert dev.inv_depth(i) == m.T_invd[at], f"{what}: inverse depth of landmark {i} (table entry {at}) changed over a tick without iterations"
        self.seen["ticks"] += 1

    def reject(self, step, events):
        self.feed(events)
        got = [win.reject_outliers(step["max_px"], capacity=1 << 16) for win in self.wins]
        removed, n = got[0]
        assert n == len(removed)
        for other, n_other in got[1:]:
            assert n_other == n and sorted(other) == sorted(removed), "the twins' outlier gates removed different features"
        self.seen["rejected"] += n
        return removed

    def finish(self):
        api, m = self.api, self.m
        for win in self.wins:
            assert win.counts()["lm_known"] == len(m.index)
            for k in m.ever_departed:
                if k in m.departed:
                    assert_parity(win.pose(k), m.departed[k], f"departed pose {k}")
                else:
                    with pytest.raises(api.LvfError):
                        win.pose(k)
            win.close()


def run_case(oracle, name):
    from lvio_fusion_amd import api
    t0 = time.perf_counter()
    case = wc.make(name)                 # (asserts the case's conditions from its mirror before anything touches the GPU)
    ctx = api.Context(0)
    m = case.mirror()
    actor = Actor(api, oracle, ctx, case, m)
    wc.play(case, m, actor)
    actor.finish()
    ctx.close()
    print(f"{name}: {time.perf_counter() - t0:.1f} s, {actor.seen}")
    return case, m, actor


@pytest.mark.parametrize("name", ["tiles_imu", "tiles_no_imu"])
def test_tiles(oracle, name):
    case, m, actor = run_case(oracle, name)
    assert actor.seen["ticks"] == case.TICKS and actor.seen["cost"] == 8 and actor.seen["rejected"] >= 20
    # the scripted sizes held on the real drive too (the gate's removals are the device's there, not the dry run's)
    for f in case.late_figures:
        assert f["added"] > f["slack"] >= 0, f"late observations: {f}"
    for a, b in zip(case.trim_figures[0::2], case.trim_figures[1::2]):
        assert a["features"] % 256 == 0 and b["features"] % 256 == 1
    assert max(s["n_tab"] for s in m.stats) > 1024 and any(s["dirty"] > 4096 and s["resident"] for s in m.stats)


def test_long(oracle):
    case, m, actor = run_case(oracle, "long")
    assert all(s["counts"]["kf"] == 64 for s in m.stats) and actor.seen["cost"] == 7


def test_big(oracle):
    case, m, actor = run_case(oracle, "big")
    assert actor.seen["cost"] == 2 and m.stats[0]["features"] > 131072 and m.stats[0]["n_tab"] > 32768


def test_empty(oracle):
    case, m, actor = run_case(oracle, "empty")
    assert actor.seen["cost"] == 3
