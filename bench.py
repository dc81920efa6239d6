#!/usr/bin/env python
"""bench.py — hot-path throughput on MI355X.

Headline (BASELINE.json metric "local-BA iters/sec (50 KF x 10k pts) + ICP Mpairs/sec"):
  workload  = configs[3]: the 50-keyframe / 10 000-landmark sliding window (10k TwoCamera + ~72k TwoFrame + ~9.6k PoseOnly + 49 IMU
              factors, SURVEY.md 8d config 4, seed 0xBA50 + rank), everything resident in HBM;
  one step  = one complete Levenberg-Marquardt iteration of that window on device: linearise all factors (r + J, Huber corrector,
              7->6 tangent projection, J^T J / J^T r), Schur-eliminate the inverse depths, sparse + dense Cholesky, back-substitute,
              evaluate the candidate, accept/reject — closed on device (lvf_problem_solve, no host round trip per iteration);
  value     = LM iterations/s summed over all ranks (one independent window per GPU: weak scaling).
The K = --steps steps are timed once, bracketed by barrier + synchronize, as solves of <= 20 iterations each from the same perturbed start,
restored on device between them (so every solve does the same work and the problem never converges into a run of rejected steps):
`ms_per_step` = the K steps' wall time (the slowest rank's) / K; the fastest, median and slowest solve ride along per step.  Warm-up runs
at least --warmup iterations and 50 ms of the same solves.  --dump-outputs DIR writes what the last timed solve returned (state + summary).

A plain run does only that.  Everything below is measured with --full:
`roofline` is ONE object: the dominant kernel of the iteration by time (kernel, bound, achieved, peak, unit, frac, traffic);
`roofline_all` lists it together with the merged linearisation (fp64 VALU issue) and the band Schur complement (MFMA).  All are timed
live inside this run: every kernel of the chain is launched with its own start / stop HIP events (hipExtLaunchKernelGGL: the dispatch
packet's timestamps, the source rocprofv3's kernel trace reads), a stage's time is the sum over its launches (lvf_problem_stage_times2).
`roofline_icp` is the same kind of object for the association kernel (k_knn3) of the metric's second half.  `legs` holds the other parts of the metric: the
batched-windows solver (8/16 windows per launch chain), the configs[1] PoseOnly pass (K1) with its HBM roofline, the ICP association
as 8d defines a pair, the window tick and the Ceres-surface solve.  `verified` says which legs were checked against the oracle in this
run.  `cpu_baseline` is the restated reference CPU path (oracle) on a bounded sample — a reported baseline, not the target.

Launch: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]; for N>1 the driver uses torch.distributed.run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# CPU-baseline leg: the reference runs Ceres with num_threads = min(8, 0.75 nproc) (estimator.cpp:10); the oracle's OpenMP team is
# sized the same way (on a 256-core host the default team makes its small dense loops slower, not faster)
os.environ.setdefault("OMP_NUM_THREADS", str(min(8, max(1, int(0.75 * (os.cpu_count() or 1))))))

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_PEAK_TFLOPS = 78.6          # MI355X fp64 vector = matrix peak (dense)
N_SIMD, CLOCK_GHZ = 1024, 2.4    # 256 CUs x 4 SIMDs; a wave64 VALU instruction occupies its SIMD for 4 clocks
VALU_PEAK_GCYC = N_SIMD * CLOCK_GHZ   # SIMD-cycles per nanosecond the chip can spend issuing VALU work
POSE_ONLY_BYTES_PER_BLOCK = 152  # ob 16 + 2 idx 8 + r 16 + J 112
KNN_BYTES = lambda Q, M: 40 * Q + 16 * M   # SURVEY 8d kNN pass
CHUNK = 20                       # LM iterations per device-loop solve inside a batch


def pmc_counters(kernel_substr):
    """Average per-dispatch PMC counters of a kernel from the committed passes (profiles/pmc_latest.json and profiles/pmc_icp_latest.json,
    written by tools/prof_summary.py / tools/prof_icp_summary.py from separate rocprofv3 --pmc runs of these same commands): bench.py
    itself cannot collect PMC counters.  Counters of the same kernel found in both files are merged (the later file wins)."""
    out, src = {}, []
    for fn in ("pmc_latest.json", "pmc_icp_latest.json"):
        path = os.path.join(ROOT, "profiles", fn)
        if not os.path.exists(path):
            continue
        try:
            d = json.load(open(path))
            for name, c in d["kernels"].items():
                if kernel_substr in name:
                    out.update(c); src.append("profiles/" + fn + " (" + d.get("tag", "?") + ")")
                    break
        except Exception:
            pass
    return (out, "; ".join(src)) if out else (None, None)


def pmc_traffic(kernel_substr):
    """HBM bytes per launch: FETCH_SIZE is doubled for the gfx950 half-count of wide coalesced reads (MI355X_MICROARCH.md, HBM
    section); counters are KiB."""
    c, src = pmc_counters(kernel_substr)
    if not c or "FETCH_SIZE" not in c or "WRITE_SIZE" not in c:
        return None
    return {"bytes": (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0, "fetch_kib_raw": c["FETCH_SIZE"], "write_kib": c["WRITE_SIZE"],
            "source": src + "; FETCH_SIZE x2 per gfx950 correction"}


def profile_avg_ns(kernel_substr):
    """Average duration (ns) rocprofv3 --kernel-trace --stats recorded for a kernel in the newest committed summary
    (profiles/r*_rocprofv3_summary.txt, tools/prof_summary.py's table: calls total_ns avg_ns min max pct name) -> (avg_ns, file) or (None, None)."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_rocprofv3_summary.txt")))
    for fn in reversed(files):
        try:
            for line in open(fn):
                if kernel_substr in line:
                    m = re.match(r"\s*(\d+)\s+(\d+)\s+([0-9.]+)\s+(\d+)\s+(\d+)\s+([0-9.]+)\s+", line)
                    if m:
                        return float(m.group(3)), "profiles/" + os.path.basename(fn)
        except Exception:
            pass
    return None, None


def batch_pmc():
    """Counter bytes per window-iteration of the batched chain (profiles/pmc_batch_latest.json, written by tools/prof_batch_pmc.sh from separate
    FETCH_SIZE / WRITE_SIZE passes over tools/run_batch.py): bench.py itself cannot collect PMC counters."""
    path = os.path.join(ROOT, "profiles", "pmc_batch_latest.json")
    if not os.path.exists(path):
        return None
    try:
        return json.load(open(path))
    except Exception:
        return None


def window_algorithmic_bytes(n_tc, n_tf, n_po, n_imu, n_kf):
    """SURVEY 8d, BA iteration, materialised mode: TwoCamera 68 B + TwoFrame 300 B + PoseOnly 152 B + ImuError 6 256 B per block, plus the
    reduced system once out and once in (2 x ld^2 x 8 B, ld = 15 n_kf + 1 padded to 16)."""
    ld = 16 * ((15 * n_kf + 1 + 15) // 16)
    return 68.0 * n_tc + 300.0 * n_tf + 152.0 * n_po + 6256.0 * n_imu + 2.0 * 8.0 * ld * ld


def build_window(api, syn, ctx, seed=None, ids_by_birth=False):
    cfg = syn.config4_window(ids_by_birth=ids_by_birth) if seed is None else syn.config4_window(seed=seed, ids_by_birth=ids_by_birth)
    pre = api.preintegrate_or_none(ctx, cfg)
    st = api.State(ctx, cfg["n_kf"], cfg["n_lm"])
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
        st.set(field, cfg[key])
    tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
    btc = api.two_camera_batch(ctx, cfg["cam0"], cfg["cam1"], tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"])
    btf = api.two_frame_batch(ctx, cfg["cam0"], cfg["cam1"], tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"])
    bpo = api.pose_only_batch(ctx, cfg["cam0"], po["ob"], po["kf_idx"], po["pw_idx"], po["pw"])
    bimu = api.imu_batch(ctx, pre, [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]]) if pre is not None else None
    prob = api.Problem(ctx, st, btc, btf, bpo, bimu)
    return cfg, prob, (btc, btf, bpo, bimu, st)


def reset_state(api, st, cfg):
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth")):
        st.set(field, cfg[key])


def fixed_iterations(api, n):
    """solver options that make lvf_problem_solve run exactly n LM iterations (tolerances off)"""
    o = api.default_solver_options()
    o.max_num_iterations = int(n); o.function_tolerance = 0.0; o.parameter_tolerance = 0.0; o.gradient_tolerance = 0.0
    return o


def dump_outputs(directory, api, st, summary, prefix=""):
    """What the last timed solve hands its caller, as float64 .npy files: the window's state after the solve (poses [n_kf][7], vel / ba / bg
    [n_kf][3], inv_depth [n_lm]) and its summary (initial_cost, final_cost, num_iterations, num_successful_steps, num_unsuccessful_steps,
    termination)."""
    os.makedirs(directory, exist_ok=True)
    arrays = {"poses": st.get(api.POSES).reshape(-1, 7), "vel": st.get(api.VEL).reshape(-1, 3), "ba": st.get(api.BA).reshape(-1, 3),
              "bg": st.get(api.BG).reshape(-1, 3), "inv_depth": st.get(api.INV_DEPTH),
              "summary": np.array([summary.initial_cost, summary.final_cost, summary.num_iterations, summary.num_successful_steps,
                                   summary.num_unsuccessful_steps, summary.termination], np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(directory, prefix + name + ".npy"), np.ascontiguousarray(a, np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed solve returned (the window's state and the solve summary) as DIR/<name>.npy, float64")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: box calibration, roofline, the other legs, the CPU baseline, the oracle checks "
                         "and, for --gpus > 1, the solo reference, the sharded relocalisation leg and ranks_seen.  A plain run only times the headline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the other legs")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="process-group backend for --gpus > 1.  nccl (= RCCL over xGMI) is the product path and needs one GPU per rank; gloo exercises the SAME multi-rank "
                         "branch (timing all-gather, solo reference, sharded relocalisation + gather) with every rank on the visible GPU(s) round-robin and CPU tensors in "
                         "the collectives — a correctness dry run on a 1-GPU box, never a scaling figure")
    ap.add_argument("--legs-file", default=os.path.join(ROOT, "bench_legs.json"), help="where the full record goes (the stdout line is the compact one)")
    ap.add_argument("--check-lvf-comm", action="store_true",
                    help="--gpus > 1, nccl: also push the gathered table through the C-ABI communicator (lvf_comm_*: the library dlopens /opt/rocm's RCCL) and compare.  "
                         "Off by default: torch brings its own RCCL into the process, and two RCCL builds in one process have been seen to refuse ncclCommInitRank "
                         "(tests/test_gpu_comm_world2.py exercises lvf_comm_* in torch-free processes instead)")
    ap.add_argument("--fail-rank", type=int, default=-1, help="test hook: this rank raises inside its share of the relocalisation leg (the collective must still complete)")
    ap.add_argument("--legs", default="all", help="with --full: comma list of legs to run (default all): batched_windows_8,batched_windows_16,batched_windows_64,small_windows_100,pose_only_K1,icp,scan_match_frame,map_maintenance,window_tick,ceres_surface_solve,relocalize_8_candidates")
    args = ap.parse_args()
    if args.legs != "all" and not args.full:
        ap.error("--legs selects legs of the --full run")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    import torch.distributed as dist
    gloo = world > 1 and args.dist_backend == "gloo"
    if gloo:
        local_rank = local_rank % max(1, torch.cuda.device_count())       # ranks share the visible GPU(s)
    torch.cuda.set_device(local_rank)
    coll_dev = torch.device("cpu") if gloo else torch.device("cuda", local_rank)      # where the collectives' tensors live
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from lvio_fusion_amd import api, synthetic as syn

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    ctx = api.Context(local_rank)
    cfg, prob, handles = build_window(api, syn, ctx, seed=syn.SEED_CFG4 + rank)
    btc, btf, bpo, bimu, st = handles
    K = max(1, args.steps)
    sizes = [CHUNK] * (K // CHUNK) + ([K % CHUNK] if K % CHUNK else [])
    st0 = api.State(ctx, cfg["n_kf"], cfg["n_lm"])        # the perturbed start, kept on device
    for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
        st0.set(field, cfg[key])
    opts = {n: fixed_iterations(api, n) for n in set(sizes)}

    def run_steps():
        """K LM iterations as solves of <= CHUNK iterations from the restored start; returns (iterations done, last summary, seconds per solve)"""
        done, s, solve_s = 0, None, []
        for n in sizes:
            t0 = time.perf_counter()
            st.copy_from(st0)
            s = prob.solve(opts[n])          # returns after the device loop has finished (the summary is read back)
            solve_s.append(time.perf_counter() - t0)
            done += int(s.num_iterations)
        return done, s, solve_s

    torch.zeros(8, dtype=torch.float64, device="cuda")   # forces torch's lazy CUDA init before timing
    # warm-up: at least --warmup iterations AND at least 50 ms of device work (clocks, caches, first-touch allocations), in solves of the
    # first timed solve's size
    done, t_w0 = 0, time.perf_counter()
    first_summary = None
    while done < args.warmup or time.perf_counter() - t_w0 < 0.05:
        st.copy_from(st0)
        s = prob.solve(opts[sizes[0]])
        first_summary = first_summary or s
        done += int(s.num_iterations)
    # single-GPU reference time for the scaling line: rank 0 alone, the other ranks idle at the barrier
    t1_solo = None
    if world > 1 and args.full:
        barrier()
        if rank == 0:
            ts = []
            for _ in range(3):
                ctx.synchronize(); t0 = time.perf_counter(); run_steps(); ts.append(time.perf_counter() - t0)
            t1_solo = float(np.median(ts))
    # the timed steps: exactly K LM iterations, once
    barrier()
    t0 = time.perf_counter()
    executed, last_summary, solve_s = run_steps()
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank = None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(x) for x in torch.cat(allt).cpu().numpy()]
        elapsed = max(per_rank)                            # the K steps end when the slowest rank's do
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, api, st, last_summary, "" if world == 1 else f"rank{rank}_")
    solve_ms_per_step = sorted(1e3 * dt / n for dt, n in zip(solve_s, sizes))

    out = None
    if rank == 0:
        out = {
            "metric": "local-BA iters/sec (50 KF x 10k pts) + ICP Mpairs/sec",
            "value": world * executed / elapsed,
            "unit": "iter/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / max(executed, 1),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "configs[3]: full sliding-window LM iteration, 50 keyframes x 10 000 landmarks "
                                   f"({btc.n} TwoCamera + {btf.n} TwoFrame + {bpo.n} PoseOnly + {bimu.n if bimu else 0} IMU factors), device-resident LM loop, "
                                   "one independent window per GPU",
                       "n_kf": cfg["n_kf"], "n_lm": cfg["n_lm"], "parallelism": f"{world} independent windows",
                       "timed_steps": K, "iterations_per_solve": CHUNK, "value_from": "the K timed steps, run once (the slowest rank's time)"},
            "steps_executed": executed,
            "solve_ms_per_step_min_median_max": [solve_ms_per_step[0], float(np.median(solve_ms_per_step)), solve_ms_per_step[-1]],
            "cost_first_to_last": [first_summary.initial_cost, first_summary.final_cost],
        }
        if world > 1:
            out["per_rank_seconds_for_K_steps"] = per_rank
            if args.full:
                out["single_gpu_seconds_same_work"] = t1_solo
                out["scaling_efficiency_T1_over_TN"] = (t1_solo / elapsed) if t1_solo else None
            out["dist_backend"] = args.dist_backend
            if gloo:
                out["dist_backend_note"] = (f"gloo dry run: {world} ranks on {torch.cuda.device_count()} visible GPU(s), CPU tensors in the collectives (RCCL refuses two ranks on one "
                                            "device); value / efficiency here say NOTHING about scaling — the product path is nccl = RCCL over xGMI, one GPU per rank")
    # ---- everything below the headline runs with --full only
    # ---- what this box is worth for the latency-bound legs (the headline moves +-20 % from box to box on the pool: VERDICT r04 weak 3)
    if rank == 0 and args.full:
        try:
            out["box_calibration"] = box_calibration(api, ctx, out["ms_per_step"])
        except Exception as e:
            out["box_calibration"] = {"error": repr(e)}
    # ---- roofline (rank 0): stage times of the iteration, live
    if rank == 0 and args.full:
        try:
            out["roofline_all"], out["iteration_stages_us"], out["event_pair_us"] = roofline(api, ctx, prob, st, cfg, handles)
            keys = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches_per_iteration", "share_of_iteration", "note")
            out["roofline"] = {k: out["roofline_all"][0].get(k) for k in keys}       # ONE object: the dominant kernel
        except Exception as e:
            out["roofline"] = {"error": repr(e)}
    verified = {}
    # ---- other legs + CPU baseline: rank 0, single-GPU runs only (keeps multi-GPU runs short)
    # (every optional leg is fenced: a failure there must never take the headline line down with it)
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        try:
            out["legs"] = legs(api, syn, ctx, local_rank, verified, args.legs)
        except Exception as e:
            out["legs"] = {"error": repr(e)}
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(api, cfg, prob, st, verified)
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)}
    if rank == 0 and args.full:
        out["verified"] = verified
    # configs[4] on N GPUs: 8 loop-closure candidates sharded rank-round-robin, one all_gather of the records over RCCL
    if world > 1 and args.full and not args.no_extras:
        from lvio_fusion_amd import relocalize as rl
        err = None
        table = rl.empty_records(rl.slots(8, world))
        dt = 0.0
        cands = None
        try:        # the local (per-GPU) parts may fail without desynchronising the ranks: barriers and the collective always run
            cands = syn.config5_candidates(8)
            for c in cands:
                rl.split_candidate(c)
            rl.evaluate_candidates_batched(api, ctx, [cands[rank % 8]])      # warm-up
        except Exception as e:
            err = repr(e)
        barrier()
        t0 = time.perf_counter()
        try:
            if cands is not None:
                mine = rl.owned(8, rank, world)          # this rank's share in ONE launch chain (lvf_scan_match_batch)
                if rank == args.fail_rank:
                    raise RuntimeError("--fail-rank: scripted failure inside this rank's share")
                for s_, (cid, res) in enumerate(zip(mine, rl.evaluate_candidates_batched(api, ctx, [cands[c] for c in mine]))):
                    table[s_] = rl.make_record(cid, res.score, np.array(res.relative_o_c[:]))
        except Exception as e:
            err = repr(e)
        rec = rl.gather_records(table, world, coll_dev)
        errs = [None] * world
        dist.all_gather_object(errs, err) if gloo else None         # (diagnostic only, and only on the dry-run backend: RCCL moves the 72-byte records alone)
        barrier()
        dt = time.perf_counter() - t0
        if rank == 0:
            live = rec[rec[:, 8] >= 0]
            best = rl.choose_best(rec)
            out["legs"] = {"relocalize_8_candidates": {"ms_total": 1e3 * dt, "candidates_per_sec": 8 / dt if dt > 0 else None, "ranks": world,
                                                       "best": None if best is None else {"candidate": best[0], "score": best[1]},
                                                       "candidates": [int(x) for x in np.sort(live[:, 8])],
                                                       "scores": [float(x) for x in live[np.argsort(live[:, 8]), 0]],
                                                       "relative_o_c": [[float(v) for v in row[1:8]] for row in live[np.argsort(live[:, 8])]],
                                                       "error": err, "errors_by_rank": errs if gloo else None}}
    # what the N > 1 record proves about itself: ranks the process group saw, one device UUID per rank, a checksum of the
    # gathered table — and, on the product backend, the same table once more through the C-ABI communicator (lvf_comm_*: RCCL opened by the library)
    if world > 1 and args.full:
        seen = ranks_seen(api, ctx, dist, torch, rank, world, local_rank, coll_dev, gloo, rec if not args.no_extras else None, args.check_lvf_comm)
        if rank == 0:
            out["ranks_seen"] = seen
    for h in (prob, st0) + tuple(handles):
        if h is not None:
            h.close()
    ctx.close()
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        emit(out, args.legs_file)


def _r(x, n=4):
    """numbers to n significant digits (the line is for a parser with an 8 KB window, the sidecar keeps full precision)"""
    if isinstance(x, float):
        return float(f"{x:.{n}g}")
    if isinstance(x, dict):
        return {k: _r(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, n) for v in x]
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def combined_speedup(out):
    """north_star's target as a number: the local-BA + ICP iteration rate of the 50-keyframe / 10 000-landmark / 100 000-lidar-point window against
    the CPU path.  One combined iteration = one LM iteration of the window + one association-and-linearisation pass over the 100 000 scan points,
    the map index rebuilt inside the pass on BOTH sides (the reference rebuilds its kd-tree per call, association.cpp:279,337).
    CPU seconds = 1 / cpu_baseline.value + 1e5 / (cpu Mpairs/s incl. tree build); GPU seconds = ms_per_step + pair_incl_index_device_cloud.ms."""
    try:
        cb = out["cpu_baseline"]
        icp = out["legs"]["icp"]
        cpu_ba_s = 1.0 / cb["value"]
        cpu_icp_s = 1e5 / (cb["icp_mpairs_per_sec"]["incl_tree_build"] * 1e6)
        gpu_ba_s = 1e-3 * out["ms_per_step"]
        gpu_icp_s = 1e-3 * icp["pair_incl_index_device_cloud"]["ms"]
        x = (cpu_ba_s + cpu_icp_s) / (gpu_ba_s + gpu_icp_s)
        return {"combined_ba_plus_icp": x, "ba_alone": cpu_ba_s / gpu_ba_s, "icp_alone_incl_index": cpu_icp_s / gpu_icp_s, "target": 10.0, "met": bool(x >= 10.0),
                "cpu_ms": [1e3 * cpu_ba_s, 1e3 * cpu_icp_s], "gpu_ms": [1e3 * gpu_ba_s, 1e3 * gpu_icp_s],
                "def": "(1/cpu it/s + 1e5/cpu pairs/s incl. kd-tree build) / (ms_per_step + ICP pass incl. index build, device cloud)"}
    except Exception as e:
        return {"error": repr(e)[:200]}


def compact_line(out):
    """The ONE stdout line the driver parses (its window is 8 KB: VERDICT r05 item 1): every object once, numbers to 4-5 digits, notes dropped.
    Everything else goes to bench_legs.json (and stderr)."""
    L = out.get("legs") if isinstance(out.get("legs"), dict) else {}
    line = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    cfg = dict(out.get("config") or {})
    line["config"] = cfg
    line["steps_executed"] = out.get("steps_executed")
    line["solve_ms_per_step_min_median_max"] = out.get("solve_ms_per_step_min_median_max")
    if "roofline" in out:
        r = out["roofline"]
        line["roofline"] = r if "error" in r else _pick(r, ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches_per_iteration", "share_of_iteration"))
        if "traffic" not in line["roofline"] and "error" not in line["roofline"]:
            line["roofline"]["traffic"] = None
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "kind", "sample", "reference_functors_eval_ms", "error"))
        if isinstance(cb.get("icp_mpairs_per_sec"), dict):
            c["icp_mpairs_per_sec"] = _pick(cb["icp_mpairs_per_sec"], ("value", "incl_tree_build", "cores"))
        if isinstance(cb.get("pose_only_K1_passes_per_sec"), dict):
            c["pose_only_K1_passes_per_sec"] = cb["pose_only_K1_passes_per_sec"].get("value")
        line["cpu_baseline"] = c
        line["speedup_vs_cpu"] = combined_speedup(out)
    icp = L.get("icp") if isinstance(L.get("icp"), dict) else {}
    if icp:
        line["icp_mpairs_per_sec"] = icp.get("icp_mpairs_per_sec")
        if isinstance(icp.get("icp_mpairs_per_sec_incl_index"), dict):
            line["icp_mpairs_per_sec_incl_index"] = _pick(icp["icp_mpairs_per_sec_incl_index"], ("host_cloud", "device_cloud"))
        if isinstance(icp.get("roofline_icp"), dict):
            line["roofline_icp"] = _pick(icp["roofline_icp"], ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us", "traffic", "traffic_over_algorithmic",
                                                              "candidates_per_query_mean", "error"))
    for key in ("batched_windows_8", "batched_windows_16", "batched_windows_64"):
        if isinstance(L.get(key), dict):
            line[key] = _pick(L[key], ("windows", "lm_iters_per_sec_aggregate", "ms_per_batched_iteration", "error"))
    b64 = L.get("batched_windows_64") if isinstance(L.get("batched_windows_64"), dict) else {}
    if isinstance(b64.get("roofline_batched"), dict):
        line["roofline_batched"] = _pick(b64["roofline_batched"], ("bound", "windows", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic"))
    if isinstance(L.get("small_windows_100"), dict):
        line["small_windows_100"] = _pick(L["small_windows_100"], ("windows", "n_kf", "lm_iters_per_sec_aggregate", "single_window_ms_per_iteration", "error"))
    if isinstance(L.get("pose_only_K1"), dict):
        line["pose_only_K1"] = _pick(L["pose_only_K1"], ("blocks", "passes_per_sec", "avg_kernel_ms", "error"))
        if isinstance(L["pose_only_K1"].get("roofline"), dict):
            line["pose_only_K1"]["hbm_frac"] = L["pose_only_K1"]["roofline"].get("frac")
    if isinstance(L.get("window_tick"), dict):
        line["window_tick_ms_1_iteration"] = L["window_tick"].get("ms_per_tick_1_iteration")
    cs = L.get("ceres_surface_solve") if isinstance(L.get("ceres_surface_solve"), dict) else {}
    if cs:
        line["ceres_surface"] = _pick(cs, ("adapt_solve_ms", "ceres_surface_tick_ms", "reference_text_tick_ms", "error"))
    if isinstance(L.get("scan_match_frame"), dict):
        line["scan_match_frame_ms"] = _pick(L["scan_match_frame"], ("ms_per_frame", "scan_match_frame_incl_index_ms"))
    rc = L.get("relocalize_8_candidates") if isinstance(L.get("relocalize_8_candidates"), dict) else {}
    if rc:
        line["relocalize_8_candidates"] = _pick(rc, ("ms_total", "candidates_per_sec", "ranks", "best", "error", "comm"))
    if "box_calibration" in out:
        line["box_calibration"] = _pick(out["box_calibration"], ("ns_per_dependent_fp64_fma", "empty_launch_us_back_to_back", "effective_sclk_mhz",
                                                                 "lm_iteration_in_dependent_fma_times", "lm_iteration_in_empty_launch_times", "error"))
    for k in ("per_rank_seconds_for_K_steps", "single_gpu_seconds_same_work", "scaling_efficiency_T1_over_TN", "dist_backend", "ranks_seen", "verified"):
        if k in out:
            line[k] = out[k]
    line["detail"] = "bench_legs.json"
    return _r(line, 5)


def ranks_seen(api, ctx, dist, torch, rank, world, local_rank, coll_dev, gloo, table, check_lvf_comm=False):
    """Collective on every rank.  Returns (rank 0) {group_world_size, backend, device_uuids[rank], distinct_devices, table_crc32, lvf_comm{...}}."""
    import threading
    import zlib
    seen = {"group_world_size": dist.get_world_size(), "backend": dist.get_backend()}
    try:
        u = str(torch.cuda.get_device_properties(local_rank).uuid)
    except Exception:
        u = f"device-{local_rank}"
    raw = np.frombuffer(u.encode()[:48].ljust(48, b" "), np.uint8).copy()
    t = torch.from_numpy(raw).to(coll_dev)
    allu = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(allu, t)
    seen["device_uuids"] = [bytes(x.cpu().numpy()).decode().strip() for x in allu]
    seen["distinct_devices"] = len(set(seen["device_uuids"]))
    if table is not None:
        seen["table_crc32"] = zlib.crc32(np.ascontiguousarray(table, np.float64).tobytes())
        seen["table_rows"] = int(np.asarray(table).reshape(-1, 9).shape[0])
    if gloo:
        seen["lvf_comm"] = {"skipped": "gloo dry run: RCCL refuses two ranks on one device"}
        return seen
    if not check_lvf_comm:
        seen["lvf_comm"] = {"skipped": "--check-lvf-comm not given (two RCCL builds in one process: see --help); covered by tests/test_gpu_comm_world2.py"}
        return seen
    # the C-ABI communicator: rank 0's unique id travels over the process group; bounded (a wedged RCCL init must not take the line down)
    res = {}

    def work():
        try:
            idt = torch.zeros(128, dtype=torch.uint8, device=coll_dev)
            if rank == 0:
                idt = torch.from_numpy(np.frombuffer(api.comm_unique_id(), np.uint8).copy()).to(coll_dev)
            dist.broadcast(idt, 0)
            comm = api.Comm(ctx, world, rank, bytes(idt.cpu().numpy()))
            res["world_size"] = comm.world_size
            if table is not None:
                mine = np.ascontiguousarray(np.asarray(table, np.float64).reshape(world, -1)[rank])
                got = comm.allgather(mine)
                res["same_table_as_process_group"] = bool(np.array_equal(got.reshape(-1), np.asarray(table, np.float64).reshape(-1), equal_nan=True))
            comm.close()
        except Exception as e:
            res["error"] = repr(e)[:200]
    th = threading.Thread(target=work, daemon=True)
    th.start(); th.join(60.0)
    if th.is_alive():
        res["error"] = "timeout after 60 s"
    seen["lvf_comm"] = res
    return seen


def emit(out, legs_file=None):
    """full record -> bench_legs.json (+ gpurun_out/ when present) and stderr; the compact record -> the final stdout line"""
    full = json.dumps(out)
    for path in (legs_file or os.path.join(ROOT, "bench_legs.json"), os.path.join(ROOT, "gpurun_out", "bench_legs.json")):
        try:
            if os.path.isdir(os.path.dirname(path)):
                with open(path, "w") as f:
                    f.write(full + "\n")
        except Exception:
            pass
    print(full, file=sys.stderr, flush=True)
    line = json.dumps(compact_line(out), separators=(",", ":"))
    if len(line) > 6000:      # never again a line the driver cannot read: shed the optional objects, largest first
        c = json.loads(line)
        for k in ("box_calibration", "relocalize_8_candidates", "ceres_surface", "small_windows_100", "pose_only_K1", "batched_windows_16", "scan_match_frame_ms", "verified"):
            c.pop(k, None)
            line = json.dumps(c, separators=(",", ":"))
            if len(line) <= 6000:
                break
    print(line, flush=True)


def box_calibration(api, ctx, ms_per_step):
    """lvf_box_calibration + the shader / memory clocks rocm-smi reports right now, and the headline re-expressed in this box's own units
    (LM iteration time in dependent-FMA times and in empty-launch times) so that two boxes' headlines can be told apart from a regression."""
    c = api.box_calibration(ctx)
    try:
        import subprocess
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
        j = json.loads(r.stdout)
        card = j[sorted(j)[0]]
        c["rocm_smi_clocks"] = {k: v for k, v in card.items() if "clock" in k.lower()}
    except Exception as e:
        c["rocm_smi_clocks"] = {"unreadable": repr(e)[:120]}
    if c.get("ns_per_dependent_fp64_fma"):
        c["lm_iteration_in_dependent_fma_times"] = 1e6 * ms_per_step / c["ns_per_dependent_fp64_fma"]
    if c.get("empty_launch_us_back_to_back"):
        c["lm_iteration_in_empty_launch_times"] = 1e3 * ms_per_step / c["empty_launch_us_back_to_back"]
    c["note"] = ("the iteration is ~12 launches of dependent fp64 chains: its time scales with ns_per_dependent_fp64_fma (shader clock under load) and "
                 "empty_launch_us (launch floor); compare lm_iteration_in_* across boxes, not it/s")
    return c


def roofline(api, ctx, prob, st, cfg, handles):
    """The iteration's launch chain timed stage by stage (10 iterations from the perturbed start): every kernel is launched with its own
    start / stop events, a stage's time is the sum of its kernels' durations — what rocprofv3 --kernel-trace reports (profiles/).  The
    span between the stream events that bracket a stage (kernels + gaps + marker cost) rides along in the table, with the cost of an empty
    event pair.  Returns (roofline entries, dominant first; stage table; event-pair cost)."""
    btc, btf, bpo, bimu, _ = handles
    reset_state(api, st, cfg)
    ev_us = api.event_pair_us(ctx)
    raw = prob.stage_times(api.default_solver_options(), radius=1e4, reps=10, spans=True)
    stages = [(n, us if la else 0.0, la) for n, us, la, _ in raw]
    total = sum(us for _, us, _ in stages)
    table = [{"stage": n, "us": us, "us_span_between_stream_events": sp, "launches": la, "share": us / total if total else None} for (n, us, la), (_, _, _, sp) in zip(stages, raw)]
    by = {n: (us, la) for n, us, la in stages}
    out = []
    d_dense = 64 * ((6 * cfg["n_kf"] + 63) // 64)
    # merged linearisation: fused-algorithmic bytes = the factor inputs + the Schur operand rows it must produce
    lin_bytes = 24 * bpo.n + (44 + 48) * btf.n + 36 * btc.n + (6256 * bimu.n if bimu else 0)

    def entry(name, us, la):
        e = {"kernel": name.split(" ")[0], "stage": name, "launches_per_iteration": la, "avg_launch_us": us / max(la, 1), "stage_us": us, "share_of_iteration": us / total if total else None}
        if "chol" in name and "backsolve" not in name:
            flops = d_dense ** 3 / 3.0 + d_dense ** 2 * 64.0     # dense Cholesky of the pose corner + the L_kk^-T blocks for the back substitution
            ach = flops / (us * 1e-6) / 1e12
            e.update({"bound": "mfma", "achieved": ach, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP64_PEAK_TFLOPS,
                      "traffic": (pmc_traffic(e["kernel"]) or {}).get("bytes"), "algorithmic_flops_per_iteration": flops,
                      "note": "dense Cholesky of the reduced system's pose corner: a dependent pivot chain (latency-bound); priced against the fp64 matrix peak"})
        elif "k_lin_visual" in name:
            # Bound by the ISSUE of fp64 vector instructions inside its waves, not by memory: 1.6 waves per SIMD, each a dependent chain of
            # ~1 400-2 800 VALU instructions.  The roofline is therefore VALU issue: SIMD-cycles the kernel's VALU
            # instructions occupy (SQ_INSTS_VALU x 4 clocks, from the committed PMC pass) per second of kernel time, against
            # 1 024 SIMDs x 2.4 GHz.  The HBM view rides along (algorithmic bytes and counter traffic).
            tr = pmc_traffic("k_lin_visual")
            c, src = pmc_counters("k_lin_visual(")
            hbm = lin_bytes / (us * 1e-6) / 1e9
            e.update({"bound": "valu", "peak": VALU_PEAK_GCYC, "unit": "G SIMD-cycles/s", "traffic": (tr or {}).get("bytes"),
                      "hbm_view": {"achieved_GBs": hbm, "frac_of_8TBs": hbm / HBM_PEAK_GBS, "algorithmic_bytes_per_launch": lin_bytes,
                                   "traffic_over_algorithmic": (tr["bytes"] / lin_bytes) if tr else None, "traffic_detail": tr},
                      "note": "merged visual + IMU linearisation: fp64 VALU issue-bound (SQ_INSTS_VALU x 4 clk / (1024 SIMDs x kernel time x 2.4 GHz)); algorithmic bytes = PoseOnly 24 B + "
                              "TwoFrame 44 B in + 48 B of E out + TwoCamera 36 B per block, IMU 6256 B per factor (DESIGN.md section 4)"})
            if c and "SQ_INSTS_VALU" in c:
                ach = 4.0 * c["SQ_INSTS_VALU"] / (us * 1e-6) / 1e9
                e.update({"achieved": ach, "frac": ach / VALU_PEAK_GCYC, "valu_instructions_per_launch": c["SQ_INSTS_VALU"], "waves_per_launch": c.get("SQ_WAVES"), "source": src})
            else:
                e.update({"achieved": None, "frac": None})
        elif "k_schur" in name:
            c, src = pmc_counters("k_schur_sp0")
            e.update({"bound": "mfma", "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "traffic": (pmc_traffic("k_schur_sp0") or {}).get("bytes"),
                      "note": "band Schur complement of the inverse depths (v_mfma_f64_16x16x4_f64) + one sparse level riding in the launch"})
            if c and "SQ_INSTS_VALU_MFMA_MOPS_F64" in c:
                flops = 512.0 * c["SQ_INSTS_VALU_MFMA_MOPS_F64"]
                e.update({"achieved": flops / (us * 1e-6) / 1e12, "frac": flops / (us * 1e-6) / 1e12 / FP64_PEAK_TFLOPS, "mfma_flops_per_launch": flops,
                          "mfma_busy_cycles": c.get("SQ_VALU_MFMA_BUSY_CYCLES"), "sq_busy_cycles": c.get("SQ_BUSY_CYCLES"),
                          # matrix-pipe busy cycles over (kernel duration x 2.4 GHz x 1024 SIMDs): the share of the chip's matrix pipes in use
                          "mfma_utilisation": (c["SQ_VALU_MFMA_BUSY_CYCLES"] / (us * 2400.0 * 1024.0)) if c.get("SQ_VALU_MFMA_BUSY_CYCLES") else None, "source": src})
            else:
                e.update({"achieved": None, "frac": None})
        else:
            e.update({"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": (pmc_traffic(e["kernel"]) or {}).get("bytes"),
                      "note": "no algorithmic model for this stage"})
        return e
    # (1) dominant stage by time, (2) merged linearisation, (3) band Schur complement
    name, (us, la) = max(by.items(), key=lambda kv: kv[1][0])
    out.append(entry(name, us, la))
    out[0]["role"] = "dominant stage of the LM iteration by time"
    for key in ("k_lin_visual", "k_schur_sp0"):
        for n, (u, l) in by.items():
            if n.startswith(key) and n != name and u > 0:
                out.append(entry(n, u, l))
    return out, table, ev_us


def legs(api, syn, ctx, device, verified, which="all"):
    want = None if which == "all" else set(which.split(","))
    c3 = [None]

    def cfg3():
        if c3[0] is None:
            c3[0] = syn.config3_icp()
        return c3[0]
    table = [("batched_windows_8", lambda: batched_windows(api, syn, ctx, 8, verified)),
             ("batched_windows_16", lambda: batched_windows(api, syn, ctx, 16, None)),
             ("batched_windows_64", lambda: batched_windows(api, syn, ctx, 64, None, iters=10, reps=3)),
             ("small_windows_100", lambda: small_windows(api, syn, ctx, verified)),
             ("pose_only_K1", lambda: pose_only_leg(api, syn, ctx, verified)),
             ("icp", lambda: icp_leg(api, syn, ctx, verified)),
             ("scan_match_frame", lambda: scan_match_frame(api, syn, ctx, cfg3())),
             ("map_maintenance", lambda: map_maintenance(api, ctx, cfg3())),
             ("window_tick", lambda: window_tick(api, syn, ctx)),
             ("ceres_surface_solve", lambda: ceres_surface(api, syn, ctx)),
             ("relocalize_8_candidates", lambda: relocalize_leg(api, syn, ctx, device=device))]
    ex = {}
    for name, fn in table:
        if want is not None and name not in want:
            continue
        try:
            ex[name] = fn()
        except Exception as e:      # one failing leg must not take the others down
            ex[name] = {"error": repr(e)}
    return ex


def batched_windows(api, syn, ctx, W, verified, iters=20, reps=5):
    """W independent configs[3] windows (the reference's RL environments / loop-closure candidates) advanced by ONE launch
    chain (blockIdx.y = window), accept/reject per window on device; aggregate LM iterations/s, median of `reps` runs."""
    wins = [build_window(api, syn, ctx, seed=0xC0FFEE + i) for i in range(W)]
    b = api.ProblemBatch(ctx, [w[1] for w in wins])
    opt = fixed_iterations(api, iters)
    rates, ss = [], None
    for r in range(reps + 1):
        for cfg, _, h in wins:
            reset_state(api, h[4], cfg)
        ctx.synchronize()
        t0 = time.perf_counter()
        ss = b.solve(opt)
        dt = time.perf_counter() - t0
        if r > 0:
            rates.append(sum(s.num_iterations for s in ss) / dt)
    out = {"windows": W, "iterations_each": iters, "table_launches": bool(b.uses_tables(opt)), "lm_iters_per_sec_aggregate": float(np.median(rates)),
           "ms_per_batched_iteration": 1e3 * W / float(np.median(rates)), "runs": reps}
    if W >= 32:
        # The throughput regime's roofline: HBM.  achieved = SURVEY 8d's materialised bytes of one window-iteration x window-iterations per
        # second; traffic = counter bytes per window-iteration from the committed PMC passes of the batched chain (tools/prof_batch_pmc.sh).
        cfg0, _, h0 = wins[0]
        alg = window_algorithmic_bytes(h0[0].n, h0[1].n, h0[2].n, h0[3].n if h0[3] else 0, cfg0["n_kf"])
        rate = float(np.median(rates))
        ach = alg * rate / 1e9
        pm = batch_pmc()
        out["roofline_batched"] = {"kernel": "batched LM iteration (the whole launch chain, blockIdx = window)", "bound": "hbm", "windows": W, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": ach / HBM_PEAK_GBS, "algorithmic_bytes_per_window_iteration": alg,
                                   "traffic": None if not pm else pm.get("bytes_per_window_iteration"),
                                   "traffic_over_algorithmic": None if not pm else pm.get("bytes_per_window_iteration") / alg,
                                   "traffic_hbm_frac": None if not pm else pm.get("bytes_per_window_iteration") * rate / 1e9 / HBM_PEAK_GBS,
                                   "traffic_source": None if not pm else f"profiles/pmc_batch_latest.json ({pm.get('tag')}, W = {pm.get('windows')}, FETCH_SIZE x2 + WRITE_SIZE summed over the chain's kernels)",
                                   "traffic_by_kernel": None if not pm else pm.get("by_kernel_bytes_per_window_iteration")}
    if verified is not None:
        # every window of the batch must land where the single-window solve of the same problem lands
        cfg, prob, h = wins[0]
        reset_state(api, h[4], cfg)
        s1 = prob.solve(opt)
        ok = abs(s1.final_cost - ss[0].final_cost) <= 1e-9 * abs(s1.final_cost) and s1.num_iterations == ss[0].num_iterations
        verified["batched_windows_vs_single"] = bool(ok)
        out["final_cost_batch_vs_single"] = [ss[0].final_cost, s1.final_cost]
    b.close()
    for _, prob, h in wins:
        for x in (prob,) + tuple(h):
            if x is not None:
                x.close()
    return out


def small_windows(api, syn, ctx, verified, W=100, n_kf=10, n_lm=1500, iters=20, reps=4):
    """The reference's independent SMALL windows: RL environments are 10-keyframe windows, 8 while training / 100 while testing
    (src/environment.cpp:18-115, rl_fusion/td3.py:44-45); the live window is 3 s of keyframes (kitti.yaml:92).  W windows of n_kf keyframes
    advanced by ONE launch chain per LM iteration (blockIdx.y = window); also one such window alone (latency).  Three of the windows are
    checked against the oracle's chained loop (final cost + step counts)."""
    wins = []
    for i in range(W):
        cfg = syn.config4_window(n_kf=n_kf, n_lm=n_lm, n_prewindow=max(100, n_lm // 5), seed=0x5A11 + i)
        pre = api.preintegrate_or_none(ctx, cfg)
        st = api.State(ctx, cfg["n_kf"], cfg["n_lm"])
        for field, key in ((api.POSES, "poses"), (api.VEL, "vel"), (api.BA, "ba"), (api.BG, "bg"), (api.INV_DEPTH, "inv_depth"), (api.W_VISUAL, "w_kf")):
            st.set(field, cfg[key])
        tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
        hs = [api.two_camera_batch(ctx, cfg["cam0"], cfg["cam1"], tc["left_ob"], tc["right_ob"], tc["lm_idx"], tc["kf_idx"]),
              api.two_frame_batch(ctx, cfg["cam0"], cfg["cam1"], tf["first_ob"], tf["ob"], tf["lm_idx"], tf["kf1_idx"], tf["kf2_idx"]),
              api.pose_only_batch(ctx, cfg["cam0"], po["ob"], po["kf_idx"], po["pw_idx"], po["pw"]),
              api.imu_batch(ctx, pre, [f["kf_i"] for f in cfg["imu"]], [f["kf_j"] for f in cfg["imu"]])]
        wins.append((cfg, st, hs, api.Problem(ctx, st, *hs)))
    opt = fixed_iterations(api, iters)
    b = api.ProblemBatch(ctx, [w[3] for w in wins])
    rates, ss = [], None
    for r in range(reps + 1):
        for cfg, st, _, _ in wins:
            reset_state(api, st, cfg)
        ctx.synchronize(); t0 = time.perf_counter(); ss = b.solve(opt); dt = time.perf_counter() - t0
        if r:
            rates.append(sum(s.num_iterations for s in ss) / dt)
    rate = float(np.median(rates))
    # one window alone: the device loop's latency at this size
    cfg, st, _, prob = wins[0]
    lat = []
    for r in range(4):
        reset_state(api, st, cfg)
        ctx.synchronize(); t0 = time.perf_counter(); s1 = prob.solve(opt); lat.append((time.perf_counter() - t0) / max(s1.num_iterations, 1))
    out = {"windows": W, "n_kf": n_kf, "n_lm": n_lm, "blocks_per_window": {"two_frame": int(len(cfg["tf"]["lm_idx"])), "two_camera": int(len(cfg["tc"]["lm_idx"])), "pose_only": int(len(cfg["po"]["kf_idx"])), "imu": len(cfg["imu"])},
           "iterations_each": iters, "table_launches": bool(b.uses_tables(opt)), "lm_iters_per_sec_aggregate": rate, "ms_per_batched_iteration": 1e3 * W / rate,
           "single_window_ms_per_iteration": 1e3 * float(np.median(lat[1:]))}
    if verified is not None:
        try:
            from oracle import pyoracle as po
            ok = True
            for i in (0, W // 2, W - 1):
                cfg = wins[i][0]
                pre = np.stack([po.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
                ref = po.Window(cfg, pre).solve(max_num_iterations=iters, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
                s = ss[i]
                ok = ok and abs(s.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"] and (s.num_iterations, s.num_successful_steps) == (ref["num_iterations"], ref["num_successful_steps"])
            verified["small_windows_100_vs_oracle_3_windows"] = bool(ok)
        except Exception as e:
            verified["small_windows_100_vs_oracle_3_windows"] = repr(e)
    b.close()
    for _, st, hs, prob in wins:
        prob.close()
        for h in hs + [st]:
            h.close()
    return out


def pose_only_leg(api, syn, ctx, verified, steps=100):
    """configs[1] (K1): batched PoseOnlyReprojection residual + Jacobian, 500 000 blocks, materialised in the Ceres layout."""
    cfg = syn.config2_pose_only(seed=syn.SEED_CFG2)
    n = cfg["ob"].shape[0]
    st = api.State(ctx, cfg["n_kf"], 0)
    st.set(api.POSES, cfg["poses"]); st.set(api.W_VISUAL, cfg["w_kf"])
    batch = api.pose_only_batch(ctx, cfg["cam0"], cfg["ob"], cfg["kf_idx"], cfg["pw_idx"], cfg["pw"])
    for _ in range(20):
        batch.evaluate(st, jacobians=True)
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(steps):
        batch.evaluate(st, jacobians=True)
    ctx.timer_end()
    ms = ctx.timer_ms() / steps
    ach = POSE_ONLY_BYTES_PER_BLOCK * n / (ms * 1e-3) / 1e9
    tr = pmc_traffic("k_pose_only_rj")
    # The figure above is the steady-state rate of back-to-back launches (the next launch's ramp overlaps the previous one's drain).  rocprofv3's
    # kernel trace reports each dispatch's own begin -> end, which is longer: the same launch timed ALONE (one event pair per launch, the
    # pair's own cost subtracted) reproduces it, and the committed trace's average rides along (0.75 vs 0.645).
    ev_us = api.event_pair_us(ctx)
    single = []
    for _ in range(30):
        ctx.synchronize(); ctx.timer_begin(); batch.evaluate(st, jacobians=True); ctx.timer_end(); single.append(1e3 * ctx.timer_ms() - ev_us)
    iso_us = float(np.median(single))
    prof_ns, prof_src = profile_avg_ns("k_pose_only_rj")
    alg = POSE_ONLY_BYTES_PER_BLOCK * n
    out = {"blocks": n, "passes_per_sec": 1e3 / ms, "avg_kernel_ms": ms,
           "roofline": {"bound": "hbm", "kernel": "k_pose_only_rj", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                        "frac_is": "steady state: 100 back-to-back launches between two events",
                        "isolated_launch_us": iso_us, "frac_isolated_launch": alg / (iso_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                        "frac_from_profiles": None if prof_ns is None else alg / (prof_ns * 1e-9) / 1e9 / HBM_PEAK_GBS,
                        "profiles_avg_ns": prof_ns, "profiles_source": prof_src,
                        "traffic": (tr or {}).get("bytes"), "traffic_detail": tr, "algorithmic_bytes_per_launch": alg}}
    try:
        from oracle import pyoracle as po
        c0 = cfg["cam0"]
        cam = po.Camera.make(c0["fx"], c0["fy"], c0["cx"], c0["cy"], c0["extrinsic"])
        sel = np.random.default_rng(7).choice(n, 20000, replace=False)
        r_ref, j_ref = po.pose_only(cfg["ob"][sel], cfg["kf_idx"][sel], cfg["pw_idx"][sel], cfg["pw"], cfg["poses"], cfg["w_kf"], cam, threads=4)
        r, jj = batch.residuals(), batch.jacobian(0)
        err = max(np.abs(r[sel] - r_ref).max(), np.abs(jj[sel].reshape(len(sel), -1) - np.asarray(j_ref).reshape(len(sel), -1)).max())
        scale = max(np.abs(j_ref).max(), 1.0)
        verified["pose_only_K1_vs_oracle_20000_blocks"] = bool(err <= 1e-9 * scale)
        out["max_abs_err_vs_oracle"] = float(err)
    except Exception as e:
        out["verify_error"] = repr(e)
    batch.close(); st.close()
    return out


def icp_leg(api, syn, ctx, verified):
    """configs[2]: 100k query points vs ~340k map points.  `knn3_*` = the association alone; `pair_*` = the unit SURVEY 8d defines (one
    query through transform -> 3-NN -> gate -> plane residual + Jacobian: association + the first linearisation pass of the ICP solve,
    lvf_icp_solve with one LM iteration, so a little MORE than a pair's work)."""
    import ctypes as C
    from lvio_fusion_amd import _lib
    ex = {}
    c3 = syn.config3_icp()
    t0 = time.perf_counter()
    mp = api.Map(ctx, c3["map"], c3["thr_ground"])
    ctx.synchronize()
    ex["map_index_build_ms"] = 1e3 * (time.perf_counter() - t0)
    sc = api.Scan(ctx, c3["query"])
    Q, M = c3["query"].shape[0], c3["map"].shape[0]
    for name, thr in (("ground_thr4.0", c3["thr_ground"]), ("surf_thr1.0", c3["thr_surf"])):
        for _ in range(3):
            api.knn3(mp, sc, c3["pose0"], thr)
        ctx.synchronize()
        reps = 20
        ctx.timer_begin()
        for _ in range(reps):
            api.knn3(mp, sc, c3["pose0"], thr)
        ctx.timer_end()
        ms = ctx.timer_ms() / reps
        stats = np.zeros((Q, 6), np.int32); lv = np.zeros((8, 4), np.float32); nl = C.c_int()
        pose = np.ascontiguousarray(c3["pose0"], dtype=np.float64)
        api._chk(ctx.L.lvf_knn3_debug_stats2(mp.h, sc.h, pose.ctypes.data_as(_lib.c_double_p), float(thr), stats.ctypes.data_as(_lib.c_int_p), 6,
                                            lv.ctypes.data_as(_lib.c_float_p), C.byref(nl)))
        cand = float(stats[:, 0].sum())
        api.knn3(mp, sc, c3["pose0"], thr)
        ex[f"knn3_{name}"] = {"Q": Q, "M": M, "ms": ms, "mpairs_per_s": Q / ms / 1e3, "hbm_frac": KNN_BYTES(Q, M) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "valid_frac": float(sc.download()[2].mean()), "candidates_per_query_mean": cand / Q,
                              "candidate_evaluations_per_sec": cand / (ms * 1e-3)}
    # the 8d pair: association + one linearisation/solve pass (ground gate, RPZ block)
    rp = np.zeros(6)
    for _ in range(3):
        rp[:] = 0.0
        api.icp_solve(mp, sc, c3["map_pose"], c3["pose0"], rp, 0, c3["thr_ground"], 1.0, 0.1, max_num_iterations=1)
    ctx.synchronize()
    reps, t0 = 20, time.perf_counter()
    for _ in range(reps):
        rp[:] = 0.0
        summ = api.icp_solve(mp, sc, c3["map_pose"], c3["pose0"], rp, 0, c3["thr_ground"], 1.0, 0.1, max_num_iterations=1)
    dt = (time.perf_counter() - t0) / reps
    ex["pair_association_plus_linearisation"] = {"Q": Q, "ms": 1e3 * dt, "mpairs_per_s": Q / dt / 1e6, "valid_blocks": int(summ.num_residual_blocks),
                                                 "note": "wall time of lvf_icp_solve(max 1 iteration) incl. its 200-byte read-back"}
    ex["icp_mpairs_per_sec"] = ex["pair_association_plus_linearisation"]["mpairs_per_s"]
    # The reference builds its kd-tree INSIDE every ScanToMapWithGround / ScanToMapWithSegmented call (association.cpp:278-279, :336-337): the
    # same pair pass with the map index built in the timed region, from a host cloud (upload + build) and from a device-resident cloud.
    try:
        dcloud = api.Cloud(ctx, c3["map"])
        for tag, src in (("host_cloud", c3["map"]), ("device_cloud", dcloud)):
            ts = []
            for r in range(6):
                rp[:] = 0.0
                ctx.synchronize(); t0 = time.perf_counter()
                m2 = api.Map(ctx, src, c3["thr_ground"])
                api.icp_solve(m2, sc, c3["map_pose"], c3["pose0"], rp, 0, c3["thr_ground"], 1.0, 0.1, max_num_iterations=1)
                ts.append(time.perf_counter() - t0)
                m2.close()
            dt2 = float(np.median(ts[1:]))
            ex[f"pair_incl_index_{tag}"] = {"ms": 1e3 * dt2, "mpairs_per_s": Q / dt2 / 1e6}
        dcloud.close()
        ex["icp_mpairs_per_sec_incl_index"] = {"host_cloud": ex["pair_incl_index_host_cloud"]["mpairs_per_s"], "device_cloud": ex["pair_incl_index_device_cloud"]["mpairs_per_s"],
                                               "note": "map index (grid pyramid) built inside the timed region, as the reference rebuilds its kd-tree per call; icp_mpairs_per_sec above has the map resident"}
    except Exception as e:
        ex["icp_mpairs_per_sec_incl_index"] = {"error": repr(e)}
    # roofline of the association kernel (the metric's second half): algorithmic pass bytes 40 Q + 16 M against HBM (it is cache / latency
    # bound: the honest companions are the counter traffic, the candidates a query evaluates and the VALU issue share)
    try:
        g = ex["knn3_ground_thr4.0"]
        c, src = pmc_counters("k_knn3<false>")
        us = g["ms"] * 1e3
        ach = KNN_BYTES(Q, M) / (us * 1e-6) / 1e9
        r = {"kernel": "k_knn3", "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "avg_launch_us": us,
             "algorithmic_bytes_per_launch": KNN_BYTES(Q, M), "traffic": None, "candidates_per_query_mean": g["candidates_per_query_mean"],
             "candidate_evaluations_per_sec": g["candidate_evaluations_per_sec"],
             "note": "3-NN association, ground gate, Q = 100 k / M = 340 k: 20 back-to-back launches between two events on the library's stream; cache / latency bound "
                     "(a query walks ~10 dependent cell look-ups); traffic and VALU share from the committed PMC passes of this leg (average over the ground and surf launches)"}
        if c and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            r["traffic"] = (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0
            r["traffic_over_algorithmic"] = r["traffic"] / KNN_BYTES(Q, M)
            r["l2_hit_rate"] = c["TCC_HIT_sum"] / (c["TCC_HIT_sum"] + c["TCC_MISS_sum"]) if "TCC_HIT_sum" in c and "TCC_MISS_sum" in c else None
            r["source"] = src + "; FETCH_SIZE x2 per gfx950 correction"
        if c and "SQ_INSTS_VALU" in c:
            r["valu_issue_frac"] = 4.0 * c["SQ_INSTS_VALU"] / (us * 1e-6) / 1e9 / VALU_PEAK_GCYC
            r["valu_instructions_per_query"] = c["SQ_INSTS_VALU"] * 64.0 / 8.0 / Q      # 8 lanes cooperate on a query
        ex["roofline_icp"] = r
    except Exception as e:
        ex["roofline_icp"] = {"error": repr(e)}
    try:
        from oracle import pyoracle as po
        nq = 4000
        sel = np.random.default_rng(11).choice(Q, nq, replace=False)
        api.knn3(mp, sc, c3["pose0"], c3["thr_ground"])
        idx, d2, valid = sc.download()
        ridx, rd2, rvalid = po.knn3(c3["map"], c3["query"][sel], c3["pose0"], c3["thr_ground"], method=0, threads=4)
        v = rvalid.astype(bool)
        ok = np.array_equal(valid[sel].astype(bool), v) and np.array_equal(idx[sel][v], ridx[v]) and np.array_equal(d2[sel][v], rd2[v])
        verified["knn3_vs_oracle_4000_queries_bit_exact"] = bool(ok)
    except Exception as e:
        ex["verify_error"] = repr(e)
    mp.close(); sc.close()
    return ex


def ceres_surface(api, syn, ctx):
    """The configs[3] window through the Ceres-shaped surface (gpu::Solve on a 91k-block ceres::Problem, host/adapter_selftest): the
    drop-in cost of the per-block accessor walk next to the window tick above."""
    import subprocess, tempfile
    exe = os.path.join(ROOT, "lvio_fusion_amd", "host", "adapter_selftest")
    if not os.path.exists(exe):
        return {"error": "lvio_fusion_amd/host/adapter_selftest not built"}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests.test_gpu_adapter import _dump, _cam_vec, _sorted_by_kf
    cfg = _sorted_by_kf(syn.config4_window())
    pre = api.preintegrate_or_none(ctx, cfg)
    d = tempfile.mkdtemp()
    tc, tf, po = cfg["tc"], cfg["tf"], cfg["po"]
    _dump(d, "meta.i32", [cfg["n_kf"], cfg["n_lm"], 1, 0, -1], np.int32)
    for name, key in (("poses", "poses"), ("vel", "vel"), ("ba", "ba"), ("bg", "bg"), ("inv_depth", "inv_depth"), ("w_kf", "w_kf")):
        _dump(d, name + ".f64", cfg[key], np.float64)
    _dump(d, "cam0.f64", _cam_vec(cfg["cam0"]), np.float64); _dump(d, "cam1.f64", _cam_vec(cfg["cam1"]), np.float64)
    _dump(d, "tc_left_ob.f64", tc["left_ob"], np.float64); _dump(d, "tc_right_ob.f64", tc["right_ob"], np.float64)
    _dump(d, "tc_lm.i32", tc["lm_idx"], np.int32); _dump(d, "tc_kf.i32", tc["kf_idx"], np.int32)
    _dump(d, "tf_first_ob.f64", tf["first_ob"], np.float64); _dump(d, "tf_ob.f64", tf["ob"], np.float64)
    _dump(d, "tf_lm.i32", tf["lm_idx"], np.int32); _dump(d, "tf_kf1.i32", tf["kf1_idx"], np.int32); _dump(d, "tf_kf2.i32", tf["kf2_idx"], np.int32)
    _dump(d, "po_ob.f64", po["ob"], np.float64); _dump(d, "po_pw.f64", po["pw"], np.float64)
    _dump(d, "po_kf.i32", po["kf_idx"], np.int32); _dump(d, "po_pw_idx.i32", po["pw_idx"], np.int32)
    _dump(d, "preint.f64", pre, np.float64)
    _dump(d, "imu_i.i32", [f["kf_i"] for f in cfg["imu"]], np.int32); _dump(d, "imu_j.i32", [f["kf_j"] for f in cfg["imu"]], np.int32)
    import re
    env = dict(os.environ, LVF_SELFTEST_REPEAT="1", LVF_SELFTEST_TICK="1")
    p = subprocess.run([exe, "window", d], capture_output=True, text=True, timeout=180, env=env)
    lines = [l for l in p.stderr.strip().splitlines() if "ms" in l]
    out = {"max_num_iterations": 1, "blocks": int(tc["lm_idx"].shape[0] + tf["lm_idx"].shape[0] + po["kf_idx"].shape[0] + len(cfg["imu"])),
           "report": lines[-4:], "rc": p.returncode}
    for l in lines:
        m = re.search(r"adapt::Solve \(warm repeat\): ([0-9.]+) ms", l)
        if m:
            out["adapt_solve_ms"] = float(m.group(1))
        m = re.search(r"ceres-surface tick \(median of 5\): ([0-9.]+) ms = build .*? ([0-9.]+) \+ adapt::Solve ([0-9.]+) \+ ~Problem ([0-9.]+)", l)
        if m:
            out["ceres_surface_tick_ms"] = float(m.group(1))
            out["ceres_surface_tick_parts_ms"] = {"build_Create_AddResidualBlock": float(m.group(2)), "adapt_Solve_1_iteration": float(m.group(3)), "problem_destructor": float(m.group(4))}
            out["tick_note"] = ("one backend tick as backend.cpp:203-211 runs it through the Ceres surface: fresh adapt::Problem, one X::Create heap functor + AddResidualBlock per block, "
                                "adapt::Solve, ~Problem; the ceres::Problem is lvf_ceres_compat.h's stand-in (Ceres is not in the image); compare window_tick.ms_per_tick_1_iteration "
                                "(the persistent lvf_window_* path)")
    return out


def scan_match_frame(api, syn, ctx, c3, reps=10):
    """Mapping::Optimize's per-frame body on configs[2]: ground (pitch,roll,z) then surf (yaw,x,y) sub-problem, each =
    association over the whole feature cloud + <= 4 LM iterations on device (lvf_scan_match, maps resident)."""
    mg, ms = c3["map"][c3["map_ground"]], c3["map"][~c3["map_ground"]]
    qg, qs = c3["query"][c3["query_ground"]], c3["query"][~c3["query_ground"]]
    opt = api.scan_match_options(0.2, outer_iterations=1, prior_weight=0.0)   # relocate-mode blocks: no visual prior pinning the step
    mpg, scg, mps, scs = api.Map(ctx, mg, opt.thr_ground), api.Scan(ctx, qg), api.Map(ctx, ms, opt.thr_surf), api.Scan(ctx, qs)
    for _ in range(2):
        res = api.scan_match(mpg, scg, mps, scs, c3["map_pose"], c3["pose0"], opt)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = api.scan_match(mpg, scg, mps, scs, c3["map_pose"], c3["pose0"], opt)
    dt = (time.perf_counter() - t0) / reps
    # with both map indices built inside the timed region (association.cpp:278-279, :336-337: one kd-tree per sub-problem call), from host
    # clouds and from device-resident clouds (Mapping::BuildMapFrame's merged cloud kept on the device: lvf_cloud_*)
    incl = {}
    try:
        dmg, dms = api.Cloud(ctx, mg), api.Cloud(ctx, ms)
        for tag, (sg, ss_) in (("host_cloud", (mg, ms)), ("device_cloud", (dmg, dms))):
            ts = []
            for r in range(6):
                ctx.synchronize(); t0 = time.perf_counter()
                a, b_ = api.Map(ctx, sg, opt.thr_ground), api.Map(ctx, ss_, opt.thr_surf)
                api.scan_match(a, scg, b_, scs, c3["map_pose"], c3["pose0"], opt)
                ts.append(time.perf_counter() - t0)
                a.close(); b_.close()
            incl[tag] = 1e3 * float(np.median(ts[1:]))
        dmg.close(); dms.close()
    except Exception as e:
        incl = {"error": repr(e)}
    out = {"Q_ground": int(len(qg)), "Q_surf": int(len(qs)), "M_ground": int(len(mg)), "M_surf": int(len(ms)), "ms_per_frame": 1e3 * dt,
           "scan_match_frame_incl_index_ms": incl,
           "frames_per_sec": 1.0 / dt, "mpairs_per_s": (len(qg) + len(qs)) / dt / 1e6,
           "valid": [res.ground.num_residual_blocks, res.surf.num_residual_blocks],
           "lm_iterations": [res.ground.num_iterations, res.surf.num_iterations],
           "pos_err_before_m": float(np.abs(c3["pose0"][4:] - c3["pose_true"][4:]).max()),
           "pos_err_after_m": float(np.abs(np.array(res.pose[:])[4:] - c3["pose_true"][4:]).max())}
    for h in (mpg, scg, mps, scs):
        h.close()
    return out


def map_maintenance(api, ctx, c3, reps=10):
    """SURVEY 8f row 2 on configs[2]'s clouds, everything device-resident: ToWorld transform of the 100k-point scan (HBM-bound:
    32 B/point), VoxelGrid (leaf 0.4), RadiusOutlierRemoval (0.8 m, 4), RANSAC ground plane on the ground points, and the map
    index build from the merged device cloud."""
    out = {}
    q = api.Cloud(ctx, c3["query"]); mp = api.Cloud(ctx, c3["map"]); qg = api.Cloud(ctx, c3["query"][c3["query_ground"]])

    def timed(fn, n=reps):
        h = fn(); ctx.synchronize()
        (h[0] if isinstance(h, tuple) else h).close()
        t0 = time.perf_counter()
        hs = [fn() for _ in range(n)]
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / n
        size = len(hs[0][0] if isinstance(hs[0], tuple) else hs[0])
        for h in hs:
            (h[0] if isinstance(h, tuple) else h).close()
        return dt, size
    dt, n = timed(lambda: q.transform(c3["pose0"]))
    out["transform"] = {"points": n, "us": 1e6 * dt, "gb_per_s_incl_alloc": 32.0 * n / dt / 1e9}
    dt, n = timed(lambda: q.voxel_filter(0.4))
    out["voxel_filter_0.4"] = {"points_in": len(q), "points_out": n, "us": 1e6 * dt}
    dt, n = timed(lambda: q.radius_outlier_filter(0.8, 4))
    out["radius_outlier_0.8_4"] = {"points_in": len(q), "points_out": n, "us": 1e6 * dt}
    dt, n = timed(lambda: qg.segment_plane(0.02, 100, 12345))
    out["segment_plane_100_hyp"] = {"points_in": len(qg), "inliers": n, "us": 1e6 * dt}
    t0 = time.perf_counter()
    for _ in range(reps):
        m = api.Map(ctx, mp, 4.0); m.close()
    ctx.synchronize()
    out["map_index_from_device_cloud_us"] = 1e6 * (time.perf_counter() - t0) / reps
    # FeatureAssociation::Process on one raw 64 x 1800 revolution (upload + projection + ground + segmentation +
    # smoothness + picks + voxel / outlier / plane tail + Sensor2Robot)
    from lvio_fusion_amd import synthetic as syn
    scan = syn.raw_scan(); ext = syn.lidar_extrinsic()
    g, s = api.lidar_extract(ctx, scan, ext); ctx.synchronize(); ng, ns = len(g), len(s); g.close(); s.close()

    def extract_ms(host_counts):
        was = api.extract_host_counts(ctx, host_counts)
        try:
            for _ in range(2):
                g, s = api.lidar_extract(ctx, scan, ext); g.close(); s.close()
            ctx.synchronize(); t0 = time.perf_counter()
            for _ in range(reps):
                g, s = api.lidar_extract(ctx, scan, ext); g.close(); s.close()
            ctx.synchronize()
            return 1e3 * (time.perf_counter() - t0) / reps
        finally:
            api.extract_host_counts(ctx, was)
    out["feature_extraction"] = {"points_in": int(scan.shape[0]), "ground_out": ng, "surf_out": ns, "ms_per_scan": extract_ms(False),
                                 "ms_per_scan_host_counted_path": extract_ms(True),
                                 "note": "ms_per_scan: counts kept on the device, one stream wait per scan (the default); host_counted_path: rounds 2-4 (a count / bounding box read back after every stage, 13 waits), same clouds bit for bit"}
    for h in (q, mp, qg):
        h.close()
    return out


def window_tick(api, syn, ctx, reps=10):
    """one backend tick through the PERSISTENT window (lvf_window_solve with max_num_iterations = 1 =
    assemble the block lists from the incremental host mirror + refill the persistent device batches + one LM iteration +
    read-back) on the configs[3]-sized window; the assembly/upload overhead is what remains after subtracting the LM
    iteration measured above."""
    cfg = syn.config4_window(n_prewindow=0)
    pre = api.preintegrate_or_none(ctx, cfg)
    win = api.Window(ctx, cfg["cam0"], cfg["cam1"], baseline=syn.baseline())
    tc, tf = cfg["tc"], cfg["tf"]
    t0 = time.perf_counter()
    order_tc = np.argsort(tc["kf_idx"], kind="stable")
    tf_by_kf = {k: np.nonzero(tf["kf2_idx"] == k)[0] for k in range(cfg["n_kf"])}
    j = 0
    for k in range(cfg["n_kf"]):
        win.add_keyframe(k, cfg["poses"][k], cfg["w_kf"][k])
        win.set_imu(k, cfg["vel"][k], cfg["ba"][k], cfg["bg"][k], pre[k - 1] if k > 0 else None)
        while j < len(order_tc) and tc["kf_idx"][order_tc[j]] == k:
            i = order_tc[j]; j += 1
            win.add_landmark(int(tc["lm_idx"][i]), k, tc["left_ob"][i], tc["right_ob"][i], cfg["inv_depth"][tc["lm_idx"][i]])
        for i in tf_by_kf[k]:
            win.add_observation(int(tf["lm_idx"][i]), k, tf["ob"][i])
    populate_s = time.perf_counter() - t0
    opt = api.default_solver_options(); opt.max_num_iterations = 1
    win.solve(opt); win.solve(opt)
    t0 = time.perf_counter()
    for _ in range(reps):
        win.solve(opt)
    dt = (time.perf_counter() - t0) / reps
    out = {"counts": win.counts(), "ms_per_tick_1_iteration": 1e3 * dt, "python_populate_s": populate_s}
    win.close()
    return out


def relocalize_leg(api, syn, ctx, n=8, device=0):
    """configs[4] unit of work on ONE GPU: n loop-closure candidates (Mapping::Relocate = 4 outer x {ground, surf}) evaluated
    back to back incl. map-index builds and uploads; on N GPUs each rank takes n/N of them and one 72-B/record all_gather
    follows (lvio_fusion_amd/relocalize.py)."""
    from lvio_fusion_amd import relocalize as rl
    cands = syn.config5_candidates(n)
    for c in cands:
        rl.split_candidate(c)          # ground / surf clouds held separately, as frame->feature_lidar does (numpy masking is not part of the path)
    rl.relocalize(api, ctx, cands[:1])
    rl.relocalize(api, ctx, cands[:2], batched=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    best, rec = rl.relocalize(api, ctx, cands)
    dt = time.perf_counter() - t0
    # ONE launch chain for all candidates (lvf_scan_match_batch): median of 5
    tb = []
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        bestb, recb = rl.relocalize(api, ctx, cands, batched=True)
        tb.append(time.perf_counter() - t0)
    dtb = float(np.median(tb))
    sameb = bool(np.array_equal(rec[:, [0, 8]], recb[:, [0, 8]]) and np.allclose(rec[:, 1:8], recb[:, 1:8], rtol=0, atol=1e-9))
    # ... with the candidates' clouds RESIDENT in HBM (api.Cloud = lvf_cloud: what a pipeline that keeps frame->feature_lidar on the device —
    # lvf_lidar_extract's outputs, lvf_cloud_concat for BuildOldMapFrame — hands over): no 6 MB of map points over PCIe per relocalisation
    for c in cands:
        rl.resident_candidate(api, ctx, c)
    rl.evaluate_candidates_batched(api, ctx, cands[:2], resident=True)
    tr = []
    for _ in range(5):
        ctx.synchronize()
        t0 = time.perf_counter()
        resr = rl.evaluate_candidates_batched(api, ctx, cands, resident=True)
        tr.append(time.perf_counter() - t0)
    dtr = float(np.median(tr))
    order = np.argsort(recb[:, 8])
    samer = bool(all(int(r.score) - rl.RELOCATE_BASE_SCORE == int(recb[order[k], 0]) and np.allclose(np.array(r.relative_o_c[:]), recb[order[k], 1:8], rtol=0, atol=1e-12)
                     for k, r in enumerate(resr)))
    for c in cands:
        for h in c.pop("resident"):
            h.close()
    # the same candidates with three more contexts (streams + host threads) on the same GPU: a candidate is a latency chain
    workers = [api.Context(int(device) if isinstance(device, int) else 0) for _ in range(3)]
    rl.relocalize(api, ctx, cands[:4], workers=workers)
    for c in [ctx] + workers:
        c.synchronize()
    t0 = time.perf_counter()
    best4, rec4 = rl.relocalize(api, ctx, cands, workers=workers)
    dt4 = time.perf_counter() - t0
    for c in workers:
        c.close()
    same = bool(np.array_equal(rec[:, [0, 8]], rec4[:, [0, 8]]) and np.allclose(rec[:, 1:8], rec4[:, 1:8], rtol=0, atol=1e-12))
    return {"candidates": n, "points_per_candidate": int(cands[0]["query"].shape[0]), "map_points": int(cands[0]["map"].shape[0]),
            "ms_total": 1e3 * dtb, "candidates_per_sec": n / dtb, "best": None if bestb is None else {"candidate": bestb[0], "score": bestb[1]},
            "note": "ms_total = all candidates in ONE launch chain (lvf_scan_match_batch) incl. 16 map-index builds and scan uploads; one_at_a_time / four_streams: the round-3 forms",
            "batched_same_records_as_one_at_a_time": sameb,
            "clouds_resident_in_hbm": {"ms_total": 1e3 * dtr, "candidates_per_sec": n / dtr, "same_records_as_uploaded_clouds": samer,
                                       "note": "the candidates' map / scan clouds are lvf_cloud objects already (lvf_map_create_batch_from_clouds, lvf_scan_create_from_cloud): index builds + the batched solve, no PCIe upload"},
            "one_at_a_time": {"ms_total": 1e3 * dt, "candidates_per_sec": n / dt},
            "scores": [float(x) for x in rec[np.argsort(rec[:, 8]), 0]],
            "four_streams": {"ms_total": 1e3 * dt4, "candidates_per_sec": n / dt4, "same_records_as_one_stream": same}}


def cpu_baseline(api, cfg, prob, st, verified):
    """The restated reference CPU path on the headline workload: the oracle's LM iteration of the SAME configs[3] window (Jet autodiff
    linearisation of every factor, exact Schur complement, dense Cholesky; OpenMP with the reference's num_threads = min(8, 0.75 nproc),
    estimator.cpp:10), bounded to ~10 s.  Also checks the GPU's first iteration against it."""
    from oracle import pyoracle as po
    from lvio_fusion_amd import synthetic as syn
    nproc = os.cpu_count() or 1
    threads = min(8, max(1, int(0.75 * nproc)))
    pre = np.stack([po.imu_preintegrate(f["samples"], f["acc0"], f["gyr0"], f["ba"], f["bg"], syn.IMU_NOISE) for f in cfg["imu"]])
    win = po.Window(cfg, pre)
    r0 = win.lm_iteration(1e4, 2.0)                     # also warms page faults and the OpenMP pool
    # GPU iteration 1 from the same start, same radius
    reset_state(api, st, cfg)
    g = prob.lm_iteration(api.default_solver_options(), 1e4, 2.0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    ok = rel(g["cost_before"], r0["cost_before"]) <= 1e-8 and rel(g["cost_after"], r0["cost_after"]) <= 1e-6 and bool(g["accepted"]) == bool(r0["accepted"])
    verified["full_window_iteration_1_cost_vs_oracle"] = bool(ok)
    # The timed call itself — prob.solve(CHUNK iterations, tolerances off) from the perturbed start — against the oracle's chained loop
    # (oracle/lm.h lm_solve: ITS radius / decrease factor, Ceres' termination order): final state, cost, step counts.  The same chain is
    # the CPU baseline's sample (CHUNK + 1 trial steps, each one LM iteration's work).
    win = po.Window(cfg, pre)
    o = fixed_iterations(api, CHUNK)
    t0 = time.perf_counter()
    ref = win.solve(max_num_iterations=CHUNK, huber_a=o.huber_a, initial_trust_region_radius=o.initial_trust_region_radius, function_tolerance=0.0,
                    gradient_tolerance=0.0, parameter_tolerance=0.0, min_relative_decrease=o.min_relative_decrease)
    dt = time.perf_counter() - t0
    k = CHUNK + 1
    reset_state(api, st, cfg)
    s = prob.solve(o)
    worst = 0.0
    for name, field in (("poses", api.POSES), ("vel", api.VEL), ("ba", api.BA), ("bg", api.BG), ("inv_depth", api.INV_DEPTH)):
        got = np.asarray(st.get(field), np.float64).ravel(); want = np.asarray(getattr(win, name), np.float64).ravel()
        worst = max(worst, float(np.max(np.abs(got - want) / (np.abs(want) + 1e-10 * np.abs(want).max() + 1e-300))))
    same_counts = (s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.termination) == \
                  (ref["num_iterations"], ref["num_successful_steps"], ref["num_unsuccessful_steps"], ref["termination"])
    verified["device_loop_K_iterations_vs_oracle"] = bool(same_counts and rel(s.final_cost, ref["final_cost"]) <= 1e-6 and worst <= 1e-6)
    out = {"value": k / dt, "unit": "iter/s", "cores": po.max_threads(), "kind": "port",
           "sample": f"{k} LM trial steps (one solve of {CHUNK} iterations) of the same configs[3] window (oracle: Jet autodiff linearisation + exact Schur + dense "
                     f"Cholesky, OpenMP {po.max_threads()} threads on a {nproc}-core host); restated reference CPU path — Ceres/PCL are not in the image",
           "gpu_vs_oracle_iteration_1": {"cost_before": [g["cost_before"], r0["cost_before"]], "cost_after": [g["cost_after"], r0["cost_after"]]},
           "gpu_vs_oracle_solve_K": {"K": CHUNK, "final_cost": [s.final_cost, ref["final_cost"]], "iterations": [s.num_iterations, ref["num_iterations"]],
                                     "successful_steps": [s.num_successful_steps, ref["num_successful_steps"]], "worst_state_rel_diff": worst}}
    # The evaluation half of the CPU path with the REFERENCE'S OWN functor text where it can be compiled (oracle/_ref: visual_error.hpp /
    # imu_error.hpp unmodified, one heap functor per block through X::Create as backend.cpp:119-160 builds them, CostFunction::Evaluate with
    # all Jacobians from `threads` workers): what one Ceres evaluation pass of this window costs the reference, beside the port's figure.
    try:
        from oracle import pyref
        if pyref.build() is not None:
            rf = pyref.window_eval_timed(cfg, pre, threads=threads, reps=3)
            out["kind_note"] = "value: whole LM iteration of the port; reference_functors: the reference's own functor text (oracle/_ref), the evaluation pass alone"
            out["reference_functors"] = {"kind": "reference", "blocks": rf["blocks"], "cores": threads, "reference_functors_eval_ms": 1e3 * rf["evaluate_s"],
                                         "reference_functors_create_ms": 1e3 * rf["create_s"], "evaluation_passes_per_sec": 1.0 / rf["evaluate_s"],
                                         "sample": "3 full passes of CostFunction::Evaluate (residuals + Jacobians) over the window's 91 k blocks after creating one heap functor per block "
                                                   "(the reference rebuilds them twice per tick); Ceres itself (Jet implementation, loss, Schur, Cholesky) is not in the image: "
                                                   "AutoDiffCostFunction runs over oracle/ref_shim's Jet"}
            out["reference_functors_eval_ms"] = 1e3 * rf["evaluate_s"]
    except Exception as e:
        out["reference_functors"] = {"error": repr(e)}
    # the other legs of the metric, bounded samples (a few seconds each)
    try:
        c2 = syn.config2_pose_only(seed=syn.SEED_CFG2)
        c0 = c2["cam0"]
        cam = po.Camera.make(c0["fx"], c0["fy"], c0["cx"], c0["cy"], c0["extrinsic"])
        reps, t0 = 0, time.perf_counter()
        while reps < 20 and time.perf_counter() - t0 < 4.0:
            po.pose_only(c2["ob"], c2["kf_idx"], c2["pw_idx"], c2["pw"], c2["poses"], c2["w_kf"], cam, threads=threads); reps += 1
        out["pose_only_K1_passes_per_sec"] = {"value": reps / (time.perf_counter() - t0), "cores": threads, "sample": f"{reps} passes over the 500000-block configs[1] window"}
        c3 = syn.config3_icp()
        nq = 20000
        build_s = po.kdtree_build_seconds(c3["map"])
        t0 = time.perf_counter()
        po.knn3(c3["map"], c3["query"][:nq], c3["pose0"], c3["thr_ground"], method=1, threads=1)
        q_s = time.perf_counter() - t0 - build_s
        out["icp_mpairs_per_sec"] = {"value": nq / max(q_s, 1e-9) / 1e6, "incl_tree_build": 100000 / (build_s + 5 * max(q_s, 1e-9)) / 1e6, "cores": 1,
                                     "sample": f"{nq} of the 100000 configs[2] queries against the 340k-point map, leaf-15 kd-tree (the reference's "
                                               "PCL/FLANN structure, rebuilt per call there: association.cpp:279), 1 thread like the reference's loop"}
    except Exception as e:   # a failing baseline must not take the GPU numbers down with it
        out["extras_error"] = repr(e)
    return out


if __name__ == "__main__":
    main()
