// solver_chain.hip — the host side of one window's LM iteration: the argument blocks of the chain (build_chain), the launches of an
// iteration (enqueue_linearize, enqueue_reduced_system, enqueue_iteration), the stage clock, and the LM driver around the device-resident
// control block.  Everything executed per enqueued iteration is in this file; the kernels are in solver_kernels.hip,
// solver_assemble.hip, solver_chol.hip and solver_back.hip.
#include <hip/hip_ext.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "solver_host.hpp"

namespace lvf {

static void fill_cost_visual(const lvf_problem* p, CostVisual& a) {
  a = CostVisual{};
  if (p->tc && p->tc->n) {
    a.n_tc = p->tc->n; a.tc_lo = (const double2*)p->tc->ob_a.p; a.tc_ro = (const double2*)p->tc->ob_b.p; a.tc_lm = p->tc->idx_a.p; a.tc_kf = p->tc->idx_b.p;
    a.tc_w = p->tc->wblk.n ? p->tc->wblk.p : nullptr; a.tc_left = p->tc->cam_a; a.tc_right = p->tc->cam_b;
  }
  if (p->tf && p->tf->n) {
    a.n_tf = p->tf->n; a.tf_fo = p->tf_fo(); a.tf_ob = p->tf_ob(); a.tf_lm = p->tf_lm(); a.tf_k1 = p->tf_k1();
    a.tf_k2 = p->tf_k2(); a.tf_left = p->tf->cam_a; a.tf_right = p->tf->cam_b;
  }
  if (p->po && p->po->n) {
    a.n_po = p->po->n; a.po_ob = (const double2*)p->po->ob_a.p; a.po_kf = p->po->idx_a.p; a.po_pwi = p->po->idx_b.p; a.po_pw = p->po->table.p; a.po_cam = p->po->cam_a;
  }
  a.g_tc = grid(a.n_tc); a.g_tf = grid(a.n_tf);
}

// accumulates 1/2 sum rho into *cost_slot at the given state (residual-only pass); not gated by the LM control block
int enqueue_cost(lvf_problem* p, const StateP& s, const lvf_state* imu_state_view, double huber, double* cost_slot) {
  hipStream_t q = p->ctx->stream;
  CostArgs c{};
  fill_cost_visual(p, c.a);
  c.n_kf = p->n_kf; c.s = s; c.huber = huber; c.cost = cost_slot; c.done = nullptr;
  c.nblocks = c.a.g_tc + c.a.g_tf + grid(c.a.n_po);
  if (c.nblocks > 0) hipLaunchKernelGGL(k_cost_visual, dim3(c.nblocks), dim3(kT), 0, q, c);
  if (p->imu && p->imu->n) {
    static_assert(kStripes == 32, "k_imu stripes its cost over 32 slots");
    LVF_TRY(launch_imu(p->imu, imu_state_view, false, cost_slot));      // residuals and their cost in one launch
  }
  if (p->prior && p->prior->n) {
    LVF_TRY(launch_pose_prior(p->prior, imu_state_view, false));
    hipLaunchKernelGGL(k_cost_sq, dim3(grid(6 * p->prior->n)), dim3(kT), 0, q, 6 * p->prior->n, p->prior->res.p, cost_slot);
  }
  if (p->lidar && p->lidar->n) hipLaunchKernelGGL(k_lidar_cost, dim3(grid(p->lidar->n)), dim3(kT), 0, q, lidar_pose_args(p->lidar), p->n_kf, s.poses, cost_slot);
  if (p->dprior) hipLaunchKernelGGL(k_dense_prior_cost, dim3(1), dim3(kDensePriorT), 0, q, dense_prior_args(p->dprior), s, cost_slot);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

static void fill_back_args(lvf_problem* p, BackArgs& ba, size_t* lds_bytes) {
  SpBack sb{};
  sb.lv = p->sp_levels; sb.rows = p->sp_rows.p; sb.owner = p->sp_owner.p; sb.W = p->sp_W.p; sb.Linv = p->sp_L.p; sb.perm = p->perm.p;
  sb.off = p->off; sb.aug = p->aug; sb.d_total = p->d;
  sb.dbg = nullptr;
  int max_count = 0;
  for (int lv = 0; lv < p->sp_levels.n; ++lv) {
    max_count = std::max(max_count, p->sp_levels.count[lv]);
    sb.item0[lv] = p->sp_item0[lv]; sb.items[lv] = p->sp_items[lv];
  }
  const int n_nodes = p->sp_levels.n ? p->sp_levels.first[p->sp_levels.n - 1] + p->sp_levels.count[p->sp_levels.n - 1] : 0;
  sb.total_items = p->sp_levels.n ? p->sp_item0[p->sp_levels.n - 1] + p->sp_items[p->sp_levels.n - 1] : 0;
  sb.n_nodes = n_nodes; sb.max_count = max_count;
  sb.nodes = p->sp_nodes.p;
  static const bool big_lds = [] {        // up to 160 KB of LDS per workgroup on gfx950; the default cap for dynamic LDS is 64 KB
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_backsolve), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_backsolve_b), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024) == hipSuccess;
  }();
  const size_t lds_cap = big_lds ? 156 * 1024 : 64 * 1024;
  size_t doubles = (size_t)p->off + (size_t)((p->ndense + 63) / 64) * 64 + (size_t)(kBParts + 1) * kNB + 9 * (size_t)max_count + kBT + (size_t)n_nodes + 2;
  sb.linv_in_lds = (doubles + 81 * (size_t)n_nodes) * sizeof(double) <= 48 * 1024 ? 1 : 0;
  if (sb.linv_in_lds) doubles += 81 * (size_t)n_nodes;
  int max_items = 0;
  for (int lv = 0; lv < p->sp_levels.n; ++lv) max_items = std::max(max_items, p->sp_items[lv]);
  sb.prod_items = ((doubles + 9 * (size_t)max_items) * sizeof(double) <= lds_cap) ? max_items : 0;
  doubles += 9 * (size_t)sb.prod_items;
  *lds_bytes = doubles * sizeof(double);
  ba.Sd = p->S.p + (size_t)p->off * (p->ld + 1); ba.ld = p->ld; ba.d = p->ndense; ba.Dinv = p->Dinv.p; ba.Ldiag = p->Ldiag.p; ba.xout = p->dxc.p; ba.sp = sb;
}

// the work list of the band Schur complement for the current rows-per-slice setting; its length is part of the launch grid
// work list of p's band Schur complement for `rows` landmark rows per slice, into buffers of the caller's (the problem's own list, or a
// batch's: a batch sums over wider slices and must not touch its members)
// `defer`: do not wait for the item count — an event is recorded behind its copy and await_band_work() collects it right before the first
// launch that needs it (the Schur complement's), by which time the linearisation launches enqueued in between have long kept the device busy
int build_band_work(lvf_problem* p, int rows_in, DevBuf<int4>& work, int* n_work, bool defer) {
  hipStream_t q = p->ctx->stream;
  const int rows = band_rows_clamped(rows_in);
  const int n_slices = (p->n_lm + rows - 1) / rows;
  const int nt = p->ldE / 16, groups_max = (nt * (nt + 1) / 2 + kBandTilesPerGroup - 1) / kBandTilesPerGroup;
  LVF_TRY(work.ensure((size_t)n_slices * groups_max)); LVF_TRY(p->n_band_work_dev.ensure(1)); LVF_TRY(p->h_n_band_work.reserve(1));
  LVF_HIP(hipMemsetAsync(p->n_band_work_dev.p, 0, sizeof(int), q));
  hipLaunchKernelGGL(k_band_work, dim3(n_slices), dim3(64), 0, q, rows, p->dp, p->lm_nactive.p, p->lm_order.p, p->lm_kmin.p, p->lm_kmax.p, work.p, p->n_band_work_dev.p);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(p->h_n_band_work.p, p->n_band_work_dev.p, sizeof(int), hipMemcpyDeviceToHost, q));
  if (defer) {
    if (!p->ev_band) LVF_HIP(hipEventCreateWithFlags(&p->ev_band, hipEventDisableTiming));
    LVF_HIP(hipEventRecord(p->ev_band, q));
    p->band_pending = true;
    *n_work = 0;
    return LVF_OK;
  }
  LVF_HIP(hipStreamSynchronize(q));
  *n_work = p->h_n_band_work[0];
  return LVF_OK;
}
static int ensure_band_work(lvf_problem* p) {
  if (!p->band_ready || p->n_lm == 0 || p->band_rows_built == p->band_rows) return LVF_OK;
  LVF_TRY(build_band_work(p, p->band_rows, p->band_work, &p->n_band_work, /*defer=*/true));
  p->band_rows_built = p->band_rows;
  return LVF_OK;
}

// the band Schur complement's dynamic LDS, and whether it shares its launch with sparse levels (k_schur_sp0)
static size_t schur_lds_bytes(const lvf_problem* p) { return p->n_lm ? ((size_t)kSchurRows * (p->ldE + 16) + kSchurRows) * sizeof(double) + kBandRowsMax * sizeof(int) : 0; }
static bool schur_merged(const lvf_problem* p) { return p->n_lm && p->band_ready && schur_lds_bytes(p) <= 64 * 1024 && p->sp_levels.n > 0 && (size_t)p->sp_shmem[0] <= 64 * 1024; }
// the merged back substitution + step tail (k_backsolve_tail) hands the pose increments over inside a launch: allowed where in-launch
// hand-overs are allowed at all (a problem whose hand-over timed out keeps its launches apart: lvf_problem::no_chain); its flag lives in the
// arrival-counter block, which is then cleared with the accumulators whether or not sparse levels are chained
static bool back_tail_wanted(const lvf_problem* p) {
  return solver_env().back_tail_merge && solver_env().chain_levels > 0 && !p->no_chain && p->n_lm > 0;
}
// the candidate state x + dx as the kernels read it
static StateP candidate_ptrs(const lvf_problem* p) { return StateP{p->poses2.p, p->vel2.p, p->ba2.p, p->bg2.p, p->invd2.p, p->st->w_visual.p}; }

// ---- the stages of build_chain, in the order it calls them: each fills its part of the chain from the problem's current buffers and from
// what the stages before it left in the chain
// what a linearisation accumulates into: the explicit clear (zero) and the clear at the end of an iteration (zero_end)
static int chain_zero_lists(lvf_problem* p, Chain& c) {
  const bool bt_wanted = back_tail_wanted(p);
  int k = 0;
  const bool tri_on = solver_env().zero_tri;
  bool overflow = false;
  auto add = [&](double* ptr, size_t n, int tri = 0) {
    if (!(ptr && n)) return;
    if (k >= kZeroListMax) { overflow = true; return; }      // (the struct travels by value: never write past its arrays)
    c.zero.p[k] = ptr; c.zero.n[k] = n; c.zero.tri[k] = (tri_on && tri % 2 == 0) ? tri : 0; ++k;
  };
  add(p->B.p, (size_t)p->dpad * p->dpad, p->dpad); add(p->gc.p, p->dpad);
  if (p->n_lm) { if (!p->compact) add(p->E.p, (size_t)p->n_lm * p->ldE); add(p->C.p, p->n_lm); add(p->gr.p, p->n_lm); }
  if (c.early) add(p->S.p, (size_t)p->ld * p->ld, p->ld);      // early sparse levels add into S before k_prepare does
  if (c.early || bt_wanted) add(p->sp_sync.p, kSpMaxLevels);     // the arrival counters of chained levels / the pose hand-over flag
  c.zero_end = c.zero; c.zero_end.count = k;         // cleared at the END of an iteration, beside the cost pass (the scalars: by the decision itself)
  add(p->scal.p, SC_N);
  c.zero.count = k;
  LVF_REQUIRE(!overflow, "build_chain: more than %d accumulator arrays (raise kZeroListMax)", kZeroListMax);
  return LVF_OK;
}
// the linearisation launch and, in compact mode, the reduction of its TwoFrame slabs
static void chain_linearize_args(lvf_problem* p, Chain& c) {
  const int* done = &p->ctl.p->done;
  const StateP s = state_ptrs(p->st), s2 = candidate_ptrs(p);
  double* cost = p->scal.p + SC_COST;
  if (c.has_imu) {
    fill_imu_args(p->imu, s.poses, s.vel, s.ba, s.bg, nullptr, nullptr, done, &c.imu_lin);
    fill_imu_args(p->imu, s2.poses, s2.vel, s2.ba, s2.bg, p->scal.p + SC_COST_NEW, nullptr, done, &c.imu_cost);
  }
  if (c.fast) {
    LinVisual& a = c.lin.v;
    a = LinVisual{};
    a.n_tfw = (int)p->tf_work.n; a.work = p->tf_work.p; a.tf_fo = p->tf_fo(); a.tf_ob = p->tf_ob();
    a.tf_lm = p->tf_lm(); a.tf_k1 = p->tf_k1(); a.tf_left = p->tf->cam_a; a.tf_right = p->tf->cam_b; a.unique_lk2 = p->tf_unique_lk2 ? 1 : 0;
    if (p->tc && p->tc->n) {
      a.n_tc = p->tc->n; a.tc_lo = (const double2*)p->tc->ob_a.p; a.tc_ro = (const double2*)p->tc->ob_b.p; a.tc_lm = p->tc->idx_a.p; a.tc_kf = p->tc->idx_b.p;
      a.tc_w = p->tc->wblk.n ? p->tc->wblk.p : nullptr; a.tc_left = p->tc->cam_a; a.tc_right = p->tc->cam_b;
    }
    if (p->po && p->po->n) {
      a.n_po = p->po->n; a.po_ob = (const double2*)p->po->ob_a.p; a.po_kf = p->po->idx_a.p; a.po_pwi = p->po->idx_b.p; a.po_pw = p->po->table.p; a.po_cam = p->po->cam_a;
    }
    a.g_tc = grid(a.n_tc); a.g_po = grid(a.n_po);
    if (c.has_imu) {
      a.n_imu = p->imu->n; a.imu_res = p->imu->res.p; a.imu_i = p->imu->idx_a.p; a.imu_j = p->imu->idx_b.p;
      for (int k = 0; k < 8; ++k) a.imu_J.j[k] = p->imu->jac[k].p;
      a.imu = ImuEvalArgs{p->imu->n, p->imu->pre.p, p->imu->sqrt_info.p, p->imu->idx_a.p, p->imu->idx_b.p};
    }
    const int staged_on = solver_env().staged ? 1 : 0;
    a.cp = TfCompact{0, nullptr, nullptr, nullptr, nullptr, staged_on};
    if (p->compact) {
      a.cp = TfCompact{1, p->tf_slot.p, p->slotB.p, p->slabP.p, p->slabQ.p, staged_on};
      TfReduceArgs& r = c.red;
      r.n_kf = p->n_kf; r.n_wg = a.n_tfw; r.run_first = p->run_first.p; r.slabP = p->slabP.p; r.slabQ = p->slabQ.p; r.B = p->B.p; r.ld = p->dpad; r.gc = p->gc.p;
      r.nblocks = p->n_kf * ((a.n_tfw + 63) / 64) + grid(p->n_kf * (p->n_kf - 1) / 2 * 36); r.done = done;
      r.own_blocks = r.nblocks; r.ride = SpArgs{}; r.ride.nblocks = 0;
    }
    c.lin.n_kf = p->n_kf; c.lin.s = s; c.lin.huber = 0.0; c.lin.pose_const = p->pose_const.p; c.lin.B = p->B.p; c.lin.ld = p->dpad; c.lin.gc = p->gc.p; c.lin.E = p->E.p;
    c.lin.ldE = p->ldE; c.lin.C = p->C.p; c.lin.gr = p->gr.p; c.lin.cost = cost; c.lin.done = done; c.lin.dbg = nullptr;
    c.lin.scal_reset = c.early ? p->scal.p : nullptr;
    c.lin.nblocks = a.n_tfw + a.g_tc + a.g_po + (a.imu.pre ? a.n_imu : (a.n_imu + 3) / 4);
    c.lin_lds = std::max((size_t)(sizeof(PoseD) / 8 + kAccSlots) * p->n_kf + 32 + 4 * (size_t)kStageWave, (size_t)std::max(kImuWaveLds, 1864 + 64)) * sizeof(double);
  }
}
// damped system: the classic k_prepare and its early form
static void chain_prepare_args(lvf_problem* p, Chain& c) {
  LmCtl* ctl = p->ctl.p;
  const int* done = &ctl->done;
  const double* radius = &ctl->radius;
  const JacobiDev jac{p->jh0.p, &ctl->jfrozen};
  PrepArgs& a = c.prep;
  a.ld = p->ld; a.dpad = p->dpad; a.iperm = p->iperm.p; a.B = p->B.p; a.gc = p->gc.p; a.radius = radius; a.S = p->S.p; a.jac = jac; a.jl0 = p->d;
  // (the lower triangle, folded: prepare_body)
  a.nS_blocks = (unsigned)(((size_t)((p->ld + 1) / 2) * (p->ld + 1) + kT - 1) / kT); a.n_lm = p->n_lm; a.dp = p->dp; a.ldE = p->ldE; a.C = p->C.p; a.gr = p->gr.p; a.Cd = p->Cd.p; a.E = p->E.p;
  a.eoff = p->lm_eoff.p; a.kmin = p->lm_kmin.p; a.kmax = p->lm_kmax.p; a.slotB = p->compact ? p->slotB.p : nullptr; a.Ct = p->Ct.p; a.grt = p->grt.p;
  a.scal = p->scal.p; a.nblocks = (int)a.nS_blocks + (p->n_lm ? grid(p->compact ? 8 * p->n_lm : p->n_lm) : 0); a.done = done;
  a.early = 0; a.off = p->off; a.own_blocks = a.nblocks; a.ride = SpArgs{}; a.ride.nblocks = 0;
  PrepArgs& e = c.prep_early;
  e = a;
  const int nn = p->ld - p->off;
  e.early = 1; e.scal = nullptr;                      // (the scalars are reset by the linearisation launch: LinArgs::scal_reset)
  e.nS_blocks = (unsigned)(((size_t)((nn + 1) / 2) * (nn + 1) + kT - 1) / kT);
  e.nblocks = e.own_blocks = (int)e.nS_blocks + (p->n_lm ? grid(p->compact ? 8 * p->n_lm : p->n_lm) : 0);
}
// the sparse levels, and how they are dealt to the launches of the iteration
static void chain_sparse_levels(lvf_problem* p, Chain& c) {
  LmCtl* ctl = p->ctl.p;
  const int* done = &ctl->done;
  const double* radius = &ctl->radius;
  const JacobiDev jac{p->jh0.p, &ctl->jfrozen};
  int* fail = reinterpret_cast<int*>(p->scal.p + SC_FAIL);
  c.n_levels = p->sp_levels.n;
  for (int lv = 0; lv < p->sp_levels.n; ++lv) {
    SpArgs& a = c.sp[lv];
    a.nodes = p->sp_nodes.p; a.first = p->sp_levels.first[lv]; a.tiles = p->sp_tiles[lv]; a.rows = p->sp_rows.p; a.S = p->S.p; a.ld = p->ld; a.W = p->sp_W.p;
    a.wstride = p->sp_wstride; a.Lout = p->sp_L.p; a.fail = fail; a.nblocks = p->sp_levels.count[lv] * p->sp_tiles[lv]; a.done = done;
    // (0.5 ms at 100 MHz before a chained level gives up on the level below — a hand-over normally takes microseconds, and a retry costs one iteration of 0.2 ms: round 4 waited 2 ms, ten iterations of latency on a shared GPU; LVF_CHAIN_TIMEOUT_US overrides; LVF_CHAIN_FENCE=0: relaxed hand-over, A/B only)
    const unsigned chain_timeout = solver_env().chain_timeout_ticks;
    const int chain_fenced = solver_env().chain_fence != 0 ? 1 : 0;
    a.src = c.early ? SpSrc{p->B.p, p->dpad, p->dp, p->gc.p, radius, p->sp_rows_nat.p, nullptr, 0, nullptr, chain_fenced, chain_timeout, p->off, solver_env().chain_rmw_read ? 1 : 0, nullptr, lv == 0 ? 1 : 0}
                    : SpSrc{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, chain_fenced, chain_timeout, p->off, 0, nullptr, 0};
    a.src.jac = jac;
    c.sp_lds[lv] = p->sp_shmem[lv];
  }
  c.merged_level0 = false;
  if (p->n_lm) {
    const int nt = p->ldE / 16, ntile = nt * (nt + 1) / 2;
    const size_t shb = schur_lds_bytes(p);
    // early form: the levels are dealt to the launches that exist anyway, in order
    int next_level = 0;
    // Where the levels go (measured, MI355X): the Schur launch hides three (one riding, two chained behind it); a level riding in
    // k_tf_reduce's launch costs ~0 us, in k_prepare's ~2 us, a launch of its own 7.6 us.  So the LAST three levels go to the Schur launch
    // and only what is left over rides in the two launches ahead (16 / 20 keyframes, three levels: 0.111 / 0.125 -> 0.098 / 0.118 ms
    // with the chain alone, 0.103 / 0.123 with riders in front of it).  LVF_RIDE_TF / LVF_RIDE_PREP = 0 | 1 override, LVF_CHAIN_LEVELS = 0..2.
    const int ride_tf_env = solver_env().ride_tf, ride_prep_env = solver_env().ride_prep;
    const int chain_n = p->no_chain ? 0 : solver_env().chain_levels;      // (a hand-over that timed out once: every level in a launch of its own from then on)
    const int excess = std::max(0, c.n_levels - (1 + chain_n));
    const bool ride_tf = ride_tf_env >= 0 ? ride_tf_env != 0 : (p->compact && excess >= 1);
    const bool ride_prep = ride_prep_env >= 0 ? ride_prep_env != 0 : (excess >= 2 || (excess >= 1 && !(ride_tf && p->compact)));
    if (c.early) {
      if (!ride_tf) {}
      else if (p->compact && next_level < c.n_levels) { c.red.ride = c.sp[next_level]; c.red.nblocks = c.red.own_blocks + c.red.ride.nblocks; c.red_lds = (size_t)c.sp_lds[next_level]; ++next_level; }
      if (ride_prep && next_level < c.n_levels) { PrepArgs& e = c.prep_early; e.ride = c.sp[next_level]; e.nblocks = e.own_blocks + e.ride.nblocks; c.prep_lds = (size_t)c.sp_lds[next_level]; ++next_level; }
    }
    if (schur_merged(p)) {
      SchurSp0Args& a = c.ssp0;
      a.rows = band_rows_clamped(p->band_rows);
      a.n_slices = (p->n_lm + a.rows - 1) / a.rows; a.n_groups = (ntile + kBandTilesPerGroup - 1) / kBandTilesPerGroup;
      a.dp = p->dp; a.ldE = p->ldE; a.E = p->E.p; a.Cd = p->Cd.p; a.order = p->lm_order.p;
      a.dbg = nullptr; a.n_active = p->lm_nactive.p; a.kmin = p->lm_kmin.p; a.kmax = p->lm_kmax.p;
      a.d_local = p->dp; a.ldS = p->ld; a.S_pose = p->S.p + (size_t)p->off_pose * (p->ld + 1);
      const int ride = c.early ? next_level : 0;       // classic: level 0 rides here
      a.sp = SpArgs{}; a.sp.nblocks = 0; a.sp_b = a.sp; a.sp_c = a.sp;
      c.ssp0_lds = shb;
      next_level = ride;
      if (ride < c.n_levels) { a.sp = c.sp[ride]; c.ssp0_lds = std::max(c.ssp0_lds, (size_t)p->sp_shmem[ride]); next_level = ride + 1; }
      // the Schur complement lasts ~20 us at this size, a level ~5: the next two levels wait for their predecessor INSIDE the launch
      if (c.early && chain_n > 0) {
        int* cnt = reinterpret_cast<int*>(p->sp_sync.p);
        SpArgs* slot[2] = {&a.sp_b, &a.sp_c};
        SpArgs* prev = &a.sp;
        for (int k = 0; k < std::min(2, chain_n) && next_level < c.n_levels && (size_t)p->sp_shmem[next_level] <= 64 * 1024; ++k) {
          *slot[k] = c.sp[next_level];
          prev->src.done_counter = cnt + 2 * (next_level - 1);
          slot[k]->src.wait_counter = cnt + 2 * (next_level - 1); slot[k]->src.wait_target = prev->nblocks;
          if (p->force_handover_timeouts > 0 && k == 0) { slot[k]->src.wait_target = prev->nblocks + 1; slot[k]->src.timeout_ticks = 2000u; }      // test hook: a producer that never arrives (20 us)
          c.ssp0_lds = std::max(c.ssp0_lds, (size_t)p->sp_shmem[next_level]);
          prev = slot[k];
          ++next_level;
        }
      }
      a.work = p->band_work.p; a.n_work = p->n_band_work;
      a.nblocks = a.n_work + a.sp.nblocks + a.sp_b.nblocks + a.sp_c.nblocks; a.done = done;
      c.merged_level0 = true;
      c.first_own_level = next_level;
    }
  }
}
// Cholesky, back substitution and step tail; the merged back substitution + tail with its product and block forms
static int chain_solve_args(lvf_problem* p, Chain& c) {
  LmCtl* ctl = p->ctl.p;
  const int* done = &ctl->done;
  const double* radius = &ctl->radius;
  const JacobiDev jac{p->jh0.p, &ctl->jfrozen};
  const StateP s = state_ptrs(p->st);
  int* fail = reinterpret_cast<int*>(p->scal.p + SC_FAIL);
  const bool bt_wanted = back_tail_wanted(p);
  c.chol.Sd = p->S.p + (size_t)p->off * (p->ld + 1); c.chol.ld = p->ld; c.chol.nb = p->nb; c.chol.fail = fail; c.chol.Dinv = p->Dinv.p; c.chol.Ldiag = p->Ldiag.p; c.chol.done = done;
  c.chol.last_cols = p->ndense + 1 - kNB * (p->nb - 1);       // (the right-hand-side row is the last real one)
  fill_back_args(p, c.back, &c.back_lds);
  c.back.done = done;
  {
    TailArgs& a = c.tail;
    // (640 workgroups take the 10 000 landmarks of the BASELINE window in one pass of 16 per workgroup; measured 1-2 % of an iteration over a cap of 256)
    a.g_lm = p->n_lm ? std::min(solver_env().tail_wgs, (p->n_lm + kT / 16 - 1) / (kT / 16)) : 0;
    a.n_lm = p->n_lm; a.dp = p->dp; a.ldE = p->ldE; a.E = p->E.p; a.C = p->compact ? p->Ct.p : p->C.p; a.Cd = p->Cd.p;
    a.gr = p->compact ? p->grt.p : p->gr.p; a.dxc = p->dxc.p; a.dxl = p->dxl.p; a.scal = p->scal.p;
    a.kmin = p->band_ready ? p->lm_kmin.p : nullptr; a.kmax = p->lm_kmax.p; a.n_kf = p->n_kf; a.s = s; a.poses2 = p->poses2.p; a.vel2 = p->vel2.p; a.ba2 = p->ba2.p;
    a.bg2 = p->bg2.p; a.invd2 = p->invd2.p; a.d = p->d; a.ld = p->dpad; a.B = p->B.p; a.gc = p->gc.p; a.radius = radius; a.nblocks = a.g_lm + grid(p->d); a.done = done; a.pose_const = p->pose_const.p; a.jac = jac;
    c.tail_lds = (size_t)p->ldE * sizeof(double);
  }
  {
    const unsigned bt_timeout = solver_env().chain_timeout_ticks;
    const int bt_fenced = solver_env().chain_fence;
    static const bool bt_big_lds = hipFuncSetAttribute(reinterpret_cast<const void*>(k_backsolve_tail), hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024) == hipSuccess;
    c.back_tail_merged = bt_wanted && c.tail.g_lm > 0;
    if (c.back_tail_merged) {
      BackTailArgs& m = c.bt;
      m.back = c.back; m.tail = c.tail;
      m.back.pose_ready = reinterpret_cast<int*>(p->sp_sync.p) + 2 * kSpMaxLevels - 2;      // (the last int pair of the arrival-counter block: the levels use pairs 0 .. n_levels - 2)
      m.back.n_pose = p->dp;
      // (one round of workgroups: the launch's register and LDS footprint is the back substitution's, so about one workgroup fits a CU, and a
      // landmark workgroup that has to wait for a CU starts after the others are done)
      m.g_lm = std::min(solver_env().back_tail_wgs, (p->n_lm + kBT / 16 - 1) / (kBT / 16));
      m.fenced = bt_fenced == 2; m.back.pose_fenced = bt_fenced == 2; m.timeout_ticks = bt_timeout; m.fail = fail;
      m.early = solver_env().back_early ? 1 : 0;
      if (p->force_handover_timeouts > 1) { m.back.pose_ready = reinterpret_cast<int*>(p->sp_sync.p) + 2 * kSpMaxLevels - 4; m.timeout_ticks = 2000u; }      // test hook (n >= 2): a flag nobody raises
      c.bt_lds = std::max(c.back_lds, c.tail_lds);
      if (c.bt_lds > 64 * 1024 && !bt_big_lds) c.back_tail_merged = false;
    }
    // The product form: on where the levels can be dealt one to a block-step launch (n_levels <= nb; level n_levels - 1 - kb rides in launch
    // kb) and the merged launch is in use.  Its G workgroups must fit the chip in ONE round beside workgroup 0, the pose workgroup and the
    // landmark workgroups (about one workgroup of this launch fits a compute unit; a workgroup that has to wait for one starts after the
    // others are done), each owns whole keyframes, one thread per unknown.
    c.back_product = false; c.gride = GRide{}; c.gride.n = 0;
    static const int n_cu = [] { int dev = 0, n = 0; return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256; }();
    if (solver_env().back_product && c.back_tail_merged && c.n_levels >= 1 && c.n_levels <= p->nb && p->ldG > 0) {
      const int room = n_cu - 2 - c.bt.g_lm;
      const int kpw = room >= 1 ? (p->n_kf + std::min(room, p->n_kf) - 1) / std::min(room, p->n_kf) : 0;
      const int n_nodes = p->sp_levels.first[c.n_levels - 1] + p->sp_levels.count[c.n_levels - 1];
      if (kpw >= 1 && 9 * kpw <= kBT) {
        LVF_TRY(p->sp_G.ensure((size_t)9 * n_nodes * p->ldG));
        BackTailArgs& m = c.bt;
        m.kpw = kpw; m.g_prod = (p->n_kf + kpw - 1) / kpw; m.ldG = p->ldG; m.G = p->sp_G.p; m.iperm = p->iperm.p;
        c.bt_lds = std::max(c.bt_lds, (size_t)(p->ldG + 9 * kpw) * sizeof(double));
        c.gride = GRide{0, 0, p->sp_nodes.p, p->sp_rows.p, p->sp_W.p, p->sp_wstride, p->sp_L.p, p->sp_gmap.p, p->sp_G.p, p->ldG, p->off, done};
        c.back_product = true;
      }
    }
    // The block form: on for every single-window chain of two or more blocks (the riders go with k_chol_step / k_chol_step_pp whether or not
    // the G product is on) whose link products fit the registers of the body that will run — five blocks for the dense-corner-only body of the
    // product form, three beside the sparse levels' items.  Off where the augmented row sits alone in the last factor block (d a multiple of
    // 64: the first solved block would take its right-hand side from a panel, not from Ldiag — a corner the plan's cost steers away from, it
    // pays a block step for one row) and in the chain-free re-run after a hand-over time-out; those read S and Dinv as before.
    c.back_blocks = false; c.tride = TRide{0, nullptr};
    if (solver_env().back_blocks && !p->no_chain && p->nb >= 2 && p->ndense % kNB != 0 && p->nb - 1 <= (c.back_product ? kBackTJ : kBackTJLevels)) {
      LVF_TRY(p->sp_T.ensure((size_t)p->nb * p->nb * kNB * kNB));
      c.tride = TRide{0, p->sp_T.p};
      c.back_blocks = true;
    }
    // The merged last launch: block step nb - 1 and k_backsolve_tail as one (k_chol_backsolve_tail).  On where the back substitution is the
    // dense-corner-only body on stored products (product and block forms), with the sub-block sweep; the batched chains, the chain-free re-run
    // after a hand-over time-out and every other form keep the two launches.  The override tap changes nothing from the block steps on, so
    // the form is the same with and without it.
    c.chol_back_merged = false;
    if (solver_env().chol_back_merge && c.back_tail_merged && c.back_product && c.back_blocks && p->nb >= 2 && solver_env().chol_subblock && !solver_env().back_tail_wgs_set) {
      constexpr size_t kCbDynMax = 88 * 1024;       // beside the 66 560 B of panel buffers and the small static arrays of the bodies: 160 KB per workgroup
      static const bool cb_lds_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_backsolve_tail), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCbDynMax) == hipSuccess;
      LVF_TRY(p->x_last.ensure(kNB));
      int* sync = reinterpret_cast<int*>(p->sp_sync.p);
      CholBackArgs& m = c.cb;
      m.chol = c.chol; m.tr = TRide{1, p->sp_T.p};
      m.g = c.gride;                                // the G riders of launch nb - 1: level n_levels - nb (none when the levels ran out earlier)
      const int glv = c.n_levels - p->nb;
      if (glv >= 0) { m.g.first = p->sp_levels.first[glv]; m.g.n = p->sp_levels.count[glv]; } else m.g.n = 0;
      // the flag shares the last int pair of the arrival-counter block with pose_ready (the levels use the first int of pairs 0 .. n_levels - 2),
      // and is cleared with it at the end of every iteration
      m.xl = XLast{p->x_last.p, sync + 2 * kSpMaxLevels - 1};
      m.bt = c.bt;
      m.bt.back.T = p->sp_T.p; m.bt.back.x_ready = sync + 2 * kSpMaxLevels - 1; m.bt.back.x_last = p->x_last.p; m.bt.back.x_timeout = bt_timeout; m.bt.back.x_fail = fail;
      if (p->force_handover_timeouts > 1) { m.bt.back.x_ready = sync + 2 * kSpMaxLevels - 3; m.bt.back.x_timeout = 2000u; }      // test hook (n >= 2): a flag nobody raises
      // one round: the two column workgroups, the back substitution, the riders, the pose workgroup and the G products leave the landmark
      // pass the rest of the chip (50 keyframes: 256 - 54 = 202, and 157 workgroups hold 10 000 landmarks in their two early passes).  Where the
      // landmarks need more, nothing depends on the fit: the riders wait for nothing and free their compute units within microseconds.
      m.bt.g_lm = std::max(1, std::min(c.bt.g_lm, n_cu - (3 + m.g.n + 1 + m.bt.g_prod)));
      // the G workgroups multiply rows that riders of this launch form: an arrival counter (a free odd int of the block: the levels count in the even ones)
      m.g_arrive = sync + 2 * kSpMaxLevels - 5; m.bt.g_ready = sync + 2 * kSpMaxLevels - 5; m.bt.g_target = m.g.n;
      // dynamic LDS: the dense-corner-only body (xs | x | partial | rhs), the landmark and pose workgroups' increments, a G workgroup's [x_dense | rows]
      const size_t nx = (size_t)((p->ndense + kNB - 1) / kNB) * kNB;
      c.cb_lds = std::max(std::max(((size_t)p->off + nx + (size_t)(kBParts + 1) * kNB) * sizeof(double), c.tail_lds),
                          std::max((size_t)p->dp, (size_t)(p->ldG + 9 * m.bt.kpw)) * sizeof(double));
      c.chol_back_merged = cb_lds_ok && c.cb_lds <= kCbDynMax;
    }
    const bool chain_info = solver_env().chain_info;
    if (chain_info) std::fprintf(stderr, "chain: n_kf %d n_lm %d fast %d has_imu %d early %d compact %d levels %d no_chain %d merged_level0 %d back_tail_merged %d (g_lm %d, lds %zu) back_product %d (nb %d, %d G workgroups of %d keyframes)\n", p->n_kf, p->n_lm, (int)c.fast, (int)c.has_imu,
                                 (int)c.early, (int)p->compact, c.n_levels, (int)p->no_chain, (int)c.merged_level0, (int)c.back_tail_merged, c.bt.g_lm, c.bt_lds,
                                 (int)c.back_product, p->nb, c.bt.g_prod, c.bt.kpw);
    if (chain_info) std::fprintf(stderr, "chain: back_blocks %d chol_back_merged %d (g_lm %d, %d G riders)\n", (int)c.back_blocks, (int)c.chol_back_merged, c.chol_back_merged ? c.cb.bt.g_lm : 0,
                                 c.chol_back_merged ? c.cb.g.n : 0);
  }
  return LVF_OK;
}
// the candidate cost pass and the decision that closes an iteration
static int chain_cost_decide_args(lvf_problem* p, Chain& c) {
  LmCtl* ctl = p->ctl.p;
  const int* done = &ctl->done;
  const StateP s2 = candidate_ptrs(p);
  fill_cost_visual(p, c.cost.a);
  c.cost.n_kf = p->n_kf; c.cost.s = s2; c.cost.huber = 0.0; c.cost.cost = p->scal.p + SC_COST_NEW; c.cost.done = done;
  c.cost.nblocks = c.cost.a.g_tc + c.cost.a.g_tf + grid(c.cost.a.n_po);
  {
    // two tiles of kT blocks per workgroup: half as many workgroups to dispatch ahead of the decision (measured -1 % of an iteration; three: same)
    const int cost_tiles = solver_env().cost_tiles;
    if (cost_tiles > 1) {
      CostArgs& k = c.cost;
      const int per = kT * cost_tiles;
      k.tiles = cost_tiles;
      k.a.g_tc = (k.a.n_tc + per - 1) / per; k.a.g_tf = (k.a.n_tf + per - 1) / per;
      k.nblocks = k.a.g_tc + k.a.g_tf + (k.a.n_po + per - 1) / per;
    }
  }
  c.cost.g_imu = 0; c.cost.imu = ImuEvalArgs{};
  c.imu_in_cost = c.fast && c.has_imu && c.cost.nblocks > 0;         // the IMU cost rides in the merged cost + decision launch
  if (c.imu_in_cost) { c.cost.imu = ImuEvalArgs{p->imu->n, p->imu->pre.p, p->imu->sqrt_info.p, p->imu->idx_a.p, p->imu->idx_b.p}; c.cost.g_imu = p->imu->n; c.cost.nblocks += p->imu->n; }
  c.cost.zero = c.zero_end; c.cost.zero_wgs = c.fast ? kEndZeroWgs : 0;
  {
    DecideArgs& a = c.dec;
    a.scal = p->scal.p; a.ctl = ctl; a.rec = p->rec; a.ticket = reinterpret_cast<int*>(p->scal.p + SC_TICKET); a.n_kf = p->n_kf; a.n_lm = p->n_lm;
    a.poses = p->st->poses.p; a.vel = p->st->vel.p; a.ba = p->st->ba.p; a.bg = p->st->bg.p; a.invd = p->st->inv_depth.p;
    a.poses2 = p->poses2.p; a.vel2 = p->vel2.p; a.ba2 = p->ba2.p; a.bg2 = p->bg2.p; a.invd2 = p->invd2.p;
    a.hist = nullptr;
    if (solver_env().lm_history) { LVF_TRY(p->dbg_hist.ensure(8 * 64)); a.hist = p->dbg_hist.p; }
  }
  return LVF_OK;
}
  // the fused chain: the compact single-window chain with every reader of the accumulators selecting its set on device (problems with
  // pose priors or lidar planes keep today's chain: those terms have no candidate linearisation)
static void chain_fused_args(lvf_problem* p, Chain& c) {
  const int* done = &p->ctl.p->done;
  const StateP s2 = candidate_ptrs(p);
  c.fused_ok = solver_env().fused_lin && c.fast && p->compact && !c.has_prior && !c.has_lidar && !c.has_dprior && c.merged_level0 && p->n_lm > 0 && c.lin.nblocks > 0 && c.cost.nblocks > 0 &&
               (!c.has_imu || (c.imu_in_cost && c.lin.v.imu.pre));
  p->acc1_ready = false;            // the second set is allocated and cleared by the first fused solve (ensure_acc1)
  if (c.fused_ok) {
    // what the candidate pass clears for the next iteration: zero_end less the accumulator sets (S, the arrival counters)
    ZeroList fz{};
    for (int k = 0; k < c.zero_end.count; ++k) {
      double* q0 = c.zero_end.p[k];
      if (q0 == p->B.p || q0 == p->gc.p || q0 == p->C.p || q0 == p->gr.p) continue;
      fz.p[fz.count] = q0; fz.n[fz.count] = c.zero_end.n[k]; fz.tri[fz.count] = c.zero_end.tri[k]; ++fz.count;
    }
    FusedArgs& f = c.fused;
    f.lin = c.lin; f.lin.s = s2; f.lin.cost = nullptr; f.lin.scal_reset = nullptr; f.lin.dbg = nullptr;
    f.dec = c.dec; f.dec.fused = 1;
    f.cost_new = p->scal.p + SC_COST_NEW; f.nblocks = c.lin.nblocks; f.done = done; f.zero = fz; f.zero_wgs = kEndZeroWgs;
  }
}

// (re)builds the argument blocks of an iteration from the problem's CURRENT buffers (call after problem_configure / set_pose_priors)
int build_chain(lvf_problem* p) {
  if (!p->chain) p->chain = new Chain();
  Chain& c = *p->chain;
  c = Chain();
  p->accum_clean = false;           // buffers may have been re-allocated
  LVF_TRY(ensure_band_work(p));
  LVF_TRY(p->ctl.ensure(1));
  if (!p->rec) {
    void* h = HostPinPool::get().take(Pool::bucket(sizeof(LmCtl)));       // (pinned blocks are recycled: lvf_internal.hpp)
    if (!h) LVF_HIP(hipHostMalloc(&h, Pool::bucket(sizeof(LmCtl)), hipHostMallocDefault));
    p->rec = static_cast<LmCtl*>(h);
    std::memset(p->rec, 0, sizeof(LmCtl));
  }
  LVF_TRY(p->jh0.ensure((size_t)p->d + p->n_lm + 1));
  c.fast = p->tf && p->tf->n && p->tf_work.n && p->n_kf <= kMaxStagedKf;
  c.has_imu = p->imu && p->imu->n;
  c.has_prior = p->prior && p->prior->n;
  c.has_lidar = p->lidar && p->lidar->n;
  c.has_dprior = p->dprior != nullptr;
  {
    // LVF_EARLY_LEVELS=0: the classic order (A/B measurements); LVF_POISON_S fills S with NaN before the assembly, which only the classic form survives
    bool fits = true;
    for (int lv = 0; lv < std::min(3, p->sp_levels.n); ++lv) fits = fits && (size_t)p->sp_shmem[lv] <= 64 * 1024;
    c.early = solver_env().early_levels && c.fast && c.has_imu && schur_merged(p) && fits && p->sp_levels.n >= 2;      // (one level: it already hides in the Schur launch)
  }
  LVF_TRY(chain_zero_lists(p, c));
  chain_linearize_args(p, c);
  chain_prepare_args(p, c);
  chain_sparse_levels(p, c);
  LVF_TRY(chain_solve_args(p, c));
  LVF_TRY(chain_cost_decide_args(p, c));
  chain_fused_args(p, c);
  c.batchable = c.fast && p->compact && c.has_imu && !c.has_prior && !c.has_lidar && !c.has_dprior && c.merged_level0 && c.lin.nblocks > 0 && c.cost.nblocks > 0;
  { const StateP sp = state_ptrs(p->st); std::memcpy(p->chain_state, &sp, sizeof(sp)); }
  p->chain_tcw = p->tc && p->tc->wblk.n ? p->tc->wblk.p : nullptr;
  p->chain_ready = true;
  return LVF_OK;
}
bool chain_stale(const lvf_problem* p) {
  if (!p->chain_ready || !p->chain) return true;
  const StateP s = state_ptrs(p->st);
  static_assert(sizeof(StateP) == sizeof(p->chain_state), "StateP is six pointers");
  if (std::memcmp(&s, p->chain_state, sizeof(StateP)) != 0) return true;      // the state's buffers were re-allocated (window grew)
  // lvf_two_camera_set_block_weights after the problem was created: the argument blocks hold the old weight pointer (or none)
  const double* w = p->tc && p->tc->wblk.n ? p->tc->wblk.p : nullptr;
  return w != p->chain_tcw;
}
// The second accumulator set, allocated and cleared on the first fused solve after a configure (a problem that is only ever solved in a batch,
// or one iteration at a time, never holds it).  E's and the slot records' zeros outside what a linearisation writes are set here, as for
// set 0 in problem_configure; B, gc, C and g_rho need nothing: the first k_tf_reduce of every fused solve clears the standby set, which is
// set 1 then (LmCtl::aset starts every solve at 0).
int ensure_acc1(lvf_problem* p) {
  Chain& c = *p->chain;
  if (!c.fused_ok || p->acc1_ready) return LVF_OK;
  hipStream_t q = p->ctx->stream;
  LVF_TRY(p->B1.ensure(p->B.n)); LVF_TRY(p->gc1.ensure(p->gc.n)); LVF_TRY(p->C1.ensure(p->C.n)); LVF_TRY(p->gr1.ensure(p->gr.n));
  LVF_TRY(p->E1.ensure(p->E.n)); LVF_TRY(p->slotB1.ensure(p->slotB.n));
  LVF_HIP(hipMemsetAsync(p->E1.p, 0, p->E1.n * 8, q));
  hipLaunchKernelGGL(k_tf_slots_zero, dim3(256), dim3(kT), 0, q, 0, 0, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr,
                     (int*)nullptr, p->n_slots.p, p->slotB1.p);
  LVF_HIP(hipGetLastError());
  c.acc = AccSel{&p->ctl.p->aset, p->B1.p, p->gc1.p, p->C1.p, p->gr1.p, p->E1.p, p->slotB1.p};
  // the standby lists: one set's B, gc, C, g_rho (as zero_end clears set 0's)
  c.stand0 = ZeroList{}; c.stand1 = ZeroList{};
  for (int k = 0; k < c.zero_end.count; ++k) {
    double* q0 = c.zero_end.p[k];
    double* q1 = q0 == p->B.p ? p->B1.p : q0 == p->gc.p ? p->gc1.p : q0 == p->C.p ? p->C1.p : q0 == p->gr.p ? p->gr1.p : nullptr;
    if (!q1) continue;
    c.stand0.p[c.stand0.count] = q0; c.stand0.n[c.stand0.count] = c.zero_end.n[k]; c.stand0.tri[c.stand0.count] = c.zero_end.tri[k]; ++c.stand0.count;
    c.stand1.p[c.stand1.count] = q1; c.stand1.n[c.stand1.count] = c.zero_end.n[k]; c.stand1.tri[c.stand1.count] = c.zero_end.tri[k]; ++c.stand1.count;
  }
  c.fused.lin.acc = c.acc;
  p->acc1_ready = true;
  return LVF_OK;
}

void stage_clock_free(StageClock* k) {
  if (!k) return;
  for (auto& r : k->ev) for (auto& e : r) (void)hipEventDestroy(e);
  if (k->kernel_events) { for (auto& r : k->kstart) for (auto& e : r) (void)hipEventDestroy(e); for (auto& r : k->kstop) for (auto& e : r) (void)hipEventDestroy(e); }
  delete k;
}
// a launch of the iteration's fast chain: plain, or — while lvf_problem_stage_times is recording — with its own start / stop events
#define LVF_CHAIN_LAUNCH(p_, stage_, kernel_, grid_, block_, lds_, q_, ...)                                                          \
  do {                                                                                                                              \
    StageClock* k__ = (p_)->clk;                                                                                                    \
    if (k__ && k__->on && k__->kernel_events && k__->nk < kClockLaunches) {                                                         \
      const int i__ = k__->nk++;                                                                                                    \
      k__->kstage[i__] = (stage_);                                                                                                  \
      hipExtLaunchKernelGGL(kernel_, grid_, block_, lds_, q_, k__->kstart[k__->rep][i__], k__->kstop[k__->rep][i__], 0, __VA_ARGS__); \
    } else hipLaunchKernelGGL(kernel_, grid_, block_, lds_, q_, __VA_ARGS__);                                                       \
  } while (0)
static inline void stage_mark(lvf_problem* p, int stage_done, int launches) {
  StageClock* k = p->clk;
  if (!k || !k->on) return;
  (void)hipEventRecord(k->ev[k->rep][stage_done + 1], p->ctx->stream);
  k->launches[stage_done] = launches;
}

// a sparse level of the fused chain reads B / gc of the active accumulator set (early form only: the classic form does not read them)
static inline void acc_patch(SpArgs& a, const AccSel* acc) {
  if (acc && a.src.B) { a.src.sel = acc->sel; a.src.B1 = (const double*)(double*)acc->B; a.src.gc1 = (const double*)(double*)acc->gc; }
}

// the linearisation at the current state: cost, B, gc, E, C, gr.  `gated`: skipped on device once the LM loop has finished
// `iteration`: the launches belong to a full LM iteration (enqueue_iteration) — only then do the early sparse levels ride along and are the
// per-step scalars reset here; a stand-alone linearisation (gradient / cost taps) leaves S and the control block alone
// `acc` (fused chain): every launch selects its accumulator set on device; `lin` == false: the active set already holds the linearisation
// (the last iteration's candidate pass), only k_tf_reduce runs
int enqueue_linearize(lvf_problem* p, double huber, bool gated, bool iteration, const AccSel* acc, bool lin) {
  hipStream_t q = p->ctx->stream;
  if (chain_stale(p)) LVF_TRY(build_chain(p));
  const Chain& c = *p->chain;
  const StateP s = state_ptrs(p->st);
  double* cost = p->scal.p + SC_COST;
  bool imu_done = false;
  // the accumulators are cleared at the END of every iteration (extra workgroups of the cost + decision launch); a launch of its own is
  // only needed when they are not known to be clean (first linearisation after a configure, stand-alone gradient / reduced-system taps)
  const bool clean = !lin || (c.fast && p->accum_clean);
  p->accum_clean = false;
  if (p->clk && p->clk->on) (void)hipEventRecord(p->clk->ev[p->clk->rep][0], q);
  if (!clean) LVF_CHAIN_LAUNCH(p, ST_IMU_LIN, k_zero_multi, dim3(512, c.zero.count), dim3(kT), 0, q, c.zero);
  if (c.fast) {
    imu_done = true;                           // the ImuError factors are evaluated inside the merged launch below
    stage_mark(p, ST_IMU_LIN, clean ? 0 : 1);
    LinArgs la = c.lin;
    la.huber = huber;
    if (!gated) la.done = nullptr;
    if (!iteration) la.scal_reset = nullptr;
    const bool lin_timing = solver_env().lin_timing;
    if (lin_timing) { LVF_TRY(p->dbg_lin.ensure((size_t)la.v.n_tfw * 24 + 8)); la.dbg = p->dbg_lin.p; }
    const size_t lds_pad = solver_env().lin_lds_pad;      // experiment: fewer workgroups per CU
    if (lin) LVF_CHAIN_LAUNCH(p, ST_LIN_VISUAL, k_lin_visual, dim3(la.nblocks), dim3(kT), c.lin_lds + lds_pad, q, la);      // (into set 0: a pass starts with LmCtl::aset = 0)
    stage_mark(p, ST_LIN_VISUAL, lin ? 1 : 0);
    if (p->compact) {
      TfReduceArgs ra = c.red;
      if (!gated) ra.done = nullptr;
      if (!iteration) { ra.nblocks = ra.own_blocks; ra.ride.nblocks = 0; }
      int zero_wgs = 0;
      if (acc) {
        ra.acc = *acc; acc_patch(ra.ride, acc);
        ra.pending = lin ? nullptr : &p->ctl.p->lin_pending;
        ra.stand0 = c.stand0; ra.stand1 = c.stand1; ra.zero_wgs = zero_wgs = kEndZeroWgs;
      }
      LVF_CHAIN_LAUNCH(p, ST_TF_REDUCE, k_tf_reduce, dim3(ra.nblocks + zero_wgs), dim3(kT), ra.ride.nblocks > 0 ? c.red_lds : 0, q, ra);
    }
    stage_mark(p, ST_TF_REDUCE, p->compact ? 1 : 0);
    if (lin_timing) {
      std::vector<unsigned long long> t((size_t)la.v.n_tfw * 8);
      LVF_HIP(hipStreamSynchronize(q));
      LVF_HIP(hipMemcpy(t.data(), p->dbg_lin.p, t.size() * 8, hipMemcpyDeviceToHost));
      double ph[5] = {0, 0, 0, 0, 0}; unsigned long long first = ~0ull, last = 0, last_start = 0;
      for (int w = 0; w < la.v.n_tfw; ++w) {
        for (int k = 0; k < 5; ++k) ph[k] += (double)(t[(size_t)w * 8 + k + 1] - t[(size_t)w * 8 + k]) * 0.01;
        first = std::min(first, t[(size_t)w * 8]); last = std::max(last, t[(size_t)w * 8 + 5]); last_start = std::max(last_start, t[(size_t)w * 8]);
      }
      {
        double mx[5] = {0, 0, 0, 0, 0}; int slow = 0; double slow_t = 0;
        for (int w = 0; w < la.v.n_tfw; ++w) {
          for (int k = 0; k < 5; ++k) mx[k] = std::max(mx[k], (double)(t[(size_t)w * 8 + k + 1] - t[(size_t)w * 8 + k]) * 0.01);
          const double tot = (double)(t[(size_t)w * 8 + 5] - t[(size_t)w * 8]) * 0.01;
          if (tot > slow_t) { slow_t = tot; slow = w; }
        }
        std::vector<TfWork> hw((size_t)la.v.n_tfw);
        LVF_HIP(hipMemcpy(hw.data(), la.v.work, hw.size() * sizeof(TfWork), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "lin_tf: per-phase MAX over the workgroups (us): %.2f | %.2f | %.2f | %.2f | %.2f ; slowest workgroup %d (k2 = %d, %d blocks): %.2f us =", mx[0], mx[1], mx[2], mx[3], mx[4], slow, hw[slow].k2, hw[slow].count, slow_t);
        for (int k = 0; k < 5; ++k) std::fprintf(stderr, " %.2f", (double)(t[(size_t)slow * 8 + k + 1] - t[(size_t)slow * 8 + k]) * 0.01);
        // histogram of workgroup durations by current keyframe decile
        {
          unsigned long long u[16];
          LVF_HIP(hipMemcpy(u, p->dbg_lin.p + (size_t)la.v.n_tfw * 8 + 8 + (size_t)slow * 16, sizeof(u), hipMemcpyDeviceToHost));
          std::fprintf(stderr, " ; its waves (eval us, k1-sum us, groups):");
          for (int wv = 0; wv < 4; ++wv) std::fprintf(stderr, " [%.2f %.2f %llu]", (double)(u[4 * wv + 1] - u[4 * wv]) * 0.01, (double)(u[4 * wv + 2] - u[4 * wv + 1]) * 0.01, u[4 * wv + 3]);
        }
        std::fprintf(stderr, " ; mean duration by k2 decile:");
        const int nk = la.n_kf;
        for (int dcl = 0; dcl < 5; ++dcl) {
          double sum = 0; int cnt = 0;
          for (int w = 0; w < la.v.n_tfw; ++w) if (hw[w].k2 * 5 / std::max(nk, 1) == dcl) { sum += (double)(t[(size_t)w * 8 + 5] - t[(size_t)w * 8]) * 0.01; ++cnt; }
          std::fprintf(stderr, " %.1f(%d)", cnt ? sum / cnt : 0.0, cnt);
        }
        std::fprintf(stderr, "\n");
      }
      std::fprintf(stderr, "lin_tf: the TwoFrame workgroups START within %.2f us of each other; starts of workgroups 0, 1/4, 1/2, 3/4, last (us after the first): %.2f %.2f %.2f %.2f %.2f\n", (double)(last_start - first) * 0.01,
                   (double)(t[0] - first) * 0.01, (double)(t[(size_t)(la.v.n_tfw / 4) * 8] - first) * 0.01, (double)(t[(size_t)(la.v.n_tfw / 2) * 8] - first) * 0.01,
                   (double)(t[(size_t)(3 * la.v.n_tfw / 4) * 8] - first) * 0.01, (double)(t[(size_t)(la.v.n_tfw - 1) * 8] - first) * 0.01);
      std::fprintf(stderr, "lin_tf phases (us, mean over %d workgroups): stage %.2f | eval+landmark atomics %.2f | k1 sums %.2f | k2 sums %.2f | flush %.2f ; first start -> last end %.2f\n",
                   la.v.n_tfw, ph[0] / la.v.n_tfw, ph[1] / la.v.n_tfw, ph[2] / la.v.n_tfw, ph[3] / la.v.n_tfw, ph[4] / la.v.n_tfw, (double)(last - first) * 0.01);
      if (la.v.imu.pre) {
        unsigned long long u[5];
        LVF_HIP(hipMemcpy(u, p->dbg_lin.p + (size_t)la.v.n_tfw * 8, sizeof(u), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "lin_imu phases of factor 0 (us): stage %.2f | raw residual + pre-weighting Jacobian (one lane) %.2f | weight + to tangent %.2f | J^T J, J^T r %.2f ; start %.2f after the first TwoFrame workgroup, end %.2f before the last one's end\n",
                     (double)(u[1] - u[0]) * 0.01, (double)(u[2] - u[1]) * 0.01, (double)(u[3] - u[2]) * 0.01, (double)(u[4] - u[3]) * 0.01, ((double)u[0] - (double)first) * 0.01, ((double)last - (double)u[4]) * 0.01);
      }
    }
  } else {
    if (p->tc && p->tc->n)
      hipLaunchKernelGGL(k_lin_tc<false>, dim3(grid(p->tc->n)), dim3(kT), 0, q, p->tc->n, (const double2*)p->tc->ob_a.p, (const double2*)p->tc->ob_b.p,
                         p->tc->idx_a.p, p->tc->idx_b.p, p->tc->wblk.n ? p->tc->wblk.p : (const double*)nullptr, s, p->tc->cam_a, p->tc->cam_b, huber, p->C.p, p->gr.p, cost);
    if (p->tf && p->tf->n)
      hipLaunchKernelGGL(k_lin_tf<false>, dim3(grid(p->tf->n)), dim3(kT), 0, q, p->tf->n, p->n_kf, (const double2*)p->tf->ob_a.p, (const double2*)p->tf->ob_b.p,
                         p->tf->idx_a.p, p->tf->idx_b.p, p->tf->idx_c.p, s, p->tf->cam_a, p->tf->cam_b, huber, p->pose_const.p, p->B.p, p->dpad,
                         p->gc.p, p->E.p, p->ldE, p->C.p, p->gr.p, cost);
    if (p->po && p->po->n)
      hipLaunchKernelGGL(k_lin_po<false>, dim3(grid(p->po->n)), dim3(kT), 0, q, p->po->n, p->n_kf, (const double2*)p->po->ob_a.p, p->po->idx_a.p,
                         p->po->idx_b.p, p->po->table.p, s, p->po->cam_a, huber, p->pose_const.p, p->B.p, p->dpad, p->gc.p, cost);
  }
  if (c.has_imu && !imu_done) {
    LVF_TRY(launch_imu(p->imu, p->st, true));
    ImuJ J;
    for (int k = 0; k < 8; ++k) J.j[k] = p->imu->jac[k].p;
    hipLaunchKernelGGL(k_lin_imu, dim3(p->imu->n), dim3(64), 0, q, p->imu->n, p->n_kf, p->imu->res.p, J, p->imu->idx_a.p, p->imu->idx_b.p,
                       p->st->poses.p, p->pose_const.p, p->B.p, p->dpad, p->gc.p, cost);
  }
  if (c.has_prior) {
    const lvf_batch* pb = p->prior;
    const PriorArgs P{pb->n, pb->idx_a.p, pb->idx_b.p, pb->table.p, pb->ob_a.p, pb->ob_b.p};
    hipLaunchKernelGGL(k_prior_lin, dim3((pb->n + 63) / 64), dim3(64), 0, q, P, p->st->poses.p, p->pose_const.p, p->B.p, p->dpad, p->gc.p, cost);
  }
  if (c.has_lidar)
    hipLaunchKernelGGL(k_lidar_lin, dim3(grid(p->lidar->n)), dim3(kT), 0, q, lidar_pose_args(p->lidar), p->n_kf, p->st->poses.p, p->pose_const.p, p->B.p, p->dpad, p->gc.p, cost);
  if (c.has_dprior)
    hipLaunchKernelGGL(k_dense_prior_lin, dim3(1), dim3(kDensePriorT), 0, q, dense_prior_args(p->dprior), p->n_kf, s, p->pose_const.p, p->B.p, p->dpad, p->gc.p, cost,
                       (double*)nullptr, (double*)nullptr);
  LVF_HIP(hipGetLastError());
  p->linearized = true;
  return LVF_OK;
}

// the deferred item count of the band work list (build_band_work) -> the Schur launch's arguments
int await_band_work(lvf_problem* p) {
  if (!p->band_pending) return LVF_OK;
  LVF_HIP(hipEventSynchronize(p->ev_band));
  p->band_pending = false;
  p->n_band_work = p->h_n_band_work[0];
  if (p->chain && p->chain->merged_level0) {
    SchurSp0Args& a = p->chain->ssp0;
    a.n_work = p->n_band_work;
    a.nblocks = a.n_work + a.sp.nblocks + a.sp_b.nblocks + a.sp_c.nblocks;
  }
  return LVF_OK;
}

static int launch_schur(hipStream_t q, int n_lm, int dp, int ldE, const double* E, const double* Cd, int d, int ldS, double* S, const LmBand& band) {
  const int nt = ldE / 16, ntile = nt * (nt + 1) / 2;
  if (band.order) {
    const size_t shb = ((size_t)kSchurRows * (ldE + 16) + kSchurRows) * sizeof(double) + kBandRowsMax * sizeof(int);
    if (shb <= 64 * 1024) {
      hipLaunchKernelGGL(k_schur_band, dim3((n_lm + kBandRows - 1) / kBandRows, (ntile + kBandTilesPerGroup - 1) / kBandTilesPerGroup), dim3(256), shb, q,
                         dp, ldE, E, Cd, band.order, band.n_active, band.kmin, band.kmax, d, ldS, S);
      LVF_HIP(hipGetLastError());
      return LVF_OK;
    }
  }
  const bool lds_path = ldE <= 320 && ntile <= kSchurGroups * 4 * kSchurTilesPerWave;
  if (lds_path) {
    const int slices = std::max(1, std::min(32, (n_lm + 4 * kSchurRows - 1) / (4 * kSchurRows)));   // 16..128 measured: 32 is the optimum at 10 k rows
    int rows_per_slice = (n_lm + slices - 1) / slices;
    rows_per_slice = ((rows_per_slice + kSchurRows - 1) / kSchurRows) * kSchurRows;
    const size_t shb = ((size_t)kSchurRows * ldE + kSchurRows) * sizeof(double);
    hipLaunchKernelGGL(k_schur_lds, dim3(kSchurGroups, (n_lm + rows_per_slice - 1) / rows_per_slice), dim3(256), shb, q, n_lm, dp, ldE, ntile, rows_per_slice, E,
                       Cd, d, ldS, S);
  } else {
    hipLaunchKernelGGL(k_schur_syrk, dim3(ntile, (n_lm + kSchurChunk - 1) / kSchurChunk), dim3(64), 0, q, n_lm, dp, ldE, ntile, E, Cd, d, ldS, S);
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

// S (elimination order) = B + D - E^T Cd^-1 E, rhs row = -(gc - E^T Cd^-1 g_rho); radius read from `radius_dev`
int enqueue_reduced_system(lvf_problem* p, const double* radius_dev, bool reset_scalars, bool gated, bool* level0_done, const AccSel* acc) {
  hipStream_t q = p->ctx->stream;
  const Chain& c = *p->chain;
  // the parity tap (level0_done == nullptr: the damped system alone, nothing eliminated) always takes the classic assembly
  const bool early = c.early && level0_done != nullptr;
  PrepArgs pa = early ? c.prep_early : c.prep;
  if (acc) { pa.acc = *acc; acc_patch(pa.ride, acc); }
  pa.radius = radius_dev;
  if (!reset_scalars) pa.scal = nullptr;
  if (!gated) pa.done = nullptr;
  // LVF_POISON_S=1 (diagnostic): every byte of S is 0xff (NaN) before the assembly, so whatever the assembly does not write — the upper
  // triangle — stays NaN; results must not change (tests/test_gpu_solver.py runs the parity cases this way too)
  if (solver_env().poison_s) LVF_HIP(hipMemsetAsync(p->S.p, 0xff, (size_t)p->ld * p->ld * 8, q));
  LVF_CHAIN_LAUNCH(p, ST_PREPARE, k_prepare, dim3(pa.nblocks), dim3(kT), pa.ride.nblocks > 0 ? c.prep_lds : 0, q, pa);
  // (k_prior_lin, k_lidar_lin and k_dense_prior_lin close the linearisation right ahead of this launch, so this stage's span holds them and its count names them.
  // The clock only runs inside enqueue_iteration, where windows with such blocks always linearise first: they never take the fused chain.)
  stage_mark(p, ST_PREPARE, 1 + (c.has_prior ? 1 : 0) + (c.has_lidar ? 1 : 0) + (c.has_dprior ? 1 : 0));
  if (!early && c.early) p->accum_clean = false;       // the tap wrote S: the next iteration must clear it
  if (level0_done) *level0_done = false;
  if (p->n_lm) {
    LVF_TRY(await_band_work(p));                       // (patches c.ssp0: `c` refers to the problem's chain)
    if (c.merged_level0) {
      SchurSp0Args sa = c.ssp0;
      if (acc) { sa.acc = *acc; acc_patch(sa.sp, acc); acc_patch(sa.sp_b, acc); acc_patch(sa.sp_c, acc); }
      if (!gated) sa.done = nullptr;
      if (!level0_done) { sa.nblocks = sa.n_work; sa.sp.nblocks = 0; sa.sp_b.nblocks = 0; sa.sp_c.nblocks = 0; }       // the Schur complement alone (parity tap)
      const bool schur_timing = solver_env().schur_timing;
      const int ns = sa.n_work;
      if (schur_timing) { LVF_TRY(p->dbg_lin.ensure((size_t)ns * 8 + 8)); LVF_HIP(hipMemsetAsync(p->dbg_lin.p, 0, (size_t)ns * 64, q)); sa.dbg = p->dbg_lin.p; }
      if (sa.nblocks > 0) LVF_CHAIN_LAUNCH(p, ST_SCHUR_SP0, k_schur_sp0, dim3(sa.nblocks), dim3(256), c.ssp0_lds, q, sa);
      stage_mark(p, ST_SCHUR_SP0, 1);
      if (schur_timing) {
        std::vector<unsigned long long> t((size_t)ns * 8);
        LVF_HIP(hipStreamSynchronize(q));
        LVF_HIP(hipMemcpy(t.data(), p->dbg_lin.p, t.size() * 8, hipMemcpyDeviceToHost));
        double ph[3] = {0, 0, 0}; int cnt = 0; unsigned long long first = ~0ull, last = 0;
        for (int w = 0; w < ns; ++w) {
          if (!t[(size_t)w * 8 + 3]) continue;
          ++cnt;
          for (int k = 0; k < 3; ++k) ph[k] += (double)(t[(size_t)w * 8 + k + 1] - t[(size_t)w * 8 + k]) * 0.01;
          first = std::min(first, t[(size_t)w * 8]); last = std::max(last, t[(size_t)w * 8 + 3]);
        }
        std::fprintf(stderr, "schur band phases (us, mean over %d of %d workgroups): setup + first fetch issue %.2f | chunks (stage + mfma) %.2f | output atomics %.2f ; first start -> last end %.2f\n",
                     cnt, ns, ph[0] / std::max(cnt, 1), ph[1] / std::max(cnt, 1), ph[2] / std::max(cnt, 1), (double)(last - first) * 0.01);
      }
      if (level0_done) *level0_done = true;
    } else {
      double* S_pose = p->S.p + (size_t)p->off_pose * (p->ld + 1);
      const LmBand band{p->band_ready ? p->lm_order.p : nullptr, p->lm_nactive.p, p->lm_kmin.p, p->lm_kmax.p};
      LVF_TRY(launch_schur(q, p->n_lm, p->dp, p->ldE, p->E.p, p->Cd.p, p->dp, p->ld, S_pose, band));
    }
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

// one complete LM iteration of one window on its stream, closed on device by k_lm_decide; nothing is waited for
// (`fused`: the kFused* flags, solver_host.hpp)
int enqueue_iteration(lvf_problem* p, bool end_zero, int fused) {
  hipStream_t q = p->ctx->stream;
  if (chain_stale(p)) LVF_TRY(build_chain(p));
  const Chain& c = *p->chain;
  const ReducedOverride* ov = p->ov.get();    // test tap (null in production)
  if (ov) LVF_REQUIRE(ov->d == p->d, "the overridden reduced system has %d unknowns, the problem now has %d: clear or set it again", ov->d, p->d);      // (before any launch)
  if (!c.fused_ok || !p->acc1_ready || ov) fused = 0;
  const AccSel* acc = (fused & kFusedOn) ? &c.acc : nullptr;
  const bool sp_timing = solver_env().sp_timing;
  if (sp_timing && c.early) {
    // diagnostic: the levels' stamps (the chain is rebuilt with the debug pointer in every level's arguments; printed by the next call)
    const int n_nodes = p->sp_levels.n ? p->sp_levels.first[p->sp_levels.n - 1] + p->sp_levels.count[p->sp_levels.n - 1] : 0;
    if (p->dbg_sp.n == 0) {
      LVF_TRY(p->dbg_sp.ensure((size_t)n_nodes * 8 + 8)); p->dbg_sp.n = (size_t)n_nodes * 8;
      LVF_HIP(hipMemsetAsync(p->dbg_sp.p, 0, (size_t)n_nodes * 64, q));
      Chain& cw = *p->chain;
      for (int lv = 0; lv < cw.n_levels; ++lv) cw.sp[lv].src.dbg = p->dbg_sp.p;
      cw.red.ride.src.dbg = p->dbg_sp.p; cw.prep_early.ride.src.dbg = p->dbg_sp.p; cw.ssp0.sp.src.dbg = p->dbg_sp.p; cw.ssp0.sp_b.src.dbg = p->dbg_sp.p; cw.ssp0.sp_c.src.dbg = p->dbg_sp.p;
    } else {
      std::vector<unsigned long long> t((size_t)n_nodes * 8);
      LVF_HIP(hipStreamSynchronize(q));
      LVF_HIP(hipMemcpy(t.data(), p->dbg_sp.p, t.size() * 8, hipMemcpyDeviceToHost));
      for (int lv = 0; lv < p->sp_levels.n; ++lv) {
        const int f0 = p->sp_levels.first[lv], cnt = p->sp_levels.count[lv];
        double ph[7] = {0, 0, 0, 0, 0, 0, 0}; unsigned long long first = ~0ull, last = 0;
        for (int k = f0; k < f0 + cnt; ++k) {
          for (int j = 0; j < 7; ++j) ph[j] += (double)(t[(size_t)k * 8 + j + 1] - t[(size_t)k * 8 + j]) * 0.01 / cnt;
          first = std::min(first, t[(size_t)k * 8]); last = std::max(last, t[(size_t)k * 8 + 7]);
        }
        std::fprintf(stderr, "sparse level %d (%d blocks, us): requests by address %.2f | wait for the level below %.2f | S entries %.2f | factor %.2f | W + first adds (returning) %.2f | arrive %.2f | rest of the adds %.2f ; start %.2f after level 0's first start, span %.2f\n",
                     lv, cnt, ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], (double)(first - t[0]) * 0.01, (double)(last - first) * 0.01);
      }
    }
  }
  // With an override the damped system is assembled the classic way (no level rides in the launches ahead: they would read B), the caller's
  // entries go over it, and every level is a launch of its own reading S alone; from the block steps on the chain is production's.
  // (iteration = false also takes the reset of the per-step scalars and of SC_FAIL out of the linearisation launch: the classic k_prepare
  // below does it, as in the chain without early levels, so a flag raised by one iteration never reaches the next.)
  LVF_TRY(enqueue_linearize(p, p->huber, true, !ov, acc, !(fused & kFusedNoLin)));
  bool level0_done = false;
  LVF_TRY(enqueue_reduced_system(p, &p->ctl.p->radius, true, true, ov ? nullptr : &level0_done, acc));
  if (ov) {
    // (a plain launch: a test-only copy is no stage of lvf_problem_stage_times.  Not gated by the loop's `done` flag either — after the end of a
    // solve it only rewrites S, which nothing reads any more)
    LVF_TRY(launch_override_reduced(q, p->d, p->ld, p->aug, p->perm.p, ov->S.p, ov->rhs.p, p->S.p));
  }
  const int own0 = level0_done ? c.first_own_level : 0;      // (levels below rode in the launches above)
  for (int lv = own0; lv < c.n_levels; ++lv) {
    SpArgs la = c.sp[lv];
    acc_patch(la, acc);
    if (ov) { SpSrc& sr = la.src; sr.B = nullptr; sr.ldB = 0; sr.dp = 0; sr.gc = nullptr; sr.radius = nullptr; sr.rows_nat = nullptr; sr.s_zero = 0; }      // the classic form
    LVF_CHAIN_LAUNCH(p, ST_SP_LEVELS, k_sp_eliminate, dim3(la.nblocks), dim3(256), c.sp_lds[lv], q, la);
  }
  stage_mark(p, ST_SP_LEVELS, std::max(0, c.n_levels - own0));
  const int nb_own = c.chol_back_merged ? p->nb - 1 : p->nb;      // (merged last launch: block step nb - 1 runs inside k_chol_backsolve_tail)
  for (int kb = 0; kb < nb_own; ++kb) {
    CholArgs cha = c.chol;
    if (solver_env().chol_timing) { LVF_TRY(p->dbg.ensure(128)); cha.dbg = p->dbg.p; }      // [0, 64): phases of 8 block steps; [64, 128): their sub-block stages
    GRide gr = c.gride;                                   // the riders that form G: the top level first, one level per launch
    const int glv = c.n_levels - 1 - kb;
    if (c.back_product && glv >= 0) { gr.first = p->sp_levels.first[glv]; gr.n = p->sp_levels.count[glv]; } else gr.n = 0;
    TRide tr = c.tride;                                   // the riders that form T_kj, k = kb - 1: both factors are final since launch kb - 1
    tr.n = (c.back_blocks && kb >= 1) ? p->nb - kb : 0;
    if (solver_env().chol_subblock) LVF_CHAIN_LAUNCH(p, ST_CHOL, k_chol_step, dim3(chol_step_grid(p->nb, kb) + gr.n + tr.n), dim3(kCT), 0, q, cha, kb, gr, tr);
    else LVF_CHAIN_LAUNCH(p, ST_CHOL, k_chol_step_pp, dim3(chol_step_grid(p->nb, kb) + gr.n + tr.n), dim3(kCT), 0, q, cha, kb, gr, tr);
  }
  {
    BackArgs ba = c.back;
    const bool back_timing = solver_env().back_timing;
    if (back_timing) { LVF_TRY(p->dbg.ensure(64)); ba.sp.dbg = p->dbg.p; }
    if (c.back_blocks) ba.T = p->sp_T.p;
    stage_mark(p, ST_CHOL, nb_own);
    if (c.chol_back_merged) {
      CholBackArgs cb = c.cb;
      if (solver_env().chol_timing) cb.chol.dbg = p->dbg.p;      // (ensured above: nb_own >= 1)
      if (back_timing) cb.bt.back.sp.dbg = p->dbg.p;
      if (acc) cb.bt.tail.acc = *acc;
      LVF_CHAIN_LAUNCH(p, ST_BACKSOLVE, k_chol_backsolve_tail, dim3(3 + cb.g.n + 1 + cb.bt.g_prod + cb.bt.g_lm), dim3(kBT), c.cb_lds, q, cb);
      stage_mark(p, ST_BACKSOLVE, 1);
      stage_mark(p, ST_STEP_TAIL, 0);
    } else if (c.back_tail_merged) {
      BackTailArgs bt = c.bt;
      if (back_timing) bt.back.sp.dbg = p->dbg.p;
      bt.back.T = ba.T;
      if (acc) bt.tail.acc = *acc;
      LVF_CHAIN_LAUNCH(p, ST_BACKSOLVE, k_backsolve_tail, dim3(2 + c.bt.g_lm + c.bt.g_prod), dim3(kBT), c.bt_lds, q, bt);
      stage_mark(p, ST_BACKSOLVE, 1);
      stage_mark(p, ST_STEP_TAIL, 0);
    } else {
      LVF_CHAIN_LAUNCH(p, ST_BACKSOLVE, k_chol_backsolve, dim3(1), dim3(kBT), c.back_lds, q, ba);
      stage_mark(p, ST_BACKSOLVE, 1);
      TailArgs ta = c.tail;
      if (acc) ta.acc = *acc;
      LVF_CHAIN_LAUNCH(p, ST_STEP_TAIL, k_step_tail, dim3(ta.nblocks), dim3(kT), c.tail_lds, q, ta);
      stage_mark(p, ST_STEP_TAIL, 1);
    }
  }
  if (fused & kFusedTail) {
    // the candidate pass linearises x + dx into the standby set and closes the iteration (k_lin_cost_decide)
    FusedArgs fa = c.fused;
    fa.lin.huber = p->huber;
    LVF_CHAIN_LAUNCH(p, ST_FUSED, k_lin_cost_decide, dim3(fa.nblocks + fa.zero_wgs), dim3(kT), c.lin_lds, q, fa);
    stage_mark(p, ST_COST, 0);
    stage_mark(p, ST_FUSED, 1);
    p->accum_clean = false;
    p->linearized = false;
    LVF_HIP(hipGetLastError());
    return LVF_OK;
  }
  // candidate cost: the small passes first, then the visual pass whose last workgroup closes the iteration
  CostArgs ca = c.cost;
  ca.huber = p->huber;
  if (c.has_imu && !c.imu_in_cost) LVF_TRY(launch_imu_args(q, c.imu_cost, false));
  if (c.has_prior) {
    const lvf_batch* pb = p->prior;
    const PriorArgs P{pb->n, pb->idx_a.p, pb->idx_b.p, pb->table.p, pb->ob_a.p, pb->ob_b.p};
    hipLaunchKernelGGL(k_prior_cost, dim3((pb->n + 63) / 64), dim3(64), 0, q, P, p->poses2.p, p->scal.p + SC_COST_NEW);
  }
  if (c.has_lidar) hipLaunchKernelGGL(k_lidar_cost, dim3(grid(p->lidar->n)), dim3(kT), 0, q, lidar_pose_args(p->lidar), p->n_kf, p->poses2.p, p->scal.p + SC_COST_NEW);
  if (c.has_dprior) hipLaunchKernelGGL(k_dense_prior_cost, dim3(1), dim3(kDensePriorT), 0, q, dense_prior_args(p->dprior), candidate_ptrs(p), p->scal.p + SC_COST_NEW);      // (reads velocity and biases too)
  if (ca.nblocks > 0) {
    if (!end_zero) ca.zero_wgs = 0;
    DecideArgs da = c.dec;
    if (solver_env().cost_timing) { LVF_TRY(p->dbg.ensure(64)); da.dbg = p->dbg.p; }
    LVF_CHAIN_LAUNCH(p, ST_COST, k_cost_decide, dim3(ca.nblocks + ca.zero_wgs), dim3(kT), 0, q, ca, da, end_zero ? 1 : 0);
    p->accum_clean = ca.zero_wgs > 0;
    if (p->accum_clean) p->linearized = false;         // the normal equations of this iteration are gone: no reduced-system tap
    stage_mark(p, ST_COST, 1 + (c.has_imu && !c.imu_in_cost ? 1 : 0) + (c.has_prior ? 1 : 0) + (c.has_lidar ? 1 : 0) + (c.has_dprior ? 1 : 0));
  } else {
    stage_mark(p, ST_COST, (c.has_imu ? 1 : 0) + (c.has_prior ? 1 : 0) + (c.has_lidar ? 1 : 0) + (c.has_dprior ? 1 : 0));
    LVF_CHAIN_LAUNCH(p, ST_DECIDE, k_lm_decide, dim3(1), dim3(kDT), 0, q, c.dec);
    stage_mark(p, ST_DECIDE, 1);
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

void ctl_from_options(const lvf_solver_options* o, double radius, double decrease, int max_iters, bool with_tolerances, LmCtl* c) {
  std::memset(c, 0, sizeof(*c));
  c->radius = radius; c->decrease = decrease; c->last_radius = radius;
  c->huber = o->huber_a; c->min_rel_decrease = o->min_relative_decrease;
  c->function_tol = with_tolerances ? o->function_tolerance : -1.0;
  c->gradient_tol = with_tolerances ? o->gradient_tolerance : -1.0;
  c->parameter_tol = with_tolerances ? o->parameter_tolerance : -1.0;
  c->max_iters = max_iters;
  c->termination = 1; c->why = LVF_WHY_MAX_ITERATIONS;
}
int upload_ctl(lvf_problem* p, const LmCtl& c) {
  if (chain_stale(p)) LVF_TRY(build_chain(p));
  *p->rec = c;                               // the host-visible mirror starts from the same values
  LVF_TRY(p->h_ctl.reserve(1));
  p->h_ctl[0] = c;
  LVF_HIP(hipMemcpyAsync(p->ctl.p, p->h_ctl.p, sizeof(LmCtl), hipMemcpyHostToDevice, p->ctx->stream));
  return LVF_OK;
}
int download_ctl(lvf_problem* p, LmCtl* out) {
  hipStream_t q = p->ctx->stream;
  LVF_TRY(p->h_ctl.reserve(2));
  LVF_HIP(hipMemcpyAsync(&p->h_ctl[1], p->ctl.p, sizeof(LmCtl), hipMemcpyDeviceToHost, q));
  LVF_HIP(hipStreamSynchronize(q));
  *out = p->h_ctl[1];
  return LVF_OK;
}

// The loop ended because a chained sparse level timed out waiting for the level below (LVF_WHY_HANDOVER; the step was neither taken nor
// counted).  The problem gives up chaining for good (its levels become launches of their own: the LVF_CHAIN_LEVELS=0 form), the control
// block is re-armed as the aborted iteration found it and the caller enqueues again.  Returns false when there is nothing to retry.
bool handover_pending(const lvf_problem* p, const LmCtl& c) { return c.done && c.why == LVF_WHY_HANDOVER && !p->no_chain; }
int rearm_after_handover(lvf_problem* p, LmCtl* c) {
  p->no_chain = true; p->unchained_solves = 0; p->chain_ready = false; p->handover_retries += 1;
  if (p->force_handover_timeouts > 0) p->force_handover_timeouts -= 1;
  c->done = 0; c->termination = 1; c->why = LVF_WHY_MAX_ITERATIONS;
  c->aset = 0; c->lin_pending = 0;           // (the re-run linearises into set 0 with today's chain)
  p->accum_clean = false;                    // (the aborted iteration's partial sums: cleared by an explicit launch before the re-run)
  return upload_ctl(p, *c);                  // rebuilds the chain
}

// exactly one LM iteration from the current state (no tolerance tests): the per-iteration parity point
int lm_iteration(lvf_problem* p, const lvf_solver_options* o, double* radius, double* decrease, IterOut* out) {
  LmCtl c;
  ctl_from_options(o, *radius, *decrease, 1, false, &c);
  p->huber = o->huber_a;
  LVF_TRY(upload_ctl(p, c));
  LVF_TRY(enqueue_iteration(p, false));
  LVF_TRY(download_ctl(p, &c));
  if (handover_pending(p, c)) {              // a chained hand-over timed out: the same iteration again, un-chained
    LVF_TRY(rearm_after_handover(p, &c));
    LVF_TRY(enqueue_iteration(p, false));
    LVF_TRY(download_ctl(p, &c));
  }
  if (p->dbg.p && solver_env().chol_timing) {
    unsigned long long t[128];
    LVF_HIP(hipMemcpy(t, p->dbg.p, sizeof(t), hipMemcpyDeviceToHost));
    for (int kb = 0; kb < p->nb && kb < 8; ++kb) {
      const unsigned long long* u = t + 8 * kb;
      if (solver_env().chol_subblock && kb + 2 < p->nb + 1) {      // a full block: per stage, sweep + exchange | tile products (seen by wave 0 of workgroup 1)
        const unsigned long long* v = t + 64 + 8 * kb;
        std::fprintf(stderr, "chol step %d stages (us): %.2f | %.2f ; %.2f | %.2f ; %.2f | %.2f ; %.2f\n", kb, (double)(v[0] - u[3]) * 0.01, (double)(v[1] - v[0]) * 0.01,
                     (double)(v[2] - v[1]) * 0.01, (double)(v[3] - v[2]) * 0.01, (double)(v[4] - v[3]) * 0.01, (double)(v[5] - v[4]) * 0.01, (double)(v[6] - v[5]) * 0.01);
      }
      if (kb == 0) std::fprintf(stderr, "chol step 0 (us): loads %.2f | factor %.2f (%llu shader clocks) | store %.2f\n", (double)(u[3] - u[0]) * 0.01, (double)(u[4] - u[3]) * 0.01, u[7] - u[6], (double)(u[5] - u[4]) * 0.01);
      else if (kb + 2 < p->nb + 1) std::fprintf(stderr, "chol step %d (us): stage %.2f | mfma %.2f | relayout %.2f | factor %.2f | store %.2f ; since previous step's end %.2f\n", kb, (double)(u[1] - u[0]) * 0.01,
                        (double)(u[2] - u[1]) * 0.01, (double)(u[3] - u[2]) * 0.01, (double)(u[4] - u[3]) * 0.01, (double)(u[5] - u[4]) * 0.01, (double)(u[0] - u[-3]) * 0.01);
    }
  }
  if (p->dbg.p && solver_env().cost_timing) {
    unsigned long long t[64];
    LVF_HIP(hipMemcpy(t, p->dbg.p, sizeof(t), hipMemcpyDeviceToHost));
    auto us = [&](int a, int b) { return ((double)t[b] - (double)t[a]) * 0.01; };
    std::fprintf(stderr, "cost+decide (us): imu wg0 stage %.2f | raw (one lane) %.2f | weight+sum %.2f ; first visual wg %.2f (starts %.2f after imu wg0) ; decision starts %.2f after imu wg0's start: sums %.2f | logic %.2f | commit %.2f | record %.2f\n",
                 us(8, 9), us(9, 10), us(10, 11), us(12, 13), us(8, 12), us(8, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5));
  }
  if (p->dbg.p && solver_env().back_timing) {
    unsigned long long t[64];
    LVF_HIP(hipMemcpy(t, p->dbg.p, sizeof(t), hipMemcpyDeviceToHost));
    std::fprintf(stderr, p->chain && p->chain->chol_back_merged ? "backsolve phases inside the merged last launch (us: requests | x_last flag seen | x_last read | links .. | published):" : "backsolve phases (us):");
    for (unsigned long long k = 1; k < t[63] && k < 55; ++k) std::fprintf(stderr, " %.2f", (double)(t[k] - t[k - 1]) * 0.01);
    if (p->chain && p->chain->back_tail_merged)
      std::fprintf(stderr, " | merged launch, us after workgroup 0's start: step applied %.2f ; first landmark workgroup starts %.2f, sees the poses %.2f, done %.2f ; last one starts %.2f, sees %.2f, done %.2f",
                   (double)(t[55] - t[0]) * 0.01, (double)(t[56] - t[0]) * 0.01, (double)(t[57] - t[0]) * 0.01, (double)(t[58] - t[0]) * 0.01, (double)(t[59] - t[0]) * 0.01,
                   (double)(t[60] - t[0]) * 0.01, (double)(t[61] - t[0]) * 0.01);
    if (p->chain && p->chain->back_tail_merged) std::fprintf(stderr, " ; pose workgroup done %.2f", (double)(t[62] - t[0]) * 0.01);
    if (p->chain && p->chain->back_product)
      std::fprintf(stderr, " | product form (\"step applied\" = workgroup 0 done): first G workgroup starts %.2f, sees the flag %.2f, has the dense solution %.2f, its rows %.2f, applied %.2f",
                   (double)(t[40] - t[0]) * 0.01, (double)(t[41] - t[0]) * 0.01, (double)(t[42] - t[0]) * 0.01, (double)(t[43] - t[0]) * 0.01, (double)(t[44] - t[0]) * 0.01);
    if (p->chain && p->chain->chol_back_merged)
      std::fprintf(stderr, " | merged last launch: the first G workgroup sees the riders' arrivals %.2f, holds its share of G %.2f", (double)(t[45] - t[0]) * 0.01, (double)(t[46] - t[0]) * 0.01);
    std::fprintf(stderr, "\n");
  }
  out->cost_before = c.cost_before; out->cost_after = c.cost_after; out->model = c.model; out->dxnorm = c.dxnorm; out->xnorm = c.xnorm; out->gmax = c.gmax;
  out->solved = c.solved != 0; out->accepted = c.accepted != 0;
  p->last_radius = c.last_radius;
  p->step_ready = true; p->last_solved = c.solved;
  *radius = c.radius; *decrease = c.decrease;
  return LVF_OK;
}

// waits until the host-visible mirror shows at least `iter` closed iterations (or the loop finished); falls back to a stream
// synchronisation when the mirror does not move (e.g. device writes to host memory only becoming visible at kernel boundaries)
int wait_for_iteration(lvf_problem* p, int iter) {
  const volatile LmCtl* r = p->rec;
  const auto t0 = std::chrono::steady_clock::now();
  while (r->iter < iter && !r->done) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05) {
      LmCtl c;
      LVF_TRY(download_ctl(p, &c));          // synchronises the stream
      *p->rec = c;
      break;
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return LVF_OK;
}

}  // namespace lvf
