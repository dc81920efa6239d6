// solver_batch.hip — a batch of windows advanced by one chain of table launches per LM iteration, and its C entry points.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>

#include "solver_host.hpp"

using namespace lvf;

// ------------------------------------------------------------------------------------------------ a batch of windows
// W independent windows advanced by ONE chain of launches per LM iteration: every kernel of the iteration takes blockIdx.y = window and
// reads that window's argument block from a device table.  A single window's iteration is a chain of ~23 small launches that leaves
// most of the 256 CUs idle (sequential pivots, 2 + k workgroups per panel step); a batch fills the same launches W times over — the
// shape of every independent-window client of the reference: RL environments (src/lvio_fusion/src/environment.cpp:18-115), loop-closure
// candidates (relocator.cpp:196-206), per-submap replays, and what ONE GPU of the 8-GPU sharding works on.
struct lvf_problem_batch {
  lvf_ctx* ctx = nullptr;
  std::vector<lvf_problem*> probs;
  bool tables = false;               // every member is batchable: table launches; otherwise the windows' own chains run back to back
  int W = 0, max_levels = 0, max_nb = 0;
  // per-stage argument tables [W] (device) and the launch shapes (max over the windows)
  lvf::DevBuf<lvf::ImuArgs> imu_lin, imu_cost; int g_imu_lin = 0, g_imu_cost = 0;
  lvf::DevBuf<lvf::LinArgs> lin; int g_lin = 0; size_t lds_lin = 0;
  lvf::DevBuf<lvf::TfReduceArgs> red; int g_red = 0; size_t lds_red = 0;
  lvf::DevBuf<lvf::PrepArgs> prep; int g_prep = 0; size_t lds_prep = 0;
  int first_own_level = 0;           // min over the windows: the first sparse level that is a launch of its own
  lvf::DevBuf<lvf::SchurSp0Args> ssp0; int g_ssp0 = 0; size_t lds_ssp0 = 0;
  lvf::DevBuf<lvf::SpArgs> sp[lvf::kSpMaxLevels]; int g_sp[lvf::kSpMaxLevels] = {0}; int lds_sp[lvf::kSpMaxLevels] = {0};
  lvf::DevBuf<lvf::CholArgs> chol;
  lvf::DevBuf<lvf::BackArgs> back; size_t lds_back = 0;
  lvf::DevBuf<lvf::TailArgs> tail; int g_tail = 0; size_t lds_tail = 0;
  lvf::DevBuf<lvf::CostArgs> cost; int g_cost = 0;
  lvf::DevBuf<lvf::DecideArgs> dec;
  lvf::DevBuf<lvf::ZeroList> zero;   // every window's full accumulator list (cleared in one launch when a window is not known clean)
  double huber_built = -1.0;
  // A batch of more than one window sums its Schur complements over wider landmark slices (fewer output atomics: LVF_BATCH_BAND_ROWS,
  // default 128).  The work lists for that width belong to the BATCH — a member's own list, slice width and chain are never touched, so a
  // window solved alone, then in a batch, then alone again runs the same arithmetic the first and the third time.
  std::vector<std::unique_ptr<lvf::DevBuf<int4>>> band_work; std::vector<int> n_band_work, band_epoch;
  bool orphaned = false;             // a member was destroyed before the batch: every later call fails with LVF_ERR_STATE
};

namespace lvf {

void batch_orphan(lvf_problem_batch* b, lvf_problem* dying) {
  b->orphaned = true;
  for (lvf_problem* p : b->probs)
    if (p != dying) p->batches.erase(std::remove(p->batches.begin(), p->batches.end(), b), p->batches.end());
  b->probs.clear();
}

template <typename T>
static int upload_table(DevBuf<T>& dst, const std::vector<T>& src, hipStream_t q) {
  LVF_TRY(dst.ensure(src.size()));
  // pageable source: the runtime stages the copy before returning, so `src` may go out of scope
  if (!src.empty()) LVF_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, q));
  return LVF_OK;
}

static int batch_build_tables(lvf_problem_batch* b, double huber) {
  hipStream_t q = b->ctx->stream;
  const int W = b->W;
  bool all = true;
  const int batch_rows = solver_env().batch_band_rows;
  if (b->orphaned) { set_error("lvf_problem_batch: a member problem was destroyed before the batch"); return LVF_ERR_STATE; }
  for (size_t w = 0; w < b->probs.size(); ++w)
    if (b->probs[w]->ov) { set_error("lvf_problem_batch: window %d has an overridden reduced system (lvf_problem_debug_override_reduced): the batched chains have no such tap", (int)w); return LVF_ERR_STATE; }
  for (lvf_problem* p : b->probs) {
    if (chain_stale(p)) LVF_TRY(build_chain(p));
    LVF_TRY(await_band_work(p));             // (the member's own list: its count shares the pinned slot build_band_work reads below)
    all = all && p->chain->batchable;
  }
  b->tables = all;
  if (!all) return LVF_OK;
  const bool wide = W > 1 && batch_rows != 64;
  if (wide) {
    b->band_work.resize(W); b->n_band_work.resize(W, 0); b->band_epoch.resize(W, -1);
    for (int w = 0; w < W; ++w) {
      lvf_problem* p = b->probs[w];
      if (!b->band_work[w]) b->band_work[w].reset(new DevBuf<int4>());
      if (b->band_epoch[w] == p->band_epoch) continue;
      LVF_TRY(build_band_work(p, batch_rows, *b->band_work[w], &b->n_band_work[w]));
      b->band_epoch[w] = p->band_epoch;
    }
  }
  std::vector<ImuArgs> il(W), ic(W); std::vector<LinArgs> li(W); std::vector<TfReduceArgs> rd(W); std::vector<PrepArgs> pr(W); std::vector<SchurSp0Args> ss(W);
  std::vector<CholArgs> ch(W); std::vector<BackArgs> bk(W); std::vector<TailArgs> tl(W); std::vector<CostArgs> co(W); std::vector<DecideArgs> de(W); std::vector<ZeroList> zl(W);
  b->max_levels = 0; b->max_nb = 0;
  b->g_red = 0; b->lds_red = 0; b->lds_prep = 0; b->first_own_level = kSpMaxLevels;
  b->g_imu_lin = b->g_imu_cost = b->g_lin = b->g_prep = b->g_ssp0 = b->g_tail = b->g_cost = 0; b->lds_ssp0 = b->lds_back = b->lds_tail = b->lds_lin = 0;
  for (int w = 0; w < W; ++w) {
    const lvf_problem* p = b->probs[w];
    const Chain& c = *p->chain;
    il[w] = c.imu_lin; ic[w] = c.imu_cost; li[w] = c.lin; li[w].huber = huber; rd[w] = c.red; if (!p->compact) rd[w].nblocks = 0;
    b->g_red = std::max(b->g_red, rd[w].nblocks); pr[w] = c.early ? c.prep_early : c.prep; ss[w] = c.ssp0; ch[w] = c.chol; bk[w] = c.back; tl[w] = c.tail;
    if (wide) {                                          // the batch's own slice width and work list (the member's chain keeps its own)
      SchurSp0Args& a = ss[w];
      a.rows = band_rows_clamped(batch_rows); a.n_slices = (p->n_lm + a.rows - 1) / a.rows;
      a.work = b->band_work[w]->p; a.n_work = b->n_band_work[w];
      a.nblocks = a.n_work + a.sp.nblocks + a.sp_b.nblocks + a.sp_c.nblocks;
    }
    if (rd[w].nblocks > rd[w].own_blocks) b->lds_red = std::max(b->lds_red, c.red_lds);
    if (pr[w].nblocks > pr[w].own_blocks) b->lds_prep = std::max(b->lds_prep, c.prep_lds);
    b->first_own_level = std::min(b->first_own_level, c.first_own_level);
    co[w] = c.cost; co[w].huber = huber; de[w] = c.dec; zl[w] = c.zero;
    if (W >= 4) {                                        // fatter cost / zeroing workgroups in a batch (see cost_visual_value)
      CostArgs& k = co[w];
      const int t = 4, per = kT * t;
      k.tiles = t;
      k.a.g_tc = (k.a.n_tc + per - 1) / per; k.a.g_tf = (k.a.n_tf + per - 1) / per;
      k.nblocks = k.g_imu + k.a.g_tc + k.a.g_tf + (k.a.n_po + per - 1) / per;
      k.zero_wgs = std::min(k.zero_wgs, 48);
      TailArgs& ta = tl[w];                              // ... and fewer landmark workgroups per window (64 windows: 203 -> 170 us with 256 instead of 640)
      const int g2 = std::min(ta.g_lm, 256);
      ta.nblocks -= ta.g_lm - g2; ta.g_lm = g2;
    }
    b->g_imu_lin = std::max(b->g_imu_lin, c.imu_lin.n + c.imu_lin.zero_wgs); b->g_imu_cost = std::max(b->g_imu_cost, c.imu_cost.n + c.imu_cost.zero_wgs);
    b->g_lin = std::max(b->g_lin, c.lin.nblocks); b->lds_lin = std::max(b->lds_lin, c.lin_lds); b->g_prep = std::max(b->g_prep, pr[w].nblocks); b->g_ssp0 = std::max(b->g_ssp0, ss[w].nblocks);
    b->lds_ssp0 = std::max(b->lds_ssp0, c.ssp0_lds); b->lds_back = std::max(b->lds_back, c.back_lds); b->g_tail = std::max(b->g_tail, tl[w].nblocks);
    b->lds_tail = std::max(b->lds_tail, c.tail_lds); b->g_cost = std::max(b->g_cost, co[w].nblocks + co[w].zero_wgs);
    b->max_levels = std::max(b->max_levels, c.n_levels); b->max_nb = std::max(b->max_nb, p->nb);
  }
  LVF_TRY(upload_table(b->imu_lin, il, q)); LVF_TRY(upload_table(b->imu_cost, ic, q)); LVF_TRY(upload_table(b->lin, li, q)); LVF_TRY(upload_table(b->red, rd, q)); LVF_TRY(upload_table(b->prep, pr, q));
  LVF_TRY(upload_table(b->ssp0, ss, q)); LVF_TRY(upload_table(b->chol, ch, q)); LVF_TRY(upload_table(b->back, bk, q)); LVF_TRY(upload_table(b->tail, tl, q));
  LVF_TRY(upload_table(b->cost, co, q)); LVF_TRY(upload_table(b->dec, de, q)); LVF_TRY(upload_table(b->zero, zl, q));
  for (int lv = b->first_own_level; lv < b->max_levels; ++lv) {        // (the levels below ride in the launches ahead: Chain::first_own_level)
    std::vector<SpArgs> sp(W);
    b->g_sp[lv] = 0; b->lds_sp[lv] = 0;
    for (int w = 0; w < W; ++w) {
      const Chain& c = *b->probs[w]->chain;
      if (lv >= c.first_own_level && lv < c.n_levels) { sp[w] = c.sp[lv]; b->g_sp[lv] = std::max(b->g_sp[lv], c.sp[lv].nblocks); b->lds_sp[lv] = std::max(b->lds_sp[lv], c.sp_lds[lv]); }
      else { sp[w] = SpArgs{}; sp[w].nblocks = 0; }
    }
    LVF_TRY(upload_table(b->sp[lv], sp, q));
  }
  b->huber_built = huber;
  return LVF_OK;
}

// one LM iteration of every window of the batch; nothing is waited for
static int batch_enqueue_iteration(lvf_problem_batch* b, bool end_zero) {
  hipStream_t q = b->ctx->stream;
  if (!b->tables) {
    for (lvf_problem* p : b->probs) LVF_TRY(enqueue_iteration(p, end_zero));
    return LVF_OK;
  }
  const unsigned W = (unsigned)b->W;
  bool clean = true;
  for (lvf_problem* p : b->probs) { clean = clean && p->accum_clean; p->accum_clean = false; }
  if (!clean) hipLaunchKernelGGL(k_zero_table, dim3(512, W), dim3(kT), 0, q, b->zero.p);
  // LVF_BATCH_TRANSPOSE (bit mask, default 127: all; measured 8 windows 20.7k -> 22.1k it/s, 32 windows 28.9k -> 29.9k): which of lin (1), tf_reduce (2), prepare (4), Schur (8), block steps (16), tail (32), cost (64) are launched with blockIdx.x = window
  const int tr = solver_env().batch_transpose;
  const bool fits_y = std::max(std::max(b->g_lin, b->g_red), std::max(b->g_prep, b->g_ssp0)) <= 65535;
  if ((tr & 1) && fits_y) hipLaunchKernelGGL(k_lin_visual_bt, dim3(W, b->g_lin), dim3(kT), b->lds_lin, q, b->lin.p);
  else hipLaunchKernelGGL(k_lin_visual_b, dim3(b->g_lin, W), dim3(kT), b->lds_lin, q, b->lin.p);
  if (b->g_red > 0) {
    if ((tr & 2) && fits_y) hipLaunchKernelGGL(k_tf_reduce_bt, dim3(W, b->g_red), dim3(kT), b->lds_red, q, b->red.p);
    else hipLaunchKernelGGL(k_tf_reduce_b, dim3(b->g_red, W), dim3(kT), b->lds_red, q, b->red.p);
  }
  if ((tr & 4) && fits_y) hipLaunchKernelGGL(k_prepare_bt, dim3(W, b->g_prep), dim3(kT), b->lds_prep, q, b->prep.p);
  else hipLaunchKernelGGL(k_prepare_b, dim3(b->g_prep, W), dim3(kT), b->lds_prep, q, b->prep.p);
  if ((tr & 8) && fits_y) hipLaunchKernelGGL(k_schur_sp0_bt, dim3(W, b->g_ssp0), dim3(256), b->lds_ssp0, q, b->ssp0.p);
  else hipLaunchKernelGGL(k_schur_sp0_b, dim3(b->g_ssp0, W), dim3(256), b->lds_ssp0, q, b->ssp0.p);
  for (int lv = b->first_own_level; lv < b->max_levels; ++lv)
    if (b->g_sp[lv] > 0) hipLaunchKernelGGL(k_sp_eliminate_b, dim3(b->g_sp[lv], W), dim3(256), b->lds_sp[lv], q, b->sp[lv].p);
  for (int kb = 0; kb < b->max_nb; ++kb) {
    if (tr & 16) hipLaunchKernelGGL(solver_env().chol_subblock ? k_chol_step_bt : k_chol_step_pp_bt, dim3(W, chol_step_grid(b->max_nb, kb)), dim3(kCT), 0, q, b->chol.p, kb);
    else hipLaunchKernelGGL(solver_env().chol_subblock ? k_chol_step_b : k_chol_step_pp_b, dim3(chol_step_grid(b->max_nb, kb), W), dim3(kCT), 0, q, b->chol.p, kb);
  }
  hipLaunchKernelGGL(k_chol_backsolve_b, dim3(1, W), dim3(kBT), b->lds_back, q, b->back.p);
  if ((tr & 32) && b->g_tail <= 65535) hipLaunchKernelGGL(k_step_tail_bt, dim3(W, b->g_tail), dim3(kT), b->lds_tail, q, b->tail.p);
  else hipLaunchKernelGGL(k_step_tail_b, dim3(b->g_tail, W), dim3(kT), b->lds_tail, q, b->tail.p);
  // (batchable windows always have visual blocks)
  if ((tr & 64) && b->g_cost <= 65535) hipLaunchKernelGGL(k_cost_decide_bt, dim3(W, b->g_cost), dim3(kT), 0, q, b->cost.p, b->dec.p, end_zero ? 1 : 0);
  else hipLaunchKernelGGL(k_cost_decide_b, dim3(b->g_cost, W), dim3(kT), 0, q, b->cost.p, b->dec.p, end_zero ? 1 : 0);
  LVF_HIP(hipGetLastError());
  for (lvf_problem* p : b->probs) { p->linearized = !end_zero; p->accum_clean = end_zero; }     // (batchable windows: the cost + decision launch clears them)
  return LVF_OK;
}

}  // namespace lvf

extern "C" {

// ---- batch of windows
int lvf_problem_batch_create(lvf_ctx* ctx, lvf_problem* const* problems, int n, lvf_problem_batch** out) {
  LVF_REQUIRE(ctx && out && n >= 1 && problems, "lvf_problem_batch_create: bad arguments");
  for (int i = 0; i < n; ++i) {
    LVF_REQUIRE(problems[i], "lvf_problem_batch_create: problem %d is null", i);
    LVF_REQUIRE(problems[i]->ctx == ctx, "lvf_problem_batch_create: problem %d belongs to another context", i);
    for (int j = 0; j < i; ++j) LVF_REQUIRE(problems[j] != problems[i] && problems[j]->st != problems[i]->st, "lvf_problem_batch_create: windows %d and %d share state", j, i);
  }
  auto* b = new lvf_problem_batch();
  b->ctx = ctx; b->W = n; b->probs.assign(problems, problems + n);
  for (lvf_problem* p : b->probs) p->batches.push_back(b);
  *out = b;
  return LVF_OK;
}
// (members are only told that the batch is gone: nothing of theirs was changed by it)
int lvf_problem_batch_destroy(lvf_problem_batch* b) {
  if (b && !b->orphaned)
    for (lvf_problem* p : b->probs) p->batches.erase(std::remove(p->batches.begin(), p->batches.end(), b), p->batches.end());
  delete b;
  return LVF_OK;
}
int lvf_problem_batch_size(const lvf_problem_batch* b) { return b ? b->W : -1; }
int lvf_problem_batch_uses_tables(lvf_problem_batch* b, const lvf_solver_options* o) {
  if (!b || !o || lvf::enter(b->ctx) != LVF_OK || batch_build_tables(b, o->huber_a) != LVF_OK) return -1;
  return b->tables ? 1 : 0;
}

// one LM iteration of every window (no tolerance tests); all arrays have one entry per window
int lvf_problem_batch_lm_iteration(lvf_problem_batch* b, const lvf_solver_options* o, double* radius, double* decrease_factor, double* cost_before,
                                   double* cost_after, int* accepted) {
  LVF_REQUIRE(b && o && radius && decrease_factor, "lvf_problem_batch_lm_iteration: null argument");
  LVF_TRY(lvf::enter(b->ctx));
  LVF_TRY(batch_build_tables(b, o->huber_a));
  for (int w = 0; w < b->W; ++w) {
    LVF_REQUIRE(radius[w] > 0.0 && decrease_factor[w] > 0.0, "radius and decrease_factor must be positive");
    LmCtl c;
    ctl_from_options(o, radius[w], decrease_factor[w], 1, false, &c);
    b->probs[w]->huber = o->huber_a;
    LVF_TRY(upload_ctl(b->probs[w], c));
  }
  LVF_TRY(batch_enqueue_iteration(b, false));
  {
    // windows whose chained hand-over timed out repeat the iteration un-chained (the others are done: their launches return at once)
    bool again = false;
    for (int w = 0; w < b->W; ++w) {
      LmCtl c;
      LVF_TRY(download_ctl(b->probs[w], &c));
      if (handover_pending(b->probs[w], c)) { LVF_TRY(rearm_after_handover(b->probs[w], &c)); again = true; }
    }
    if (again) { LVF_TRY(batch_build_tables(b, o->huber_a)); LVF_TRY(batch_enqueue_iteration(b, false)); }
  }
  for (int w = 0; w < b->W; ++w) {
    LmCtl c;
    LVF_TRY(download_ctl(b->probs[w], &c));
    b->probs[w]->last_radius = c.last_radius;
    radius[w] = c.radius; decrease_factor[w] = c.decrease;
    if (cost_before) cost_before[w] = c.cost_before;
    if (cost_after) cost_after[w] = c.cost_after;
    if (accepted) accepted[w] = c.accepted;
  }
  return LVF_OK;
}

int lvf_problem_batch_solve(lvf_problem_batch* b, const lvf_solver_options* o, lvf_solver_summary* summaries) {
  LVF_REQUIRE(b && o && summaries, "lvf_problem_batch_solve: null argument");
  LVF_TRY(lvf::enter(b->ctx));
  LVF_TRY(batch_build_tables(b, o->huber_a));
  if (o->max_num_iterations <= 0) {
    for (int w = 0; w < b->W; ++w) LVF_TRY(lvf_problem_solve(b->probs[w], o, &summaries[w]));
    return LVF_OK;
  }
  for (int w = 0; w < b->W; ++w) {
    LmCtl c;
    ctl_from_options(o, o->initial_trust_region_radius, 2.0, o->max_num_iterations, true, &c);
    b->probs[w]->huber = o->huber_a;
    LVF_TRY(upload_ctl(b->probs[w], c));
  }
  const auto wall0 = std::chrono::steady_clock::now();
  std::vector<LmCtl> cs((size_t)b->W);
  for (int round = 0;; ++round) {
    // (after a hand-over retry the windows stand at different iteration counts: the wait is for "one more than when this pass started")
    int base = o->max_num_iterations;
    for (int w = 0; w < b->W; ++w) if (!b->probs[w]->rec->done) base = std::min(base, (int)b->probs[w]->rec->iter);
    for (int it = base; it < o->max_num_iterations; ++it) {
      LVF_TRY(batch_enqueue_iteration(b, true));
      bool all_done = true;
      for (int w = 0; w < b->W; ++w) {
        if (it >= base + 1) LVF_TRY(wait_for_iteration(b->probs[w], it));
        all_done = all_done && b->probs[w]->rec->done;
      }
      if (all_done) break;
      if (o->max_solver_time_in_seconds > 0.0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() >= o->max_solver_time_in_seconds) break;
    }
    bool again = false;
    for (int w = 0; w < b->W; ++w) {
      LVF_TRY(download_ctl(b->probs[w], &cs[w]));
      if (handover_pending(b->probs[w], cs[w])) { LVF_TRY(rearm_after_handover(b->probs[w], &cs[w])); again = true; }
    }
    if (!again) break;
    LVF_TRY(batch_build_tables(b, o->huber_a));        // the re-armed windows' chains changed shape
  }
  for (int w = 0; w < b->W; ++w) {
    b->probs[w]->last_radius = cs[w].last_radius;
    summary_from_ctl(b->probs[w], cs[w], &summaries[w]);
  }
  return LVF_OK;
}

}  // extern "C"
