// solver_api.hip — the C entry points of a single problem (lvf_problem_*): creation, the solve loop around the chain of solver_chain.hip,
// the stage times, the parity and debug taps.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>

#include "solver_host.hpp"

lvf_problem::~lvf_problem() {
  // a batch that still borrows this problem must never dereference it again: it is marked orphaned (its calls fail with LVF_ERR_STATE)
  // and forgets every member, so destroying it later touches nothing
  for (lvf_problem_batch* b : batches) lvf::batch_orphan(b, this);
  delete chain;
  lvf::stage_clock_free(clk);
  if (rec && !lvf::HostPinPool::get().give(rec, lvf::Pool::bucket(sizeof(lvf::LmCtl)))) (void)hipHostFree(rec);
  if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
  if (ev_band) (void)hipEventDestroy(ev_band);
}

namespace lvf {

static const char* const kStageNames[ST_N] = {"k_zero_multi (only when the accumulators are not known clean)", "k_lin_visual", "k_tf_reduce (+ sparse level 0)", "k_prepare (+ sparse level 1)", "k_schur_sp0 (+ a sparse level)", "k_sp_eliminate (the levels left)",
                                             "k_chol_step (the block steps launched on their own: all of them, or all but the last where the merged last launch is in use)",
                                             "k_chol_backsolve / k_backsolve_tail / k_chol_backsolve_tail (the last block step + the back substitution + the step tail)", "k_step_tail", "k_cost_decide (candidate cost incl. the ImuError factors; its last workgroup closes the iteration; + prior passes)", "k_lm_decide (windows without visual blocks)",
                                             "k_lin_cost_decide (fused chain: linearisation at the candidate + its cost; its last workgroup closes the iteration)"};

void summary_from_ctl(const lvf_problem* p, const LmCtl& c, lvf_solver_summary* s) {
  std::memset(s, 0, sizeof(*s));
  s->num_residual_blocks = (p->tc ? p->tc->n : 0) + (p->tf ? p->tf->n : 0) + (p->po ? p->po->n : 0) + (p->imu ? p->imu->n : 0) + (p->prior ? p->prior->n : 0) +
                           (p->lidar ? p->lidar->n : 0) + (p->dprior ? 1 : 0);
  s->initial_cost = c.initial_cost; s->final_cost = c.cost; s->num_iterations = c.iter; s->num_successful_steps = c.successes; s->termination = c.termination;
  s->num_unsuccessful_steps = c.rejected; s->termination_reason = c.why; s->hand_over_retries = p->handover_retries;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

void lvf_solver_options_default(lvf_solver_options* o) {
  if (!o) return;
  o->max_num_iterations = 50; o->max_solver_time_in_seconds = 0.0; o->huber_a = 1.0;
  o->initial_trust_region_radius = 1e4; o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8; o->min_relative_decrease = 1e-3;
}

int lvf_problem_create(lvf_ctx* ctx, lvf_state* st, lvf_batch* two_camera, lvf_batch* two_frame, lvf_batch* pose_only,
                       lvf_batch* imu, lvf_problem** out) {
  LVF_REQUIRE(ctx && st && out, "lvf_problem_create: null argument");
  LVF_REQUIRE(st->ctx == ctx, "lvf_problem_create: state belongs to another context");
  LVF_REQUIRE(!two_camera || two_camera->kind == LVF_K_TWO_CAMERA, "two_camera batch has the wrong kind");
  LVF_REQUIRE(!two_frame || two_frame->kind == LVF_K_TWO_FRAME, "two_frame batch has the wrong kind");
  LVF_REQUIRE(!pose_only || pose_only->kind == LVF_K_POSE_ONLY, "pose_only batch has the wrong kind");
  LVF_REQUIRE(!imu || imu->kind == LVF_K_IMU, "imu batch has the wrong kind");
  for (lvf_batch* b : {two_camera, two_frame, pose_only, imu})
    if (b) {
      LVF_REQUIRE(b->ctx == ctx, "batch belongs to another context");
      LVF_REQUIRE(b->min_n_kf <= st->n_kf && b->min_n_lm <= st->n_lm, "batch indices exceed the state (n_kf=%d n_lm=%d)", st->n_kf, st->n_lm);
    }
  LVF_REQUIRE(st->n_kf > 0, "lvf_problem_create: empty window");
  LVF_TRY(lvf::enter(ctx));
  auto* p = new lvf_problem();
  p->ctx = ctx; p->st = st; p->tc = two_camera; p->tf = two_frame; p->po = pose_only; p->imu = imu;
  const int rc = problem_configure(p);
  if (rc != LVF_OK) { delete p; return rc; }
  *out = p;
  return LVF_OK;
}
int lvf_problem_destroy(lvf_problem* p) { delete p; return LVF_OK; }

int lvf_problem_set_pose_priors(lvf_problem* p, lvf_batch* pose_priors) {
  LVF_REQUIRE(p, "lvf_problem_set_pose_priors: null problem");
  if (pose_priors) {
    LVF_REQUIRE(pose_priors->kind == LVF_K_POSE_PRIOR, "pose_priors batch has the wrong kind");
    LVF_REQUIRE(pose_priors->ctx == p->ctx, "batch belongs to another context");
    LVF_REQUIRE(pose_priors->min_n_kf <= p->n_kf, "pose-prior batch references keyframe %d but the window has %d", pose_priors->min_n_kf - 1, p->n_kf);
  }
  p->prior = pose_priors;
  p->linearized = false;
  p->chain_ready = false;
  return LVF_OK;
}

int lvf_problem_set_lidar_planes(lvf_problem* p, lvf_batch* lidar_planes) {
  LVF_REQUIRE(p, "lvf_problem_set_lidar_planes: null problem");
  if (lidar_planes) {
    LVF_REQUIRE(lidar_planes->kind == LVF_K_LIDAR_POSE, "lidar_planes batch has the wrong kind");
    LVF_REQUIRE(lidar_planes->ctx == p->ctx, "batch belongs to another context");
    LVF_REQUIRE(lidar_planes->min_n_kf <= p->n_kf, "lidar-plane batch references keyframe %d but the window has %d", lidar_planes->min_n_kf - 1, p->n_kf);
  }
  p->lidar = lidar_planes;
  p->linearized = false;
  p->chain_ready = false;
  return LVF_OK;
}

int lvf_problem_set_vbb_constant(lvf_problem* p, int kf, int v_constant, int ba_constant, int bg_constant) {
  LVF_REQUIRE(p, "null problem");
  LVF_REQUIRE(kf >= 0 && kf < p->n_kf, "keyframe %d out of range", kf);
  p->pose_const_h[kf] = (uint8_t)((p->pose_const_h[kf] & 1) | (v_constant ? 2 : 0) | (ba_constant ? 4 : 0) | (bg_constant ? 8 : 0));
  LVF_HIP(hipMemcpyAsync(p->pose_const.p, p->pose_const_h.data(), p->n_kf, hipMemcpyHostToDevice, p->ctx->stream));
  LVF_HIP(hipStreamSynchronize(p->ctx->stream));
  return LVF_OK;
}

int lvf_problem_set_pose_constant(lvf_problem* p, int kf, int is_constant) {
  LVF_REQUIRE(p, "null problem");
  LVF_REQUIRE(kf >= 0 && kf < p->n_kf, "keyframe %d out of range", kf);
  p->pose_const_h[kf] = (uint8_t)((p->pose_const_h[kf] & ~1) | (is_constant ? 1 : 0));
  LVF_HIP(hipMemcpyAsync(p->pose_const.p, p->pose_const_h.data(), p->n_kf, hipMemcpyHostToDevice, p->ctx->stream));
  LVF_HIP(hipStreamSynchronize(p->ctx->stream));
  return LVF_OK;
}

int lvf_problem_cost(lvf_problem* p, const lvf_solver_options* o, double* cost) {
  LVF_REQUIRE(p && o && cost, "lvf_problem_cost: null argument");
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  LVF_HIP(hipMemsetAsync(p->scal.p, 0, SC_N * 8, q));
  LVF_TRY(enqueue_cost(p, state_ptrs(p->st), p->st, o->huber_a, p->scal.p + SC_COST));
  double hc[kStripes];
  LVF_HIP(hipMemcpyAsync(hc, p->scal.p + SC_COST, sizeof(hc), hipMemcpyDeviceToHost, q));
  // the stripes go back to zero: a following linearisation that trusts `accum_clean` (after a device-loop solve nothing else clears
  // SC_COST) adds its cost into them — solve -> cost -> solve would otherwise start from a doubled cost_before
  LVF_HIP(hipMemsetAsync(p->scal.p + SC_COST, 0, kStripes * 8, q));
  LVF_HIP(hipStreamSynchronize(q));
  *cost = stripe_sum(hc, 0);
  return LVF_OK;
}

int lvf_problem_stage_count(void) { return ST_N; }
const char* lvf_problem_stage_name(int stage) { return stage >= 0 && stage < ST_N ? kStageNames[stage] : ""; }

// `reps` LM iterations from the problem's current state (they ARE iterations: accepted steps move the state), HIP events on the
// library's stream between the stages; us[k] = average duration of stage k, launches[k] = kernel launches it consists of.
int lvf_problem_stage_times2(lvf_problem* p, const lvf_solver_options* o, double radius, int reps, double* us, double* spans_us, int* launches) {
  LVF_REQUIRE(p && o && us && reps > 0, "lvf_problem_stage_times: bad argument");
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  if (!p->clk) {
    p->clk = new StageClock();
    for (auto& r : p->clk->ev) for (auto& e : r) LVF_HIP(hipEventCreate(&e));
    for (auto& r : p->clk->kstart) for (auto& e : r) LVF_HIP(hipEventCreate(&e));
    for (auto& r : p->clk->kstop) for (auto& e : r) LVF_HIP(hipEventCreate(&e));
    p->clk->kernel_events = true;
  }
  StageClock& k = *p->clk;
  for (int i = 0; i < ST_N; ++i) { us[i] = 0.0; k.launches[i] = 0; }
  std::vector<double> span(ST_N, 0.0), kern(ST_N, 0.0);
  std::vector<int> kcount(ST_N, 0);
  reps = std::min(reps, kClockReps);
  LmCtl c;
  ctl_from_options(o, radius, 2.0, reps + 2, false, &c);
  p->huber = o->huber_a;
  LVF_TRY(upload_ctl(p, c));
  // the device loop's chain: with the fused chain every timed iteration starts at k_tf_reduce and ends with the candidate pass
  const bool fz = p->chain->fused_ok && !p->no_chain;
  if (fz) LVF_TRY(ensure_acc1(p));
  LVF_TRY(enqueue_iteration(p, true, fz ? kFusedOn | kFusedTail : 0));             // (un-timed: the timed iterations queue up behind it)
  int nk = 0;
  for (int r = 0; r < reps; ++r) {
    k.on = true; k.rep = r; k.nk = 0;
    const int rc = enqueue_iteration(p, true, fz ? kFusedOn | kFusedNoLin | kFusedTail : 0);
    k.on = false;
    nk = k.nk;
    LVF_TRY(rc);
  }
  if (fz) LVF_TRY(enqueue_iteration(p, true, kFusedOn | kFusedNoLin));          // (un-timed: the plain cost pass leaves both accumulator sets clean)
  LVF_HIP(hipStreamSynchronize(q));
  for (int r = 0; r < reps; ++r) {
    for (int i = 0; i < ST_N; ++i) {
      if (k.launches[i] == 0) continue;
      int prev = i;                                   // the event after the closest earlier stage that launched something (or event 0)
      while (prev > 0 && k.launches[prev - 1] == 0) --prev;
      float ms = 0.f;
      LVF_HIP(hipEventElapsedTime(&ms, k.ev[r][prev], k.ev[r][i + 1]));
      span[i] += 1e3 * (double)ms / reps;
    }
    for (int j = 0; j < nk; ++j) {                    // the kernels' own durations (dispatch timestamps)
      float ms = 0.f;
      LVF_HIP(hipEventElapsedTime(&ms, k.kstart[r][j], k.kstop[r][j]));
      kern[k.kstage[j]] += 1e3 * (double)ms / reps;
      if (r == 0) kcount[k.kstage[j]] += 1;
    }
  }
  // a stage whose launches all carried their own events reports the sum of the kernel durations; others (generic paths: stand-alone IMU /
  // prior passes) keep the between-stage span
  for (int i = 0; i < ST_N; ++i) us[i] = (k.launches[i] > 0 && kcount[i] == k.launches[i]) ? kern[i] : span[i];
  if (spans_us) for (int i = 0; i < ST_N; ++i) spans_us[i] = span[i];
  if (launches) for (int i = 0; i < ST_N; ++i) launches[i] = k.launches[i];
  return LVF_OK;
}
int lvf_problem_stage_times(lvf_problem* p, const lvf_solver_options* o, double radius, int reps, double* us, int* launches) {
  return lvf_problem_stage_times2(p, o, radius, reps, us, nullptr, launches);
}

// Problem::Evaluate's gradient: J^T r with the loss function's Corrector applied and pose blocks in tangent coordinates, at the current
// state — exactly what the linearisation accumulates.  gc [15 n_kf] in the reduced-system order (6 x n_kf pose tangents | 9 x n_kf (v, ba, bg)),
// gl [n_lm] (may be NULL) the inverse-depth entries.
int lvf_problem_gradient(lvf_problem* p, const lvf_solver_options* o, double* gc, double* gl) {
  LVF_REQUIRE(p && o && gc, "lvf_problem_gradient: null argument");
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  LVF_TRY(enqueue_linearize(p, o->huber_a, false));
  const double* gr = p->gr.p;
  if (gl && p->n_lm && p->compact) {
    // atomic-free linearisation: a landmark's gradient entry is completed from its slot records by k_prepare (grt = gr + the slots)
    LmCtl c;
    ctl_from_options(o, o->initial_trust_region_radius, 2.0, 1, false, &c);
    LVF_TRY(upload_ctl(p, c));
    PrepArgs pa = p->chain->prep;
    pa.radius = &p->ctl.p->radius; pa.scal = nullptr; pa.done = nullptr;
    hipLaunchKernelGGL(k_prepare, dim3(pa.nblocks), dim3(kT), 0, q, pa);
    LVF_HIP(hipGetLastError());
    gr = p->grt.p;
  }
  LVF_HIP(hipMemcpyAsync(gc, p->gc.p, (size_t)p->d * 8, hipMemcpyDeviceToHost, q));
  if (gl && p->n_lm) LVF_HIP(hipMemcpyAsync(gl, gr, (size_t)p->n_lm * 8, hipMemcpyDeviceToHost, q));
  LVF_HIP(hipStreamSynchronize(q));
  return LVF_OK;
}

int lvf_problem_lm_iteration(lvf_problem* p, const lvf_solver_options* o, double* radius, double* decrease_factor,
                             double* cost_before, double* cost_after, int* accepted) {
  LVF_REQUIRE(p && o && radius && decrease_factor, "lvf_problem_lm_iteration: null argument");
  LVF_REQUIRE(*radius > 0.0 && *decrease_factor > 0.0, "radius and decrease_factor must be positive");
  LVF_TRY(lvf::enter(p->ctx));
  IterOut it;
  LVF_TRY(lm_iteration(p, o, radius, decrease_factor, &it));
  if (cost_before) *cost_before = it.cost_before;
  if (cost_after) *cost_after = it.cost_after;
  if (accepted) *accepted = it.accepted ? 1 : 0;
  return LVF_OK;
}

// The device LM loop: iterations are enqueued back to back, each closed on device (k_lm_decide); the host only watches a mirror of the
// control block to stop enqueueing once the loop has finished (an iteration enqueued after the end costs ~20 empty launches).
int lvf_problem_solve(lvf_problem* p, const lvf_solver_options* o, lvf_solver_summary* summary) { return lvf_problem_solve_then(p, o, summary, nullptr, nullptr); }

// lvf_problem_solve with a caller's launches enqueued BEHIND the last iteration and AHEAD of the wait that ends the solve (`tail(user)`,
// called once per pass of the hand-over retry loop, i.e. once in practice): the persistent window packs and copies its state back in
// the same stream wait instead of a second one (window.hip).
int lvf_problem_solve_then(lvf_problem* p, const lvf_solver_options* o, lvf_solver_summary* summary, int (*tail)(void*), void* user) {
  LVF_REQUIRE(p && o && summary, "lvf_problem_solve: null argument");
  LVF_TRY(lvf::enter(p->ctx));
  LmCtl c;
  ctl_from_options(o, o->initial_trust_region_radius, 2.0, o->max_num_iterations, true, &c);
  p->huber = o->huber_a;
  if (o->max_num_iterations <= 0) {          // nothing to iterate: report the cost at the start
    double cost = 0.0;
    LVF_TRY(lvf_problem_cost(p, o, &cost));
    c.initial_cost = c.cost = cost;
    summary_from_ctl(p, c, summary);
    if (tail) LVF_TRY(tail(user));
    return LVF_OK;
  }
  // a problem that lost its chained launches to a hand-over time-out gets them back after kUnchainedSolves solves (a time-out then simply sets it again)
  constexpr int kUnchainedSolves = 32;
  if (p->no_chain && ++p->unchained_solves > kUnchainedSolves && p->force_handover_timeouts == 0) { p->no_chain = false; p->unchained_solves = 0; p->chain_ready = false; }
  LVF_TRY(upload_ctl(p, c));
  const auto wall0 = std::chrono::steady_clock::now();
  bool timed_out = false;
  for (int first = 0;;) {
    // the fused chain (Chain::fused_ok): the pass's first iteration linearises at the state as today, every later one starts from the
    // linearisation the previous iteration's candidate pass made, and the last one enqueued for the solve ends with the plain cost pass (a
    // re-run after a hand-over time-out takes today's chain: no_chain)
    const bool fz = p->chain->fused_ok && !p->no_chain && !p->ov && o->max_num_iterations - first >= 2;
    if (fz) LVF_TRY(ensure_acc1(p));
    bool fused_tail = false;
    for (int it = first; it < o->max_num_iterations; ++it) {
      const int f = fz ? kFusedOn | (it > first ? kFusedNoLin : 0) | (it + 1 < o->max_num_iterations ? kFusedTail : 0) : 0;
      LVF_TRY(enqueue_iteration(p, true, f));
      fused_tail = (f & kFusedTail) != 0;
      if (it >= first + 1) LVF_TRY(wait_for_iteration(p, it));          // iteration it-1 is closed; iteration `it` keeps the device busy meanwhile
      if (p->rec->done) break;
      if (o->max_solver_time_in_seconds > 0.0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() >= o->max_solver_time_in_seconds) { timed_out = true; break; }
    }
    if (fused_tail) {
      // the loop ended before the last iteration: the active set was not cleared by a plain cost pass — both sets are, here, with the cost stripes
      const Chain& ch = *p->chain;
      ZeroList z = ch.stand0;
      for (int k = 0; k < ch.stand1.count && z.count < kZeroListMax; ++k) { z.p[z.count] = ch.stand1.p[k]; z.n[z.count] = ch.stand1.n[k]; z.tri[z.count] = ch.stand1.tri[k]; ++z.count; }
      hipLaunchKernelGGL(k_zero_multi, dim3(512, z.count), dim3(kT), 0, p->ctx->stream, z);
      LVF_HIP(hipGetLastError());
      LVF_HIP(hipMemsetAsync(p->scal.p + SC_COST, 0, kStripes * 8, p->ctx->stream));
      p->accum_clean = ch.stand0.count + ch.stand1.count <= kZeroListMax;
    }
    // the caller's launches ride behind the last iteration — unless the host already KNOWS this pass ended in a hand-over time-out (the mirror
    // carries `why`): the state is not final then, the re-run's pass enqueues them.  (A time-out in the very last iteration enqueued is only
    // seen after the wait: the tail then runs twice, the second time on the final state.)
    const bool known_handover = p->rec->done && p->rec->why == LVF_WHY_HANDOVER && !p->no_chain;
    if (tail && !known_handover) LVF_TRY(tail(user));
    LVF_TRY(download_ctl(p, &c));
    if (!handover_pending(p, c)) break;
    LVF_TRY(rearm_after_handover(p, &c));     // a chained hand-over timed out: the loop goes on from the same point, un-chained
    first = c.iter;
  }
  p->last_radius = c.last_radius;
  p->step_ready = true; p->last_solved = c.solved;
  summary_from_ctl(p, c, summary);
  if (timed_out && !c.done) summary->termination_reason = LVF_WHY_TIME;
  return LVF_OK;
}

int lvf_problem_reduced_dim(lvf_problem* p) { return p ? p->d : -1; }

// the DAMPED reduced system of the last lm_iteration, rebuilt (the factorisation overwrote S): S [d x d] symmetric, rhs [d]
int lvf_problem_download_reduced(lvf_problem* p, double* S, double* rhs) {
  LVF_REQUIRE(p && S && rhs, "lvf_problem_download_reduced: null argument");
  if (!p->linearized || !p->chain_ready) { set_error("no linearisation yet"); return LVF_ERR_STATE; }
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  const size_t nS = (size_t)p->ld * p->ld;
  LVF_TRY(enqueue_reduced_system(p, &p->ctl.p->last_radius, false, false, nullptr));
  std::vector<double> h(nS);
  LVF_HIP(hipMemcpyAsync(h.data(), p->S.p, nS * 8, hipMemcpyDeviceToHost, q));
  LVF_HIP(hipStreamSynchronize(q));
  const int d = p->d, ld = p->ld;
  const std::vector<int>& pm = p->perm_h;          // natural unknown -> S row
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) {
      const double v = h[(size_t)std::max(pm[i], pm[j]) * ld + std::min(pm[i], pm[j])];
      S[(size_t)i * d + j] = v; S[(size_t)j * d + i] = v;
    }
  for (int j = 0; j < d; ++j) rhs[j] = h[(size_t)p->aug * ld + pm[j]];
  return LVF_OK;
}

// test tap (see lvf.h): the caller's reduced system replaces the assembled one in every iteration of this problem; both NULL clears it
int lvf_problem_debug_override_reduced(lvf_problem* p, const double* S, const double* rhs) {
  LVF_REQUIRE(p, "lvf_problem_debug_override_reduced: null problem");
  LVF_REQUIRE((S == nullptr) == (rhs == nullptr), "lvf_problem_debug_override_reduced: S and rhs must both be given, or both be NULL (clear)");
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  if (!S) {
    LVF_HIP(hipStreamSynchronize(q));          // (launches that read the copies may still be in flight)
    p->ov.reset();
    return LVF_OK;
  }
  LVF_REQUIRE(p->d > 0, "lvf_problem_debug_override_reduced: the problem has no unknowns");
  std::unique_ptr<ReducedOverride> ov(new ReducedOverride());
  ov->d = p->d;
  LVF_TRY(ov->S.upload(S, (size_t)p->d * p->d, q));
  LVF_TRY(ov->rhs.upload(rhs, (size_t)p->d, q));
  LVF_HIP(hipStreamSynchronize(q));            // the caller's arrays are free from here on (and the previous copies are no longer read)
  p->ov = std::move(ov);
  return LVF_OK;
}
// the reduced step of the last iteration (natural order, the coordinates of the system: the chain solves the unscaled system, the Jacobi
// scaling only enters the damping) and the raw SC_FAIL flag
int lvf_problem_debug_download_step(lvf_problem* p, double* x, int* fail) {
  LVF_REQUIRE(p && x && fail, "lvf_problem_debug_download_step: null argument");
  if (!p->step_ready) { set_error("lvf_problem_debug_download_step: no iteration yet"); return LVF_ERR_STATE; }
  LVF_TRY(lvf::enter(p->ctx));
  hipStream_t q = p->ctx->stream;
  LVF_HIP(hipMemcpyAsync(x, p->dxc.p, (size_t)p->d * 8, hipMemcpyDeviceToHost, q));
  LVF_HIP(hipMemcpyAsync(fail, reinterpret_cast<const int*>(p->scal.p + SC_FAIL), sizeof(int), hipMemcpyDeviceToHost, q));
  LVF_HIP(hipStreamSynchronize(q));
  return LVF_OK;
}
int lvf_problem_debug_last_solved(lvf_problem* p) { return (p && p->step_ready) ? p->last_solved : -1; }
// the layout the elimination plan gave the factorised matrix: block steps of the dense corner; per keyframe, whether its (v, ba, bg) block stayed there
int lvf_problem_debug_plan(lvf_problem* p, int* nb, int* dense_kf) {
  LVF_REQUIRE(p && nb, "lvf_problem_debug_plan: null argument");
  if ((int)p->perm_h.size() < p->d || p->d != 15 * p->n_kf) { set_error("lvf_problem_debug_plan: no elimination plan yet"); return LVF_ERR_STATE; }
  *nb = p->nb;
  if (dense_kf) for (int k = 0; k < p->n_kf; ++k) dense_kf[k] = p->perm_h[(size_t)p->dp + 9 * k] >= p->off ? 1 : 0;
  return LVF_OK;
}
int lvf_debug_landmark_window(void) { return 16 * kLmEPre; }
void lvf_debug_fail_codes(int* sparse_base, int* handover_base) {
  if (sparse_base) *sparse_base = kFailSparse;
  if (handover_base) *handover_base = kFailHandover;
}
// diagnostic (LVF_LM_HISTORY=1): {iteration, cost_before, cost_new, model, accepted, fail flag, radius, gradient max} of the passes of the last solve
int lvf_problem_debug_history(lvf_problem* p, double* out512) {
  LVF_REQUIRE(p && out512, "lvf_problem_debug_history: null argument");
  if (!p->dbg_hist.p) { set_error("lvf_problem_debug_history: LVF_LM_HISTORY is not set"); return LVF_ERR_STATE; }
  LVF_TRY(lvf::enter(p->ctx));
  LVF_HIP(hipMemcpyAsync(out512, p->dbg_hist.p, 512 * 8, hipMemcpyDeviceToHost, p->ctx->stream));
  LVF_HIP(hipStreamSynchronize(p->ctx->stream));
  return LVF_OK;
}
// 1: the current chain runs the dense back substitution on the stored block products T_kj, 0: on S and Dinv (builds the chain if stale)
int lvf_problem_debug_back_blocks(lvf_problem* p) {
  if (!p || lvf::enter(p->ctx) != LVF_OK) return -1;
  if (chain_stale(p) && build_chain(p) != LVF_OK) return -1;
  return p->chain->back_blocks ? 1 : 0;
}
// 1: the current chain takes the sparse back substitution as a product with G, 0: it runs the sequential levels (builds the chain if stale)
int lvf_problem_debug_back_product(lvf_problem* p) {
  if (!p || lvf::enter(p->ctx) != LVF_OK) return -1;
  if (chain_stale(p) && build_chain(p) != LVF_OK) return -1;
  return p->chain->back_product ? 1 : 0;
}
// test hook (see lvf.h)
int lvf_problem_debug_force_handover_timeout(lvf_problem* p, int n) {
  LVF_REQUIRE(p && n >= 0, "lvf_problem_debug_force_handover_timeout: bad argument");
  p->force_handover_timeouts = n; p->no_chain = false; p->chain_ready = false;
  return LVF_OK;
}

}  // extern "C"
