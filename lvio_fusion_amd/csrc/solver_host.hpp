// solver_host.hpp — what the host-side files of the LM chain share: the argument blocks of one iteration (Chain), the stage clock, and the
// functions called across them.  solver_chain.hip builds and enqueues the chain and drives the LM loop; solver_plan.hip makes the elimination
// plan and configures a problem; solver_batch.hip advances a batch of windows; solver_api.hip holds the C entry points.
#pragma once
#include "solver_args.hpp"

namespace lvf {

static inline StateP state_ptrs(const lvf_state* st) { return StateP{st->poses.p, st->vel.p, st->ba.p, st->bg.p, st->inv_depth.p, st->w_visual.p}; }
static inline int grid(int n) { return (n + kT - 1) / kT; }
static inline int band_rows_clamped(int rows) { return std::min(kBandRowsMax, std::max(16, rows)); }

// The argument blocks of ONE LM iteration of a window.  Nothing in them changes from iteration to iteration (the trust-region radius,
// the accept / reject state and the termination flag live in the device-resident LmCtl; an accepted candidate is COPIED into the state
// buffers by k_lm_decide), so they are built once per problem_configure and
//   * passed by value to the single-window launches, or
//   * stored as one entry per window in device tables, every launch of the chain then covering a whole batch of windows (blockIdx.y).
struct Chain {
  bool fast = false;            // merged linearisation (sorted TwoFrame work list) available
  bool batchable = false;       // every launch of the iteration has a table form (fast + band Schur merged with sparse level 0 + no priors)
  bool has_imu = false, has_prior = false, imu_in_cost = false;
  ZeroList zero_end{};
  ZeroList zero{};              // everything a linearisation accumulates into (explicit k_zero_multi when the accumulators are not known clean)
  ImuArgs imu_lin{}, imu_cost{};
  LinArgs lin{}; size_t lin_lds = 0;
  TfReduceArgs red{}; size_t red_lds = 0;     // compact mode: the slabs of the TwoFrame linearisation -> B, gc
  PrepArgs prep{};              // classic form (stores the whole lower triangle); also what the parity taps use
  // Early sparse levels.  The (v, ba, bg) columns only ever receive ImuError terms, the LM damping and the updates of lower levels, so a
  // level can form its columns from B itself (SpSrc) as soon as the linearisation launch is over: level 0 rides in the k_tf_reduce
  // launch, level 1 in k_prepare's, level 2 in the Schur complement's, and only what is left takes launches of its own (at 50 keyframes
  // two instead of four).  For that S is cleared with the accumulators and k_prepare ADDS the dense corner (prep_early).
  bool early = false;
  PrepArgs prep_early{}; size_t prep_lds = 0;
  int first_own_level = 0;      // sparse levels [first_own_level, n_levels) are launches of their own
  bool merged_level0 = false;
  SchurSp0Args ssp0{}; size_t ssp0_lds = 0;
  int n_levels = 0; SpArgs sp[kSpMaxLevels]; int sp_lds[kSpMaxLevels] = {0};
  CholArgs chol{};
  BackArgs back{}; size_t back_lds = 0;
  TailArgs tail{}; size_t tail_lds = 0;
  bool back_tail_merged = false; BackTailArgs bt{}; size_t bt_lds = 0;      // k_backsolve_tail (single-window chain, chained levels allowed)
  // the sparse back substitution as ONE product with G, formed by riders of the block-step launches (GRide; LVF_BACK_PRODUCT=0 turns it off)
  bool back_product = false; GRide gride{};
  // the dense back substitution on stored block products T_kj, formed by riders of the block-step launches (TRide; LVF_BACK_BLOCKS=0 turns it off)
  bool back_blocks = false; TRide tride{};
  CostArgs cost{};
  DecideArgs dec{};
  // the fused chain (AccSel; LVF_FUSED_LIN=0 turns it off): the second accumulator set's pointers and the standby clears (k_tf_reduce: stand0
  // clears set 0, stand1 set 1) — both filled by ensure_acc1 — and the candidate pass
  bool fused_ok = false;
  AccSel acc{};
  ZeroList stand0{}, stand1{};
  FusedArgs fused{};
};

// HIP events between the stages of one LM iteration (lvf_problem_stage_times): event 0 before the first launch, event k + 1 after stage k
// (the stages' names: kStageNames in solver_api.hip)
enum { ST_IMU_LIN = 0, ST_LIN_VISUAL, ST_TF_REDUCE, ST_PREPARE, ST_SCHUR_SP0, ST_SP_LEVELS, ST_CHOL, ST_BACKSOLVE, ST_STEP_TAIL, ST_COST, ST_DECIDE, ST_FUSED, ST_N };
// (one event set per timed iteration: the iterations are enqueued back to back and waited for ONCE, so every stage — the first one of an
// iteration included — starts behind a busy queue like in the device loop; with a wait per iteration the first stage absorbed the idle
// queue's start-up, ~6 us of k_lin_visual's figure)
constexpr int kClockReps = 16, kClockLaunches = 48;
// Two sources per timed iteration: ev[] — events between the STAGES on the stream (a span: kernels + the gaps between them + the marker's own
// cost) — and kstart[] / kstop[] — a start / stop event pair recorded WITH every kernel launch of the fast chain (hipExtLaunchKernelGGL: the
// dispatch packet's own timestamps, i.e. what rocprofv3 --kernel-trace reports as the kernel's duration).  Stage times are the sums of the
// second kind, so bench.py's roofline entries follow profiles/ for short stages too (the event-pair subtraction left k_lin_visual 18 % high).
struct StageClock {
  hipEvent_t ev[kClockReps][ST_N + 1]; int launches[ST_N]; bool on = false; int rep = 0;
  hipEvent_t kstart[kClockReps][kClockLaunches], kstop[kClockReps][kClockLaunches]; int kstage[kClockLaunches]; int nk = 0; bool kernel_events = false;
};

// one complete LM iteration of one window on its stream (enqueue_iteration in solver_chain.hip)
// `fused` (Chain::fused_ok, a device-loop solve only): kFusedOn = every launch selects its accumulator set on device; kFusedNoLin = the iteration
// starts at k_tf_reduce (the last one's candidate pass linearised); kFusedTail = it ends with the candidate pass k_lin_cost_decide
enum { kFusedOn = 1, kFusedNoLin = 2, kFusedTail = 4 };

struct IterOut { double cost_before, cost_after, model, dxnorm, xnorm, gmax; bool accepted, solved; };

// ---- solver_chain.hip
bool chol_subblock_on();      // LVF_CHOL_SUBBLOCK=0: the pair-pivot sweep of the dense Cholesky (k_chol_step_pp*) instead of the 16-pivot sub-block sweep
void stage_clock_free(StageClock* k);
int enqueue_cost(lvf_problem* p, const StateP& s, const lvf_state* imu_state_view, double huber, double* cost_slot);
int build_band_work(lvf_problem* p, int rows_in, DevBuf<int4>& work, int* n_work, bool defer = false);
int await_band_work(lvf_problem* p);
int build_chain(lvf_problem* p);
bool chain_stale(const lvf_problem* p);
int ensure_acc1(lvf_problem* p);
int enqueue_linearize(lvf_problem* p, double huber, bool gated, bool iteration = false, const AccSel* acc = nullptr, bool lin = true);
int enqueue_reduced_system(lvf_problem* p, const double* radius_dev, bool reset_scalars, bool gated, bool* level0_done, const AccSel* acc = nullptr);
int enqueue_iteration(lvf_problem* p, bool end_zero, int fused = 0);
void ctl_from_options(const lvf_solver_options* o, double radius, double decrease, int max_iters, bool with_tolerances, LmCtl* c);
int upload_ctl(lvf_problem* p, const LmCtl& c);
int download_ctl(lvf_problem* p, LmCtl* out);
bool handover_pending(const lvf_problem* p, const LmCtl& c);
int rearm_after_handover(lvf_problem* p, LmCtl* c);
int lm_iteration(lvf_problem* p, const lvf_solver_options* o, double* radius, double* decrease, IterOut* out);
int wait_for_iteration(lvf_problem* p, int iter);
// ---- solver_batch.hip
void batch_orphan(lvf_problem_batch* b, lvf_problem* dying);
// ---- solver_api.hip
void summary_from_ctl(const lvf_problem* p, const LmCtl& c, lvf_solver_summary* s);

}  // namespace lvf
