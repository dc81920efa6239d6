// solver_host.hpp — what the host-side files of the LM chain share: the argument blocks of one iteration (Chain), the stage clock, and the
// functions called across them.  solver_chain.hip builds and enqueues the chain and drives the LM loop; solver_plan.hip makes the elimination
// plan and configures a problem; solver_batch.hip advances a batch of windows; solver_api.hip holds the C entry points.
#pragma once
#include "solver_args.hpp"

namespace lvf {

static inline StateP state_ptrs(const lvf_state* st) { return StateP{st->poses.p, st->vel.p, st->ba.p, st->bg.p, st->inv_depth.p, st->w_visual.p}; }
static inline int grid(int n) { return (n + kT - 1) / kT; }
static inline int band_rows_clamped(int rows) { return std::min(kBandRowsMax, std::max(16, rows)); }

// The solver's environment switches: every LVF_* value that solver_chain.hip, solver_plan.hip and solver_batch.hip read — one
// field per name, filled once per process when the solver is first used (solver_env()).  "unless 0": on unless the value starts with '0';
// "if set": on when the variable exists, whatever its value; integers go through atoi.
struct SolverEnv {
  // ---- forms of the chain (the defaults are the production chain; the other forms are also reached by problem shape)
  bool sparse_vb;             // LVF_SPARSE_VB        unless 0   the (v, ba, bg) blocks eliminated level by level ahead of the dense Cholesky
  int force_levels;           // LVF_FORCE_LEVELS     0          > 0: at most this many sparse levels (experiment)
  bool schur_band;            // LVF_SCHUR_BAND       unless 0   band-limited Schur complement over sorted landmark tracks
  bool compact;               // LVF_COMPACT          unless 0   atomic-free TwoFrame linearisation (slabs and track slots, summed by k_tf_reduce / k_prepare)
  bool tf_k1sort;             // LVF_TF_K1SORT        unless 0   TwoFrame blocks of a current keyframe ordered by first keyframe
  bool staged;                // LVF_STAGED           unless 0   segmented first-keyframe sums through the wave's LDS stage (TfCompact::staged)
  bool zero_tri;              // LVF_ZERO_TRI         unless 0   clears of lower-triangular accumulators skip the upper blocks
  bool early_levels;          // LVF_EARLY_LEVELS     unless 0   sparse levels ride in k_tf_reduce / k_prepare / the Schur launch; off when LVF_POISON_S is set
  int ride_tf, ride_prep;     // LVF_RIDE_TF / _PREP  -1         >= 0 forces a level to ride (non-zero) or not (0) in k_tf_reduce / k_prepare; -1: by the plan
  int chain_levels;           // LVF_CHAIN_LEVELS     2          clamped to 0..2: levels chained inside one launch; the merged back substitution needs > 0
  int chain_fence;            // LVF_CHAIN_FENCE      1          0 relaxed hand-over between chained levels, otherwise fenced; 2: full release in k_backsolve_tail too
                              //                                 (atoi for both uses: text that is no number counts as 0, "02" as 2)
  unsigned chain_timeout_ticks; // LVF_CHAIN_TIMEOUT_US 500      how long a chained workgroup waits for its hand-over, kept in 100 MHz ticks (at least 1 us)
  bool chain_rmw_read;        // LVF_CHAIN_RMW_READ   if set     chained levels read by returning atomics instead of agent-scope loads (SpSrc::rmw_read)
  bool chol_subblock;         // LVF_CHOL_SUBBLOCK    unless 0   16-pivot sub-block sweep of the dense Cholesky (k_chol_step*); 0: pair-pivot sweep (k_chol_step_pp*)
  bool back_tail_merge;       // LVF_BACK_TAIL_MERGE  unless 0   back substitution and step tail as one launch (k_backsolve_tail)
  bool back_product;          // LVF_BACK_PRODUCT     unless 0   sparse back substitution as one product with G (GRide)
  bool back_blocks;           // LVF_BACK_BLOCKS      unless 0   dense back substitution on stored block products T_kj (TRide)
  bool back_early;            // LVF_BACK_EARLY       unless 0   landmark and pose workgroups of k_backsolve_tail request their operands ahead of the wait
  bool chol_back_merge;       // LVF_CHOL_BACK_MERGE  unless 0   the last block step and k_backsolve_tail as one launch (k_chol_backsolve_tail); 0: two launches (A/B)
  bool fused_lin;             // LVF_FUSED_LIN        unless 0   candidate pass linearises (k_lin_cost_decide, two accumulator sets)
  // ---- launch shapes (A/B)
  int tail_wgs;               // LVF_TAIL_WGS         640        cap on the landmark workgroups of k_step_tail
  int back_tail_wgs;          // LVF_BACK_TAIL_WGS    224        cap on the landmark workgroups of k_backsolve_tail (at least 1); set: that kernel's shape is
                              //                                 the experiment, so k_chol_backsolve_tail (which sizes its own grid) stays off
  bool back_tail_wgs_set;
  int cost_tiles;             // LVF_COST_TILES       2          tiles of kT blocks per workgroup of the candidate-cost pass
  size_t lin_lds_pad;         // LVF_LIN_LDS_PAD      0          bytes of dynamic LDS added to k_lin_visual (fewer workgroups per CU)
  int batch_band_rows;        // LVF_BATCH_BAND_ROWS  128        landmark rows per slice of a batch's band Schur complement
  int batch_transpose;        // LVF_BATCH_TRANSPOSE  127        bit per table launch of a batch: window index in blockIdx.x (transposed) instead of .y
  // ---- diagnostics
  bool poison_s;              // LVF_POISON_S         if set     S filled with NaN bytes before each reduced system (proves every entry is written)
  bool chain_info;            // LVF_CHAIN_INFO       if set     build_chain prints the chain's form ("chain: ..." on stderr)
  bool lm_history;            // LVF_LM_HISTORY       if set     the decision records its scalars per iteration (DecideArgs::hist)
  bool configure_timing;      // LVF_CONFIGURE_TIMING if set     problem_configure prints its phases' host times
  // (phase stamps: written by the stage's kernels into a debug buffer and printed on stderr; the enqueue and the read-back test the same field)
  bool lin_timing;            // LVF_LIN_TIMING       if set     phase stamps of k_lin_visual's TwoFrame workgroups and waves
  bool schur_timing;          // LVF_SCHUR_TIMING     if set     phase stamps of the band Schur complement's workgroups
  bool sp_timing;             // LVF_SP_TIMING        if set     phase stamps of the early sparse levels
  bool chol_timing;           // LVF_CHOL_TIMING      if set     phase stamps of the first 8 block steps of the dense Cholesky
  bool back_timing;           // LVF_BACK_TIMING      if set     phase stamps of the back substitution
  bool cost_timing;           // LVF_COST_TIMING      if set     phase stamps of the candidate-cost pass and the decision
};
inline const SolverEnv& solver_env() {
  static const SolverEnv env = [] {
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    auto unless0 = [](const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); };
    auto num = [](const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    SolverEnv v{};
    v.sparse_vb = unless0("LVF_SPARSE_VB"); v.force_levels = num("LVF_FORCE_LEVELS", 0); v.schur_band = unless0("LVF_SCHUR_BAND");
    v.compact = unless0("LVF_COMPACT"); v.tf_k1sort = unless0("LVF_TF_K1SORT"); v.staged = unless0("LVF_STAGED"); v.zero_tri = unless0("LVF_ZERO_TRI");
    v.poison_s = set("LVF_POISON_S");
    v.early_levels = unless0("LVF_EARLY_LEVELS") && !v.poison_s;
    v.ride_tf = num("LVF_RIDE_TF", -1); v.ride_prep = num("LVF_RIDE_PREP", -1);
    v.chain_levels = std::max(0, std::min(2, num("LVF_CHAIN_LEVELS", 2)));
    v.chain_fence = num("LVF_CHAIN_FENCE", 1);
    v.chain_timeout_ticks = (unsigned)std::max(1, num("LVF_CHAIN_TIMEOUT_US", 500)) * 100u;
    v.chain_rmw_read = set("LVF_CHAIN_RMW_READ");
    v.chol_subblock = unless0("LVF_CHOL_SUBBLOCK"); v.back_tail_merge = unless0("LVF_BACK_TAIL_MERGE"); v.back_product = unless0("LVF_BACK_PRODUCT");
    v.back_blocks = unless0("LVF_BACK_BLOCKS"); v.back_early = unless0("LVF_BACK_EARLY"); v.chol_back_merge = unless0("LVF_CHOL_BACK_MERGE");
    v.back_tail_wgs_set = set("LVF_BACK_TAIL_WGS"); v.fused_lin = unless0("LVF_FUSED_LIN");
    v.tail_wgs = num("LVF_TAIL_WGS", 640); v.back_tail_wgs = std::max(1, num("LVF_BACK_TAIL_WGS", 224)); v.cost_tiles = num("LVF_COST_TILES", 2);
    v.lin_lds_pad = (size_t)num("LVF_LIN_LDS_PAD", 0); v.batch_band_rows = num("LVF_BATCH_BAND_ROWS", 128); v.batch_transpose = num("LVF_BATCH_TRANSPOSE", 127);
    v.chain_info = set("LVF_CHAIN_INFO"); v.lm_history = set("LVF_LM_HISTORY"); v.configure_timing = set("LVF_CONFIGURE_TIMING");
    v.lin_timing = set("LVF_LIN_TIMING"); v.schur_timing = set("LVF_SCHUR_TIMING"); v.sp_timing = set("LVF_SP_TIMING");
    v.chol_timing = set("LVF_CHOL_TIMING"); v.back_timing = set("LVF_BACK_TIMING"); v.cost_timing = set("LVF_COST_TIMING");
    return v;
  }();
  return env;
}

// The argument blocks of ONE LM iteration of a window.  Nothing in them changes from iteration to iteration (the trust-region radius,
// the accept / reject state and the termination flag live in the device-resident LmCtl; an accepted candidate is COPIED into the state
// buffers by k_lm_decide), so they are built once per problem_configure and
//   * passed by value to the single-window launches, or
//   * stored as one entry per window in device tables, every launch of the chain then covering a whole batch of windows (blockIdx.y).
struct Chain {
  bool fast = false;            // merged linearisation (sorted TwoFrame work list) available
  bool batchable = false;       // every launch of the iteration has a table form (fast + band Schur merged with sparse level 0 + no priors, no lidar planes)
  bool has_imu = false, has_prior = false, has_lidar = false, imu_in_cost = false;
  bool has_dprior = false;      // a dense keyframe prior (solver_dense_prior.hip): like has_prior, no fused candidate pass and no table launches
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
  // block step nb - 1 and k_backsolve_tail as ONE launch (k_chol_backsolve_tail; LVF_CHOL_BACK_MERGE=0 turns it off): on with the product and
  // block forms, two or more blocks and the sub-block sweep; cb.bt is bt with a landmark grid sized so that the whole launch is one round
  bool chol_back_merged = false; CholBackArgs cb{}; size_t cb_lds = 0;
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
// ---- solver_plan.hip
int problem_set_dense_prior(lvf_problem* p, lvf_dense_prior* prior);
// ---- solver_batch.hip
void batch_orphan(lvf_problem_batch* b, lvf_problem* dying);
// ---- solver_api.hip
void summary_from_ctl(const lvf_problem* p, const LmCtl& c, lvf_solver_summary* s);

}  // namespace lvf
