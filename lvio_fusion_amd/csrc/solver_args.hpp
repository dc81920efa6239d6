// solver_args.hpp — what the kernels of the LM iteration (solver_kernels.hip, solver_assemble.hip, solver_chol.hip, solver_back.hip) and its host side (solver_chain.hip, solver_plan.hip,
// solver_batch.hip, solver_api.hip) share: the problem object, every kernel argument block, the constants that size grids and LDS, and a
// prototype of every kernel the host launches.  The kernels themselves, with their __launch_bounds__, are defined in those four units, each in exactly one.
#pragma once
#include <memory>
#include <vector>

#include "factor_eval.hpp"
#include "lvf_internal.hpp"

namespace lvf {
struct TfWork;
struct LmCtl;
struct Chain;
struct StageClock;
// one (v, ba, bg) block eliminated ahead of the dense factorisation: its 9 columns start at `col`, its `m` neighbour rows
// (later-ordered (v, ba, bg) blocks, poses, the augmented row; ascending) sit at rows[row_off .. row_off + m)
struct SpNode { int col, row_off, m, id; };
constexpr int kSpMaxLevels = 12, kSpMaxRows = 768;
struct SpLevels { int n; int first[kSpMaxLevels]; int count[kSpMaxLevels]; };
// "Early" sparse levels (see Chain::early): the level reads its columns as  B (natural order, what the ImuError factors accumulated) +
// LM damping + the updates of the levels below (all S holds there), instead of entries k_prepare assembled — so it does not have to wait
// for k_prepare and can ride in an earlier launch.  B == nullptr: the classic form (S holds the assembled entries).
// Ceres' Jacobi column scaling (Solver::Options::jacobi_scaling, a default the reference leaves on: backend.cpp:206-211; declared in
// oracle/lm.h's header): s_j = 1 / (1 + sqrt(H0_jj)) with H0 = diag(J^T J) of the solve's FIRST linearisation, frozen for the solve; the LM
// diagonal is clamped on the SCALED system, which in unscaled terms is D_jj = clamp(s_j^2 H_jj, 1e-6, 1e32) / s_j^2 (lm_damping).  h0 holds
// H0 in the natural order [15 n_kf camera unknowns | n_lm inverse depths]; while *frozen == 0 (the first pass of a solve) the kernels that
// form the damping store H_jj there, afterwards they read it (k_lm_decide raises the flag).
struct JacobiDev { GP<double> h0; GP<const int> frozen; };
struct SpSrc {
  GP<const double> B; int ldB, dp; GP<const double> gc; GP<const double> radius; GP<const int> rows_nat;
  // levels CHAINED inside one launch (the Schur complement's: it lasts long enough for three of them): the level waits until `wait_target`
  // workgroups of the level below have arrived at *wait_counter, and arrives at *done_counter itself.  What it reads of the level
  // below are RETURNING atomic adds into S (agent scope), read back with agent-scope atomic loads; the arrival is a RELEASE add, the
  // waiting side follows its spin with an agent-scope ACQUIRE fence in every wave (`fenced`, default; LVF_CHAIN_FENCE=0: the relaxed
  // round-3 form for A/B timing).  Producers carry lower workgroup numbers than their consumers, so they are normally dispatched
  // first — nothing DEPENDS on that: a consumer that does not see its producers within `timeout_ticks` raises the hand-over flag
  // (SC_FAIL >= kFailHandover), the decision ends the loop WITHOUT taking or counting the step (LVF_WHY_HANDOVER) and the host re-runs
  // the iteration with every level in a launch of its own (lvf_problem::no_chain) — a scheduling delay never becomes a numerical outcome.
  GP<int> wait_counter; int wait_target; GP<int> done_counter;
  int fenced; unsigned timeout_ticks;      // wall_clock64() ticks (100 MHz) before the hand-over is given up
  int strip_end;           // S rows / columns below it belong to sparse blocks (lvf_problem::off)
  int rmw_read;            // diagnostic: chained reads by returning atomics instead of agent-scope loads
  GP<unsigned long long> dbg; // LVF_SP_TIMING=1: eight wall_clock64() stamps per workgroup (tile 0 of every node), else null
  int s_zero;              // the level has nothing below it (level 0, early form): its part of S is still all zeros, not read
  JacobiDev jac{nullptr, nullptr};
  // fused chain (AccSel): *sel != 0 -> B and gc are read from the second accumulator set
  GP<const int> sel{nullptr}; GP<const double> B1{nullptr}, gc1{nullptr};
};
struct SpArgs {          // one sparse level
  GP<const SpNode> nodes; int first, tiles; GP<const int> rows; GP<double> S; int ld; GP<double> W; int wstride; GP<double> Lout; GP<int> fail; int nblocks; GP<const int> done;
  SpSrc src;
};
// SC_FAIL codes (raised with atomicMax: the largest wins): 1 + kb = dense block step kb met a non-positive pivot, kFailSparse + id = sparse
// block id did, kFailHandover + id = a chained level gave up waiting for the level below (NOT a property of the problem: see SpSrc)
constexpr int kFailSparse = 100000, kFailHandover = 300000;
// Test tap (lvf_problem_debug_override_reduced): a caller's reduced system S [d x d] / rhs [d] in the natural unknown order, written over the
// assembled one before any elimination level starts
struct ReducedOverride { int d = 0; DevBuf<double> S, rhs; };
// (debug_taps.hip: the copy kernel lives in a translation unit of its own, so the kernel units' device code is what it is without the tap)
int launch_override_reduced(hipStream_t q, int d, int ld, int aug, const int* perm, const double* Sov, const double* rhs, double* S);
constexpr int kDensePriorMaxKf = 8;
}
// A dense prior on the 15 tangent unknowns of n_sel keyframes (solver_dense_prior.hip; declared semantics: tests/dense_prior_ref.py):
// cost = c0 + eta^T e + 1/2 e^T info e with e = x [-] x0.  kf = the keyframes' positions in the state the prior is evaluated on.
struct lvf_dense_prior {
  lvf_ctx* ctx = nullptr;
  int n_sel = 0, m = 0;
  double c0 = 0.0;
  std::vector<int32_t> kf_h;                    // [n_sel]
  lvf::DevBuf<int> kf;                          // [n_sel]
  lvf::DevBuf<double> x0, info, eta;            // [n_sel][16] (pose 7, v 3, ba 3, bg 3) | [m][m], the lower triangle is read | [m]
  lvf::DevBuf<double> out;                      // lvf_dense_prior_evaluate: gradient [m] | matrix [m][m] | 32 cost stripes
};
struct lvf_problem {
  lvf_ctx* ctx = nullptr;
  lvf_state* st = nullptr;
  lvf_batch *tc = nullptr, *tf = nullptr, *po = nullptr, *imu = nullptr, *prior = nullptr, *lidar = nullptr;
  lvf_dense_prior* dprior = nullptr;            // borrowed (lvf_problem_set_dense_prior); its keyframes stay in the dense corner of the plan
  int n_kf = 0, n_lm = 0, d = 0, dp = 0, ldE = 0, dpad = 0, nb = 0;
  // layout of the factorised matrix S (see "elimination order" in solver_assemble.hip): [sparse (v,ba,bg) blocks | dense (v,ba,bg) blocks | poses | rhs row | pad]
  int ld = 0, off = 0, off_pose = 0, ndense = 0, aug = 0, sp_wstride = 0;
  lvf::SpLevels sp_levels{};
  std::vector<int> sp_tiles, sp_shmem;          // per level: workgroups per node, dynamic LDS bytes
  std::vector<int> sp_item0, sp_items;          // per level: its slice of sp_rows
  std::vector<int32_t> plan_key;                // (n_kf, IMU index pairs, keyframes of the dense prior) the current plan was built for
  lvf::DevBuf<lvf::SpNode> sp_nodes;
  lvf::DevBuf<int> sp_rows, sp_rows_nat, sp_owner, perm, iperm;      // sp_rows_nat: the natural-order unknown of every entry of sp_rows (-2 = the right-hand-side row)
  lvf::DevBuf<int> lm_kmin, lm_kmax, lm_order, lm_nactive;   // per-landmark keyframe track [kmin, kmax]; Schur row order; #rows with pose blocks
  bool band_ready = false;
  // compact landmark layout + slabs of the atomic-free TwoFrame linearisation (see TfCompact)
  bool compact = false;
  lvf::DevBuf<int> lm_eoff, n_slots, tf_slot, run_first;
  lvf::DevBuf<double> slotB, slabP, slabQ, Ct, grt;
  lvf::StageClock* clk = nullptr;     // lvf_problem_stage_times
  bool accum_clean = false;           // B / gc / C / g_rho / cost stripes are zero (left so by the last iteration's cost + decision launch)
  const double* chain_tcw = nullptr;      // the TwoCamera per-block weight array the current chain was built with
  int band_rows = 64;           // landmark rows per slice of the band Schur complement (a batch uses more: fewer output atomics)
  lvf::DevBuf<int4> band_work; lvf::DevBuf<int> n_band_work_dev; lvf::HostPin<int> h_n_band_work;
  int n_band_work = 0, band_rows_built = 0;
  bool band_pending = false; hipEvent_t ev_band = nullptr;      // the item count of the list is still on its way (awaited just before the Schur launch)
  int band_epoch = 0;                 // bumped whenever the landmark bands change (a batch keeps its own, wider-slice work lists: lvf_problem_batch)
  std::vector<lvf_problem_batch*> batches;      // the batches that borrow this problem (they are told when it is destroyed)
  lvf::HostPin<int> h_run_first;
  lvf::DevBuf<unsigned long long> dbg, dbg_lin, dbg_sp;
  lvf::DevBuf<double> dbg_hist;                 // LVF_LM_HISTORY=1: the decisions of the last solve (lvf_problem_debug_history)
  lvf::DevBuf<double> sp_sync;                  // arrival counters of sparse levels chained inside one launch (one 8-byte slot per level, an int in each; cleared with the accumulators)
  lvf::DevBuf<double> sp_W, sp_L, Dinv;         // Dinv: L_kk^-T of every 64x64 diagonal block of the dense corner
  // product form of the sparse back substitution (lvf::GRide): G [9 n_nodes][ldG], allocated by the chain that uses it; sp_gmap [n_nodes][ldG]:
  // which of a node's own rows (index into sp_rows) a dense-corner / augmented column is, or -1
  lvf::DevBuf<double> sp_G; lvf::DevBuf<int> sp_gmap; int ldG = 0;
  lvf::DevBuf<double> sp_T;      // block form of the dense back substitution (lvf::TRide): nb x nb blocks of 64 x 64, block (k, j) used for k < j
  lvf::DevBuf<double> x_last;    // merged last launch (lvf::XLast): the solution's last block, handed from the last block step to the back substitution
  lvf::DevBuf<double> Ldiag;                    // the factored diagonal blocks L_kk [nb][64][64] (NOT stored back into S: see chol_step_body)
  std::vector<int> perm_h;
  lvf::DevBuf<double> B, gc, C, gr, E, Cd, S, dxc, dxl, scal;
  lvf::DevBuf<double> B1, gc1, C1, gr1, E1, slotB1;    // the second accumulator set of the fused chain (lvf::AccSel)
  lvf::DevBuf<double> jh0;                      // Jacobi scaling of the running solve: diag(J^T J) of its first pass (JacobiDev)
  lvf::DevBuf<double> poses2, vel2, ba2, bg2, invd2;   // candidate state x + dx
  lvf::DevBuf<uint8_t> pose_const;
  lvf::DevBuf<int> fail;
  lvf::DevBuf<lvf::TfWork> tf_work;   // per-workgroup runs of same-k2 blocks (empty => generic atomic path)
  lvf::HostPin<lvf::TfWork> h_tf_work;
  std::vector<uint8_t> pose_const_h;
  bool linearized = false;
  bool acc1_ready = false;            // the fused chain's second accumulator set is allocated and cleared for the current configuration (ensure_acc1)
  // TwoFrame blocks as the solver reads them: the batch's own arrays, or — when the blocks of a current-keyframe run come with their first
  // keyframes in no order (landmark ids not in creation order) — copies sorted by (current, first) keyframe made at problem_configure, so
  // that a wave's 64 blocks share a few first keyframes and their sums go through the group-wise reductions instead of 63 LDS atomics per
  // block (the slowest workgroup of k_lin_visual: 18 -> 12 us).  The batch itself is never reordered (lvf_batch_evaluate keeps its order).
  lvf::DevBuf<double2> tfs_fo, tfs_ob;
  lvf::DevBuf<int> tfs_lm, tfs_k1, tfs_k2, tfs_perm;
  lvf::HostPin<int> h_tfs_perm;     // pinned staging of the permutation (the upload is asynchronous)
  bool tf_sorted_copy = false;
  const double2* tf_fo() const { return tf_sorted_copy ? tfs_fo.p : (const double2*)tf->ob_a.p; }
  const double2* tf_ob() const { return tf_sorted_copy ? tfs_ob.p : (const double2*)tf->ob_b.p; }
  const int* tf_lm() const { return tf_sorted_copy ? tfs_lm.p : tf->idx_a.p; }
  const int* tf_k1() const { return tf_sorted_copy ? tfs_k1.p : tf->idx_b.p; }
  const int* tf_k2() const { return tf_sorted_copy ? tfs_k2.p : tf->idx_c.p; }
  bool tf_unique_lk2 = false;   // no (landmark, current keyframe) pair occurs twice in the TwoFrame batch
  bool tf_k1_first = false;     // every TwoFrame block's first keyframe precedes its current keyframe
  double last_radius = 0;
  // the device-resident LM loop
  lvf::DevBuf<lvf::LmCtl> ctl;        // control block (radius, costs, accept / reject, termination) in HBM
  lvf::LmCtl* rec = nullptr;          // host-visible mirror written by k_lm_decide (hipHostMalloc)
  lvf::HostPin<lvf::LmCtl> h_ctl;     // pinned staging for uploads / read-backs of the control block
  lvf::Chain* chain = nullptr;        // argument blocks of one iteration
  bool chain_ready = false;
  bool no_chain = false;              // a chained hand-over timed out: this problem's levels are launches of their own until kUnchainedSolves solves have gone by
  int unchained_solves = 0;           // solves taken since no_chain was set (chaining is tried again after kUnchainedSolves of them: one scheduling blip
                                      // under Relocator traffic — relocator.cpp:188 — must not cost a persistent window its chained launches for good)
  int handover_retries = 0;           // iterations re-run because of that (reported in lvf_solver_summary::hand_over_retries)
  int force_handover_timeouts = 0;    // test hook (lvf_problem_debug_force_handover_timeout): the next chain is built with an unreachable wait target
  const void* chain_state[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // the state pointers the chain was built for
  double huber = 1.0;
  hipGraphExec_t graph_exec = nullptr;
  std::unique_ptr<lvf::ReducedOverride> ov;     // test tap: non-null while a reduced system is overridden (enqueue_iteration)
  bool step_ready = false;            // dxc / the fail flag hold the step of an iteration (lvf_problem_debug_download_step)
  int last_solved = -1;               // LmCtl::solved of the last iteration (lvf_problem_debug_last_solved)
  ~lvf_problem();
};

namespace lvf {
constexpr int kT = 256;
// device scalar slots
// Each sum slot is STRIPED over kStripes addresses (workgroup b adds into stripe b % kStripes, the host adds the stripes up): a
// cost pass issues one atomic per wave, ~1100 of them at configs[3], and on ONE address they serialise in L2 (measured: the
// residual-only TwoFrame pass spent 2/3 of its 16 us there).  SC_GMAX is a max (striped too; the decision takes the max over the stripes).
constexpr int kStripes = 32;
enum { SC_COST = 0, SC_COST_NEW = 1 * kStripes, SC_MODEL = 2 * kStripes, SC_DXNORM = 3 * kStripes, SC_XNORM = 4 * kStripes, SC_GMAX = 5 * kStripes,
       SC_N = 6 * kStripes, SC_FAIL = SC_N /* int flag */, SC_TICKET = SC_N + 1 /* int: workgroups of the candidate-cost pass that are done */, SC_ALLOC = SC_N + 2 };
static inline double stripe_sum(const double* h, int slot) { double s = 0.0; for (int k = 0; k < kStripes; ++k) s += h[slot + k]; return s; }

struct StateP { GP<const double> poses, vel, ba, bg, inv_depth, w_kf; };

// The fused chain (LVF_FUSED_LIN, default on) linearises at the CANDIDATE inside the cost + decision pass, so a problem keeps two sets of what
// a linearisation writes — B, gc, C, g_rho, the E rows and the TwoFrame slot records — and LmCtl::aset names the set that holds the
// linearisation at the current state.  An argument block whose `sel` is set picks its set on device (set 1: the pointers here; set 0: the
// block's own); sel == nullptr (today's chain, the taps, a batch) always means set 0.
struct AccSel { GP<const int> sel; GP<double> B, gc, C, gr, E, slotB; };

// Device-resident control block of one window's Levenberg-Marquardt loop.  Everything that changes from one iteration to the next
// lives here (trust-region radius, costs, accept / reject, termination), so the arguments of every kernel of an iteration are
// constant across iterations: the host enqueues iteration after iteration without waiting, k_lm_decide closes each one on device
// (what the reference's ceres::Solve does on the host between evaluations).
struct LmCtl {
  double radius, decrease;                         // trust region (in: start values; updated by every iteration)
  double last_radius;                              // the radius the last iteration's step was computed with
  double cost, initial_cost;                       // cost at the current state / at the first linearisation
  double cost_before, cost_after, model, dxnorm, xnorm, gmax;   // scalars of the last iteration
  double huber, function_tol, gradient_tol, parameter_tol, min_rel_decrease;
  int max_iters;
  int iter, successes, invalid_run;                // iterations taken / accepted steps / consecutive unsolvable steps
  int accepted, solved;                            // of the last iteration
  int done, termination;                           // done != 0: the remaining launches of this window return immediately
  int why, rejected;                               // LVF_WHY_* reason of the termination ; rejected / invalid steps so far
  int jfrozen;                                     // Jacobi scaling taken (JacobiDev): 0 until the solve's first pass has been decided on
  int aset;                                        // fused chain: the accumulator set holding the linearisation at the state (AccSel)
  int lin_pending;                                 // fused chain: that set's TwoFrame slabs are not yet reduced into B / gc (an accepted candidate pass)
};

// ---- the argument blocks and sizing constants, in the order of the chain (each launch is described where its kernel is defined)
// ---- linearisation and candidate cost (k_lin_visual, k_tf_reduce, k_cost_visual / k_cost_decide, k_lin_imu, k_prior_*)
struct TfWork { int first, count, k2; };
// Atomic-free outputs of the sorted TwoFrame linearisation ("compact" mode).  Measured on MI355X: the 8 landmark-indexed global f64
// atomics per block were 18 of the 21 us a workgroup spent between loading its blocks and its reductions, and together with the
// per-workgroup flush of the keyframe-indexed sums (~1 M atomics per linearisation at configs[3]) they are a chip-wide L2 bottleneck
// (~30 atomics / ns) that a batch of windows hits W times over.  Instead:
//   * the k2 columns of a landmark's (dense) E row have exactly one writer: plain stores.  The row is NOT cleared per linearisation: its
//     non-zero pattern (the landmark's track) is fixed for a problem, so E is zeroed once per problem_configure and every entry inside
//     the pattern is overwritten by every linearisation;
//   * every block owns a SLOT s = eoff[l] + (k2 - k1 - 1) of its landmark's track and writes there, with plain 16-byte stores, one
//     64-byte record: its contributions to the k1 columns of E (6), to C and to g_rho.  k_prepare reads a landmark's slots as one
//     contiguous range, sums them and completes the row (k1 columns, g_rho column) and Cd;
//   * every workgroup writes its LDS table of keyframe-indexed sums to its own slab (slabP[wg][k1][64], slabQ[wg][32]); k_tf_reduce adds
//     the slabs of a run into B / gc, each entry of B having exactly one owner there.
struct TfCompact { int on; GP<const int> slot; GP<double> slotB, slabP, slabQ; int staged; };
constexpr int kSlabRow = 64, kSlabQ = 32;
constexpr int kAccSlots = 63;   // 21 (B[k1,k1] lower) + 6 (g[k1]) + 36 (cross block, rows = k2 tangent, cols = k1 tangent)
constexpr int kStageWave = 64 * 9 + 32;   // doubles of LDS staging per wave (segmented first-keyframe sums): 64 x (8 + 1 pad) values + 64 ints
struct CostVisual {
  int n_tc, n_tf, n_po, g_tc, g_tf;
  GP<const double2> tc_lo, tc_ro; GP<const int> tc_lm, tc_kf; GP<const double> tc_w; CamD tc_left, tc_right;
  GP<const double2> tf_fo, tf_ob; GP<const int> tf_lm, tf_k1, tf_k2; CamD tf_left, tf_right;
  GP<const double2> po_ob; GP<const int> po_kf, po_pwi; GP<const double> po_pw; CamD po_cam;
};
struct ImuEvalArgs { int n; GP<const double> pre, sqrt_info; GP<const int> kf_i, kf_j; };      // ImuError factors evaluated inside a merged launch
struct CostArgs {
  CostVisual a; int n_kf; StateP s; double huber; GP<double> cost; int nblocks; GP<const int> done;
  ImuEvalArgs imu; int g_imu;       // workgroups [0, g_imu) evaluate one ImuError factor each, the visual passes follow
  int tiles;                        // tiles of kT blocks per visual workgroup (0 = 1)
  ZeroList zero; int zero_wgs;      // workgroups [nblocks, nblocks + zero_wgs) of the merged cost + decision launch clear the accumulators for the NEXT linearisation
};
struct ImuJ { GP<const double> j[8]; };
constexpr int kEndZeroWgs = 192;       // workgroups of the cost + decision launch that clear the accumulators
constexpr int kImuWaveLds = 225 + 480 + 480 + 16 + 16 + 16 + 248 + 32 + 2;      // + the pre-integration's head (OFF_COV doubles) + the two keyframes' states
struct LinVisual {
  int n_tfw, g_tc;
  // TwoFrame
  GP<const TfWork> work; GP<const double2> tf_fo, tf_ob; GP<const int> tf_lm, tf_k1; CamD tf_left, tf_right; int unique_lk2; TfCompact cp;
  // TwoCamera
  int n_tc; GP<const double2> tc_lo, tc_ro; GP<const int> tc_lm, tc_kf; GP<const double> tc_w; CamD tc_left, tc_right;
  // PoseOnly
  int n_po, g_po; GP<const double2> po_ob; GP<const int> po_kf, po_pwi; GP<const double> po_pw; CamD po_cam;
  // ImuError: evaluated inside the launch (imu.pre != nullptr) or ahead of it by k_imu<true> (imu_res / imu_J)
  int n_imu; GP<const double> imu_res; ImuJ imu_J; GP<const int> imu_i, imu_j; ImuEvalArgs imu;
};
struct LinArgs {
  LinVisual v; int n_kf; StateP s; double huber; GP<const uint8_t> pose_const; GP<double> B; int ld; GP<double> gc; GP<double> E; int ldE; GP<double> C, gr, cost;
  int nblocks; GP<const int> done; GP<unsigned long long> dbg; int rows;
  GP<double> scal_reset;      // early sparse levels: the per-step scalars and the fail flag are reset HERE (the levels start before k_prepare, which resets them otherwise)
  AccSel acc;                 // the second accumulator set (the fused candidate pass writes the set that is not active)
};
struct TfReduceArgs {
  int n_kf, n_wg; GP<const int> run_first; GP<const double> slabP, slabQ; GP<double> B; int ld; GP<double> gc; int nblocks; GP<const int> done;
  int own_blocks; SpArgs ride;       // workgroups [own_blocks, nblocks): a sparse level riding in this launch (early form)
  // fused chain: B / gc of the active set (acc); `pending` (LmCtl::lin_pending) == 0: the active set was reduced by an earlier iteration (the
  // last step was rejected) and this launch leaves it alone; workgroups [nblocks, nblocks + zero_wgs) clear the set that is NOT active
  // (stand0 when set 1 is active, stand1 otherwise) for the candidate pass at the end of the iteration — never gated
  AccSel acc; GP<const int> pending; ZeroList stand0, stand1; int zero_wgs;
};
struct PriorArgs { int n; GP<const int> kf_a, kf_b; GP<const double> target, weight, vv; };

// ---- damped system, Schur complement, sparse levels (k_prepare, k_schur_*, k_schur_sp0)
struct PrepArgs {
  int ld, dpad, jl0 /* = d: the first landmark slot of jac.h0 */; GP<const int> iperm; GP<const double> B, gc; GP<const double> radius; GP<double> S; unsigned nS_blocks; int n_lm, dp, ldE; GP<const double> C, gr;
  GP<double> Cd, E, scal; int nblocks; GP<const int> done;
  // atomic-free mode (slotB != nullptr): per-landmark totals from the slot records
  GP<const int> eoff, kmin, kmax; GP<const double> slotB; GP<double> Ct, grt;
  // early form (early != 0): S was cleared with the accumulators and sparse levels may already have added into the dense corner, so the
  // corner's entries (rows / columns >= off) are ADDED, and the columns of the sparse blocks are left alone (the levels form them themselves)
  int early, off;
  int own_blocks; SpArgs ride;       // workgroups [own_blocks, nblocks): a sparse level riding in this launch
  JacobiDev jac;
  AccSel acc;                        // fused chain: B, gc, C, g_rho, the slot records and E of the active set
};
constexpr int kSchurChunk = 512;
constexpr int kSchurGroups = 8, kSchurTilesPerWave = 8, kSchurRows = 16;
constexpr int kBandTilesPerWave = 8;        // output tiles (16 x 16 accumulators) a wave of the band Schur complement carries.  (Measured round 4, same box: 16 — one
// workgroup covers most slices' whole band, E read once instead of ~2x — needs > 256 VGPRs: 0.204 -> 0.254 ms / iteration spilling under the two-waves-per-SIMD
// attribute of k_schur_sp0, 0.206 / 8 windows 0.375 -> 0.435 ms with one wave per SIMD; 4 — more, smaller workgroups — 8 windows 0.43 -> 0.59 ms.  The launch is bound by
// how many workgroups overlap their fetch -> LDS -> matrix-core chains, not by E's bytes.)
constexpr int kBandRows = 64, kBandRowsMax = 256, kBandTilesPerGroup = 4 * kBandTilesPerWave;     // rows per slice: 64 for one window, up to 256 in a batch (fewer output atomics)
struct LmBand { GP<const int> order; GP<const int> n_active; GP<const int> kmin; GP<const int> kmax; };   // null order => dense SYRK
struct SchurSp0Args {
  int n_slices, n_groups, dp, ldE; GP<const double> E, Cd; GP<const int> order, n_active, kmin, kmax; int d_local, ldS; GP<double> S_pose;
  SpArgs sp;             // the sparse level riding in the launch (sp.nblocks == 0: Schur complement only): level 0, or — early form — the first one left
  SpArgs sp_b, sp_c;     // early form: the next two levels, chained behind it inside the launch (SpSrc::wait_counter)
  int nblocks; GP<const int> done; GP<unsigned long long> dbg; int rows;
  GP<const int4> work; int n_work;      // (slice, group, band lo | hi << 16, slice end) items; the sparse levels run in the first workgroups, the items behind
  AccSel acc;                           // fused chain: E of the active set
};

// ---- blocked Cholesky (k_chol_step*), with the riders that form the back substitution's products G (GRide) and T_kj (TRide)
constexpr int kNB = 64, kLd = 65;
constexpr int kPG = 2, kCT = 512, kGW = 16 / kPG;                    // pivots per group, threads, groups per wave
struct CholArgs { GP<double> Sd; int ld, nb; GP<int> fail; GP<double> Dinv; GP<const int> done; GP<unsigned long long> dbg; int last_cols; GP<double> Ldiag; };   // dbg: LVF_CHOL_TIMING stamps; last_cols: real (un-padded) columns of the last block
__host__ __device__ inline int chol_step_grid(int nb, int kb) {
  const int below = nb - kb - 1;
  return kb >= nb ? 0 : 2 + below + (kb > 0 ? below * (below + 1) / 2 : 0);
}
struct TRide { int n; GP<double> T; };
// The merged last launch (k_chol_backsolve_tail): the inverse workgroup of block step nb - 1 holds L_kk^-T and the forward-substituted
// right-hand side when its sweep ends, forms the solution's last block x_last = L_kk^-T y_last and publishes its 64 values, then the flag
// (agent-scope atomic stores, as the pose increments travel: BackArgs::pose_ready).  null flag: nothing is published (k_chol_step*).
struct XLast { GP<double> x = nullptr; GP<int> flag = nullptr; };
struct GRide { int n, first; GP<const SpNode> nodes; GP<const int> rows; GP<const double> W; int wstride; GP<const double> Linv; GP<const int> map; GP<double> G; int ldG, off; GP<const int> done; };

// ---- back substitution and step tail (k_chol_backsolve, k_step_tail, k_backsolve_tail)
struct SpBack {                    // what the back substitution needs of the plan
  SpLevels lv;
  int item0[kSpMaxLevels], items[kSpMaxLevels];   // the level's slice of rows/owner/W
  GP<const SpNode> nodes; GP<const int> rows; GP<const int> owner; GP<const double> W; GP<const double> Linv; GP<const int> perm;
  int off, aug, d_total, total_items, n_nodes, max_count, linv_in_lds;
  int prod_items;                  // > 0: LDS room for that many (row x 9) products => conflict-free two-stage sums; 0: LDS atomics
  GP<unsigned long long> dbg;         // LVF_BACK_TIMING=1: wall_clock64() stamps (100 MHz) at the phase boundaries, else null
};
constexpr int kBT = 512, kBParts = kBT / 64, kBackPre = 256 / kBParts, kBackInv = 64 / kBParts, kTailPre = 6;
// pose_ready (merged back-substitution + step tail, k_backsolve_tail): once the dense corner is solved the POSE part of the step (natural
// unknowns [0, n_pose)) is written out and *pose_ready is raised (release, agent scope) — what the landmark back-substitution waits for
// T (block form, back_block_ride): the stored products T_kj of this iteration's factor, or null for the form that reads S and Dinv
// x_ready (merged last launch, block form only): the back substitution does not solve its first block but waits — bounded by x_timeout
// ticks, then kFailHandover is raised at x_fail — for the flag of XLast and reads the block from x_last
struct BackArgs { GP<const double> Sd; int ld, d; GP<const double> Dinv; GP<double> xout; SpBack sp; GP<const int> done; GP<const double> Ldiag; GP<int> pose_ready = nullptr; int n_pose = 0; int pose_fenced = 0;
                  GP<const double> T = nullptr;
                  GP<const int> x_ready = nullptr; GP<const double> x_last = nullptr; unsigned x_timeout = 0; GP<int> x_fail = nullptr; };
// block form: links j = nblk - 1 .. 1 whose products a thread holds in registers, eight doubles per block (k, j), k < j.  The dense-corner-only
// body has the room for a corner of five blocks (ten products); beside the sparse levels' items they take the place of the gather operands
// (three products: three blocks).  A corner with more blocks keeps the S / Dinv form (build_chain).
constexpr int kBackTJ = 4, kBackTJLevels = 2;
constexpr int kLmEPre = 8;
struct TailArgs {
  int g_lm, n_lm, dp, ldE; GP<const double> E, C, Cd, gr, dxc; GP<double> dxl, scal; GP<const int> kmin, kmax; int n_kf; StateP s;
  GP<double> poses2, vel2, ba2, bg2, invd2; int d, ld; GP<const double> B, gc; GP<const double> radius; int nblocks; GP<const int> done;
  GP<const unsigned char> pose_const; JacobiDev jac;
  AccSel acc;             // fused chain: E, B, gc of the active set (C, gr here are k_prepare's single totals Ct / grt: the chain needs compact mode)
};
struct BackTailArgs { BackArgs back; TailArgs tail; int g_lm; int fenced; unsigned timeout_ticks; GP<int> fail;
                      int g_prod = 0, kpw = 0, ldG = 0; GP<const double> G = nullptr; GP<const int> iperm = nullptr;
                      int early = 1;
                      // merged last launch: the G rows of the last level are formed by riders of the SAME launch — the G workgroups wait (bounded)
                      // until g_target of them have arrived at *g_ready before they request anything of G, and read G at the coherence point
                      GP<const int> g_ready = nullptr; int g_target = 0; };      // early: the landmark and pose workgroups request their operands before the wait (LVF_BACK_EARLY=0: behind it)
// k_chol_backsolve_tail: block step nb - 1 and k_backsolve_tail as ONE launch (Chain::chol_back_merged).  Workgroups by blockIdx.x, producers
// first: [0, 2) the column of the last block step (chol_step_body; the second one publishes x_last), 2 the back substitution, [3, 3 + g.n) the
// G riders of this launch, then the pose workgroup, bt.g_prod G-product workgroups and bt.g_lm landmark workgroups of k_backsolve_tail.
struct CholBackArgs { CholArgs chol; GRide g; GP<int> g_arrive; TRide tr; XLast xl; BackTailArgs bt; };

// ---- closing an iteration (k_lm_decide, k_cost_decide, k_lin_cost_decide)
struct DecideArgs {
  GP<const double> scal; GP<LmCtl> ctl; GP<LmCtl> rec; GP<int> ticket;
  int n_kf, n_lm;
  GP<double> poses, vel, ba, bg, invd;                 // the state
  GP<const double> poses2, vel2, ba2, bg2, invd2;      // the candidate
  GP<unsigned long long> dbg;                              // LVF_COST_TIMING=1: wall_clock64() stamps (100 MHz), else null
  GP<double> hist;                                         // LVF_LM_HISTORY=1: eight doubles per closed pass (64 passes), else null
  int fused;                                               // closes a fused candidate pass (k_lin_cost_decide): see lm_decide_body
};
constexpr int kDT = 256;
struct FusedArgs { LinArgs lin; DecideArgs dec; GP<double> cost_new; int nblocks; GP<const int> done; ZeroList zero; int zero_wgs; };

// ------------------------------------------------------------------------------------------------ kernels launched from the host side
// (prototypes only: the definitions carry the launch bounds and occupancy attributes — k_tf_reduce*, k_prepare*, the Schur, layout and sparse-level
// kernels in solver_assemble.hip, k_chol_step* in solver_chol.hip, k_chol_backsolve*, k_step_tail*, k_backsolve_tail and k_chol_backsolve_tail in solver_back.hip, the
// linearisation, cost and decision kernels in solver_kernels.hip)
__global__ void k_zero_multi(ZeroList z);
__global__ void k_zero_multi_ranges(ZeroList z, int n_lm, int* __restrict__ kmin, int* __restrict__ kmax);
__global__ void k_zero_table(const ZeroList* __restrict__ t);
template <bool COST_ONLY>
__global__ void k_lin_tc(int n, const double2* __restrict__ lo, const double2* __restrict__ ro, const int* __restrict__ lm, const int*
    __restrict__ kf, const double* __restrict__ wblk, StateP s, CamD left, CamD right, double huber, double* __restrict__ C, double*
    __restrict__ gr, double* __restrict__ cost);
template <bool COST_ONLY>
__global__ void k_lin_tf(int n, int n_kf, const double2* __restrict__ fo, const double2* __restrict__ ob, const int* __restrict__ lm, const
    int* __restrict__ kf1, const int* __restrict__ kf2, StateP s, CamD left, CamD right, double huber, const uint8_t* __restrict__
    pose_const, double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ E, int ldE, double* __restrict__ C, double*
    __restrict__ gr, double* __restrict__ cost);
__global__ void k_cost_visual(CostArgs a);
template <bool COST_ONLY>
__global__ void k_lin_po(int n, int n_kf, const double2* __restrict__ ob, const int* __restrict__ kf, const int* __restrict__ pwi, const
    double* __restrict__ pw, StateP s, CamD cam, double huber, const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
    double* __restrict__ gc, double* __restrict__ cost);
__global__ void k_lin_imu(int n, int n_kf, const double* __restrict__ res, ImuJ J, const int* __restrict__ kf_i, const int* __restrict__
    kf_j, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld, double* __restrict__ gc,
    double* __restrict__ cost);
__global__ void k_lin_visual(LinArgs a);
__global__ void k_lin_visual_b(const LinArgs* __restrict__ t);
__global__ void k_lin_visual_bt(const LinArgs* __restrict__ t);
__global__ void k_tf_reduce(TfReduceArgs a);
__global__ void k_tf_reduce_b(const TfReduceArgs* __restrict__ t);
__global__ void k_tf_reduce_bt(const TfReduceArgs* __restrict__ t);
__global__ void k_prior_lin(PriorArgs P, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const, double* __restrict__ B,
    int ld, double* __restrict__ gc, double* __restrict__ cost);
__global__ void k_prior_cost(PriorArgs P, const double* __restrict__ poses, double* __restrict__ cost);
__global__ void k_cost_sq(int n, const double* __restrict__ res, double* __restrict__ cost);
// LiDAR planes on keyframe poses (solver_lidar.hip): p | pa | nrm SoA [3][n], the block's keyframe, weight and Huber a (<= 0: no loss)
struct LidarPoseArgs { int n; GP<const double> p, pa, nrm; GP<const int> kf; GP<const double> w, a; };
static inline LidarPoseArgs lidar_pose_args(const lvf_batch* b) { return LidarPoseArgs{b->n, b->lp.p, b->lpa.p, b->lnrm.p, b->idx_a.p, b->ob_a.p, b->ob_b.p}; }
__global__ void k_lidar_lin(LidarPoseArgs L, int n_kf, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const, double* __restrict__ B,
    int ld, double* __restrict__ gc, double* __restrict__ cost);
__global__ void k_lidar_cost(LidarPoseArgs L, int n_kf, const double* __restrict__ poses, double* __restrict__ cost);
// The dense keyframe prior (solver_dense_prior.hip): one workgroup.  B / gc: the lower triangle in the natural order (pose rows 6 k,
// (v, ba, bg) rows dp + 9 k).  gout / Hout non-null: the materialised parity mode, gradient [m] and matrix [m][m] instead of B / gc.
struct DensePriorArgs { int n_sel, m; GP<const int> kf; GP<const double> x0, info, eta; double c0; };
static inline DensePriorArgs dense_prior_args(const lvf_dense_prior* d) { return DensePriorArgs{d->n_sel, d->m, d->kf.p, d->x0.p, d->info.p, d->eta.p, d->c0}; }
constexpr int kDensePriorT = 256;
__global__ void k_dense_prior_lin(DensePriorArgs P, int n_kf, StateP s, const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
    double* __restrict__ gc, double* __restrict__ cost, double* __restrict__ gout, double* __restrict__ Hout);
__global__ void k_dense_prior_cost(DensePriorArgs P, StateP s, double* __restrict__ cost);
__global__ void k_prepare(PrepArgs a);
__global__ void k_prepare_b(const PrepArgs* __restrict__ t);
__global__ void k_prepare_bt(const PrepArgs* __restrict__ t);
__global__ void k_schur_syrk(int n_lm, int dp, int ldE, int ntile, const double* __restrict__ E, const double* __restrict__ Cd, int d, int
    ldS, double* __restrict__ S);
__global__ void k_schur_lds(int n_lm, int dp, int ldE, int ntile, int rows_per_slice, const double* __restrict__ E, const double*
    __restrict__ Cd, int d, int ldS, double* __restrict__ S);
__global__ void k_lm_range(int n, const int* __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2, int* __restrict__
    kmin, int* __restrict__ kmax);
__global__ void k_lm_sort(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ order, int*
    __restrict__ n_active);
__global__ void k_lm_sort_offsets(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ order,
    int* __restrict__ n_active, int* __restrict__ eoff, int* __restrict__ n_slots);
__global__ void k_tf_slots_zero(int n, int g_slots, const int* __restrict__ lm, const int* __restrict__ k2, const int* __restrict__ kmin,
    const int* __restrict__ eoff, int* __restrict__ slot, const int* __restrict__ n_slots, double* __restrict__ slotB);
__global__ void k_tf_gather(int n, const int* __restrict__ perm, const double2* __restrict__ fo, const double2* __restrict__ ob, const int*
    __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2, double2* __restrict__ fo_s, double2* __restrict__ ob_s, int*
    __restrict__ lm_s, int* __restrict__ k1_s, int* __restrict__ k2_s);
__global__ void k_schur_band(int dp, int ldE, const double* __restrict__ E, const double* __restrict__ Cd, const int* __restrict__ order,
    const int* __restrict__ n_active_p, const int* __restrict__ kmin, const int* __restrict__ kmax, int d, int ldS, double* __restrict__ S);
__global__ void k_chol_step(CholArgs a, int kb, GRide g, TRide tr);
__global__ void k_chol_step_b(const CholArgs* __restrict__ t, int kb);
__global__ void k_chol_step_bt(const CholArgs* __restrict__ t, int kb);
__global__ void k_chol_step_pp(CholArgs a, int kb, GRide g, TRide tr);
__global__ void k_chol_step_pp_b(const CholArgs* __restrict__ t, int kb);
__global__ void k_chol_step_pp_bt(const CholArgs* __restrict__ t, int kb);
__global__ void k_band_work(int rows, int dp, const int* __restrict__ n_active_p, const int* __restrict__ order, const int* __restrict__
    kmin, const int* __restrict__ kmax, int4* __restrict__ work, int* __restrict__ n_work);
__global__ void k_sp_eliminate(SpArgs a);
__global__ void k_sp_eliminate_b(const SpArgs* __restrict__ t);
__global__ void k_schur_sp0(SchurSp0Args a);
__global__ void k_schur_sp0_b(const SchurSp0Args* __restrict__ t);
__global__ void k_schur_sp0_bt(const SchurSp0Args* __restrict__ t);
__global__ void k_chol_backsolve(BackArgs a);
__global__ void k_chol_backsolve_b(const BackArgs* __restrict__ t);
__global__ void k_step_tail(TailArgs a);
__global__ void k_step_tail_b(const TailArgs* __restrict__ t);
__global__ void k_step_tail_bt(const TailArgs* __restrict__ t);
__global__ void k_backsolve_tail(BackTailArgs a);
__global__ void k_chol_backsolve_tail(CholBackArgs a);
__global__ void k_lm_decide(DecideArgs a);
__global__ void k_cost_decide(CostArgs a, DecideArgs d, int end_zero);
__global__ void k_cost_decide_b(const CostArgs* __restrict__ t, const DecideArgs* __restrict__ d, int end_zero);
__global__ void k_cost_decide_bt(const CostArgs* __restrict__ t, const DecideArgs* __restrict__ d, int end_zero);
__global__ void k_lin_cost_decide(FusedArgs a);

}  // namespace lvf
