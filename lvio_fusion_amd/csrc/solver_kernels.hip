// solver_kernels.hip — the evaluation side of the LM iteration on device: the clears, the fused robustified linearisation of every factor
// type, the residual-only cost passes, and the decision that closes an iteration.  The decision kernels live HERE, with the linearisation,
// because k_cost_decide* and k_lin_cost_decide run the linearisation and cost bodies themselves (lin_visual_run, cost_visual_value): in a unit
// of their own they would need those 670 lines in a shared header.  The other stages are solver_assemble.hip (slab reduction, damping, Schur
// forms, layout kernels, sparse levels), solver_chol.hip (blocked Cholesky) and solver_back.hip (back substitution, step tail); what kernels
// of more than one unit call is in solver_dev.hpp; the trust-region rule the decision applies is LmState (lm_rule.hpp).  Replaces what
// ceres::Solve does under adapt::Solve for Backend::Optimize (src/lvio_fusion/include/lvio_fusion/adapt/problem.h:83-88;
// src/lvio_fusion/src/backend.cpp:96-183, 206-211).
// Device code only: the argument blocks and constants are in solver_args.hpp, the host side that builds and launches the chain in
// solver_chain.hip, solver_plan.hip, solver_batch.hip and solver_api.hip.
#include "factor_eval.hpp"
#include "prior_eval.hpp"
#include "lvf_internal.hpp"
#include "imu_eval.hpp"
#include "solver_args.hpp"
#include "solver_dev.hpp"

namespace lvf {

// lower-triangle accumulation of a 6x6 block pair J_a^T J_b into B at (ra, rb) block offsets (ra >= rb required
// for off-diagonal; for ra == rb only the lower half is written)
__device__ __forceinline__ void add_block66(double* __restrict__ B, int ld, int ra, int rb, const double Ja[12], const double Jb[12]) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      if (ra == rb && j > i) continue;
      atomicAdd(&B[(size_t)(ra + i) * ld + rb + j], Ja[i] * Jb[j] + Ja[6 + i] * Jb[6 + j]);
    }
}

// ------------------------------------------------------------------------------------------------ housekeeping
// one launch zeroes every accumulator of a linearisation (B, gc, E, C, gr, scalars) instead of six fill kernels
// (ZeroList: lvf_internal.hpp)
__global__ __launch_bounds__(kT) void k_zero_multi(ZeroList z) {
  double* p = z.p[blockIdx.y];
  if (z.tri[blockIdx.y] > 0) { zero_lower(p, z.tri[blockIdx.y], (unsigned long long)blockIdx.x * (kT / 64) + (threadIdx.x >> 6), (unsigned long long)gridDim.x * (kT / 64)); return; }
  const unsigned long long n = z.n[blockIdx.y], n2 = n / 2;
  double2* p2 = reinterpret_cast<double2*>(p);
  for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < n2; i += (unsigned long long)gridDim.x * kT) p2[i] = make_double2(0.0, 0.0);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = 0.0;
}
// k_zero_multi with one more slice (problem_configure): slice z.count of the grid's y sets the landmark tracks to "none yet"
// (kmin = INT_MAX, kmax = -1, what k_lm_range then narrows)
__global__ __launch_bounds__(kT) void k_zero_multi_ranges(ZeroList z, int n_lm, int* __restrict__ kmin, int* __restrict__ kmax) {
  if ((int)blockIdx.y == z.count) {
    for (int l = blockIdx.x * kT + threadIdx.x; l < n_lm; l += gridDim.x * kT) { kmin[l] = 0x7fffffff; kmax[l] = -1; }
    return;
  }
  double* p = z.p[blockIdx.y];
  const unsigned long long n = z.n[blockIdx.y], n2 = n / 2;
  double2* p2 = reinterpret_cast<double2*>(p);
  for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < n2; i += (unsigned long long)gridDim.x * kT) p2[i] = make_double2(0.0, 0.0);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = 0.0;
}
// one launch for a batch of windows: blockIdx.y = window
__global__ __launch_bounds__(kT) void k_zero_table(const ZeroList* __restrict__ t) { zero_list_share(t[blockIdx.y], blockIdx.x, gridDim.x); }

// ------------------------------------------------------------------------------------------------ TwoCamera
template <bool COST_ONLY>
__device__ __forceinline__ void lin_tc_body(const int vb, int n, const double2* __restrict__ lo, const double2* __restrict__ ro,
                                               const int* __restrict__ lm, const int* __restrict__ kf, const double* __restrict__ wblk, StateP s,
                                               CamD left, CamD right, double huber, double* __restrict__ C,
                                               double* __restrict__ gr, double* __restrict__ cost) {
  const int i = vb * kT + threadIdx.x;
  double c = 0.0;
  if (i < n) {
    const int l = lm[i];
    const double2 a = lo[i], b = ro[i];
    double r[2], J[2];
    eval_two_camera<!COST_ONLY>(left, right, a.x, a.y, b.x, b.y, s.inv_depth[l], wblk ? wblk[i] : 5.0 * s.w_kf[kf[i]], r, J);
    double rho;
    const double sc = robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
    c = 0.5 * rho;
    if (!COST_ONLY) {
      const double s2 = sc * sc;
      atomicAdd(&C[l], s2 * (J[0] * J[0] + J[1] * J[1]));
      atomicAdd(&gr[l], s2 * (J[0] * r[0] + J[1] * r[1]));
    }
  }
  block_add(c, cost);
}
template <bool COST_ONLY>
__global__ __launch_bounds__(kT) void k_lin_tc(int n, const double2* __restrict__ lo, const double2* __restrict__ ro,
                                               const int* __restrict__ lm, const int* __restrict__ kf, const double* __restrict__ wblk, StateP s,
                                               CamD left, CamD right, double huber, double* __restrict__ C,
                                               double* __restrict__ gr, double* __restrict__ cost) { lin_tc_body<COST_ONLY>(blockIdx.x, n, lo, ro, lm, kf, wblk, s, left, right, huber, C, gr, cost); }

// ------------------------------------------------------------------------------------------------ TwoFrame
template <bool COST_ONLY>
__global__ __launch_bounds__(kT) void k_lin_tf(int n, int n_kf, const double2* __restrict__ fo, const double2* __restrict__ ob,
                                               const int* __restrict__ lm, const int* __restrict__ kf1,
                                               const int* __restrict__ kf2, StateP s, CamD left, CamD right, double huber,
                                               const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
                                               double* __restrict__ gc, double* __restrict__ E, int ldE,
                                               double* __restrict__ C, double* __restrict__ gr, double* __restrict__ cost) {
  __shared__ PoseD s_pose[kMaxStagedKf];
  stage_poses<kT>(s_pose, s.poses, n_kf);
  const int i = blockIdx.x * kT + threadIdx.x;
  double c = 0.0;
  if (i < n) {
    const int l = lm[i], k1 = kf1[i], k2 = kf2[i];
    const double2 a = fo[i], b = ob[i];
    const PoseD P1 = fetch_pose(s_pose, s.poses, n_kf, k1), P2 = fetch_pose(s_pose, s.poses, n_kf, k2);
    double r[2], Jd[2], L1[12], L2[12];
    if (COST_ONLY) { double J1[14], J2[14]; eval_two_frame<false>(P1, P2, left, right, a.x, a.y, b.x, b.y, s.inv_depth[l], s.w_kf[k2], r, Jd, J1, J2); }
    else eval_two_frame_local(P1, P2, left, right, a.x, a.y, b.x, b.y, s.inv_depth[l], s.w_kf[k2], r, Jd, L1, L2);
    double rho;
    const double sc = robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
    c = 0.5 * rho;
    if (!COST_ONLY) {
      {
        const double s1 = (pose_const[k1] & 1) ? 0.0 : sc, s2 = (pose_const[k2] & 1) ? 0.0 : sc;
#pragma unroll
        for (int q = 0; q < 12; ++q) { L1[q] *= s1; L2[q] *= s2; }
      }
      const double r0 = sc * r[0], r1 = sc * r[1], d0 = sc * Jd[0], d1 = sc * Jd[1];
      atomicAdd(&C[l], d0 * d0 + d1 * d1);
      atomicAdd(&gr[l], d0 * r0 + d1 * r1);
      if (k1 == k2) {   // degenerate: both pose blocks are the same parameter
#pragma unroll
        for (int q = 0; q < 12; ++q) L1[q] += L2[q];
        add_block66(B, ld, 6 * k1, 6 * k1, L1, L1);
#pragma unroll
        for (int q = 0; q < 6; ++q) { atomicAdd(&gc[6 * k1 + q], L1[q] * r0 + L1[6 + q] * r1); atomicAdd(&E[(size_t)l * ldE + 6 * k1 + q], L1[q] * d0 + L1[6 + q] * d1); }
      } else {
        add_block66(B, ld, 6 * k1, 6 * k1, L1, L1);
        add_block66(B, ld, 6 * k2, 6 * k2, L2, L2);
        if (k2 > k1) add_block66(B, ld, 6 * k2, 6 * k1, L2, L1); else add_block66(B, ld, 6 * k1, 6 * k2, L1, L2);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          atomicAdd(&gc[6 * k1 + q], L1[q] * r0 + L1[6 + q] * r1);
          atomicAdd(&gc[6 * k2 + q], L2[q] * r0 + L2[6 + q] * r1);
          atomicAdd(&E[(size_t)l * ldE + 6 * k1 + q], L1[q] * d0 + L1[6 + q] * d1);
          atomicAdd(&E[(size_t)l * ldE + 6 * k2 + q], L2[q] * d0 + L2[6 + q] * d1);
        }
      }
    }
  }
  block_add(c, cost);
}

// TwoFrame linearisation, fast path: blocks sorted by CURRENT keyframe k2 and every workgroup handed a run of blocks that
// share one k2 (host-built work list).  Then
//   * B[k2,k2] and g[k2] are wave-shuffle reductions (one LDS add per wave, one global flush per workgroup),
//   * B[k1,k1], g[k1] and the cross block B[k2,k1] only depend on k1 <= n_kf: accumulated with ds_add_f64 in a
//     [n_kf][63] LDS table and flushed once per workgroup (non-zero entries only),
//   * only the landmark-indexed sums (C, g_rho, E rows) remain global atomics: 14 per block instead of 134.
// DYN: the LDS tables are carved from the launch's dynamic LDS, sized by the window's n_kf (k_lin_visual: 32 KB at 50 keyframes instead of
// 79 KB of static arrays sized for 64 — three workgroups per CU instead of two)
template <bool DYN = false>
__device__ __forceinline__ void lin_tf_sorted_body(const int vb, const TfWork* __restrict__ work, int n_kf, const double2* __restrict__ fo,
                                                      const double2* __restrict__ ob, const int* __restrict__ lm,
                                                      const int* __restrict__ kf1, StateP s, CamD left, CamD right, double huber,
                                                      const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
                                                      double* __restrict__ gc, double* __restrict__ E, int ldE,
                                                      double* __restrict__ C, double* __restrict__ gr, double* __restrict__ cost, int unique_lk2,
                                                      unsigned long long* dbg = nullptr, const TfCompact cp = TfCompact{0, nullptr, nullptr, nullptr, nullptr, 1}, const int dbg_nw = 0) {
  __shared__ PoseD s_pose_st[DYN ? 1 : kMaxStagedKf];
  __shared__ double s_acc_st[DYN ? 1 : kMaxStagedKf * kAccSlots];
  __shared__ double s_k2_st[DYN ? 1 : 27];
  extern __shared__ double lin_lds[];
  PoseD* s_pose = DYN ? reinterpret_cast<PoseD*>(lin_lds) : s_pose_st;
  double* s_acc = DYN ? lin_lds + (sizeof(PoseD) / 8) * n_kf : s_acc_st;
  double* s_k2 = DYN ? s_acc + kAccSlots * n_kf : s_k2_st;
  // per-wave staging of the segmented first-keyframe sums (DYN only): [64 lanes][8 slots + 1 pad] doubles + the lanes' first keyframes
  double* s_stage = DYN ? s_k2 + 32 + (threadIdx.x >> 6) * kStageWave : nullptr;
  int* s_stage_k1 = reinterpret_cast<int*>(s_stage + 64 * 9);
  const TfWork w = work[vb];
  auto mark = [&](int k) { if (dbg && threadIdx.x == 0) dbg[(size_t)vb * 8 + k] = wall_clock64(); };   // LVF_LIN_TIMING=1: phase stamps (100 MHz)
  // ... and per wave (lane 0 of each): [0] before the evaluation, [1] after it, [2] after the first-keyframe sums, [3] = number of first-keyframe groups
  unsigned long long* dbgw = dbg ? dbg + (size_t)dbg_nw * 8 + 8 + (size_t)vb * 16 + (threadIdx.x >> 6) * 4 : nullptr;
  auto markw = [&](int k) { if (dbgw && (threadIdx.x & 63) == 0) dbgw[k] = wall_clock64(); };
  mark(0);
  for (int e = threadIdx.x; e < n_kf * kAccSlots; e += kT) s_acc[e] = 0.0;
  if (threadIdx.x < 27) s_k2[threadIdx.x] = 0.0;
  stage_poses<kT>(s_pose, s.poses, n_kf);   // ends with __syncthreads()
  mark(1);
  const int k2 = w.k2;
  double c = 0.0;
  double v[27];
#pragma unroll
  for (int q = 0; q < 27; ++q) v[q] = 0.0;
  const bool active = (int)threadIdx.x < w.count;
  markw(0);
  int k1 = 0;
  double L1[12], L2[12], r0 = 0.0, r1 = 0.0;
#pragma unroll
  for (int q = 0; q < 12; ++q) { L1[q] = 0.0; L2[q] = 0.0; }
  if (active) {
    const int i = w.first + threadIdx.x;
    const int l = lm[i];
    k1 = kf1[i];
    const double2 a = fo[i], b = ob[i];
    double r[2], Jd[2];
    eval_two_frame_local(s_pose[k1], s_pose[k2], left, right, a.x, a.y, b.x, b.y, s.inv_depth[l], s.w_kf[k2], r, Jd, L1, L2);      // pose rows in tangent coordinates, closed form
    double rho;
    const double sc = robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
    c = 0.5 * rho;
    {
      const double s1 = (pose_const[k1] & 1) ? 0.0 : sc, s2 = (pose_const[k2] & 1) ? 0.0 : sc;
#pragma unroll
      for (int q = 0; q < 12; ++q) { L1[q] *= s1; L2[q] *= s2; }
    }
    r0 = sc * r[0]; r1 = sc * r[1];
    const double d0 = sc * Jd[0], d1 = sc * Jd[1];
    if (cp.on) {
      // atomic-free mode: the k2 columns of the landmark's E row have ONE writer (plain stores); the contributions to C, g_rho and to the
      // k1 columns go to this block's slot of the landmark's track as one 64-byte record (summed per landmark by k_prepare)
      double* el = E + (size_t)l * ldE + 6 * k2;
      double2* rec = reinterpret_cast<double2*>(cp.slotB + (size_t)cp.slot[i] * 8);
      double e1[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) { e1[q] = L1[q] * d0 + L1[6 + q] * d1; el[q] = L2[q] * d0 + L2[6 + q] * d1; }
      rec[0] = make_double2(e1[0], e1[1]); rec[1] = make_double2(e1[2], e1[3]); rec[2] = make_double2(e1[4], e1[5]);
      rec[3] = make_double2(d0 * d0 + d1 * d1, d0 * r0 + d1 * r1);
    } else {
      atomicAdd(&C[l], d0 * d0 + d1 * d1);
      atomicAdd(&gr[l], d0 * r0 + d1 * r1);
      double* el = E + (size_t)l * ldE;
      // E[l][k2 columns] has exactly ONE writer when no landmark is observed twice by a keyframe (checked on the host when the batch
      // is created; always true for what BuildProblem builds): plain stores.
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        atomicAdd(&el[6 * k1 + q], L1[q] * d0 + L1[6 + q] * d1);
        const double e2 = L2[q] * d0 + L2[6 + q] * d1;
        if (unique_lk2) el[6 * k2 + q] = e2; else atomicAdd(&el[6 * k2 + q], e2);
      }
    }
  }
  mark(2); markw(1);
  // k1-indexed sums (B[k1,k1], g[k1], cross block).  A live front-end hands out landmark ids in creation order, so the blocks of a
  // wave usually share their first keyframe (per-lane ds_add_f64 on ONE address serialises 64-fold: +10 us on this kernel with ids in
  // birth order).
  {
    // the k2-indexed products v[27] (reduced below)
    {
      int q = 0;
#pragma unroll
      for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = 0; y <= x; ++y) v[q++] = L2[x] * L2[y] + L2[6 + x] * L2[6 + y];
#pragma unroll
      for (int x = 0; x < 6; ++x) v[21 + x] = L2[x] * r0 + L2[6 + x] * r1;
    }
    // The 63 k1-indexed products, slot order = [B(k1,k1) 21 | g(k1) 6 | cross (k2,k1) 36].  Lanes that share their first keyframe
    // are reduced TOGETHER (two transposed reductions of 32 slots, formed one batch at a time to keep the register count where three
    // workgroups fit a CU) — up to four groups of >= 16 lanes per wave, which covers whole waves and the waves that straddle a boundary
    // between two first keyframes; whatever is left (random landmark ids: nearly every lane its own keyframe) goes through per-lane
    // LDS atomics, which are only slow when many lanes hit one address.
    const int lane = threadIdx.x & 63;
    unsigned long long remaining = __ballot(active);
    bool mine_done = !active;
    // a wave with at most four first keyframes (creation-order ids: one or two long runs and a short one at a boundary) is reduced
    // group by group whatever the group sizes: a 10-lane group left to the atomics serialises 10-fold on each of its 63 addresses
    int n_groups = 0;
    for (unsigned long long rem = remaining; rem && n_groups < 5; ++n_groups)
      rem &= ~__ballot(active && k1 == __builtin_amdgcn_readlane(k1, (int)__ffsll((long long)rem) - 1));
    const int min_group = n_groups <= 4 ? 1 : 16;
    if (dbgw && lane == 0) dbgw[3] = (unsigned long long)n_groups;
#pragma unroll 1
    for (int round = 0; round < 4 && remaining; ++round) {
      const int k1u = __builtin_amdgcn_readlane(k1, (int)__ffsll((long long)remaining) - 1);
      const bool sel = active && !mine_done && k1 == k1u;
      const unsigned long long m = __ballot(sel);
      if (__popcll(m) < min_group) break;
      double* accu = s_acc + k1u * kAccSlots;
      // the group's lanes keep their first-keyframe Jacobian, everyone else contributes zeros; the scale is opaque to the compiler so
      // that the 63 products are formed inside this loop (hoisted out of it as loop invariants they cost 126 registers)
      double z = sel ? 1.0 : 0.0;
      asm volatile("" : "+v"(z));
      double M[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) M[i] = L1[i] * z;
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) {
        double t[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) t[i] = 0.0;
        int q = 0;
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int y = 0; y <= x; ++y) { if ((q >> 5) == bt) t[q & 31] = M[x] * L1[y] + M[6 + x] * L1[6 + y]; ++q; }
#pragma unroll
        for (int x = 0; x < 6; ++x) { if ((q >> 5) == bt) t[q & 31] = M[x] * r0 + M[6 + x] * r1; ++q; }
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int y = 0; y < 6; ++y) { if ((q >> 5) == bt) t[q & 31] = L2[x] * M[y] + L2[6 + x] * M[6 + y]; ++q; }
        const double tot = wave_sum32(t);
        const int slot = 32 * bt + (lane >> 1);
        if (!(lane & 1) && slot < 63 && tot != 0.0) atomicAdd(&accu[slot], tot);
      }
      mine_done = mine_done || sel;
      remaining &= ~m;
    }
    if (DYN && n_groups > 4 && cp.staged) {
      // Many first keyframes in one wave (the old tail of a late keyframe's run: dozens of groups of one to three blocks; or landmark ids
      // in no order).  LDS f64 atomics retire at ~2 lane-operations per clock per CU (measured: 63 per lane cost a wave 8-10 us with
      // three workgroups on the CU), so their NUMBER is what counts: the 63 products go through a wave-private LDS tile eight slots
      // at a time, lane (slot s, part) walks 8 consecutive lanes' values and adds one partial sum per run of equal first keyframes —
      // 63 x (segments + 7) atomics per wave instead of 63 x 64 (blocks sorted by first keyframe: a few hundred instead of 4 032).
      // (lanes the group rounds above have served contribute zeros below)
      double z = (active && !mine_done) ? 1.0 : 0.0;
      asm volatile("" : "+v"(z));
      double M[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) M[i] = L1[i] * z;
      s_stage_k1[lane] = (active && !mine_done) ? k1 : -1;
      const int ss = lane & 7, part = lane >> 3;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // the first keyframes of this lane's 8 rows (and of the row behind them), once: everything the segment logic needs sits in registers
      // before the first atomic (the compiler orders LDS reads behind LDS atomics it cannot tell apart from them)
      int kk[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) kk[j] = (8 * part + j < 64) ? s_stage_k1[8 * part + j] : -2;
#pragma unroll
      for (int ch = 0; ch < 8; ++ch) {
        double t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = 0.0;
        int q = 0;
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int y = 0; y <= x; ++y) { if ((q >> 3) == ch) t[q & 7] = M[x] * L1[y] + M[6 + x] * L1[6 + y]; ++q; }
#pragma unroll
        for (int x = 0; x < 6; ++x) { if ((q >> 3) == ch) t[q & 7] = M[x] * r0 + M[6 + x] * r1; ++q; }
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
          for (int y = 0; y < 6; ++y) { if ((q >> 3) == ch) t[q & 7] = L2[x] * M[y] + L2[6 + x] * M[6 + y]; ++q; }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i) s_stage[lane * 9 + i] = t[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int slot = 8 * ch + ss;
        double val[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = s_stage[(8 * part + j) * 9 + ss];
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          run += val[j];
          if (j == 7 || kk[j + 1] != kk[j]) {
            if (kk[j] >= 0 && slot < kAccSlots && run != 0.0) atomicAdd(&s_acc[kk[j] * kAccSlots + slot], run);
            run = 0.0;
          }
        }
      }
    } else if (!mine_done) {
      double* acc = s_acc + k1 * kAccSlots;
      int q = 0;
#pragma unroll
      for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = 0; y <= x; ++y) atomicAdd(&acc[q++], L1[x] * L1[y] + L1[6 + x] * L1[6 + y]);
#pragma unroll
      for (int x = 0; x < 6; ++x) atomicAdd(&acc[21 + x], L1[x] * r0 + L1[6 + x] * r1);
#pragma unroll
      for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = 0; y < 6; ++y) atomicAdd(&acc[27 + 6 * x + y], L2[x] * L1[y] + L2[6 + x] * L1[6 + y]);
    }
  }
  mark(3); markw(2);
  {
    // the 27 sums of the wave in one transposed reduction: lane l ends up with the total of value l >> 1, the even lanes add them
    double v32[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v32[q] = q < 27 ? v[q] : 0.0;
    const double tot = wave_sum32(v32);
    const int lane = threadIdx.x & 63;
    if (!(lane & 1) && (lane >> 1) < 27 && tot != 0.0) atomicAdd(&s_k2[lane >> 1], tot);
  }
  block_add(c, cost);
  __syncthreads();
  mark(4);
  if (cp.on) {
    // the workgroup's sums leave as plain, fully coalesced stores into its own slab (rows k1 < k2 only; k_tf_reduce reads exactly those)
    if (threadIdx.x < kSlabQ) cp.slabQ[(size_t)vb * kSlabQ + threadIdx.x] = threadIdx.x < 27 ? s_k2[threadIdx.x] : 0.0;
    double* P = cp.slabP + (size_t)vb * n_kf * kSlabRow;
    for (int e = threadIdx.x; e < k2 * kSlabRow; e += kT) {
      const int kk = e >> 6, slot = e & 63;
      P[e] = slot < kAccSlots ? s_acc[kk * kAccSlots + slot] : 0.0;
    }
  } else {
  if (threadIdx.x < 27) {
    const double val = s_k2[threadIdx.x];
    if (val != 0.0) {
      if (threadIdx.x < 21) {
        int x = 0, rem = threadIdx.x;
        while (rem > x) { rem -= x + 1; ++x; }
        atomicAdd(&B[(size_t)(6 * k2 + x) * ld + 6 * k2 + rem], val);
      } else atomicAdd(&gc[6 * k2 + threadIdx.x - 21], val);
    }
  }
  for (int e = threadIdx.x; e < n_kf * kAccSlots; e += kT) {
    const double val = s_acc[e];
    if (val == 0.0) continue;
    const int k1 = e / kAccSlots, slot = e % kAccSlots;
    if (slot < 21) {
      int x = 0, rem = slot;
      while (rem > x) { rem -= x + 1; ++x; }
      atomicAdd(&B[(size_t)(6 * k1 + x) * ld + 6 * k1 + rem], val);
    } else if (slot < 27) {
      atomicAdd(&gc[6 * k1 + slot - 21], val);
    } else {
      const int x = (slot - 27) / 6, y = (slot - 27) % 6;   // x: k2 tangent index, y: k1 tangent index
      if (k2 > k1) atomicAdd(&B[(size_t)(6 * k2 + x) * ld + 6 * k1 + y], val);
      else atomicAdd(&B[(size_t)(6 * k1 + y) * ld + 6 * k2 + x], val);
    }
  }
  }
  __syncthreads();
  mark(5);
}
// ------------------------------------------------------------------------------------------------ candidate cost, visual factors
// One launch for the residual-only passes of the three reprojection batches (the workgroups of the launch are split into a
// TwoCamera, a TwoFrame and a PoseOnly segment): as three back-to-back launches of 4-9 us they were mostly launch boundaries.
// the calling thread's share of the candidate cost (workgroup b of the pass)
__device__ __forceinline__ double cost_visual_value(const int b, const CostArgs& A) {
  const CostVisual& a = A.a;
  const int n_kf = A.n_kf; const StateP s = A.s; const double huber = A.huber;
  const int tiles = A.tiles > 0 ? A.tiles : 1;          // tiles of kT blocks per workgroup (a batch of windows uses fatter workgroups: with
                                                        // 8 x 600 thin ones the launch took 52 us, with a quarter of them 31)
  __shared__ PoseD s_pose[kMaxStagedKf];
  double c = 0.0;
  if (b < a.g_tc) {
    for (int rp = 0; rp < tiles; ++rp) {
      const int i = (b * tiles + rp) * kT + threadIdx.x;
      if (i < a.n_tc) {
        const int l = a.tc_lm[i];
        const double2 lo = a.tc_lo[i], ro = a.tc_ro[i];
        double r[2], J[2];
        eval_two_camera<false>(a.tc_left, a.tc_right, lo.x, lo.y, ro.x, ro.y, s.inv_depth[l], a.tc_w ? a.tc_w[i] : 5.0 * s.w_kf[a.tc_kf[i]], r, J);
        double rho;
        (void)robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
        c += 0.5 * rho;
      }
    }
  } else {
    stage_poses<kT>(s_pose, s.poses, n_kf);     // ends with __syncthreads(); the branch is workgroup-uniform
    if (b < a.g_tc + a.g_tf) {
      for (int rp = 0; rp < tiles; ++rp) {
        const int i = ((b - a.g_tc) * tiles + rp) * kT + threadIdx.x;
        if (i < a.n_tf) {
          const int l = a.tf_lm[i], k1 = a.tf_k1[i], k2 = a.tf_k2[i];
          const double2 fo = a.tf_fo[i], ob = a.tf_ob[i];
          const PoseD P1 = fetch_pose(s_pose, s.poses, n_kf, k1), P2 = fetch_pose(s_pose, s.poses, n_kf, k2);
          double r[2], Jd[2], J1[14], J2[14];
          eval_two_frame<false>(P1, P2, a.tf_left, a.tf_right, fo.x, fo.y, ob.x, ob.y, s.inv_depth[l], s.w_kf[k2], r, Jd, J1, J2);
          double rho;
          (void)robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
          c += 0.5 * rho;
        }
      }
    } else {
      for (int rp = 0; rp < tiles; ++rp) {
        const int i = ((b - a.g_tc - a.g_tf) * tiles + rp) * kT + threadIdx.x;
        if (i < a.n_po) {
          const int k = a.po_kf[i], l = a.po_pwi[i];
          const double2 o = a.po_ob[i];
          const PoseD P = fetch_pose(s_pose, s.poses, n_kf, k);
          const double pwl[3] = {a.po_pw[3 * l], a.po_pw[3 * l + 1], a.po_pw[3 * l + 2]};
          double r[2], J[14];
          eval_pose_only<false>(P, a.po_cam, o.x, o.y, pwl, s.w_kf[k], r, J);
          double rho;
          (void)robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
          c += 0.5 * rho;
        }
      }
    }
  }
  return c;
}
__device__ __forceinline__ void cost_visual_body(const int b, const CostArgs& A) {
  if (b >= A.nblocks || (A.done && *A.done)) return;
  block_add(cost_visual_value(b, A), A.cost);
}
__global__ __launch_bounds__(kT) void k_cost_visual(CostArgs a) { cost_visual_body(blockIdx.x, a); }

// ------------------------------------------------------------------------------------------------ PoseOnly
template <bool COST_ONLY, bool DYN = false>
__device__ __forceinline__ void lin_po_body(const int vb, int n, int n_kf, const double2* __restrict__ ob, const int* __restrict__ kf,
                                               const int* __restrict__ pwi, const double* __restrict__ pw, StateP s, CamD cam,
                                               double huber, const uint8_t* __restrict__ pose_const, double* __restrict__ B,
                                               int ld, double* __restrict__ gc, double* __restrict__ cost) {
  __shared__ PoseD s_pose_st[DYN ? 1 : kMaxStagedKf];
  extern __shared__ double lin_lds[];
  PoseD* s_pose = DYN ? reinterpret_cast<PoseD*>(lin_lds) : s_pose_st;
  stage_poses<kT>(s_pose, s.poses, n_kf);
  const int i = vb * kT + threadIdx.x;
  double c = 0.0;
  int k = -1;
  double v[27];
#pragma unroll
  for (int q = 0; q < 27; ++q) v[q] = 0.0;
  if (i < n) {
    k = kf[i];
    const int l = pwi[i];
    const double2 o = ob[i];
    const PoseD P = fetch_pose(s_pose, s.poses, n_kf, k);
    const double pwl[3] = {pw[3 * l], pw[3 * l + 1], pw[3 * l + 2]};
    double r[2], Lc[12];
    if (COST_ONLY) { double J[14]; eval_pose_only<false>(P, cam, o.x, o.y, pwl, s.w_kf[k], r, J); }
    else eval_pose_only_local(P, cam, o.x, o.y, pwl, s.w_kf[k], r, Lc);
    double rho;
    const double sc = robust_scale(huber, r[0] * r[0] + r[1] * r[1], rho);
    c = 0.5 * rho;
    if (!COST_ONLY) {
      {
        const double sl = (pose_const[k] & 1) ? 0.0 : sc;
#pragma unroll
        for (int q = 0; q < 12; ++q) Lc[q] *= sl;
      }
      const double r0 = sc * r[0], r1 = sc * r[1];
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) v[q++] = Lc[a] * Lc[b] + Lc[6 + a] * Lc[6 + b];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[21 + a] = Lc[a] * r0 + Lc[6 + a] * r1;
    }
  }
  if (!COST_ONLY) {
    // blocks are normally sorted by keyframe: when the whole wave shares one pose block, reduce the 21+6 sums with wave shuffles
    // (the per-pose-block JtJ/Jtr reduction of the north star).  The wave sums then meet in a per-workgroup LDS table
    // [n_kf][27] and only its non-zero entries go to global memory: ~15 waves per keyframe used to hit the SAME 27 addresses of B
    // with global atomics, which serialise in L2.
    __shared__ double s_acc_st[DYN ? 1 : kMaxStagedKf * 27];
    double* s_acc = DYN ? lin_lds + (sizeof(PoseD) / 8) * n_kf : s_acc_st;
    const bool lds_path = n_kf <= kMaxStagedKf;
    if (lds_path) {
      for (int e = threadIdx.x; e < n_kf * 27; e += kT) s_acc[e] = 0.0;
      __syncthreads();
    }
    const int k0 = __shfl(k, 0);
    const bool uniform = __all(k == k0) && k0 >= 0;
    if (uniform) {
#pragma unroll
      for (int q = 0; q < 27; ++q) v[q] = wave_sum(v[q]);
      if ((threadIdx.x & 63) == 0) {
        if (lds_path) { for (int q = 0; q < 27; ++q) atomicAdd(&s_acc[k0 * 27 + q], v[q]); }
        else {
          int q = 0;
          for (int a = 0; a < 6; ++a) for (int b = 0; b <= a; ++b) atomicAdd(&B[(size_t)(6 * k0 + a) * ld + 6 * k0 + b], v[q++]);
          for (int a = 0; a < 6; ++a) atomicAdd(&gc[6 * k0 + a], v[21 + a]);
        }
      }
    } else if (k >= 0) {
      if (lds_path) { for (int q = 0; q < 27; ++q) atomicAdd(&s_acc[k * 27 + q], v[q]); }
      else {
        int q = 0;
        for (int a = 0; a < 6; ++a) for (int b = 0; b <= a; ++b) atomicAdd(&B[(size_t)(6 * k + a) * ld + 6 * k + b], v[q++]);
        for (int a = 0; a < 6; ++a) atomicAdd(&gc[6 * k + a], v[21 + a]);
      }
    }
    if (lds_path) {
      __syncthreads();
      for (int e = threadIdx.x; e < n_kf * 27; e += kT) {
        const double val = s_acc[e];
        if (val == 0.0) continue;
        const int kk = e / 27, slot = e - kk * 27;
        if (slot < 21) {
          int x = 0, rem = slot;
          while (rem > x) { rem -= x + 1; ++x; }
          atomicAdd(&B[(size_t)(6 * kk + x) * ld + 6 * kk + rem], val);
        } else atomicAdd(&gc[6 * kk + slot - 21], val);
      }
    }
  }
  block_add(c, cost);
}
template <bool COST_ONLY>
__global__ __launch_bounds__(kT) void k_lin_po(int n, int n_kf, const double2* __restrict__ ob, const int* __restrict__ kf,
                                               const int* __restrict__ pwi, const double* __restrict__ pw, StateP s, CamD cam,
                                               double huber, const uint8_t* __restrict__ pose_const, double* __restrict__ B,
                                               int ld, double* __restrict__ gc, double* __restrict__ cost) { lin_po_body<COST_ONLY>(blockIdx.x, n, n_kf, ob, kf, pwi, pw, s, cam, huber, pose_const, B, ld, gc, cost); }

// ------------------------------------------------------------------------------------------------ IMU
// consumes the materialised ImuError outputs (res[n][15], eight Jacobian blocks) of launch_imu; one wave per factor
__global__ __launch_bounds__(64) void k_lin_imu(int n, int n_kf, const double* __restrict__ res, ImuJ J, const int* __restrict__ kf_i,
                                                const int* __restrict__ kf_j, const double* __restrict__ poses,
                                                const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
                                                double* __restrict__ gc, double* __restrict__ cost) {
  __shared__ double sJ[15 * 30];   // local Jacobian: [pose_i 6 | vbb_i 9 | pose_j 6 | vbb_j 9]
  __shared__ double sr[15];
  __shared__ int sidx[30];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int ki = kf_i[f], kj = kf_j[f];
  if (lane < 15) sr[lane] = res[(size_t)f * 15 + lane];
  if (lane < 30) {
    int g;
    if (lane < 6) g = 6 * ki + lane; else if (lane < 15) g = 6 * n_kf + 9 * ki + (lane - 6);
    else if (lane < 21) g = 6 * kj + (lane - 15); else g = 6 * n_kf + 9 * kj + (lane - 21);
    sidx[lane] = g;
  }
  // pose blocks: 15 rows x (7 -> 6)
  for (int e = lane; e < 30; e += 64) {
    const int row = e % 15, which = e / 15;            // which: 0 = pose_i, 1 = pose_j
    const double* Jr = (which ? J.j[4] : J.j[0]) + (size_t)f * 105 + 7 * row;
    const int kk = which ? kj : ki;
    const double* q = poses + 7 * kk;
    const double sc = (pose_const[kk] & 1) ? 0.0 : 1.0;
    double l3[3];
    quat_row_to_local(Jr, q, l3);
    double* o = sJ + row * 30 + (which ? 15 : 0);
    o[0] = sc * l3[0]; o[1] = sc * l3[1]; o[2] = sc * l3[2]; o[3] = sc * Jr[4]; o[4] = sc * Jr[5]; o[5] = sc * Jr[6];
  }
  for (int e = lane; e < 15 * 18; e += 64) {           // six 15x3 blocks
    const int row = e / 18, c = e % 18, blk = c / 3, cc = c % 3;   // blk 0..2 -> (v,ba,bg)_i ; 3..5 -> _j
    const int src = blk < 3 ? 1 + blk : 5 + (blk - 3);
    const double* jp = src == 1 ? J.j[1] : (src == 2 ? J.j[2] : (src == 3 ? J.j[3] : (src == 5 ? J.j[5] : (src == 6 ? J.j[6] : J.j[7]))));
    const double scv = ((pose_const[blk < 3 ? ki : kj] >> (1 + blk % 3)) & 1) ? 0.0 : 1.0;      // constant (v | ba | bg) block: bits 1..3 of the mask
    sJ[row * 30 + (blk < 3 ? 6 + 3 * blk : 21 + 3 * (blk - 3)) + cc] = scv * jp[(size_t)f * 45 + 3 * row + cc];
  }
  __syncthreads();
  double c = 0.0;
  if (lane < 15) c = 0.5 * sr[lane] * sr[lane];
  c = wave_sum(c);
  if (lane == 0) atomicAdd(cost + (blockIdx.x & (kStripes - 1)), c);
  for (int e = lane; e < 30 * 30; e += 64) {
    const int a = e / 30, b = e % 30;
    const int ga = sidx[a], gb = sidx[b];
    if (gb > ga || (ga == gb && a != b)) continue;    // lower triangle in GLOBAL indices (kf_i != kf_j is validated)
    double h = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) h += sJ[k * 30 + a] * sJ[k * 30 + b];
    atomicAdd(&B[(size_t)ga * ld + gb], h);
  }
  if (lane < 30) {
    double g = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) g += sJ[k * 30 + lane] * sr[k];
    atomicAdd(&gc[sidx[lane]], g);
  }
}

// the same accumulation for use inside a 256-thread workgroup: wave w of virtual block vb takes factor 4 vb + w
template <bool DYN = false>
__device__ __forceinline__ void lin_imu_body4(const int vb, int n, int n_kf, const double* __restrict__ res, ImuJ J, const int* __restrict__ kf_i,
                                              const int* __restrict__ kf_j, const double* __restrict__ poses,
                                              const uint8_t* __restrict__ pose_const, double* __restrict__ B, int ld,
                                              double* __restrict__ gc, double* __restrict__ cost) {
  __shared__ double sJ4[DYN ? 1 : 4 * 15 * 30];
  __shared__ double sr4[DYN ? 1 : 4 * 16];
  __shared__ int sidx4[DYN ? 1 : 4 * 32];
  extern __shared__ double lin_lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = 4 * vb + w;
  const bool active = f < n;
  double* sJ = (DYN ? lin_lds : sJ4) + w * 450;
  double* sr = (DYN ? lin_lds + 1800 : sr4) + w * 16;
  int* sidx = (DYN ? reinterpret_cast<int*>(lin_lds + 1864) : sidx4) + w * 32;
  if (active) {
    const int ki = kf_i[f], kj = kf_j[f];
    if (lane < 15) sr[lane] = res[(size_t)f * 15 + lane];
    if (lane < 30) {
      int g;
      if (lane < 6) g = 6 * ki + lane; else if (lane < 15) g = 6 * n_kf + 9 * ki + (lane - 6);
      else if (lane < 21) g = 6 * kj + (lane - 15); else g = 6 * n_kf + 9 * kj + (lane - 21);
      sidx[lane] = g;
    }
    // (static indices only: indexing the by-value pointer table with a run-time value puts it in scratch memory, and a kernel with a
    // scratch segment pays several microseconds of dispatch set-up.  A select between two entries by a run-time value is folded into
    // exactly such an index, so the block loops below are unrolled: every entry is named by a constant)
#pragma unroll
    for (int which = 0; which < 2; ++which) {            // which: 0 = pose_i, 1 = pose_j
      if (lane < 15) {
        const int row = lane;
        const double* Jr = J.j[which ? 4 : 0] + (size_t)f * 105 + 7 * row;
        const int kk = which ? kj : ki;
        const double* q = poses + 7 * kk;
        const double sc = (pose_const[kk] & 1) ? 0.0 : 1.0;
        double l3[3];
        quat_row_to_local(Jr, q, l3);
        double* o = sJ + row * 30 + (which ? 15 : 0);
        o[0] = sc * l3[0]; o[1] = sc * l3[1]; o[2] = sc * l3[2]; o[3] = sc * Jr[4]; o[4] = sc * Jr[5]; o[5] = sc * Jr[6];
      }
    }
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {                  // six 15x3 blocks: blk 0..2 -> (v,ba,bg)_i = J.j[1..3] ; 3..5 -> _j = J.j[5..7]
      const double* jp = J.j[blk < 3 ? 1 + blk : 2 + blk];
      // a constant velocity / bias block (bits 1..3 of the keyframe's mask; Environment::Optimize holds all of them, environment.cpp:62-68) keeps
      // its residual but gets no Jacobian columns
      const double scv = ((pose_const[blk < 3 ? ki : kj] >> (1 + blk % 3)) & 1) ? 0.0 : 1.0;
      if (lane < 45) {
        const int row = lane / 3, cc = lane % 3;
        sJ[row * 30 + (blk < 3 ? 6 + 3 * blk : 21 + 3 * (blk - 3)) + cc] = scv * jp[(size_t)f * 45 + 3 * row + cc];
      }
    }
  }
  __syncthreads();
  double c = 0.0;
  if (active && lane < 15) c = 0.5 * sr[lane] * sr[lane];
  c = wave_sum(c);
  if (!active) return;
  if (lane == 0) atomicAdd(cost + (f & (kStripes - 1)), c);
  for (int e = lane; e < 30 * 30; e += 64) {
    const int a = e / 30, b = e % 30;
    const int ga = sidx[a], gb = sidx[b];
    if (gb > ga || (ga == gb && a != b)) continue;    // lower triangle in GLOBAL indices (kf_i != kf_j is validated)
    double h = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) h += sJ[k * 30 + a] * sJ[k * 30 + b];
    atomicAdd(&B[(size_t)ga * ld + gb], h);
  }
  if (lane < 30) {
    double g = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) g += sJ[k * 30 + lane] * sr[k];
    atomicAdd(&gc[sidx[lane]], g);
  }
}

// ------------------------------------------------------------------------------------------------ linearisation, visual factors
// The TwoFrame (sorted fast path), TwoCamera and PoseOnly linearisations as ONE launch: workgroups [0, n_tfw) take the TwoFrame
// work list, the next g_tc the TwoCamera blocks, the rest the PoseOnly blocks.  The two small passes (4.6 + 8.8 us as launches of
// their own) disappear under the TwoFrame pass; all three only meet in B, gc, C, g_rho through atomics.  A fourth segment
// accumulates the ImuError blocks (four factors per workgroup) from the Jacobians k_imu<true> materialised just before.
// ImuError factors of the merged linearisation launch: EVALUATED and accumulated by the same workgroup (one factor per workgroup), so the linearisation needs no IMU launch ahead of it and the weighted Jacobian never leaves LDS:
//   stage sqrt_info -> one lane forms the raw residual and the 15 x 32 pre-weighting Jacobian -> all lanes weight them ->
//   pose columns to tangent coordinates -> J^T J / J^T r into B / gc, 1/2 |r|^2 into the cost.
// LDS (doubles): sS 225 | sM 480 (later the local 15 x 30 Jacobian) | sJw 480 | sr0 16 | sr 16 | sidx 16  = kImuWaveLds.
__device__ __forceinline__ void lin_imu_eval_body(const int f, const ImuEvalArgs& I, int n_kf, const StateP& s, const uint8_t* __restrict__ pose_const,
                                                  double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost, unsigned long long* dbg) {
  // ONE factor per workgroup: the evaluation's serial part (one lane) is what it is, everything around it is spread over all kT threads
  extern __shared__ double lin_lds[];
  const int tid = threadIdx.x;
  if (f >= I.n) return;
  if (f != 0 || tid != 0) dbg = nullptr;               // LVF_LIN_TIMING: factor 0 stamps its phases
  if (dbg) dbg[0] = wall_clock64();
  double* sS = lin_lds;
  double* sM = sS + 225;
  double* sJw = sM + 480;
  double* sr0 = sJw + 480;
  double* sr = sr0 + 16;
  int* sidx = reinterpret_cast<int*>(sr + 16);
  double* sP = reinterpret_cast<double*>(sidx + 32);      // [248] what the one-lane section reads of the pre-integration
  double* sX = sP + 248;                                  // [32] pose, v, ba, bg of keyframe i (0..15) and j (16..31)
  // everything the one-lane section reads is staged by the whole workgroup first (as single-lane global reads they were two cold round trips of its 3.6 us)
  const int ki = I.kf_i[f], kj = I.kf_j[f];
  for (int k = tid; k < 225; k += kT) sS[k] = I.sqrt_info[(size_t)f * 225 + k];
  for (int k = tid; k < OFF_COV; k += kT) sP[k] = I.pre[(size_t)f * kPre + k];
  if (tid < 32) {
    const int kk = tid < 16 ? ki : kj, c = tid & 15;
    sX[tid] = c < 7 ? s.poses[7 * kk + c] : (c < 10 ? s.vel[3 * kk + c - 7] : (c < 13 ? s.ba[3 * kk + c - 10] : s.bg[3 * kk + c - 13]));
  }
  int* smask = reinterpret_cast<int*>(sX + 32);           // the two keyframes' constant-block masks
  if (tid >= 32 && tid < 34) smask[tid - 32] = pose_const[tid == 32 ? ki : kj];
  for (int k = tid; k < 480; k += kT) sM[k] = 0.0;
  __syncthreads();
  if (dbg) dbg[1] = wall_clock64();
  if (tid == 0) imu_raw16<true>(sP, sX, sr0, sM);
  __syncthreads();
  if (dbg) dbg[2] = wall_clock64();
  {
    const double r = imu_weighted_residual(tid, sS, sr0);
    if (tid < 15) sr[tid] = r;
    for (int e = tid; e < 480; e += kT) sJw[e] = imu_weighted_jacobian(e, sS, sM);
    if (tid < 30) {
      int g;
      if (tid < 6) g = 6 * ki + tid; else if (tid < 15) g = 6 * n_kf + 9 * ki + (tid - 6);
      else if (tid < 21) g = 6 * kj + (tid - 15); else g = 6 * n_kf + 9 * kj + (tid - 21);
      sidx[tid] = g;
    }
  }
  __syncthreads();                                   // sM is dead from here: it becomes the local Jacobian sJ[15][30]
  double* sJ = sM;
  if (tid < 30) {
    const int row = tid % 15, which = tid / 15;          // which: 0 = pose_i, 1 = pose_j
    const double* Jr = sJw + 32 * row + (which ? 16 : 0);
    const double sc = (smask[which] & 1) ? 0.0 : 1.0;
    double l3[3];
    quat_row_to_local(Jr, sX + 16 * which, l3);
    double* o = sJ + row * 30 + (which ? 15 : 0);
    o[0] = sc * l3[0]; o[1] = sc * l3[1]; o[2] = sc * l3[2]; o[3] = sc * Jr[4]; o[4] = sc * Jr[5]; o[5] = sc * Jr[6];
  }
  for (int e = tid; e < 15 * 18; e += kT) {              // six 15x3 blocks: (v, ba, bg)_i = columns 7..15, (v, ba, bg)_j = columns 23..31
    const int row = e / 18, c = e % 18;
    const int cg = c < 9 ? c / 3 : (c - 9) / 3;          // 0 = v, 1 = ba, 2 = bg
    const double scv = ((smask[c < 9 ? 0 : 1] >> (1 + cg)) & 1) ? 0.0 : 1.0;      // constant (v | ba | bg) block: bits 1..3 of the mask
    sJ[row * 30 + (c < 9 ? 6 + c : 21 + (c - 9))] = scv * sJw[32 * row + (c < 9 ? 7 + c : 23 + (c - 9))];
  }
  __syncthreads();
  if (dbg) dbg[3] = wall_clock64();
  if (tid < 64) {
    double c = tid < 15 ? 0.5 * sr[tid] * sr[tid] : 0.0;
    c = wave_sum(c);
    if (tid == 0) atomicAdd(cost + (f & (kStripes - 1)), c);
  }
  for (int e = tid; e < 30 * 30; e += kT) {
    const int a = e / 30, b = e % 30;
    const int ga = sidx[a], gb = sidx[b];
    if (gb > ga || (ga == gb && a != b)) continue;    // lower triangle in GLOBAL indices (kf_i != kf_j is validated)
    double h = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) h += sJ[k * 30 + a] * sJ[k * 30 + b];
    atomicAdd(&B[(size_t)ga * ld + gb], h);
  }
  if (tid < 30) {
    double g = 0.0;
#pragma unroll
    for (int k = 0; k < 15; ++k) g += sJ[k * 30 + tid] * sr[k];
    atomicAdd(&gc[sidx[tid]], g);
  }
  if (dbg) dbg[4] = wall_clock64();
}

// set: the accumulator set written (1: A.acc's pointers); s: the state linearised at; cost: where 1/2 sum rho goes (striped)
__device__ __forceinline__ void lin_visual_run(const int bx, const LinArgs& A, const int set, const StateP s, double* cost) {
  const LinVisual& a = A.v;
  // the ImuError workgroups come FIRST: each is a ~12 us chain with a one-lane section, and dispatched last (of the last window of a
  // batch) it would stick out behind everything else
  const int g_imu_first = a.imu.pre ? a.n_imu : 0;
  const int b = bx - g_imu_first;
  const int n_kf = A.n_kf; const double huber = A.huber; const uint8_t* pose_const = A.pose_const;
  // (the set's pointers by arithmetic: a select between two fields of the by-value argument block is folded into a run-time index into it,
  // which puts the block in scratch memory)
  auto pick = [set](GP<double> p0, GP<double> p1) -> double* { return (double*)(p0.p + (p1.p - p0.p) * (ptrdiff_t)set); };
  double* B = pick(A.B, A.acc.B); const int ld = A.ld; double* gc = pick(A.gc, A.acc.gc); double* E = pick(A.E, A.acc.E); const int ldE = A.ldE;
  double* C = pick(A.C, A.acc.C); double* gr = pick(A.gr, A.acc.gr);
  TfCompact cp = a.cp;
  cp.slotB = pick(a.cp.slotB, A.acc.slotB);
  if (bx < g_imu_first)
    lin_imu_eval_body(bx, a.imu, n_kf, s, pose_const, B, ld, gc, cost, A.dbg ? A.dbg + (size_t)a.n_tfw * 8 : nullptr);
  else if (b < a.n_tfw)
    lin_tf_sorted_body<true>(b, a.work, n_kf, a.tf_fo, a.tf_ob, a.tf_lm, a.tf_k1, s, a.tf_left, a.tf_right, huber, pose_const, B, ld, gc, E, ldE, C, gr, cost,
                       a.unique_lk2, A.dbg, cp, a.n_tfw);
  else if (b < a.n_tfw + a.g_tc)
    lin_tc_body<false>(b - a.n_tfw, a.n_tc, a.tc_lo, a.tc_ro, a.tc_lm, a.tc_kf, a.tc_w, s, a.tc_left, a.tc_right, huber, C, gr, cost);
  else if (b < a.n_tfw + a.g_tc + a.g_po)
    lin_po_body<false, true>(b - a.n_tfw - a.g_tc, a.n_po, n_kf, a.po_ob, a.po_kf, a.po_pwi, a.po_pw, s, a.po_cam, huber, pose_const, B, ld, gc, cost);
  else
    lin_imu_body4<true>(b - a.n_tfw - a.g_tc - a.g_po, a.n_imu, n_kf, a.imu_res, a.imu_J, a.imu_i, a.imu_j, s.poses, pose_const, B, ld, gc, cost);
}
__device__ __forceinline__ void lin_visual_body(const int bx, const LinArgs& A) {
  if (bx >= A.nblocks || (A.done && *A.done)) return;
  if (bx == 0 && A.scal_reset) reset_step_scalars(A.scal_reset);
  lin_visual_run(bx, A, 0, A.s, A.cost);
}
// (three workgroups per CU: the register allocator is told so — left alone it lands one VGPR above the limit)
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(3))) void k_lin_visual(LinArgs a) { lin_visual_body(blockIdx.x, a); }
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(3))) void k_lin_visual_b(const LinArgs* __restrict__ t) { lin_visual_body(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(3))) void k_lin_visual_bt(const LinArgs* __restrict__ t) { lin_visual_body(blockIdx.y, t[blockIdx.x]); }

// ------------------------------------------------------------------------------------------------ pose priors
// accumulates one PoseGraphError / PoseError block; no loss function (backend.cpp:171,176).  <= n_kf blocks: one thread per block,
// global atomics.
// (res, ja, jb: THIS block's 6 residuals and 6 x 7 ambient Jacobian rows — the thread's own copies in k_prior_lin)
__device__ __forceinline__ void lin_prior_block(const int i, const int a, const int b, const double* __restrict__ res, const double* __restrict__ ja,
                                                const double* __restrict__ jb, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const,
                                                double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost) {
  double r[6], La[36], Lb[36];   // local Jacobians, row-major 6 x 6
  double c = 0.0;
  for (int k = 0; k < 6; ++k) { r[k] = res[k]; c += 0.5 * r[k] * r[k]; }
  for (int k = 0; k < 6; ++k) {
    const double* row = jb + 7 * k;
    const double sc = (pose_const[b] & 1) ? 0.0 : 1.0;
    double l3[3];
    quat_row_to_local(row, poses + 7 * b, l3);
    Lb[6 * k] = sc * l3[0]; Lb[6 * k + 1] = sc * l3[1]; Lb[6 * k + 2] = sc * l3[2];
    Lb[6 * k + 3] = sc * row[4]; Lb[6 * k + 4] = sc * row[5]; Lb[6 * k + 5] = sc * row[6];
    if (a >= 0) {
      const double* rowa = ja + 7 * k;
      const double sa = (pose_const[a] & 1) ? 0.0 : 1.0;
      quat_row_to_local(rowa, poses + 7 * a, l3);
      La[6 * k] = sa * l3[0]; La[6 * k + 1] = sa * l3[1]; La[6 * k + 2] = sa * l3[2];
      La[6 * k + 3] = sa * rowa[4]; La[6 * k + 4] = sa * rowa[5]; La[6 * k + 5] = sa * rowa[6];
    }
  }
  atomicAdd(cost + (i & (kStripes - 1)), c);
  for (int x = 0; x < 6; ++x) {
    double g = 0.0;
    for (int k = 0; k < 6; ++k) g += Lb[6 * k + x] * r[k];
    atomicAdd(&gc[6 * b + x], g);
    for (int y = 0; y <= x; ++y) {
      double h = 0.0;
      for (int k = 0; k < 6; ++k) h += Lb[6 * k + x] * Lb[6 * k + y];
      atomicAdd(&B[(size_t)(6 * b + x) * ld + 6 * b + y], h);
    }
  }
  if (a >= 0) {
    for (int x = 0; x < 6; ++x) {
      double g = 0.0;
      for (int k = 0; k < 6; ++k) g += La[6 * k + x] * r[k];
      atomicAdd(&gc[6 * a + x], g);
      for (int y = 0; y <= x; ++y) {
        double h = 0.0;
        for (int k = 0; k < 6; ++k) h += La[6 * k + x] * La[6 * k + y];
        atomicAdd(&B[(size_t)(6 * a + x) * ld + 6 * a + y], h);
      }
      for (int y = 0; y < 6; ++y) {   // cross block, stored in the lower triangle of B
        double h = 0.0;
        for (int k = 0; k < 6; ++k) h += La[6 * k + x] * Lb[6 * k + y];
        if (a > b) atomicAdd(&B[(size_t)(6 * a + x) * ld + 6 * b + y], h);
        else atomicAdd(&B[(size_t)(6 * b + y) * ld + 6 * a + x], h);
      }
    }
  }
}
// Evaluation (prior_eval.hpp) and accumulation in one launch: the block's residuals and ambient Jacobians never leave the thread, so the
// LM loop's path has no k_pose_prior launch ahead of it (a window with weak frames pays it every iteration) and nothing is materialised.
__global__ __launch_bounds__(64) void k_prior_lin(PriorArgs P, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const,
                                                  double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= P.n) return;
  double res[6], ja[42], jb[42];
  const int a = P.kf_a[i], b = P.kf_b[i];
  pose_prior_eval<true>(a, b, P.target + 7 * i, P.weight[i], P.vv[i], poses, res, ja, jb);
  lin_prior_block(i, a, b, res, ja, jb, poses, pose_const, B, ld, gc, cost);
}
// 1/2 |r|^2 of every prior block at `poses` (the candidate), added to the striped cost: k_pose_prior<false> + k_cost_sq in one launch
__global__ __launch_bounds__(64) void k_prior_cost(PriorArgs P, const double* __restrict__ poses, double* __restrict__ cost) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= P.n) return;
  double res[6];
  pose_prior_eval<false>(P.kf_a[i], P.kf_b[i], P.target + 7 * i, P.weight[i], P.vv[i], poses, res, nullptr, nullptr);
  double c = 0.0;
  for (int k = 0; k < 6; ++k) c += 0.5 * res[k] * res[k];
  atomicAdd(cost + (i & (kStripes - 1)), c);
}
__global__ __launch_bounds__(kT) void k_cost_sq(int n, const double* __restrict__ res, double* __restrict__ cost) {
  const int i = blockIdx.x * kT + threadIdx.x;
  double c = 0.0;
  if (i < n) { const double r = res[i]; c = 0.5 * r * r; }
  block_add(c, cost);
}
// ------------------------------------------------------------------------------------------------ closing an iteration on device
// One workgroup per window: the step-quality test, the trust-region update, the commit of an accepted candidate (a copy of a few tens
// of kilobytes: the window's poses, velocities, biases and inverse depths) and the termination tests — what ceres::Solve's
// TrustRegionMinimizer does on the host between evaluations (declared semantics: oracle/lm.h).  The scalars arrive as 32-way striped
// sums (block_add); `rec` (optional, host-mapped) receives a copy of the control block so a waiting host sees progress without a copy.
// COHERENT: the sums are read past the caches (the caller is the last workgroup of the launch that produced part of them)
template <bool COHERENT = false>
__device__ __forceinline__ void lm_decide_body(const DecideArgs& A) {
  __shared__ int s_commit, s_skip, s_iter, s_done;
  __shared__ double s_sum[8];
  LmCtl* c = A.ctl;
  if (A.dbg && threadIdx.x == 0) A.dbg[1] = wall_clock64();
  if (threadIdx.x == 0) s_skip = c->done;
  // the six striped sums: wave w adds the 32 stripes of slots w, w + 4 (lanes 32..63 contribute zero)
  {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int slot = wv; slot < 6; slot += kDT / 64) {
      double v = lane < kStripes ? (COHERENT ? __hip_atomic_load(A.scal + slot * kStripes + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : A.scal[slot * kStripes + lane]) : 0.0;
      if (slot == SC_GMAX / kStripes) { for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o)); }      // the gradient's max norm: a max over its stripes
      else v = wave_sum(v);
      if (lane == 0) s_sum[slot] = v;
    }
  }
  __syncthreads();
  if (s_skip) return;
  if (A.dbg && threadIdx.x == 0) A.dbg[2] = wall_clock64();
  if (!A.fused && threadIdx.x < kStripes) const_cast<double*>((const double*)A.scal)[SC_COST + threadIdx.x] = 0.0;      // read above; the next linearisation adds into it
  if (threadIdx.x == 0) {
    // the fields of the control block are read up front (independent requests, one wait) into the rule's state (LmState, lm_rule.hpp) and written
    // back once at the end: read and written where the logic uses them they were 1.2 us of dependent traffic.  (A whole-struct copy goes
    // through a scratch segment.)
    const int it = c->iter;
    LmState s(c->radius);
    s.decrease = c->decrease; s.cost = c->cost; s.initial_cost = c->initial_cost;
    s.iters = it; s.successes = c->successes; s.invalid_run = c->invalid_run; s.termination = c->termination; s.why = c->why; s.first = it == 0;
    const LmOpts o{c->max_iters, c->function_tol, c->gradient_tol, c->parameter_tol, c->min_rel_decrease, 0.0};
    int rejected = c->rejected;
    const double stored_cost = s.cost, last_radius = s.radius;
    const int hfail = *reinterpret_cast<const int*>(A.scal + SC_FAIL);
    const double cost_before = s_sum[SC_COST / kStripes], cost_new = s_sum[SC_COST_NEW / kStripes], model = -s_sum[SC_MODEL / kStripes];
    const double dx2 = s_sum[SC_DXNORM / kStripes], x2 = s_sum[SC_XNORM / kStripes];
    const double gmax = s_sum[SC_GMAX / kStripes];             // a max over the stripes (the stored bit patterns are the doubles')
    const bool solved = hfail == 0 && isfinite(cost_new) && isfinite(model);
    // the rule judges against the cost summed by THIS pass; the stored cost (c->cost) follows the first pass and the accepted candidates
    const bool first = s.linearized(cost_before);
    bool accepted = false, done;
    // ceres::Solve's TrustRegionMinimizer (declared semantics + citations: oracle/lm.h lm_solve), its iteration split over the launches:
    // Top of the loop (FinalizeIterationAndCheckIfMinimizerCanContinue): the gradient at the point this pass linearised — it ends the
    // solve before a step is taken, so the pass is NOT an iteration; the smallest trust region likewise.
    // a chained sparse level gave up waiting for the level below (SpSrc): nothing about this step is judged — the loop stops where it is
    // (state, radius and counters untouched) and the host re-runs the iteration with un-chained launches
    if (hfail >= kFailHandover) done = s.end(2, LVF_WHY_HANDOVER);
    else if (s.gradient(o, gmax) || s.min_radius()) done = true;
    else {
      // (num_iterations = what Ceres records in Summary::iterations: accepted, rejected and invalid steps; a trial step that ends the solve
      // through the parameter / function tolerance returns before it is recorded)
      if (!s.valid_step(solved, model)) { rejected += 1; done = s.invalid_step(); }      // ComputeTrustRegionStep: solver failure or model_cost_change <= 0
      // parameter tolerance, then function tolerance: both BEFORE the step-quality test, and neither takes the candidate
      else if (s.parameter_tol(o, dx2, x2) || s.function_tol(o, cost_new)) done = true;
      else { done = false; accepted = s.accept(o, cost_new, model); if (!accepted) rejected += 1; }
      // after the step, Finalize's order again: the iteration cap first, then the smallest trust region (the gradient at an accepted point is
      // only known to the next pass)
      if (!done) done = s.cap(o) || s.min_radius();
    }
    s_commit = accepted ? 1 : 0;
    c->radius = s.radius; c->decrease = s.decrease; c->last_radius = last_radius; c->cost = first || accepted ? s.cost : stored_cost; c->initial_cost = s.initial_cost;
    c->cost_before = cost_before; c->cost_after = accepted ? cost_new : (solved ? cost_new : cost_before); c->model = model; c->dxnorm = sqrt(dx2); c->xnorm = sqrt(x2); c->gmax = gmax;
    c->iter = s.iters; c->successes = s.successes; c->invalid_run = s.invalid_run; c->accepted = accepted ? 1 : 0; c->solved = solved ? 1 : 0;
    c->done = done ? 1 : 0; c->termination = s.termination; c->why = s.why; c->rejected = rejected;
    if (hfail < kFailHandover) c->jfrozen = 1;      // the Jacobi scaling of this solve is the first pass's (a pass that is re-run after a hand-over time-out takes it again)
    if (A.fused) {
      // the candidate pass linearised x + dx into the standby set: accepted, that set becomes the active one, its TwoFrame slabs still to be
      // reduced (k_tf_reduce); rejected, the active set keeps the linearisation at x, already reduced
      c->lin_pending = accepted ? 1 : 0;
      if (accepted) c->aset = c->aset ^ 1;
    }
    s_iter = s.iters; s_done = done ? 1 : 0;
    if (A.hist) {                                      // diagnostic: what this pass decided on
      double* h = A.hist + 8 * (it & 63);
      h[0] = (double)it; h[1] = cost_before; h[2] = cost_new; h[3] = model; h[4] = accepted ? 1.0 : 0.0; h[5] = (double)hfail; h[6] = last_radius; h[7] = gmax;
    }
    if (A.dbg) A.dbg[3] = wall_clock64();
  }
  __syncthreads();
  if (s_commit) {
    // (eight 16-byte requests per thread in flight: as a load-store loop the 80 KB of inverse depths took 3.9 us of this one workgroup)
    const double2* __restrict__ p2 = reinterpret_cast<const double2*>((const double*)A.invd2);
    double2* __restrict__ q2 = reinterpret_cast<double2*>((double*)A.invd);
    const int n2 = A.n_lm / 2;
    for (int i0 = 0; i0 < n2; i0 += 8 * kDT) {      // (n2 > 0 inside)
      double vx[8], vy[8];             // (scalars: an array of double2 is not split into registers and lands in scratch)
#pragma unroll
      for (int u = 0; u < 8; ++u) { const double2 t = p2[min(i0 + u * kDT + (int)threadIdx.x, n2 - 1)]; vx[u] = t.x; vy[u] = t.y; }      // (unconditional, clamped)
#pragma unroll
      for (int u = 0; u < 8; ++u) q2[min(i0 + u * kDT + (int)threadIdx.x, n2 - 1)] = make_double2(vx[u], vy[u]);      // (past the end: the last element again, same value)
    }
    if ((A.n_lm & 1) && threadIdx.x == 0) A.invd[A.n_lm - 1] = A.invd2[A.n_lm - 1];
    for (int i = threadIdx.x; i < 7 * A.n_kf; i += kDT) A.poses[i] = A.poses2[i];
    for (int i = threadIdx.x; i < 3 * A.n_kf; i += kDT) { A.vel[i] = A.vel2[i]; A.ba[i] = A.ba2[i]; A.bg[i] = A.bg2[i]; }
  }
  if (A.fused) {
    // no linearisation launch follows: the cost at the state the next iteration starts from is the candidate's (accepted) or stays what it
    // was (rejected), and the per-step scalars are reset here (what k_lin_visual / k_prepare do in today's chain).  Stripe t is carried and
    // cleared by thread t.  A pass that ENDS the loop clears the cost stripes as today's decision does: the launches behind it are gated, and
    // the next solve's linearisation adds into them (lvf_problem::accum_clean)
    double* sc = const_cast<double*>((const double*)A.scal);
    if (threadIdx.x < kStripes) {
      if (s_done) sc[SC_COST + threadIdx.x] = 0.0;
      else if (s_commit) sc[SC_COST + threadIdx.x] = __hip_atomic_load(sc + SC_COST_NEW + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    reset_step_scalars(sc);
  }
  if (A.dbg && threadIdx.x == 0) A.dbg[4] = wall_clock64();
  // the host only polls `iter` and `done` of its mirror (wait_for_iteration): two uncached stores to the pinned record instead of a
  // system-scope fence and a copy of the whole block; LAST, so that no load of this workgroup queues behind a write that crosses PCIe
  if (A.rec && threadIdx.x == 0) {
    __hip_atomic_store(&A.rec->why, c->why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);        // (ahead of `done`: a host that sees done also sees why the loop ended)
    __hip_atomic_store(&A.rec->done, s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&A.rec->iter, s_iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__global__ __launch_bounds__(kDT) void k_lm_decide(DecideArgs a) { lm_decide_body(a); }

// The candidate-cost pass and the decision in ONE launch: every workgroup adds its share of the candidate cost, takes a ticket, and the
// one that draws the last ticket closes the iteration (the sums live in atomics, so a plain completion wait orders them before the
// ticket; nothing else this launch writes is read by the decision).  Saves the k_lm_decide launch (~8 us of an iteration).
static_assert(kDT == kT, "the last workgroup of the cost pass runs the decision with its own threads");
__device__ __forceinline__ void cost_decide_body(const int b, const CostArgs& A, const DecideArgs& D, const int end_zero) {
  if (b >= A.nblocks) {
    // the accumulators of the linearisation (B, gc, C, g_rho, ...) were last read by k_step_tail: cleared here, beside the cost pass, for
    // the next iteration (never gated: a finished solve leaves them clean for the next one)
    if (end_zero && b - A.nblocks < A.zero_wgs) zero_list_share(A.zero, b - A.nblocks, A.zero_wgs);
    return;
  }
  if (A.done && *A.done) return;
  __shared__ double s_part[kT / 64];
  if (D.dbg && threadIdx.x == 0 && (b == 0 || b == A.g_imu)) D.dbg[b == 0 ? 8 : 12] = wall_clock64();
  {
    // the workgroup's sum goes out as a RETURNING atomic: its result can only come back once the add has been performed, and the
    // ticket below is drawn after it — so every add of this workgroup is in the sum before its ticket is drawn (a release fence here would write
    // the L2 back once per workgroup: measured 7 % slower for 8 windows than the separate decision launch)
    double c;
    if (b >= A.g_imu) c = cost_visual_value(b - A.g_imu, A);
    else {                                             // one ImuError factor at the candidate: 1/2 |sqrt_info r|^2
      __shared__ double sS[225];
      __shared__ double sP[OFF_COV];                     // sum_dt, linearisation biases, deltas and the 15 x 15 Jacobian of the pre-integration
      __shared__ double sr0[16];
      const int f = b;
      for (int k = threadIdx.x; k < 225; k += kT) sS[k] = A.imu.sqrt_info[(size_t)f * 225 + k];
      for (int k = threadIdx.x; k < OFF_COV; k += kT) sP[k] = A.imu.pre[(size_t)f * kPre + k];
      __syncthreads();
      // (from LDS the one lane's ~60 operand reads cost nothing to repeat, so the compiler does not hold them all in registers: this
      // path shares its kernel with the visual cost pass, whose occupancy it would otherwise set)
      if (D.dbg && threadIdx.x == 0 && b == 0) D.dbg[9] = wall_clock64();
      if (threadIdx.x == 0) imu_raw<false>(f, sP, A.imu.kf_i, A.imu.kf_j, A.s.poses, A.s.vel, A.s.ba, A.s.bg, sr0, nullptr);
      __syncthreads();
      if (D.dbg && threadIdx.x == 0 && b == 0) D.dbg[10] = wall_clock64();
      const double r = imu_weighted_residual(threadIdx.x, sS, sr0);      // rows 0..14 in lanes 0..14 of wave 0
      c = threadIdx.x < 15 ? 0.5 * r * r : 0.0;
    }
    // one add per WORKGROUP (the four wave sums meet in LDS first): the adds of a stripe serialise at their address
    const double v = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  }
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < kT / 64; ++k) v += s_part[k];
    if (v != 0.0) {
      const double old = atomicAdd(A.cost + (b & (kStripes - 1)), v);
      asm volatile("" ::"v"(old) : "memory");
    }
    if (D.dbg && (b == 0 || b == A.g_imu)) D.dbg[b == 0 ? 11 : 13] = wall_clock64();
    const int t = atomicAdd(D.ticket, 1);
    s_last = t == A.nblocks - 1;
    if (s_last) atomicExch(D.ticket, 0);
  }
  __syncthreads();
  if (s_last) lm_decide_body<true>(D);
  if (s_last && D.dbg && threadIdx.x == 0) D.dbg[5] = wall_clock64();
}
// end_zero = 0 keeps the accumulators of this iteration's linearisation (per-call API: lvf_problem_download_reduced rebuilds the damped system from them)
__global__ __launch_bounds__(kT) void k_cost_decide(CostArgs a, DecideArgs d, int end_zero) { cost_decide_body(blockIdx.x, a, d, end_zero); }
__global__ __launch_bounds__(kT) void k_cost_decide_b(const CostArgs* __restrict__ t, const DecideArgs* __restrict__ d, int end_zero) { cost_decide_body(blockIdx.x, t[blockIdx.y], d[blockIdx.y], end_zero); }
__global__ __launch_bounds__(kT) void k_cost_decide_bt(const CostArgs* __restrict__ t, const DecideArgs* __restrict__ d, int end_zero) { cost_decide_body(blockIdx.y, t[blockIdx.x], d[blockIdx.x], end_zero); }

// The fused chain's candidate pass: k_lin_visual's workgroups (same bodies, same block-to-workgroup mapping) at the candidate x + dx, into
// the accumulator set that is NOT active, with the candidate cost taken from the residuals they form; the last workgroup closes the
// iteration (lm_decide_body, fused mode: an accepted step makes this set the active one).  The next iteration then starts at k_tf_reduce —
// the candidate is not evaluated a second time — and a rejected step re-uses the linearisation at x it already has.  The workgroup's cost
// parts meet in LDS and leave as ONE returning atomic before its ticket (cost_decide_body has the ordering argument); workgroups
// [nblocks, nblocks + zero_wgs) clear S and the arrival counters for the next iteration (the accumulator sets: k_tf_reduce).
__device__ __forceinline__ void lin_cost_decide_body(const int b, const FusedArgs& A) {
  if (b >= A.nblocks) {
    if (b - A.nblocks < A.zero_wgs) zero_list_share(A.zero, b - A.nblocks, A.zero_wgs);
    return;
  }
  if (A.done && *A.done) return;
  __shared__ double s_cost[kStripes];
  __shared__ int s_last;
  if (threadIdx.x < kStripes) s_cost[threadIdx.x] = 0.0;
  const int standby = acc_set(A.lin.acc) ^ 1;
  __syncthreads();
  lin_visual_run(b, A.lin, standby, A.lin.s, s_cost);
  __syncthreads();
  if (threadIdx.x < 64) {
    double v = threadIdx.x < kStripes ? s_cost[threadIdx.x] : 0.0;
    v = wave_sum(v);
    if (threadIdx.x == 0) {
      if (v != 0.0) {
        const double old = atomicAdd(A.cost_new + (b & (kStripes - 1)), v);
        asm volatile("" ::"v"(old) : "memory");
      }
      const int t = atomicAdd(A.dec.ticket, 1);
      s_last = t == A.nblocks - 1;
      if (s_last) atomicExch(A.dec.ticket, 0);
    }
  }
  __syncthreads();
  if (s_last) lm_decide_body<true>(A.dec);
}
__global__ __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(3))) void k_lin_cost_decide(FusedArgs a) { lin_cost_decide_body(blockIdx.x, a); }

// the instantiations the host side launches (enqueue_linearize in solver_chain.hip: a window without a sorted TwoFrame work list)
template __global__ void k_lin_tc<false>(int, const double2*, const double2*, const int*, const int*, const double*, StateP, CamD, CamD, double, double*, double*, double*);
template __global__ void k_lin_tf<false>(int, int, const double2*, const double2*, const int*, const int*, const int*, StateP, CamD, CamD, double, const uint8_t*, double*, int,
                                         double*, double*, int, double*, double*, double*);
template __global__ void k_lin_po<false>(int, int, const double2*, const int*, const int*, const double*, StateP, CamD, double, const uint8_t*, double*, int, double*, double*);

}  // namespace lvf
