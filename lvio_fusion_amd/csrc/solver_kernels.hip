// solver_kernels.hip — the sliding-window BA problem on device: fused robustified linearisation, Schur
// elimination of the 1x1 inverse-depth blocks (MFMA f64), dense Cholesky of the reduced camera system, step
// evaluation.  Replaces what ceres::Solve does under adapt::Solve for Backend::Optimize
// (src/lvio_fusion/include/lvio_fusion/adapt/problem.h:83-88; src/lvio_fusion/src/backend.cpp:96-183, 206-211).
//
// Unknown ordering (reduced system, d = 15 n_kf):  [ pose tangent 6 x n_kf | (v, ba, bg) 9 x n_kf ].
// H = [B E^T; E C], C diagonal (one inverse depth per landmark).  LM step: (H + D^2/radius) dx = -g with
// D^2 = clamp(diag H, 1e-6, 1e32).  S = B + Dc - E^T diag(1/(C + Dl)) E touches only the pose-pose corner, so E is
// kept dense [n_lm x ldE] (ldE = 6 n_kf rounded up to 16, +1 column carrying g_rho) and the rank-n_lm update is one
// v_mfma_f64_16x16x4_f64 SYRK ("MFMA only for the dense Schur reduce").  The right-hand side rides along as an
// augmented ROW of S (index d), so the forward substitution comes out of the Cholesky for free.
// Device code only: the argument blocks and constants are in solver_args.hpp, the host side that builds and launches the chain in
// solver_chain.hip, solver_plan.hip, solver_batch.hip and solver_api.hip.
#include "factor_eval.hpp"
#include "prior_eval.hpp"
#include "lvf_internal.hpp"
#include "imu_eval.hpp"
#include "solver_args.hpp"

namespace lvf {

template <bool SEL = false>
__device__ __forceinline__ void sp_ride(const int vb, const SpArgs& a);     // workgroup vb of the level (defined with k_sp_eliminate)

typedef double double4_t __attribute__((ext_vector_type(4)));

// The LM loop's `done` flag gates every launch of an iteration.  Tested at the top of a kernel it is a dependent global round trip
// (~0.5-1 us) in front of everything; issued FIRST and tested after the kernel's own first loads have been issued, its latency hides
// under theirs (loads return in order: the test waits for the oldest one only).
__device__ __forceinline__ int done_flag_issue(const int* done) { return done ? *reinterpret_cast<const volatile int*>(done) : 0; }

__device__ __forceinline__ void block_add(double v, double* dst) {
  v = wave_sum(v);
  // (x + y: a table launch may carry the window in either grid dimension — the stripes must be spread by the workgroup's number inside the window)
  if ((threadIdx.x & 63) == 0 && v != 0.0) atomicAdd(dst + ((blockIdx.x + blockIdx.y) & (kStripes - 1)), v);
}


__device__ __forceinline__ int acc_set(const AccSel& a) { return a.sel ? *a.sel : 0; }
// SEL = false (the batched table launches, which never run the fused chain): set 0, the selection compiled out
template <bool SEL> __device__ __forceinline__ int acc_set_t(const AccSel& a) { return SEL ? acc_set(a) : 0; }


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
// rows of a lower-triangular matrix (leading dimension ld, even): one wave per row, columns [0, end of the row's 64-column block)
__device__ __forceinline__ void zero_lower(double* __restrict__ p, const int ld, const unsigned long long wave, const unsigned long long n_waves) {
  const int lane = threadIdx.x & 63;
  for (unsigned long long r = wave; r < (unsigned long long)ld; r += n_waves) {
    double2* row = reinterpret_cast<double2*>(p + r * (unsigned long long)ld);
    const int end2 = min(ld, (((int)r | 63) + 1)) / 2;
    for (int c = lane; c < end2; c += 64) row[c] = make_double2(0.0, 0.0);
  }
}
__global__ __launch_bounds__(kT) void k_zero_multi(ZeroList z) {
  double* p = z.p[blockIdx.y];
  if (z.tri[blockIdx.y] > 0) { zero_lower(p, z.tri[blockIdx.y], (unsigned long long)blockIdx.x * (kT / 64) + (threadIdx.x >> 6), (unsigned long long)gridDim.x * (kT / 64)); return; }
  const unsigned long long n = z.n[blockIdx.y], n2 = n / 2;
  double2* p2 = reinterpret_cast<double2*>(p);
  for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < n2; i += (unsigned long long)gridDim.x * kT) p2[i] = make_double2(0.0, 0.0);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = 0.0;
}
// k_zero_multi + k_lm_range_init in one launch (problem_configure): slice z.count of the grid's y sets the landmark tracks to "none yet"
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
// workgroup `wg` of `n_wgs` (kT threads each) clears its share of every array of the list
// (static indices only: a run-time index into the by-value pointer table would put it in scratch memory)
__device__ __forceinline__ void zero_list_share(const ZeroList& zero, const int wg, const int n_wgs) {
  const unsigned long long t = (unsigned long long)wg * kT + threadIdx.x, nt = (unsigned long long)n_wgs * kT;
#pragma unroll
  for (int a = 0; a < kZeroListMax; ++a) {
    if (a >= zero.count) break;
    double* p = zero.p[a];
    if (zero.tri[a] > 0) { zero_lower(p, zero.tri[a], (unsigned long long)wg * (kT / 64) + (threadIdx.x >> 6), (unsigned long long)n_wgs * (kT / 64)); continue; }
    const unsigned long long cnt = zero.n[a], n2 = cnt / 2;
    double2* p2 = reinterpret_cast<double2*>(p);
    for (unsigned long long i = t; i < n2; i += nt) p2[i] = make_double2(0.0, 0.0);
    if ((cnt & 1) && t == 0) p[cnt - 1] = 0.0;
  }
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
__global__ __launch_bounds__(kT) void k_cost_visual_b(const CostArgs* __restrict__ t) { cost_visual_body(blockIdx.x, t[blockIdx.y]); }

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

__device__ __forceinline__ void reset_step_scalars(double* scal) {
  for (int k = SC_COST_NEW + threadIdx.x; k < SC_N; k += kT) scal[k] = 0.0;
  if (threadIdx.x == 0) { *reinterpret_cast<int*>(scal + SC_FAIL) = 0; *reinterpret_cast<int*>(scal + SC_TICKET) = 0; }
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

// Adds the TwoFrame slabs of a linearisation into B / gc (compact mode).  Workgroups are sorted by current keyframe: run(k) =
// workgroups [run_first[k], run_first[k+1]).  Every entry of B has ONE owner thread here (plain read-modify-write; the other factor
// types' atomic contributions were complete when the linearisation launch ended):
//   workgroups [0, n_kf)         keyframe k: B[k,k] (21) and g[k] (6) = sum of slabQ over run(k) (k as current keyframe)
//                                                                      + sum of slabP[.][k][0..27) over every later workgroup (k as first keyframe)
//   the rest                     one thread per (k2, k1 < k2, entry of the 6x6 cross block) = sum of slabP[.][k1][27..63) over run(k2)
template <bool SEL>
__device__ __forceinline__ void tf_reduce_body(const int bx0, const TfReduceArgs& A) {
  if (bx0 >= A.nblocks) {
    const int zw = (int)bx0 - A.nblocks;
    if (SEL && zw < A.zero_wgs) {
      if (acc_set(A.acc)) zero_list_share(A.stand0, zw, A.zero_wgs);
      else zero_list_share(A.stand1, zw, A.zero_wgs);
    }
    return;
  }
  if (A.done && *A.done) return;
  // (the riding level takes the FIRST workgroups: it is the longest piece of the launch, and in a batch the first workgroups of every
  // window are dispatched first — see the transposed table launches)
  if (bx0 < A.ride.nblocks) { sp_ride<SEL>(bx0, A.ride); return; }
  if (SEL && A.pending && !*A.pending) return;
  const bool s1 = acc_set_t<SEL>(A.acc) != 0;
  double* const Bs = s1 ? (double*)A.acc.B : (double*)A.B;
  double* const gcs = s1 ? (double*)A.acc.gc : (double*)A.gc;
  const int bx = bx0 - A.ride.nblocks;
  const int n_kf = A.n_kf;
  const int nchunk = (A.n_wg + 63) / 64;
  if (bx < n_kf * nchunk) {
    // keyframe k, chunk c of 64 workgroups: 8 groups of 32 lanes (lane v < 27 owns one value), 8 slab rows per thread, all requested at
    // once; the chunk's 27 sums go to B / gc with one atomic each (n_kf x nchunk x 27 per linearisation)
    __shared__ double part[8][32];
    const int k = bx / nchunk, c = bx - k * nchunk, v = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int r0 = A.run_first[k], r1 = A.run_first[k + 1];
    double acc = 0.0;
    if (v < 27) {
      // the eight slab values are requested together — the row (P or Q slab) chosen by address, the workgroup index clamped — and added in
      // order afterwards: as `if (wg >= r1) acc += P[..]; else if (wg >= r0) acc += Q[..]` every load sat in its own branch behind the
      // previous addition, eight dependent round trips per thread
      const double* slabP = A.slabP; const double* slabQ = A.slabQ;
      double t8[8]; bool keep[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int wg = 64 * c + g + 8 * u, wgc = min(wg, A.n_wg - 1);
        const bool useP = wgc >= r1;               // k as the blocks' first keyframe (later workgroups); else k as their current keyframe
        keep[u] = (wg < A.n_wg) & (wgc >= r0);
        const double* src = useP ? slabP + ((size_t)wgc * n_kf + k) * kSlabRow + v : slabQ + (size_t)wgc * kSlabQ + v;
        t8[u] = *src;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = keep[u] ? acc + t8[u] : acc;
    }
    part[g][v] = acc;
    __syncthreads();
    if (threadIdx.x < 27) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < 8; ++q) t += part[q][threadIdx.x];
      if (t != 0.0) {
        if (threadIdx.x < 21) {
          int x = 0, rem = threadIdx.x;
          while (rem > x) { rem -= x + 1; ++x; }
          atomicAdd(&Bs[(size_t)(6 * k + x) * A.ld + 6 * k + rem], t);
        } else atomicAdd(&gcs[6 * k + threadIdx.x - 21], t);
      }
    }
    return;
  }
  const int e = (bx - n_kf * nchunk) * kT + threadIdx.x;
  const int npair = n_kf * (n_kf - 1) / 2;
  if (e >= npair * 36) return;
  const int pr = e / 36, el = e - 36 * pr;
  int k2 = (int)((1.0 + sqrt(1.0 + 8.0 * pr)) * 0.5);                 // pr = k2 (k2 - 1) / 2 + k1, k1 < k2
  while (k2 * (k2 - 1) / 2 > pr) --k2;
  while ((k2 + 1) * k2 / 2 <= pr) ++k2;
  const int k1 = pr - k2 * (k2 - 1) / 2;
  double acc = 0.0;
  {
    const double* slabP = A.slabP;
    const int w0 = A.run_first[k2], w1 = A.run_first[k2 + 1];
    for (int wg = w0; wg < w1; wg += 4) {            // four rows per round trip (index clamped), added in order
      double t4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t4[u] = slabP[((size_t)min(wg + u, w1 - 1) * n_kf + k1) * kSlabRow + 27 + el];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = (wg + u < w1) ? acc + t4[u] : acc;
    }
  }
  if (acc != 0.0) {
    const int x = el / 6, y = el - 6 * x;                              // x: k2 tangent index, y: k1 tangent index
    Bs[(size_t)(6 * k2 + x) * A.ld + 6 * k1 + y] += acc;
  }
}
__global__ __launch_bounds__(kT) void k_tf_reduce(TfReduceArgs a) { tf_reduce_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_tf_reduce_b(const TfReduceArgs* __restrict__ t) { tf_reduce_body<false>(blockIdx.x, t[blockIdx.y]); }
// (transposed: blockIdx.x = window.  Workgroups are dispatched x-fastest, so the first workgroups of EVERY window — the riding / chained
// sparse levels, the ImuError factors — start together at the head of the launch instead of each window's behind the previous window's bulk)
__global__ __launch_bounds__(kT) void k_tf_reduce_bt(const TfReduceArgs* __restrict__ t) { tf_reduce_body<false>(blockIdx.y, t[blockIdx.x]); }


// ------------------------------------------------------------------------------------------------ pose priors
// consumes the materialised PoseGraphError / PoseError outputs of launch_pose_prior (res[n][6], ja/jb [n][6][7]); no loss
// function (backend.cpp:171,176).  <= n_kf blocks: one thread per block, global atomics.
// (res, ja, jb: THIS block's 6 residuals and 6 x 7 ambient Jacobian rows — global arrays of launch_pose_prior, or the thread's own copies)
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
__global__ __launch_bounds__(64) void k_lin_prior(int n, const double* __restrict__ res, const double* __restrict__ ja,
                                                  const double* __restrict__ jb, const int* __restrict__ kf_a, const int* __restrict__ kf_b,
                                                  const double* __restrict__ poses, const uint8_t* __restrict__ pose_const,
                                                  double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  lin_prior_block(i, kf_a[i], kf_b[i], res + 6 * i, ja + (size_t)42 * i, jb + (size_t)42 * i, poses, pose_const, B, ld, gc, cost);
}
// The same with the evaluation inside (prior_eval.hpp): the block's residuals and ambient Jacobians never leave the thread — one launch
// instead of k_pose_prior + k_lin_prior on the LM loop's path (a window with weak frames pays it every iteration), nothing materialised.
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

// ------------------------------------------------------------------------------------------------ damping / assembly
// (the fp64 square root and two divisions of the literal form cost k_prepare / k_tf_reduce / k_step_tail 6.6 us per iteration between them
// when every diagonal entry took them — profiles/r05_a; they are only needed where the clamp can act:  s^2 h >= 1e-6  <=  h >= 2e-6 (1 + h0),
// because (1 + sqrt(h0))^2 <= 2 (1 + h0); there clamp(s^2 h) / s^2 = h up to one rounding.  A column that was empty at iteration 0 has s = 1.)
__device__ __forceinline__ double lm_damping(double h, double h0) {
  if (h >= 2e-6 * (1.0 + h0) && h < 1e32) return h;
  if (h0 == 0.0) return fmin(fmax(h, 1e-6), 1e32);
  const double sj = 1.0 / (1.0 + sqrt(h0)), s2 = sj * sj;
  return fmin(fmax(h * s2, 1e-6), 1e32) / s2;
}
// the damping of unknown `slot` whose diagonal entry is h in this pass; the thread that OWNS the entry's assembly records H0 in the first
// pass.  h0_loaded = jac.h0[slot], requested by the caller together with its other loads (so that it is not a dependent round trip here).
__device__ __forceinline__ double lm_damping_own(double h, const JacobiDev& j, int slot, int frozen, double h0_loaded) {
  double h0 = h0_loaded;
  if (!frozen) { h0 = h; j.h0[slot] = h; }
  return lm_damping(h, h0);
}

// One launch prepares the damped system of a step:
//   blocks [0, nS_blocks)      : S (lower, in ELIMINATION order: S row I holds unknown iperm[I]) = B (lower, natural order) + Dc on
//                                the diagonal; augmented row (iperm = -2) = -gc ; padding rows (iperm = -1) = identity
//   blocks [nS_blocks, ...)    : Cd = C + clamp(C)/radius ; E[l][dp] = gr[l] (the extra column that makes the SYRK also
//                                produce E^T Cd^-1 g_rho)
//   block 0 / thread 0         : resets the per-step scalars (candidate cost, model change, norms) and the Cholesky fail flag
template <bool SEL>
__device__ __forceinline__ void prepare_body(const unsigned bx0, const PrepArgs& A) {
  if (bx0 >= (unsigned)A.nblocks || (A.done && *A.done)) return;
  if (bx0 < (unsigned)A.ride.nblocks) { sp_ride<SEL>((int)bx0, A.ride); return; }      // (riders first: tf_reduce_body)
  const unsigned bx = bx0 - (unsigned)A.ride.nblocks;
  const bool s1 = acc_set_t<SEL>(A.acc) != 0;
  const int ld = A.ld, dpad = A.dpad; const int* __restrict__ iperm = A.iperm; const double* __restrict__ B = s1 ? (const double*)A.acc.B : (const double*)A.B;
  const double* __restrict__ gc = s1 ? (const double*)A.acc.gc : (const double*)A.gc;
  const double inv_radius = 1.0 / *A.radius;
  const int jf = *A.jac.frozen;
  double* __restrict__ S = A.S; const unsigned nS_blocks = A.nS_blocks; const int n_lm = A.n_lm, dp = A.dp, ldE = A.ldE;
  const double* __restrict__ C = s1 ? (const double*)A.acc.C : (const double*)A.C; const double* __restrict__ gr = s1 ? (const double*)A.acc.gr : (const double*)A.gr;
  double* __restrict__ Cd = A.Cd; double* __restrict__ E = s1 ? (double*)A.acc.E : (double*)A.E; double* __restrict__ scal = A.scal;
  const double* const slotB = (s1 && A.slotB) ? (const double*)A.acc.slotB : (const double*)A.slotB;
  if (bx == 0 && scal) reset_step_scalars(scal);
  if (bx >= nS_blocks) {
    if (slotB) {
      // atomic-free mode: C, g_rho of the landmark = its TwoCamera part (C, gr: atomics of the linearisation) + its slot records; the k1
      // columns of its E row = the sum of the records' first-keyframe parts.  8 lanes per landmark (lane j takes slots j, j + 8, ...: the
      // loads of a track are issued together instead of one dependent loop), DPP sum over the 8 lanes.  The totals go to separate arrays
      // so the pass can be repeated (lvf_problem_download_reduced).
      const int l = ((bx - nS_blocks) * kT + threadIdx.x) >> 3, j0 = threadIdx.x & 7;
      const bool live = l < n_lm;
      const int lc = live ? l : 0;
      const int k1 = A.kmin[lc], len = live ? max(0, A.kmax[lc] - k1) : 0;
      const double h0l = A.jac.h0[A.jl0 + lc];
      const double2* sb = reinterpret_cast<const double2*>(slotB + (size_t)A.eoff[lc] * 8);
      double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int j = j0; j < len; j += 8) {
        const double2 b0 = sb[4 * j], b1 = sb[4 * j + 1], b2 = sb[4 * j + 2], cg = sb[4 * j + 3];
        v[0] += cg.x; v[1] += cg.y; v[2] += b0.x; v[3] += b0.y; v[4] += b1.x; v[5] += b1.y; v[6] += b2.x; v[7] += b2.y;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) { v[q] = quad_sum(v[q]); v[q] += quad_perm<0x141>(v[q]); }      // sum over the aligned group of 8 lanes
      if (live && j0 == 0) {
        const double c = C[l] + v[0], g = gr[l] + v[1];
        A.Ct[l] = c; A.grt[l] = g;
        Cd[l] = c + lm_damping_own(c, A.jac, A.jl0 + l, jf, h0l) * inv_radius;
        double* el = E + (size_t)l * ldE;
        el[dp] = g;
        if (len > 0) {
#pragma unroll
          for (int q = 0; q < 6; ++q) el[6 * k1 + q] = v[2 + q];
        }
      }
      return;
    }
    const int l = (bx - nS_blocks) * kT + threadIdx.x;
    if (l >= n_lm) return;
    const double c = C[l], h0l = A.jac.h0[A.jl0 + l];
    Cd[l] = c + lm_damping_own(c, A.jac, A.jl0 + l, jf, h0l) * inv_radius;
    E[(size_t)l * ldE + dp] = gr[l];
    return;
  }
  // Only the LOWER triangle is assembled (nothing downstream reads an entry right of the diagonal as a value: the factorisations work
  // on lower tiles, and what they carry in the upper halves of diagonal tiles only ever feeds those same entries).  The triangle is
  // folded into a rectangle so that consecutive threads still write consecutive entries of a row: rectangle row q holds matrix row q
  // (columns 0..q) followed by matrix row ld-1-q (columns 0..ld-1-q), ld + 1 entries in all.
  const size_t e = (size_t)bx * kT + threadIdx.x;
  const int n0 = A.early ? A.off : 0, nn = ld - n0;                   // early form: the dense corner only
  const int half = (nn + 1) / 2;
  if (e >= (size_t)half * (nn + 1)) return;
  const int q = (int)(e / (nn + 1)), cc = (int)(e % (nn + 1));
  int I, J;
  if (cc <= q) { I = q; J = cc; }
  else { I = nn - 1 - q; J = cc - q - 1; if (I == q) return; }      // (odd size: the middle row is its own partner)
  I += n0; J += n0;
  const int oi = iperm[I], oj = iperm[J];
  double v = 0.0;
  if (oi >= 0) {
    if (oj >= 0 && J <= I) {
      const double h0d = I == J ? A.jac.h0[oi] : 0.0;
      v = B[(size_t)max(oi, oj) * dpad + min(oi, oj)];
      if (I == J) v += lm_damping_own(v, A.jac, oi, jf, h0d) * inv_radius;
    }
  } else if (oi == -2) {
    v = (oj >= 0) ? -gc[oj] : (J == I ? 1e300 : 0.0);   // huge corner keeps the augmented matrix positive definite
  } else if (I == J) {
    v = 1.0;
  }
  if (!A.early) S[(size_t)I * ld + J] = v;
  else if (v != 0.0) atomicAdd(&S[(size_t)I * ld + J], v);
}
__global__ __launch_bounds__(kT) void k_prepare(PrepArgs a) { prepare_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_prepare_b(const PrepArgs* __restrict__ t) { prepare_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(kT) void k_prepare_bt(const PrepArgs* __restrict__ t) { const PrepArgs a = t[blockIdx.x]; prepare_body<false>(blockIdx.y, a); }

// ------------------------------------------------------------------------------------------------ Schur reduce (MFMA f64)
// T = Ea^T diag(1/Cd) Ea with Ea = [E | g_rho] (n_lm x ldE).  One wave per (16x16 output tile, K-chunk); tiles on or
// below the diagonal only.  v_mfma_f64_16x16x4_f64: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// D: col = lane&15, row = (lane>>4) + 4*reg.   S[i][j] -= T[i][j] (i,j < dp);  S[d][i] += T[dp][i].
__global__ __launch_bounds__(64) void k_schur_syrk(int n_lm, int dp, int ldE, int ntile, const double* __restrict__ E,
                                                   const double* __restrict__ Cd, int d, int ldS, double* __restrict__ S) {
  // decode lower-triangular tile index
  int t = blockIdx.x, ti = 0;
  while (t >= ti + 1) { t -= ti + 1; ++ti; }
  const int tj = t;
  const int lane = threadIdx.x, lk = lane >> 4, lc = lane & 15;
  const int k_begin = blockIdx.y * kSchurChunk, k_end = min(n_lm, k_begin + kSchurChunk);
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = k_begin; k0 < k_end; k0 += 4) {
    const int l = k0 + lk;
    double a = 0.0, b = 0.0;
    if (l < k_end) {
      const double* row = E + (size_t)l * ldE;
      a = row[ti * 16 + lc] / Cd[l];
      b = row[tj * 16 + lc];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = ti * 16 + lk + 4 * r, gj = tj * 16 + lc;
    const double v = acc[r];
    if (v == 0.0) continue;
    if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
    else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
  }
}

// LDS-staged variant (used whenever ldE <= 320, i.e. up to 53 keyframes; larger windows fall back to k_schur_syrk): workgroup = (tile group g of kSchurGroups, K slice).  The slice's rows
// of Ea are streamed through LDS in 16-row chunks with fully coalesced loads (the next chunk is prefetched into registers while
// the current one feeds the matrix cores); every wave keeps up to kSchurTilesPerWave 16x16 accumulators in registers across
// the whole slice and the workgroup touches S once at the end.  Versus one wave per (tile, 512-row chunk) with strided 8-byte
// global operand loads: the same MFMA count, 1/8 of the atomics, and E is read once per tile group instead of once per tile.
__global__ __launch_bounds__(256) void k_schur_lds(int n_lm, int dp, int ldE, int ntile, int rows_per_slice, const double* __restrict__ E,
                                                   const double* __restrict__ Cd, int d, int ldS, double* __restrict__ S) {
  extern __shared__ double sh[];          // Es[kSchurRows][ldE] | icd[kSchurRows]
  double* Es = sh;
  double* icd = sh + kSchurRows * ldE;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lk = lane >> 4, lc = lane & 15;
  const int g = blockIdx.x, slice = blockIdx.y;
  const int k_begin = slice * rows_per_slice, k_end = min(n_lm, k_begin + rows_per_slice);
  // this wave's tiles: t = g + kSchurGroups * (w + 4 * s), s = 0..; decode (ti, tj) of the lower-triangular enumeration
  int ti[kSchurTilesPerWave], tj[kSchurTilesPerWave], nt = 0;
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) {
    const int t = g + kSchurGroups * (w + 4 * s_);
    ti[s_] = 0; tj[s_] = 0;
    if (t < ntile) {
      int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      while (a * (a + 1) / 2 > t) --a;
      ti[s_] = a; tj[s_] = t - a * (a + 1) / 2;
      nt = s_ + 1;
    }
  }
  double4_t acc[kSchurTilesPerWave];
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) acc[s_] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int per_row = ldE;                 // doubles per staged row
  const int total = kSchurRows * per_row;  // elements per chunk
  constexpr int kPf = 20;                  // prefetch registers per thread: 256 * 20 >= 16 * 304 (ldE <= 320 on this path; larger ldE loops)
  double pf[kPf];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      const int e = tid + 256 * u;
      double v = 0.0;
      if (e < total) { const int rr = e / per_row, cc = e - rr * per_row; if (k0 + rr < k_end) v = E[(size_t)(k0 + rr) * ldE + cc]; }
      pf[u] = v;
    }
  };
  auto fetch_tail = [&](int k0) {         // elements beyond 256 * kPf (only when ldE > 320): straight to LDS
    for (int e = tid + 256 * kPf; e < total; e += 256) {
      const int rr = e / per_row, cc = e - rr * per_row;
      Es[e] = (k0 + rr < k_end) ? E[(size_t)(k0 + rr) * ldE + cc] : 0.0;
    }
  };
  if (k_begin < k_end) fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += kSchurRows) {
    __syncthreads();                       // the previous chunk has been consumed
#pragma unroll
    for (int u = 0; u < kPf; ++u) { const int e = tid + 256 * u; if (e < total) Es[e] = pf[u]; }
    fetch_tail(k0);
    if (tid < kSchurRows) icd[tid] = (k0 + tid < k_end) ? 1.0 / Cd[k0 + tid] : 0.0;
    __syncthreads();
    if (k0 + kSchurRows < k_end) fetch(k0 + kSchurRows);   // in flight while the matrix cores work
#pragma unroll
    for (int kk = 0; kk < kSchurRows; kk += 4) {
      const double* row = Es + (kk + lk) * per_row;
      const double wgt = icd[kk + lk];
#pragma unroll
      for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_)
        if (s_ < nt) acc[s_] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ti[s_] + lc] * wgt, row[16 * tj[s_] + lc], acc[s_], 0, 0, 0);
    }
  }
#pragma unroll
  for (int s_ = 0; s_ < kSchurTilesPerWave; ++s_) {
    if (s_ >= nt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = ti[s_] * 16 + lk + 4 * r, gj = tj[s_] * 16 + lc;
      const double v = acc[s_][r];
      if (v == 0.0) continue;
      if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
      else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
    }
  }
}
// ---- band-limited variant.  A landmark's row of E is non-zero only at the keyframes that observe it, a contiguous track
// [kmin_l, kmax_l] of the window.  Landmarks are ordered by (track-length class, kmin) once per problem (k_lm_range + k_lm_sort),
// so a slice of kBandRows consecutive landmarks touches a narrow BAND of 16-column tiles [t0, t1]: the workgroup stages only
// those columns (plus the tile holding the g_rho column) and only forms the band's lower-triangular tiles.  At configs[3]
// that is ~1/5 of the MFMAs and ~1/30 of the E bytes of the dense SYRK.  Correctness never depends on the ordering: the
// band of each slice is computed from the actual kmin/kmax of its rows.
__global__ __launch_bounds__(kT) void k_lm_range(int n, const int* __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2,
                                                 int* __restrict__ kmin, int* __restrict__ kmax) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int l = lm[i], a = min(k1[i], k2[i]), b = max(k1[i], k2[i]);
  atomicMin(&kmin[l], a); atomicMax(&kmax[l], b);
}
__global__ __launch_bounds__(kT) void k_lm_range_init(int n_lm, int* __restrict__ kmin, int* __restrict__ kmax) {
  const int l = blockIdx.x * kT + threadIdx.x;
  if (l < n_lm) { kmin[l] = 0x7fffffff; kmax[l] = -1; }
}
__device__ __forceinline__ int lm_sort_key(int kmin, int kmax, int n_kf) {
  // (branch-free on purpose: with `if (kmax < 0) return ..` in front, the compiler sinks the caller's kmin load into the branch behind the
  // kmax load's wait — two dependent round trips per landmark instead of one)
  const int len = kmax - kmin + 1;
  const int cls = (len > 8) + (len > 16) + (len > 32);
  const int none = kmax >> 31;                          // all ones: no pose-dependent block — nothing to eliminate, ordered last
  return (none & (4 * n_kf)) | (~none & (cls * n_kf + kmin));
}
// counting sort by key, one workgroup (n_lm is ~1e4; 4 n_kf + 1 buckets in LDS)
// (per-wave copies of the histogram — 16x fewer lanes per address — measured SLOWER, 15.7 vs 13.6 us: the two passes are bound by their
// dependent load -> LDS atomic round trips, not by address conflicts)
__device__ __forceinline__ void lm_sort_body(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax,
                                             int* __restrict__ order, int* __restrict__ n_active) {
  extern __shared__ int bucket[];
  const int nb = 4 * n_kf + 1;
  for (int b = threadIdx.x; b < nb; b += 1024) bucket[b] = 0;
  __syncthreads();
  // (16 landmarks per thread and pass, their tracks requested together and the keys kept for the second sweep: as `for (l ..) atomicAdd(&bucket[
  // key(kmin[l], kmax[l])], 1)` every iteration waited for its own two loads before its LDS atomic — twice ten dependent round trips at 10 k landmarks)
  constexpr int kG = 16;
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int key[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int lc = min(sb + g * 1024 + (int)threadIdx.x, n_lm - 1); key[g] = lm_sort_key(kmin[lc], kmax[lc], n_kf); }
#pragma unroll
    for (int g = 0; g < kG; ++g) if (sb + g * 1024 + (int)threadIdx.x < n_lm) atomicAdd(&bucket[key[g]], 1);
  }
  __syncthreads();
  if (nb <= 1024) {                         // exclusive scan of the bucket counts: 16 wave scans + 16 wave totals
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = tid < nb ? bucket[tid] : 0;
    const int incl = wave_incl_scan(c);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    if (tid < nb) bucket[tid] = base + incl - c;
    if (tid == nb - 1) *n_active = base + incl - c;
  } else if (threadIdx.x == 0) {
    int run = 0;
    for (int b = 0; b < nb; ++b) { const int c = bucket[b]; bucket[b] = run; run += c; }
    *n_active = bucket[nb - 1];
  }
  __syncthreads();
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int key[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int lc = min(sb + g * 1024 + (int)threadIdx.x, n_lm - 1); key[g] = lm_sort_key(kmin[lc], kmax[lc], n_kf); }
#pragma unroll
    for (int g = 0; g < kG; ++g) { const int l = sb + g * 1024 + (int)threadIdx.x; if (l < n_lm) order[atomicAdd(&bucket[key[g]], 1)] = l; }
  }
}
__global__ __launch_bounds__(1024) void k_lm_sort(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax,
                                                  int* __restrict__ order, int* __restrict__ n_active) {
  lm_sort_body(n_lm, n_kf, kmin, kmax, order, n_active);
}

// ---- compact landmark layout, built once per problem_configure
// eoff[l] = first slot of landmark l, len_l = kmax_l - kmin_l slots (one per keyframe after the first); *n_slots = their total
__device__ __forceinline__ void lm_offsets_body(int n_lm, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ eoff,
                                                int* __restrict__ n_slots) {
  // 16 k landmarks per pass: every thread requests its 16 (kmin, kmax) pairs up front (a load inside the per-1024 loop was waited for
  // before the next was issued: 10 dependent round trips at 10 k landmarks), scans run inside waves, two workgroup barriers per pass
  constexpr int kG = 16;
  __shared__ int s_cnt[kG * 16];                    // [chunk][wave] totals, then their exclusive prefix
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0;
  for (int sb = 0; sb < n_lm; sb += kG * 1024) {
    int c[kG], ex[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid, lc = min(l, n_lm - 1);
      const int lo = kmin[lc], hi = kmax[lc];
      c[g] = max(0, hi - lo) & -(int)((l < n_lm) & (hi >= 0));      // (branch-free: behind `l < n_lm && hi >= 0 ? .. : 0` the kmin load was sunk into a branch behind the kmax load's wait, 32 dependent round trips)
    }
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int incl = wave_incl_scan(c[g]);
      ex[g] = incl - c[g];
      if (lane == 63) s_cnt[g * 16 + wave] = incl;
    }
    __syncthreads();
    if (wave == 0) {                                 // exclusive scan of the 256 totals (chunk-major = ascending landmark order)
      int carry = 0;
#pragma unroll
      for (int base = 0; base < kG * 16; base += 64) {
        const int v = s_cnt[base + lane];
        const int inc = wave_incl_scan(v);
        s_cnt[base + lane] = carry + inc - v;
        carry += __shfl(inc, 63);
      }
      if (lane == 0) s_total = carry;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid;
      if (l < n_lm) eoff[l] = total + s_cnt[g * 16 + wave] + ex[g];
    }
    total += s_total;
    __syncthreads();
  }
  if (tid == 0) *n_slots = total;
}
__global__ __launch_bounds__(1024) void k_lm_offsets(int n_lm, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ eoff,
                                                     int* __restrict__ n_slots) {
  lm_offsets_body(n_lm, kmin, kmax, eoff, n_slots);
}
// the counting sort and the slot offsets are two one-workgroup chains over the same (kmin, kmax) with nothing in common but their inputs:
// ONE launch of two workgroups runs them side by side (a persistent window reconfigures every tick: 14 us + 9 us + a launch gap became 14 us)
__global__ __launch_bounds__(1024) void k_lm_sort_offsets(int n_lm, int n_kf, const int* __restrict__ kmin, const int* __restrict__ kmax, int* __restrict__ order,
                                                          int* __restrict__ n_active, int* __restrict__ eoff, int* __restrict__ n_slots) {
  if (blockIdx.x == 0) lm_sort_body(n_lm, n_kf, kmin, kmax, order, n_active);
  else lm_offsets_body(n_lm, kmin, kmax, eoff, n_slots);
}
__global__ __launch_bounds__(kT) void k_tf_slots(int n, const int* __restrict__ lm, const int* __restrict__ k2, const int* __restrict__ kmin,
                                                 const int* __restrict__ eoff, int* __restrict__ slot) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int l = lm[i];
  slot[i] = eoff[l] + (k2[i] - kmin[l] - 1);
}
// k_tf_slots and k_zero_slots in one launch: workgroups [0, g_slots) take the blocks, the rest clear the slot records
__global__ __launch_bounds__(kT) void k_tf_slots_zero(int n, int g_slots, const int* __restrict__ lm, const int* __restrict__ k2, const int* __restrict__ kmin,
                                                      const int* __restrict__ eoff, int* __restrict__ slot, const int* __restrict__ n_slots, double* __restrict__ slotB) {
  if ((int)blockIdx.x < g_slots) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int l = lm[i];
    slot[i] = eoff[l] + (k2[i] - kmin[l] - 1);
    return;
  }
  const size_t nz = (size_t)*n_slots * 4;     // double2 elements
  double2* b = reinterpret_cast<double2*>(slotB);
  const size_t gz = gridDim.x - g_slots;
  for (size_t i = (size_t)(blockIdx.x - g_slots) * kT + threadIdx.x; i < nz; i += gz * kT) b[i] = make_double2(0.0, 0.0);
}
// slots of keyframes that do not observe their landmark (gaps in a track) are never written by the linearisation: cleared once here
// sorted copies of the TwoFrame block arrays: block i of the copy = block perm[i] of the batch
__global__ __launch_bounds__(kT) void k_tf_gather(int n, const int* __restrict__ perm, const double2* __restrict__ fo, const double2* __restrict__ ob,
                                                   const int* __restrict__ lm, const int* __restrict__ k1, const int* __restrict__ k2,
                                                   double2* __restrict__ fo_s, double2* __restrict__ ob_s, int* __restrict__ lm_s, int* __restrict__ k1_s, int* __restrict__ k2_s) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const int j = perm[i];
  fo_s[i] = fo[j]; ob_s[i] = ob[j]; lm_s[i] = lm[j]; k1_s[i] = k1[j]; k2_s[i] = k2[j];
}
__global__ __launch_bounds__(kT) void k_zero_slots(const int* __restrict__ n_slots, double* __restrict__ slotB) {
  const size_t n = (size_t)*n_slots * 4;     // double2 elements
  double2* b = reinterpret_cast<double2*>(slotB);
  for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < n; i += (size_t)gridDim.x * kT) b[i] = make_double2(0.0, 0.0);
}

__device__ __forceinline__ void schur_band_body(const int bx, const int by, int dp, int ldE, const double* __restrict__ E,
                                                const double* __restrict__ Cd, const int* __restrict__ order, const int* __restrict__ n_active_p,
                                                const int* __restrict__ kmin, const int* __restrict__ kmax, int d, int ldS,
                                                double* __restrict__ S, unsigned long long* dbg = nullptr, const int rows = kBandRows,
                                                const int4* __restrict__ item = nullptr) {
  extern __shared__ double sh[];          // Es[kSchurRows][ldl] | icd[kSchurRows] | rowid (int)[kBandRows]
  auto mark = [&](int k) { if (dbg && threadIdx.x == 0) dbg[k] = wall_clock64(); };   // LVF_SCHUR_TIMING=1: phase stamps of this workgroup
  mark(0);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lk = lane >> 4, lc = lane & 15;
  // the slice's extent and band: from the work item when there is one (k_band_work computed them once per configure: three dependent
  // global round trips — n_active, order[], kmin/kmax[] — off the front of every workgroup), else every wave reduces them for itself
  const int k_begin = bx * rows;
  int k_end, lo = 0x7fffffff, hi = -1;
  if (item) { const int4 it = *item; k_end = it.w; lo = it.z & 0xffff; hi = it.z >> 16; }
  else {
    k_end = min(*n_active_p, k_begin + rows);
    if (k_begin >= k_end) return;
    for (int r = k_begin + lane; r < k_end; r += 64) { const int l = order[r]; lo = min(lo, kmin[l]); hi = max(hi, kmax[l]); }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  }
  const int t0 = (6 * lo) >> 4, t1 = (6 * hi + 5) >> 4, tl = dp >> 4;
  const int nbt = t1 - t0 + 1, tri = nbt * (nbt + 1) / 2;
  const bool extra = tl > t1;                                  // the g_rho column's tile lies outside the band
  const int ntiles = tri + (extra ? nbt : 0);
  const int tbase = by * kBandTilesPerGroup;
  if (tbase >= ntiles) return;
  const int ldl = 16 * (nbt + (extra ? 1 : 0));                // staged doubles per row
  double* Es = sh;
  double* icd = sh + kSchurRows * (ldE + 16);
  int* rowid = reinterpret_cast<int*>(icd + kSchurRows);
  for (int r = tid; r < rows; r += 256) rowid[r] = (k_begin + r < k_end) ? order[k_begin + r] : -1;
  // this wave's tiles: t = tbase + w + 4 s; local tile columns (a = row tile, b = column tile), extra row tile = index nbt
  int ta[kBandTilesPerWave], tb[kBandTilesPerWave], nt = 0;
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) {
    const int t = tbase + w + 4 * s_;
    ta[s_] = 0; tb[s_] = 0;
    if (t < ntiles) {
      if (t < tri) {
        int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while ((a + 1) * (a + 2) / 2 <= t) ++a;
        while (a * (a + 1) / 2 > t) --a;
        ta[s_] = a; tb[s_] = t - a * (a + 1) / 2;
      } else { ta[s_] = nbt; tb[s_] = t - tri; }
      nt = s_ + 1;
    }
  }
  double4_t acc[kBandTilesPerWave];
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) acc[s_] = double4_t{0.0, 0.0, 0.0, 0.0};
  // staging: thread (row fr = tid >> 4, column fc = tid & 15) carries column fc of every staged 16-column tile of its row:
  // no index arithmetic beyond one add per tile, 128-byte runs per 16 lanes
  constexpr int kPf = 20;                  // tiles prefetched in registers (ldl <= 320); wider bands finish through fetch_tail
  double pf[kPf];
  double pf_cd = 1.0;
  const int fr = tid >> 4, fc = tid & 15, nst = ldl >> 4;
  __syncthreads();                         // rowid
  auto fetch = [&](int k0) {
    const int l = rowid[k0 - k_begin + fr];
    const double* src = E + (size_t)max(l, 0) * ldE + fc;
    if (fc == 0) pf_cd = (l >= 0) ? Cd[l] : 1.0;
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      double v = 0.0;
      if (u < nst && l >= 0) v = src[16 * (u < nbt ? t0 + u : tl)];
      pf[u] = v;
    }
  };
  auto fetch_tail = [&](int k0) {
    const int l = rowid[k0 - k_begin + fr];
    for (int u = kPf; u < nst; ++u) Es[fr * ldl + 16 * u + fc] = (l >= 0) ? E[(size_t)l * ldE + 16 * (u < nbt ? t0 + u : tl) + fc] : 0.0;
  };
  fetch(k_begin);
  mark(1);
  for (int k0 = k_begin; k0 < k_end; k0 += kSchurRows) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPf; ++u) if (u < nst) Es[fr * ldl + 16 * u + fc] = pf[u];
    fetch_tail(k0);
    if (fc == 0) icd[fr] = (rowid[k0 - k_begin + fr] >= 0) ? 1.0 / pf_cd : 0.0;
    __syncthreads();
    if (k0 + kSchurRows < k_end) fetch(k0 + kSchurRows);
#pragma unroll
    for (int kk = 0; kk < kSchurRows; kk += 4) {
      const double* row = Es + (kk + lk) * ldl;
      const double wgt = icd[kk + lk];
#pragma unroll
      for (int s_ = 0; s_ < kBandTilesPerWave; ++s_)
        if (s_ < nt) acc[s_] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ta[s_] + lc] * wgt, row[16 * tb[s_] + lc], acc[s_], 0, 0, 0);
    }
  }
  mark(2);
#pragma unroll
  for (int s_ = 0; s_ < kBandTilesPerWave; ++s_) {
    if (s_ >= nt) continue;
    const int gti = ta[s_] < nbt ? t0 + ta[s_] : tl, gtj = t0 + tb[s_];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = gti * 16 + lk + 4 * r, gj = gtj * 16 + lc;
      const double v = acc[s_][r];
      if (v == 0.0) continue;
      if (gi < dp && gj < dp) { if (gj <= gi) atomicAdd(&S[(size_t)gi * ldS + gj], -v); }
      else if (gi == dp && gj < dp) atomicAdd(&S[(size_t)d * ldS + gj], v);
    }
  }
  mark(3);
}

__global__ __launch_bounds__(256) void k_schur_band(int dp, int ldE, const double* __restrict__ E, const double* __restrict__ Cd,
                                                    const int* __restrict__ order, const int* __restrict__ n_active_p,
                                                    const int* __restrict__ kmin, const int* __restrict__ kmax, int d, int ldS,
                                                    double* __restrict__ S) {
  schur_band_body(blockIdx.x, blockIdx.y, dp, ldE, E, Cd, order, n_active_p, kmin, kmax, d, ldS, S);
}

// ------------------------------------------------------------------------------------------------ blocked Cholesky (64)
// Right-looking, block 64, ONE launch per block step (k_chol_step): every workgroup of the step's column re-factors the 64x64 diagonal
// block (redundantly: all of them run it concurrently, which removes a dependent launch) while its own panel block rides along in the
// same sweep, and the trailing update of the previous step is folded into the same launch (chol_step_body).
// The sequential critical path is ~64 x (rsqrt + broadcast) per block; everything else is wide.  Two sweeps over the 64 pivots exist: the
// 16-pivot sub-block sweep (sub_pivots, the default) and the pair-pivot sweep it replaced (factor_diag_wave / factor_panel_wave,
// LVF_CHOL_SUBBLOCK=0); loads, the previous step's update, the stores and everything another launch reads are common to both.

__device__ __forceinline__ void load_row64(const double* __restrict__ g, double a[kNB]) {
  const double2* g2 = reinterpret_cast<const double2*>(g);
#pragma unroll
  for (int c = 0; c < kNB / 2; ++c) { const double2 v = g2[c]; a[2 * c] = v.x; a[2 * c + 1] = v.y; }
}
__device__ __forceinline__ void store_row64(double* __restrict__ g, const double a[kNB]) {
  double2* g2 = reinterpret_cast<double2*>(g);
#pragma unroll
  for (int c = 0; c < kNB / 2; ++c) g2[c] = make_double2(a[2 * c], a[2 * c + 1]);
}


// Factor + panel solve of one 64-wide block column by ONE workgroup of 512 threads = 8 waves, thread = row r = tid & 63:
//   waves 0..3 ("diagonal" waves) hold the diagonal block, wave Q the columns 16Q..16Q+15 of every row;
//   waves 4..7 ("panel" waves) hold the workgroup's panel block the same way; X L^T = A is solved in the same sweep: once column j of L
//   is known, x_rj = b_rj / L_jj is final and the row's later columns take the rank-1 term x_rj L_tj.
// One wave issues at most one VALU instruction per ~8 clocks (tools/ubench), so what a wave costs is its instruction count; the 64
// pivots are a dependent chain through the diagonal waves, and everything that is not the chain is kept out of their instruction stream.
// The wave-uniform operands L_tj of the rank-1 updates are fetched with ONE 8-byte LDS read per pivot (lane t of each 16-lane row takes
// L_tj) and handed out by the DPP row_newbcast operand of v_fmac_f64: as 16-byte broadcast reads they occupied the LDS pipe for 8 clocks
// each, 8 per pivot and wave, and that pipe — shared by all waves — set the pace (measured 375 clocks per pivot with 4 waves, 512 with
// 8); through v_readlane + SGPR operands it was slower still (900).
//   * pivots are taken kPG at a time: the owning wave finishes a group of kPG columns on its own (the later columns of the group take
//     the earlier ones' rank-1 terms from registers and lane broadcasts) and publishes them (Lcol[j][r], 1/L_jj); the other diagonal
//     waves apply a group ONE STEP after it was published, so the owner never waits for them: one workgroup barrier per step, at which
//     the consumers — who have less to do per step — are already waiting when the owner arrives;
//   * the panel arithmetic (three quarters of the flops) lives in its own four waves, which run one more step behind on the published
//     columns: they share the barriers but never hold the chain up;
//   * 1/sqrt is the hardware estimate plus one second-order correction (the library call adds range checks and two dependent selects
//     per pivot); a non-positive pivot is flagged and its NaN/inf only lives until the step is rejected.  Lane j holds A_jj itself, so
//     scaling its entry gives L_jj with no select.
// acc += (lane N of each 16-lane row of lv) * m: the DPP row_newbcast operand of v_fmac_f64 hands a row-uniform value to all 16 lanes
// inside the multiply-add itself (no LDS broadcast read, no v_readlane + SGPR operand)
template <int N>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double lv, double m) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(lv), "v"(m), "n"(N));
}
// (`from` folds to a constant once the caller's loops are unrolled)
__device__ __forceinline__ void rank1_row_bcast(const int from, double a[16], double lv, double m) {
  asm volatile("s_nop 4");                           // (an EXEC change needs 5 wait states before a DPP read; inline asm is not hazard-checked)
  if (from <= 0) fmac_row_bcast<0>(a[0], lv, m);
  if (from <= 1) fmac_row_bcast<1>(a[1], lv, m);
  if (from <= 2) fmac_row_bcast<2>(a[2], lv, m);
  if (from <= 3) fmac_row_bcast<3>(a[3], lv, m);
  if (from <= 4) fmac_row_bcast<4>(a[4], lv, m);
  if (from <= 5) fmac_row_bcast<5>(a[5], lv, m);
  if (from <= 6) fmac_row_bcast<6>(a[6], lv, m);
  if (from <= 7) fmac_row_bcast<7>(a[7], lv, m);
  if (from <= 8) fmac_row_bcast<8>(a[8], lv, m);
  if (from <= 9) fmac_row_bcast<9>(a[9], lv, m);
  if (from <= 10) fmac_row_bcast<10>(a[10], lv, m);
  if (from <= 11) fmac_row_bcast<11>(a[11], lv, m);
  if (from <= 12) fmac_row_bcast<12>(a[12], lv, m);
  if (from <= 13) fmac_row_bcast<13>(a[13], lv, m);
  if (from <= 14) fmac_row_bcast<14>(a[14], lv, m);
  if (from <= 15) fmac_row_bcast<15>(a[15], lv, m);
}
struct FactorLds { double* Lcol; double* Xcol; double* Linv; };       // Lcol/Xcol: [64 columns][64 rows]

// diagonal wave Q, steps s = kGW qj + i (i unrolled, qj a real loop: the code of one column group is reused four times).  In step s the
// owner of group s runs its pivots while every other diagonal wave applies group s - 1 (published at the end of step s - 1); the
// workgroup meets at one barrier per step.
// `nsteps` (<= kNB / kPG + 1): the last block of the corner is padded with identity rows / columns — their pivots are 1 and nothing
// real depends on them — so the sweep stops one step after the last real pivot group (every wave of the workgroup gets the same count:
// the barriers stay matched)
__device__ __forceinline__ bool factor_diag_wave(double a[16], const int r, const int Q, const FactorLds& F, const int nsteps = kNB / kPG + 1) {
  bool bad = false;
#pragma unroll 1
  for (int qj = 0; qj <= kNB / 16; ++qj) {
#pragma unroll
    for (int i = 0; i < kGW; ++i) {
      if ((qj == kNB / 16 && i > 0) || kGW * qj + i >= nsteps) break;
      const int j0 = 16 * qj + kPG * i;                   // first pivot of group s
      const int prev_owner = i > 0 ? qj : qj - 1;         // owner of group s - 1
      if (j0 > 0 && prev_owner < Q) {                     // columns right of group s - 1: all 16
#pragma unroll
        for (int g = 0; g < kPG; ++g) {
          const int j = j0 - kPG + g;
          const double cr = F.Lcol[j * kNB + r], lv = F.Lcol[j * kNB + 16 * Q + (r & 15)];
          rank1_row_bcast(0, a, lv, -cr);                 // A_rt -= L_rj L_tj (meaningful for r >= t)
        }
      }
      if (qj == Q) {                                      // own group: pivots j0 .. j0 + kPG - 1
#pragma unroll
        for (int g = 0; g < kPG; ++g) {
          const int jj = kPG * i + g, j = j0 + g;
          const double djj = lane_bcast(a[jj], j);        // pivot A_jj sits in lane j (= row j) of this wave
          bad |= !(djj > 0.0);
          const double y0 = __builtin_amdgcn_rsq(djj);
          const double e = fma(-djj * y0, y0, 1.0);
          const double inv_l = fma(y0 * e, fma(e, 0.375, 0.5), y0);
          a[jj] *= inv_l;
          F.Lcol[j * kNB + r] = a[jj];
          F.Linv[j] = inv_l;                              // (every lane stores the same value: no exec juggling on the chain)
#pragma unroll
          for (int h = g + 1; h < kPG; ++h) a[kPG * i + h] -= a[jj] * lane_bcast(a[jj], j0 + h);
        }
        // the rest of this wave's own columns: L_tj of its own rows t comes back from the column it has just published
#pragma unroll
        for (int g = 0; g < kPG; ++g)
          if (kPG * (i + 1) < 16) rank1_row_bcast(kPG * (i + 1), a, F.Lcol[(j0 + g) * kNB + 16 * Q + (r & 15)], -a[kPG * i + g]);
      }
      __syncthreads();
    }
  }
  return bad;
}

// panel wave Q: owns the x columns 16Q..16Q+15 of its rows and runs one step behind the diagonal waves: in step s it applies the x
// group s - 2 its left neighbours published in step s - 1, then — if it owns group s - 1 — finishes those x columns and publishes them.
__device__ __forceinline__ void factor_panel_wave(double b[16], const int r, const int Q, const FactorLds& F, const int nsteps = kNB / kPG + 1) {
#pragma unroll 1
  for (int qj = 0; qj <= kNB / 16; ++qj) {
#pragma unroll
    for (int i = 0; i < kGW; ++i) {
      if ((qj == kNB / 16 && i > 0) || kGW * qj + i >= nsteps) break;
      const int j0 = 16 * qj + kPG * i;
      const int o2 = i > 1 ? qj : qj - 1;                 // owner of group s - 2
      if (j0 >= 2 * kPG && o2 < Q) {
#pragma unroll
        for (int g = 0; g < kPG; ++g) {
          const int j = j0 - 2 * kPG + g;
          const double cx = F.Xcol[j * kNB + r], lv = F.Lcol[j * kNB + 16 * Q + (r & 15)];
          rank1_row_bcast(0, b, lv, -cx);
        }
      }
      const int o1 = i > 0 ? qj : qj - 1, i1 = (i + kGW - 1) % kGW;     // owner of group s - 1 and its index within the wave
      if (j0 > 0 && o1 == Q) {
#pragma unroll
        for (int g = 0; g < kPG; ++g) {
          const int jj = kPG * i1 + g, j = 16 * o1 + jj;
          const double lv = F.Lcol[j * kNB + 16 * Q + (r & 15)];
          b[jj] *= F.Linv[j];
          F.Xcol[j * kNB + r] = b[jj];
          if (jj + 1 < 16) rank1_row_bcast(jj + 1, b, lv, -b[jj]);
        }
      }
      __syncthreads();
    }
  }
}

// ---- 16-pivot sub-blocks (the default sweep; LVF_CHOL_SUBBLOCK=0 selects the pair-pivot sweep above)
// The 64 pivots of a block are four stages of 16.  Both halves of the block live in LDS between the stages (the diagonal block in Pj,
// the panel block in Pi, row stride kLd); in stage q ONE diagonal wave (q) and ONE panel wave take the column group 16q..16q+15 of their
// half into registers, run the 16 pivots with no LDS access and no barrier, and put the finished columns back; the next column group
// then takes the stage's contribution as 16x16 tile products on the matrix cores (one tile per wave), and the column groups behind it
// take theirs under the next stage's sweep, from waves that do not sweep.
// Inside the sweep every operand that is uniform over a row group comes from the DPP row_newbcast operand: the 16x16 diagonal tile D sits
// replicated in all four 16-lane rows (lane i of each row holds row i of D in d[0..15]), so lane t of ANY row can hand out L_tj, and the
// same instructions carry one 16-row group per DPP row in b[0..15] (rows 16g+i of the wave's half: x_j = b_j / L_jj, b_t -= x_j L_tj).
// Hazards the assembler does not check for inline asm: a VALU write of a VGPR needs 2 wait states before a DPP instruction reads it
// (the scaled column is written by an asm multiply that carries its own s_nop; the pivot broadcast waits in front), an EXEC change needs 5
// (the first broadcast of a sweep waits for them).
template <int N>
__device__ __forceinline__ void fnmac_row_bcast(double& acc, double lv, double m) {     // acc -= (lane N of each 16-lane row of lv) * m
  asm("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(lv), "v"(m), "n"(N));
}
template <int T>
__device__ __forceinline__ void sub_rank1(double d[16], double b[16], const double dj, const double xj) {
  if constexpr (T < 16) {
    fnmac_row_bcast<T>(d[T], dj, dj);                 // D_it -= L_ij L_tj  (the next pivot's own column first)
    fnmac_row_bcast<T>(b[T], dj, xj);                 // B_rt -= x_rj L_tj
    sub_rank1<T + 1>(d, b, dj, xj);
  }
}
// H[16g.., 16c..] -= H[16g.., 16s..] * Pj[16c.., 16s..]^T on the matrix cores (H: Pj, the diagonal block, or Pi, the panel block; A[i = lc][k = lk],
// B[k = lk][j = lc], D: col = lc, row = lk + 4 reg, as in chol_update_tile)
__device__ __forceinline__ void sub_tile_update(double* H, const double* Pj, const int g, const int c, const int s, const int lk, const int lc) {
  double* Tc = H + (16 * g + lk) * kLd + 16 * c + lc;
  const double* Ta = H + (16 * g + lc) * kLd + 16 * s + lk;
  const double* Tb = Pj + (16 * c + lc) * kLd + 16 * s + lk;
  double4_t ac;
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) ac[rg] = Tc[4 * rg * kLd];
#pragma unroll
  for (int k0 = 0; k0 < 16; k0 += 4) ac = __builtin_amdgcn_mfma_f64_16x16x4f64(-Ta[k0], Tb[k0], ac, 0, 0, 0);
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) Tc[4 * rg * kLd] = ac[rg];
}
template <int J>
__device__ __forceinline__ void sub_pivots(double d[16], double b[16], bool& bad) {
  double djj = 0.0;                                   // D_jj of lane j, to every lane of the row: 0 + bcast * 1 (exact)
  if (J == 0) asm("s_nop 4\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(djj) : "v"(d[J]), "v"(1.0), "n"(J));
  else asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(djj) : "v"(d[J]), "v"(1.0), "n"(J));
  bad |= !(djj > 0.0);
  const double y0 = __builtin_amdgcn_rsq(djj);
  const double e = fma(-djj * y0, y0, 1.0);
  const double inv_l = fma(y0 * e, fma(e, 0.375, 0.5), y0);
  double dj;
  asm("v_mul_f64 %0, %1, %2\n\ts_nop 1" : "=v"(dj) : "v"(d[J]), "v"(inv_l));
  const double xj = b[J] * inv_l;
  d[J] = dj; b[J] = xj;
  if constexpr (J < 15) { sub_rank1<J + 1>(d, b, dj, xj); sub_pivots<J + 1>(d, b, bad); }
}

// ONE launch per block step kb (grid = chol_step_grid), 512 threads per workgroup:
//   workgroups [0, 2 + below)  — the column of step kb.  For kb > 0 each first applies step kb-1's trailing update to the two tiles it
//       reads, A_kk -= P_k P_k^T (diagonal waves) and A_ik -= P_i P_k^T (panel waves) (P = the panel of column kb-1, staged in LDS;
//       v_mfma_f64_16x16x4_f64), instead of waiting for a separate update launch.  Then: workgroup 0 stores the factored diagonal
//       block; workgroups 1..below solve their panel block X L^T = A; the last workgroup solves against the identity and leaves
//       L_kk^-T for the back substitution.
//   workgroups behind them     — the rest of step kb-1's trailing update, A[bi][bj] -= P_bi P_bj^T for kb < bj <= bi, which nothing in
//       this launch reads (the next step does).

// staging of a 64x64 block at g (leading dimension ld) into LDS with row stride kLd by 256 threads (t = 0..255): all eight 16-byte
// loads of a thread are in flight before the first LDS write (written as one loop the compiler waits for each load in turn)
struct Stage64 { double2 v[8]; };
__device__ __forceinline__ void stage_issue(const double* g, int ld, int t, Stage64& st) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = t + 256 * i, rr = e >> 5, c = (e & 31) * 2;
    st.v[i] = *reinterpret_cast<const double2*>(g + (size_t)rr * ld + c);
  }
}
__device__ __forceinline__ void stage_commit(const Stage64& st, int t, double* __restrict__ L) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = t + 256 * i, rr = e >> 5, c = (e & 31) * 2;
    L[rr * kLd + c] = st.v[i].x; L[rr * kLd + c + 1] = st.v[i].y;
  }
}

// the two 64 x 65 panel buffers of a block-step workgroup: ONE pair per kernel, shared by the column / trailing-update workgroups and by the
// riders that form the back substitution's block products (a pair of their own would double the launch's static LDS)
struct PanelLds { double* Pi; double* Pj; };
__device__ __forceinline__ PanelLds panel_lds() {
  __shared__ double Pi[kNB * kLd];
  __shared__ double Pj[kNB * kLd];
  return PanelLds{Pi, Pj};
}

// trailing update of one tile: A[bi][bj] -= P_bi P_bj^T with the panels of column kp.  Wave wv produces rows 16 (wv & 3) .. + 15 of the
// column half wv >> 2 (A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4) + 4 reg).
__device__ __forceinline__ void chol_update_tile(double* S, int ld, int kp, int bi, int bj, double* Pi, double* Pj) {
  // the tile being updated is requested FIRST (it does not depend on the product) so its round trip hides under the panel
  // staging and the matrix-core work; S is not __restrict__ so the loads stay where they are written
  const int wv = threadIdx.x >> 6, w = wv & 3, ch = wv >> 2, lane = threadIdx.x & 63, lk = lane >> 4, lc = lane & 15;
  double* out = S + (size_t)(bi * kNB + 16 * w) * ld + bj * kNB + 32 * ch;
  double o[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) o[ct][rg] = out[(size_t)(lk + 4 * rg) * ld + 16 * ct + lc];
  {
    Stage64 st;
    const int t = threadIdx.x & 255;
    stage_issue(S + (size_t)((ch ? bj : bi) * kNB) * ld + kp * kNB, ld, t, st);
    stage_commit(st, t, ch ? Pj : Pi);
  }
  __syncthreads();
  double4_t acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int k0 = 0; k0 < kNB; k0 += 4) {
    const double av = Pi[(16 * w + lc) * kLd + k0 + lk];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Pj[(32 * ch + 16 * ct + lc) * kLd + k0 + lk], acc[ct], 0, 0, 0);
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) out[(size_t)(lk + 4 * rg) * ld + 16 * ct + lc] = o[ct][rg] - acc[ct][rg];
}

// The block form of the dense back substitution (Chain::back_blocks).  x_k = Dinv_k (y_k - sum_{j > k} L_jk^T x_j) is a chain of nb links
// with two products each; with T_kj = -Dinv_k L_jk^T it is x_k = sum_{j > k} T_kj x_j (y rides along as column d of the last block row,
// met by a -1 in the multiplier), one short product per link.  Both factors of T_kj are final when launch k ends, and nothing in launch
// k + 1 writes them: rider vb of launch kb forms the block k = kb - 1, j = kb + vb like a trailing-update tile (P_i = L_jk, P_j = Dinv_k,
// two 16x16 tiles per wave on the matrix cores).  Stored TRANSPOSED, block (k, j) at T + (k nb + j) 64^2, entry [r][c] = T_kj[c][r]: the
// back substitution's wave `part` reads rows 8 part .. 8 part + 7, each one contiguous run of 64 doubles.
// Riders wait for nothing and raise no flag; a poisoned factor sends its NaN through here into a step the failure flag rejects.
__device__ __forceinline__ void back_block_ride(const int vb, const CholArgs& A, const int kb, const TRide& R) {
  if (vb >= R.n || kb < 1 || kb + vb >= A.nb) return;
  if (A.done && *A.done) return;
  const int k = kb - 1, j = kb + vb;
  const PanelLds PL = panel_lds();
  const int wv = threadIdx.x >> 6, w = wv & 3, ch = wv >> 2, lane = threadIdx.x & 63, lk = lane >> 4, lc = lane & 15;
  {
    Stage64 st;
    const int t = threadIdx.x & 255;
    if (ch) stage_issue((const double*)A.Dinv + (size_t)k * kNB * kNB, kNB, t, st);
    else stage_issue((const double*)A.Sd + (size_t)(j * kNB) * A.ld + k * kNB, A.ld, t, st);
    stage_commit(st, t, ch ? PL.Pj : PL.Pi);
  }
  __syncthreads();
  double4_t acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int k0 = 0; k0 < kNB; k0 += 4) {
    const double av = PL.Pi[(16 * w + lc) * kLd + k0 + lk];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, PL.Pj[(32 * ch + 16 * ct + lc) * kLd + k0 + lk], acc[ct], 0, 0, 0);
  }
  double* out = (double*)R.T + ((size_t)k * A.nb + j) * kNB * kNB + (size_t)(16 * w) * kNB + 32 * ch;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) out[(lk + 4 * rg) * kNB + 16 * ct + lc] = -acc[ct][rg];
}

// SUB: the 16-pivot sub-block sweep (default); !SUB: the pair-pivot sweep (factor_diag_wave / factor_panel_wave)
template <bool SUB>
__device__ __forceinline__ void chol_step_body(const int bx, const CholArgs& A, const int kb) {
  const int below = A.nb - kb - 1;
  if (bx >= chol_step_grid(A.nb, kb)) return;                          // (workgroup-uniform: no barrier is skipped by part of a workgroup)
  const int dv = done_flag_issue(A.done);
  double* S = A.Sd; const int ld = A.ld; int* __restrict__ fail = A.fail; double* __restrict__ Dinv = A.Dinv;
  const PanelLds PL = panel_lds();
  double* const Pi = PL.Pi; double* const Pj = PL.Pj;
  __shared__ double Linv[kNB];
  if (bx >= 2 + below) {                              // trailing tiles of step kb-1 right of column kb
    int t = bx - (2 + below), ii = 0;
    while (t >= ii + 1) { t -= ii + 1; ++ii; }
    if (dv) return;
    chol_update_tile(S, ld, kb - 1, kb + 1 + ii, kb + 1 + t, Pi, Pj);
    return;
  }
  const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
  const bool panel_wave = wv >= 4;                    // wave-uniform
  // column group of the wave.  Waves land on SIMD wv % 4: the panel wave of group q sits two SIMDs away from the diagonal wave of group q,
  // so the two waves that are busiest at the same time (the pivot owner and the panel owner one step behind it) do not share an issue port
  const int q = panel_wave ? ((wv + 2) & 3) : wv;
  unsigned long long* dbg = (A.dbg && bx == 1 && tid == 0) ? A.dbg + 8 * kb : nullptr;
  if (dbg) dbg[0] = wall_clock64();
  const bool inverse_wg = bx == 1 + below, panel_wg = bx > 0 && !inverse_wg;
  double* brow = inverse_wg ? Dinv + (size_t)kb * kNB * kNB + (size_t)r * kNB + 16 * q
                            : S + (size_t)((kb + bx) * kNB + r) * ld + kb * kNB + 16 * q;
  double* drow = S + (size_t)(kb * kNB + r) * ld + kb * kNB + 16 * q;
  double a[16];                                       // diagonal waves: row r of A_kk; panel waves: row r of the panel block / identity
  if (!panel_wave || panel_wg) {
    const double2* g2 = reinterpret_cast<const double2*>(panel_wave ? brow : drow);
#pragma unroll
    for (int c = 0; c < 8; ++c) { const double2 v = g2[c]; a[2 * c] = v.x; a[2 * c + 1] = v.y; }
  } else {
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = (inverse_wg && 16 * q + c == r) ? 1.0 : 0.0;
  }
  if (dv) return;                                     // (the tile loads above are in flight behind the flag's)
  if (kb > 0) {
    // step kb-1's update of the tiles just requested: diagonal wave q forms rows 16q..16q+15 of P_k P_k^T (lower tiles only), panel wave q
    // those of P_i P_k^T; the products go through LDS into the row-per-lane layout of the factorisation
    const int lane = tid & 63, lk = lane >> 4, lc = lane & 15;
    {
      Stage64 st;
      const int t = tid & 255;
      const bool mine = !panel_wave || panel_wg;
      if (mine) stage_issue(S + (size_t)((panel_wave ? kb + bx : kb) * kNB) * ld + (kb - 1) * kNB, ld, t, st);
      if (mine) stage_commit(st, t, panel_wave ? Pi : Pj);
    }
    __syncthreads();
    if (dbg) dbg[1] = wall_clock64();
    // 10 lower tiles of P_k P_k^T + (panel workgroups) 16 tiles of P_i P_k^T, dealt round-robin to the 8 waves (two waves share a SIMD's
    // matrix pipe: 6.5 tile products per SIMD instead of up to 8 with one strip per wave)
    const int n_tiles = panel_wg ? 26 : 10;
    double4_t ac[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    int t_m[4], t_c[4]; bool t_own[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int t = wv + 8 * n;
      t_own[n] = t >= 10;
      if (t_own[n]) { t_m[n] = (t - 10) >> 2; t_c[n] = (t - 10) & 3; }
      else { int m = 0, u = t; while (u > m) { u -= m + 1; ++m; } t_m[n] = m; t_c[n] = u; }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (wv + 8 * n < n_tiles) {
        const double* Pa = (t_own[n] ? Pi : Pj) + (16 * t_m[n] + lc) * kLd + lk;
        const double* Pb = Pj + (16 * t_c[n] + lc) * kLd + lk;
#pragma unroll
        for (int k0 = 0; k0 < kNB; k0 += 4) ac[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(Pa[k0], Pb[k0], ac[n], 0, 0, 0);
      }
    __syncthreads();                                  // every wave is done reading the panels: the products take their place
    if (dbg) dbg[2] = wall_clock64();
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (wv + 8 * n < n_tiles) {
        double* Pw = t_own[n] ? Pi : Pj;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) Pw[(16 * t_m[n] + lk + 4 * rg) * kLd + 16 * t_c[n] + lc] = ac[n][rg];
      }
    __syncthreads();
    double* Pw = panel_wave ? Pi : Pj;
    if (!panel_wave || panel_wg)
#pragma unroll
      for (int c = 0; c < 16; ++c) a[c] -= Pw[r * kLd + 16 * q + c];     // (entries right of the diagonal are never read as values of A)
    if (SUB && (!panel_wave || bx > 0))               // the updated halves stay in LDS, in place of the products (own entries only)
#pragma unroll
      for (int c = 0; c < 16; ++c) Pw[r * kLd + 16 * q + c] = a[c];
    __syncthreads();                                  // the factorisation reuses both buffers
  } else if (SUB) {
    double* Pw = panel_wave ? Pi : Pj;
    if (!panel_wave || bx > 0)
#pragma unroll
      for (int c = 0; c < 16; ++c) Pw[r * kLd + 16 * q + c] = a[c];
    __syncthreads();
  }
  if (dbg) { dbg[3] = wall_clock64(); dbg[6] = clock64(); }
  const FactorLds F{Pi, Pj, Linv};
  bool bad = false;
  // pivot groups to run: all of them, except in the last block where only the real columns (the rest is identity padding) need any
  const int ncols = (kb == A.nb - 1 && A.last_cols > 0) ? min(A.last_cols, kNB) : kNB;
  if constexpr (SUB) {
    // stages to run: those that hold a real column (the padding's pivots are 1 and its off-diagonal entries 0: a stage made of padding
    // alone changes nothing, and neither does the update it would take from the stages before it).  Workgroup-uniform: barriers match.
    const int nstages = (ncols + 15) >> 4;
    const int wu = __builtin_amdgcn_readfirstlane(wv), qu = wu >= 4 ? ((wu + 2) & 3) : wu;      // scalar copies: the branches below are not EXEC masks
    const bool has_panel = bx > 0;
    const int lane = tid & 63, lk = lane >> 4, lc = lane & 15;
    double* Ph = wu >= 4 ? Pi : Pj;                   // the wave's half: diagonal block / panel block (identity in the inverse workgroup)
    unsigned long long* dbs = (dbg && kb < 8) ? A.dbg + 64 + 8 * kb : nullptr;
#pragma unroll 1
    for (int s = 0; s < nstages; ++s) {
      if (qu == s && (wu < 4 || has_panel)) {
        double d[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = Ph[r * kLd + 16 * s + c];
#pragma unroll
        for (int c = 0; c < 16; ++c) d[c] = Pj[(16 * s + (r & 15)) * kLd + 16 * s + c];
        sub_pivots<0>(d, a, bad);
        // L[:, 16s..] / X[:, 16s..] go back for the tile products; a[] keeps them for the stores.  The diagonal wave puts back the rows
        // BELOW the tile only: the panel wave of this stage reads D from Pj with no barrier between, so D must stay as it is (nothing
        // reads rows <= 16s + 15 of this column group from LDS afterwards: the products take row groups > s, the Ldiag store takes a[])
        if (wu >= 4 || r >= 16 * (s + 1))
#pragma unroll
          for (int c = 0; c < 16; ++c) Ph[r * kLd + 16 * s + c] = a[c];
      }
      else if (s > 0 && (((wu - s) & 1) != 0)) {
        // the tiles right of column group s take stage s - 1's columns NOW, under the sweep of stage s: the sweeping waves read and write
        // column group s only, these waves read column group s - 1 (final since the last stage) and write column groups > s.  Dealt to
        // the four waves on the two SIMDs that host no sweeping wave
        const int sp = s - 1, nd = 3 - sp, rd = nd * (nd - 1) / 2, n_def = rd + (has_panel ? 4 * (nd - 1) : 0);
        const int slot = (((wu - s - 1) & 3) >> 1) * 2 + (wu >> 2);
#pragma unroll 1
        for (int u = slot; u < n_def; u += 4) {
          if (u < rd) { const bool first = u < nd - 1; sub_tile_update(Pj, Pj, first ? sp + 2 + u : sp + 3, first ? sp + 2 : sp + 3, sp, lk, lc); }
          else sub_tile_update(Pi, Pj, (u - rd) & 3, sp + 2 + ((u - rd) >> 2), sp, lk, lc);
        }
      }
      __syncthreads();
      if (dbs) dbs[2 * s] = wall_clock64();
      if (s + 1 < nstages) {
        // column group s + 1 takes stage s's columns before its own sweep: L21 L21^T on the 3 - s lower tiles of the diagonal block and
        // X L21^T on the four panel tiles, one tile per wave.  A tile is updated by one wave, in place; the column group s it is
        // updated from is not written in this phase.
        const int nd = 3 - s;
        if (wu < nd) sub_tile_update(Pj, Pj, s + 1 + wu, s + 1, s, lk, lc);
        else if (has_panel && wu < nd + 4) sub_tile_update(Pi, Pj, wu - nd, s + 1, s, lk, lc);
        __syncthreads();
        if (dbs) dbs[2 * s + 1] = wall_clock64();
      }
    }
  } else {
    const int nsteps = (ncols + kPG - 1) / kPG + 1;
    if (panel_wave) factor_panel_wave(a, r, q, F, nsteps);
    else bad = factor_diag_wave(a, r, q, F, nsteps);
  }
  if (dbg) { dbg[4] = wall_clock64(); dbg[7] = clock64(); }
  if (bad && r == 0) atomicMax(fail, 1 + kb);
  if (bx == 0 && !panel_wave) {
    // The factored diagonal block goes to a SIDE buffer, never back into S: every workgroup of this column loads A_kk from S when it starts,
    // and a workgroup that is dispatched late — a second context's kernels filling the chip (Backend::Optimize beside Relocator,
    // relocator.cpp:188) — would find L_kk there instead of A_kk and factor garbage (measured: 197 of 400 solves took a step as invalid
    // under chip-filling traffic; the per-launch "everyone has loaded long before workgroup 0 stores" held only on an otherwise idle GPU).
    // What reads L_kk afterwards — the right-hand-side row inside the last block, by the back substitution — reads it from there.
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) if (16 * q + tt > r) a[tt] = 0.0;
    double2* g2 = reinterpret_cast<double2*>(A.Ldiag + (size_t)kb * kNB * kNB + (size_t)r * kNB + 16 * q);
#pragma unroll
    for (int c = 0; c < 8; ++c) g2[c] = make_double2(a[2 * c], a[2 * c + 1]);
  }
  if (bx > 0 && panel_wave) {
    double2* g2 = reinterpret_cast<double2*>(brow);
#pragma unroll
    for (int c = 0; c < 8; ++c) g2[c] = make_double2(a[2 * c], a[2 * c + 1]);
  }
  if (dbg) dbg[5] = wall_clock64();
}
// The product form of the sparse back substitution (Chain::back_product).  x_b = L_bb^-T (y_b - W_b^T x_N) is linear in the dense-corner
// solution: composed over the levels, x_sparse = G [x_dense ; -1] with nine rows of G per eliminated (v, ba, bg) node and one column per
// dense-corner unknown plus the augmented column (leading dimension ldG, a multiple of 16; the padding columns are zero).  With node b's row
// list N, its stored W (component-major) and Linv = L_bb^-1:
//     G_b[q][:] = sum_{t >= q} Linv_b[t][q] * sum_{r in N} (-W_b[r][t]) X_r[:]
// where X_r is the unit row of column r for a dense-corner / augmented row and the G row of the owning node for a sparse row (always of a
// higher level; the node of sparse column c is c / 9, so that row is G row c).  Nothing here depends on the step, and W / Linv are final
// before the first block step of the dense factorisation: the rows are formed by workgroups riding BEHIND the block-step launches (which
// leave most of the chip idle), level n_levels - 1 - kb in launch kb, so the launch boundaries order the levels.  One workgroup per node, one
// thread per column, no LDS and no barrier: the row list is ascending, i.e. the sparse neighbours come first, and `map` (host-built with the
// plan) tells a column which of the node's own rows it is.
__device__ __forceinline__ void back_product_ride(const int vb, const GRide& R) {
  if (vb >= R.n) return;
  if (R.done && *R.done) return;
  const int b = R.first + vb;
  const SpNode nd = R.nodes[b];
  const int* rows = R.rows + nd.row_off;
  const double* W = R.W + nd.row_off;                  // component t of the node's row r: W[t * wstride + r]
  const double* Li = R.Linv + (size_t)b * 81;
  double* G = R.G;
  int ms = 0;
  while (ms < nd.m && rows[ms] < R.off) ++ms;          // the sparse neighbours' rows
  for (int j = threadIdx.x; j < R.ldG; j += kCT) {
    double T[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) T[t] = 0.0;
    for (int r = 0; r < ms; ++r) {
      const double x = G[(size_t)rows[r] * R.ldG + j];
#pragma unroll
      for (int t = 0; t < 9; ++t) T[t] -= W[(size_t)t * R.wstride + r] * x;
    }
    const int g = R.map[(size_t)b * R.ldG + j];        // (global item index: already includes row_off)
    if (g >= 0) {
#pragma unroll
      for (int t = 0; t < 9; ++t) T[t] -= R.W[(size_t)t * R.wstride + g];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      double v = 0.0;
#pragma unroll
      for (int t = q; t < 9; ++t) v += Li[t * 9 + q] * T[t];
      G[(size_t)(9 * b + q) * R.ldG + j] = v;
    }
  }
}
// (the column and trailing-update workgroups keep the lowest indices — they are the critical path and are dispatched first; the riders sit behind them)
// (behind the G riders: the nb - kb riders of the back substitution's block products, back_block_ride)
__device__ __forceinline__ void chol_step_riders(const int vb, const CholArgs& a, const int kb, const GRide& g, const TRide& tr) {
  if (vb < g.n) back_product_ride(vb, g);
  else back_block_ride(vb - g.n, a, kb, tr);
}
__global__ __launch_bounds__(kCT) void k_chol_step(CholArgs a, int kb, GRide g, TRide tr) {
  const int own = chol_step_grid(a.nb, kb);
  if ((int)blockIdx.x >= own) { chol_step_riders((int)blockIdx.x - own, a, kb, g, tr); return; }
  chol_step_body<true>(blockIdx.x, a, kb);
}
__global__ __launch_bounds__(kCT) void k_chol_step_b(const CholArgs* __restrict__ t, int kb) { chol_step_body<true>(blockIdx.x, t[blockIdx.y], kb); }
__global__ __launch_bounds__(kCT) void k_chol_step_bt(const CholArgs* __restrict__ t, int kb) { chol_step_body<true>(blockIdx.y, t[blockIdx.x], kb); }
// LVF_CHOL_SUBBLOCK=0: the pair-pivot sweep, as second instantiations (no branch inside the chain)
__global__ __launch_bounds__(kCT) void k_chol_step_pp(CholArgs a, int kb, GRide g, TRide tr) {
  const int own = chol_step_grid(a.nb, kb);
  if ((int)blockIdx.x >= own) { chol_step_riders((int)blockIdx.x - own, a, kb, g, tr); return; }
  chol_step_body<false>(blockIdx.x, a, kb);
}
__global__ __launch_bounds__(kCT) void k_chol_step_pp_b(const CholArgs* __restrict__ t, int kb) { chol_step_body<false>(blockIdx.x, t[blockIdx.y], kb); }
__global__ __launch_bounds__(kCT) void k_chol_step_pp_bt(const CholArgs* __restrict__ t, int kb) { chol_step_body<false>(blockIdx.y, t[blockIdx.x], kb); }

// ------------------------------------------------------------------------------------------------ elimination order
// The (v, ba, bg) blocks only meet each other and the poses through ImuError factors, i.e. along the IMU chain: block k touches
// blocks k-1, k+1 and poses k-1, k, k+1.  Factorising them FIRST, in nested-dissection order (level 0 = every other block of the
// chain, level 1 = every other one of what is left, ...; any coupling graph works, the levels are greedy independent sets with
// fill-in tracked on the host), costs 9 sequential pivots per LEVEL instead of 9 per block, and leaves only the pose corner
// (6 n_kf) for the dense blocked factorisation: at 50 keyframes 6 x 9 + 300 sequential pivots instead of 750.
// k_sp_eliminate, one launch per level, `tiles` workgroups per block b with neighbour rows N (|N| = m):
//   L_bb = chol(S_bb) (wave 0, lane = row, pivots broadcast by v_readlane);  W = S_Nb L_bb^-T (thread per row);
//   S_NN -= W W^T (pairs split over the tiles; atomics, because blocks of one level share neighbours).
// W and L_bb go to side buffers (the eliminated columns of S are never read again), so the tiles of a block never race.
__device__ __forceinline__ void sp_eliminate_body(const int vb, const SpNode* __restrict__ nodes, int first, int tiles, const int* __restrict__ rows,
                                                  double* __restrict__ S, int ld, double* __restrict__ W, int wstride,
                                                  double* __restrict__ Lout, int* __restrict__ fail, const int* done = nullptr,
                                                  const SpSrc src = SpSrc{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1, 200000u, 0, 0, nullptr, 0}) {
  extern __shared__ double sp_sm[];        // Ws[m][9] | L[81] | linv[9] | rws[m] (int) | rnat[m] (int, early form)
  const int dv = done_flag_issue(done);
  const int ni = first + vb / tiles, tile = vb % tiles, tid = threadIdx.x;
  unsigned long long* stamp = (src.dbg && tile == 0 && tid == 0) ? src.dbg + (size_t)ni * 8 : nullptr;
  if (stamp) stamp[0] = wall_clock64();
  const SpNode nd = nodes[ni];
  const double radius = src.B ? *src.radius : 1.0;
  if (dv) return;
  const bool chained = src.wait_counter != nullptr;
  // an entry of S the level below may have added into during THIS launch: an agent-scope atomic load behind the acquire fence that
  // follows the wait (the adds it must see were RETURNING atomics performed before the producer's release arrival; the wrong results
  // round 3 chased — 5 of 12 runs of the 8-keyframe / 20 000-landmark case — came from RETURNLESS adds on the producer side, not from
  // this load).  rmw_read (LVF_CHAIN_RMW_READ=1, diagnostic): a returning atomic adding zero instead — same results, 7 us slower.
  auto ld_s = [&](double* ptr) -> double {
    if (!chained) return *ptr;
    return src.rmw_read ? __hip_atomic_fetch_add(ptr, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int m = nd.m, col = nd.col;
  double* Ws = sp_sm;
  double* L = sp_sm + 9 * m;
  double* linv = L + 81;
  int* rws = reinterpret_cast<int*>(linv + 9);
  int* rnat = rws + m;
  const int nb0 = src.dp + 9 * nd.id;      // early form: the block's first unknown in the natural order (poses | 9 per keyframe)
  // The level is a chain of dependent round trips (node -> row list -> rows -> factor -> W -> updates), so everything is requested as early
  // as its address is known, and the rows are dealt to waves 1..3 first: their requests are in flight while wave 0 factors the block
  // (wave 0 only takes rows when there are more than 192).  Each thread keeps its FIRST row in registers; further rows (m > 256) follow
  // the classic loop behind the barrier.
  const int r0 = (tid + 192) & 255;
  // ---- phase A: what does not depend on the level below
  const bool has0 = r0 < m;
  int rw0 = 0, rn0 = -1;
  if (has0) { rw0 = rows[nd.row_off + r0]; if (src.B) rn0 = src.rows_nat[nd.row_off + r0]; }
  for (int r = tid; r < m; r += 256) { rws[r] = rows[nd.row_off + r]; if (src.B) rnat[r] = src.rows_nat[nd.row_off + r]; }
  double bd[9], sv0[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { bd[c] = 0.0; sv0[c] = 0.0; }
  if (src.B) {
    if (tid < 9) {                         // what k_prepare would have stored in the diagonal block: B + clamp(diag B) / radius
      const double inv_radius = 1.0 / radius;
      const int jf = *src.jac.frozen;
      const double h0d = src.jac.h0[nb0 + tid];
      // (the row's nine entries are requested together, column clamped to the diagonal: as `c <= tid ? B[..] : 0` each load sat behind its own
      // branch and was waited for there — nine dependent round trips at the head of every sparse level)
      double braw[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) braw[c] = src.B[(size_t)(nb0 + tid) * src.ldB + nb0 + min(c, tid)];
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        double b = c <= tid ? braw[c] : 0.0;
        if (c == tid) b += lm_damping_own(b, src.jac, nb0 + tid, jf, h0d) * inv_radius;      // (every tile workgroup of the node stores the same H0)
        bd[c] = b;
      }
    }
    if (has0) {                            // the row's entries of B (lower triangle, natural order) / of -gc (the right-hand-side row)
      if (rn0 == -2) {
#pragma unroll
        for (int c = 0; c < 9; ++c) sv0[c] = -src.gc[nb0 + c];
      } else if (rn0 >= 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { const int oj = nb0 + c; sv0[c] = src.B[(size_t)max(rn0, oj) * src.ldB + min(rn0, oj)]; }
      }
    }
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[1] = wall_clock64(); }      // (timing only: phase A's requests have landed)
  if (chained) {
    // bounded: if the level below does not arrive in time (workgroups of another stream or process took the CUs its producers needed, or
    // a dispatch order this code does not expect) the hand-over flag is raised instead of hanging; the step is then NOT judged: see SpSrc
    if (tid == 0) {
      const unsigned long long t0 = wall_clock64();
      while (__hip_atomic_fetch_add((int*)src.wait_counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < src.wait_target) {
        __builtin_amdgcn_s_sleep(4);
        if (wall_clock64() - t0 > (unsigned long long)src.timeout_ticks) { atomicMax(fail, kFailHandover + nd.id); break; }
      }
    }
    asm volatile("s_barrier" ::: "memory");           // (not __syncthreads(): the requests above stay in flight across it)
    // every wave orders its reads of S behind the producers' release arrivals (agent scope: the L1 copy of a line an earlier level's
    // plain loads brought in is dropped; phase A's requests have long landed while the wave sat at the barrier)
    if (src.fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  if (stamp) stamp[2] = wall_clock64();
  // ---- phase B: what the level below added into S
  double a[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) a[c] = 0.0;
  if (tid < 9) {
    double sraw[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) sraw[c] = 0.0;
    if (!src.s_zero) {                      // (all nine requested together, column clamped to the diagonal: see phase A)
#pragma unroll
      for (int c = 0; c < 9; ++c) sraw[c] = ld_s(&S[(size_t)(col + tid) * ld + col + min(c, tid)]);
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) a[c] = (c <= tid ? sraw[c] : 0.0) + bd[c];
  }
  if (has0 && !src.s_zero) {
    double* srow = S + (size_t)rw0 * ld + col;
#pragma unroll
    for (int c = 0; c < 9; ++c) sv0[c] += ld_s(srow + c);
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[3] = wall_clock64(); }      // (timing only: the S entries are here)
  if (tid < 64) {
    const int lane = tid;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const double djj = lane_bcast(a[j], j);
      bad |= !(djj > 0.0);
      // hardware estimate + one second-order correction (as in the dense corner); lane j holds A_jj itself, so no select
      const double y0 = __builtin_amdgcn_rsq(djj);
      const double e = fma(-djj * y0, y0, 1.0);
      const double inv_l = fma(y0 * e, fma(e, 0.375, 0.5), y0);
      a[j] *= inv_l;
      if (lane == j) linv[j] = inv_l;
      // A_rt -= L_rj L_tj (meaningful for t <= r): L_tj sits in lane t of the same 16-lane row — the DPP row broadcast hands it to the
      // multiply-add directly (one instruction per column instead of two v_readlane + one FMA)
      {
        const double m = -a[j];
        asm volatile("s_nop 4");
        if (j < 1) fmac_row_bcast<1>(a[1], a[j], m);
        if (j < 2) fmac_row_bcast<2>(a[2], a[j], m);
        if (j < 3) fmac_row_bcast<3>(a[3], a[j], m);
        if (j < 4) fmac_row_bcast<4>(a[4], a[j], m);
        if (j < 5) fmac_row_bcast<5>(a[5], a[j], m);
        if (j < 6) fmac_row_bcast<6>(a[6], a[j], m);
        if (j < 7) fmac_row_bcast<7>(a[7], a[j], m);
        if (j < 8) fmac_row_bcast<8>(a[8], a[j], m);
      }
    }
    if (lane < 9) {
#pragma unroll
      for (int c = 0; c < 9; ++c) L[lane * 9 + c] = (c <= lane) ? a[c] : 0.0;
    }
    if (bad && lane == 0) atomicMax(fail, kFailSparse + nd.id);
  }
  if (stamp) stamp[4] = wall_clock64();
  __syncthreads();
  auto finish_row = [&](const int r, const double sv[9]) {     // W_r = S_rb L_bb^-T
    double w[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      double v = sv[c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= w[k] * L[c * 9 + k];
      w[c] = v * linv[c];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) Ws[r * 9 + c] = w[c];
    if (tile == 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c) W[(size_t)c * wstride + nd.row_off + r] = w[c];     // component-major: coalesced here and in the back substitution
    }
  };
  if (has0) finish_row(r0, sv0);
  for (int r = r0 + 256; r < m; r += 256) {
    double* srow = S + (size_t)rws[r] * ld + col;
    double sv[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) sv[c] = src.s_zero ? 0.0 : ld_s(srow + c);
    if (src.B) {
      const int oi = rnat[r];
      if (oi == -2) {
#pragma unroll
        for (int c = 0; c < 9; ++c) sv[c] -= src.gc[nb0 + c];
      } else if (oi >= 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) { const int oj = nb0 + c; sv[c] += src.B[(size_t)max(oi, oj) * src.ldB + min(oi, oj)]; }
      }
    }
    finish_row(r, sv);
  }
  if (tile == 0 && tid < 9) {              // column tid of L_bb^-1 (forward substitution against e_tid), for the back substitution
    double xcol[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      double v = (r == tid) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < r; ++k) v -= L[r * 9 + k] * xcol[k];
      xcol[r] = v * linv[r];
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) Lout[(size_t)ni * 81 + r * 9 + tid] = xcol[r];
  }
  __syncthreads();
  // S_NN -= W W^T.  The pairs whose COLUMN belongs to a sparse block (rows [0, ns): later (v, ba, bg) blocks come first in the ascending
  // row list) are what the next level reads; they go first, and a chained level signals its successor as soon as THEY are acknowledged —
  // the bulk (the dense corner's entries, four fifths at the top level) and its acknowledgement stay off the chain.
  int ns = 0;
  if (src.done_counter && src.strip_end > 0) {                  // (binary search: rws is ascending)
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (rws[mid] < src.strip_end) lo = mid + 1; else hi = mid; }
    ns = lo;
  }
  auto pair_value = [&](const int r, const int c2) {
    const double* wr = Ws + r * 9;
    const double* wc = Ws + c2 * 9;
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) v += wr[c] * wc[c];
    return v;
  };
  auto pair_update = [&](const int r, const int c2) {
    const double v = pair_value(r, c2);
    if (v != 0.0) atomicAdd(&S[(size_t)rws[r] * ld + rws[c2]], -v);
  };
  if (ns > 0) {
    // RETURNING atomics: the value only comes back once the add has been performed where the next level will read it, so the barrier
    // below (which waits for the returns) really orders them ahead of the arrival.  With returnless adds the acknowledgement that
    // releases vmcnt came first often enough: 5 of 12 runs of the 8-keyframe / 20 000-landmark case had the next level read entries short of an update.
    double sink = 0.0;
    for (int q = tile * 256 + tid; q < ns * m; q += tiles * 256) {      // the m x ns rectangle, its r < c2 corner skipped
      const int r = q / ns, c2 = q - r * ns;
      if (r >= c2) {
        const double v = pair_value(r, c2);
        if (v != 0.0) sink += __hip_atomic_fetch_add(&S[(size_t)rws[r] * ld + rws[c2]], -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (sink == -1.2345678901234567e301) atomicMax(fail, 50000);     // (never: keeps the returns alive)
  }
  if (stamp) stamp[5] = wall_clock64();
  if (src.done_counter) {
    __syncthreads();                       // every wave has its returns (the barrier drains vmcnt)
    if (tid == 0) {
      if (src.fenced) __hip_atomic_fetch_add((int*)src.done_counter, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_add((int*)src.done_counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (stamp) stamp[6] = wall_clock64();
  const int m2 = m - ns, P = m2 * (m2 + 1) / 2;                          // the triangle over rows / columns [ns, m)
  for (int p = tile * 256 + tid; p < P; p += tiles * 256) {
    int r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= p) ++r;
    while (r * (r + 1) / 2 > p) --r;
    const int c2 = p - r * (r + 1) / 2;
    pair_update(r + ns, c2 + ns);
  }
  if (stamp) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp[7] = wall_clock64(); }
}
// Work list of the band Schur complement: one item per (slice, tile group) that has tiles to form.  The 2-D grid slices x groups is sized
// for the widest possible band, but most slices (short tracks) need one group: three quarters of its workgroups had nothing to do and
// their dispatch — each needs its LDS slice — was most of the launch's span.  Built once per problem_configure (the bands are fixed).
__global__ __launch_bounds__(64) void k_band_work(int rows, int dp, const int* __restrict__ n_active_p, const int* __restrict__ order,
                                                  const int* __restrict__ kmin, const int* __restrict__ kmax, int4* __restrict__ work, int* __restrict__ n_work) {
  const int n_active = *n_active_p, lane = threadIdx.x;
  const int k_begin = blockIdx.x * rows, k_end = min(n_active, k_begin + rows);
  if (k_begin >= k_end) return;
  int lo = 0x7fffffff, hi = -1;
  for (int r = k_begin + lane; r < k_end; r += 64) { const int l = order[r]; lo = min(lo, kmin[l]); hi = max(hi, kmax[l]); }
  for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
  if (lane == 0) {
    const int t0 = (6 * lo) >> 4, t1 = (6 * hi + 5) >> 4, tl = dp >> 4, nbt = t1 - t0 + 1;
    const int ntiles = nbt * (nbt + 1) / 2 + (tl > t1 ? nbt : 0);
    const int groups = (ntiles + kBandTilesPerGroup - 1) / kBandTilesPerGroup;
    const int base = atomicAdd(n_work, groups);
    for (int g = 0; g < groups; ++g) work[base + g] = make_int4((int)blockIdx.x, g, lo | (hi << 16), k_end);
  }
}

template <bool SEL>
__device__ __forceinline__ void sp_ride(const int vb, const SpArgs& a) {
  if (vb >= a.nblocks) return;
  if (!SEL) { sp_eliminate_body(vb, a.nodes, a.first, a.tiles, a.rows, a.S, a.ld, a.W, a.wstride, a.Lout, a.fail, a.done, a.src); return; }
  SpSrc src = a.src;
  if (src.sel && *src.sel) { src.B = src.B1; src.gc = src.gc1; }      // (fused chain: the active accumulator set)
  sp_eliminate_body(vb, a.nodes, a.first, a.tiles, a.rows, a.S, a.ld, a.W, a.wstride, a.Lout, a.fail, a.done, src);
}
__global__ __launch_bounds__(256) void k_sp_eliminate(SpArgs a) { sp_ride<true>(blockIdx.x, a); }
__global__ __launch_bounds__(256) void k_sp_eliminate_b(const SpArgs* __restrict__ t) { sp_ride<false>(blockIdx.x, t[blockIdx.y]); }
// The band-limited Schur complement and the FIRST sparse level in one launch: both only ADD (atomically) into entries of S the other
// does not read — the Schur complement touches the pose corner and the pose part of the rhs row, level 0 reads its own (v,ba,bg)
// columns — so they are independent; later levels depend on level 0 and stay launches of their own.
template <bool SEL>
__device__ __forceinline__ void schur_sp0_body(const int b, const SchurSp0Args& A) {
  if (b >= A.nblocks) return;
  if (A.work) {
    const int n_a = A.sp.nblocks, n_b = A.sp_b.nblocks, n_c = A.sp_c.nblocks, n_sp = n_a + n_b + n_c;
    if (b < n_a) sp_ride<SEL>(b, A.sp);
    else if (b < n_a + n_b) sp_ride<SEL>(b - n_a, A.sp_b);
    else if (b < n_sp) sp_ride<SEL>(b - n_a - n_b, A.sp_c);
    else {
      const int dv = done_flag_issue(A.done);
      const int set = acc_set_t<SEL>(A.acc);
      const int4* item = A.work + (b - n_sp);
      const int4 it = *item;
      if (dv) return;
      schur_band_body(it.x, it.y, A.dp, A.ldE, set ? (const double*)A.acc.E : (const double*)A.E, A.Cd, A.order, A.n_active, A.kmin, A.kmax, A.d_local, A.ldS, A.S_pose, A.dbg ? A.dbg + (size_t)(b - n_sp) * 8 : nullptr, A.rows, item);
    }
    return;
  }
  if (A.done && *A.done) return;
  const int ns = A.n_slices * A.n_groups;
  if (b < ns) schur_band_body(b % A.n_slices, b / A.n_slices, A.dp, A.ldE, acc_set_t<SEL>(A.acc) ? (const double*)A.acc.E : (const double*)A.E, A.Cd, A.order, A.n_active, A.kmin, A.kmax, A.d_local, A.ldS, A.S_pose, A.dbg ? A.dbg + (size_t)b * 8 : nullptr, A.rows);
  else sp_ride<SEL>(b - ns, A.sp);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0(SchurSp0Args a) { schur_sp0_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0_b(const SchurSp0Args* __restrict__ t) { schur_sp0_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_schur_sp0_bt(const SchurSp0Args* __restrict__ t) { schur_sp0_body<false>(blockIdx.y, t[blockIdx.x]); }

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait for the global prefetches
// that are meant to stay in flight across it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// back substitution x = L^-T y with y = augmented row L[d][0..d); ONE workgroup of 512 threads.  S points at the DENSE corner
// (row/column `off` of the full matrix), d = its unknowns, Dinv holds L_kk^-T of its 64x64 diagonal blocks.
// Nothing this kernel LOADS from global memory depends on x, so the chain is kept free of global latency:
//   * at entry every thread requests its share of the sparse levels' (row, owner, W[9]) items (registers) and the stored
//     L_bb^-1 (LDS): they arrive while the dense corner is being solved;
//   * dense corner, bottom-up:  rhs = y_blk - sum_{rows r below} L[r][blk]^T x_r  (thread (column c, part) takes rows part,
//     part + 8, ...), x_blk = Dinv_blk rhs (64x64 mat-vec split 8 ways); the gather operands and inverse block of the NEXT block
//     are prefetched while the current one is reduced;
//   * sparse levels in reverse, x_b = L_bb^-T (y_b - W_b^T x_N): the pre-loaded items are multiplied with x from LDS, summed per
//     block (wave-wide when a wave holds one block's rows, LDS atomics otherwise), one thread per (block, component) applies
//     L_bb^-1.  The solution leaves in the natural unknown order through `perm`.
// (S and Dinv are deliberately NOT __restrict__/invariant: LLVM would sink the prefetch loads past the barriers to their uses.)
template <typename T>
__device__ __forceinline__ T ld_off32(const T* base, unsigned byte_off) {     // wave-uniform base + 32-bit lane offset (saddr + voffset form)
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
// LEVELS = false (the product form, k_backsolve_tail with Chain::back_product): the dense corner only.  The WHOLE dense-corner solution is
// published — the plan may leave (v, ba, bg) blocks in the corner's padding, and the sibling workgroups' product with G reads them — and the
// sparse items, the stored L_bb^-1 and the levels are neither requested nor run.
template <bool LEVELS = true>
__device__ __forceinline__ void chol_backsolve_body(const BackArgs& A) {
  const int dv = done_flag_issue(A.done);
  const double* S = A.Sd; const int ld = A.ld, d = A.d; const double* Dinv = A.Dinv; double* xout = A.xout; const SpBack& sp = A.sp;
  extern __shared__ double sm[];          // xs[off] | x[nblk*64] | partial[kBParts][64] | rhs[64] | accs[9 max_count] | linv[81 n_nodes]
  const int tid = threadIdx.x, c = tid & 63, part = tid >> 6;
  const double* Tb = A.T;
  const bool blocks = Tb != nullptr;       // (where it is set nblk - 1 <= kBackTJ / kBackTJLevels and d is no multiple of 64, so the factor has nblk blocks: build_chain)
  const int nblk = (d + kNB - 1) / kNB, n = nblk * kNB;
  double* x = sm + sp.off;
  double* partial = x + n;
  double* rhs = partial + kBParts * kNB;
  double* accs = rhs + kNB;
  double* linv = accs + 9 * sp.max_count;
  double* part1 = linv + (sp.linv_in_lds ? 81 * sp.n_nodes : 0);     // [kBT] stage-1 partial sums
  double* prod = part1 + kBT;                                        // [prod_items][9]
  int* snode = reinterpret_cast<int*>(prod + 9 * (size_t)sp.prod_items);   // [n_nodes][2] = (row_off, m)
  int stamp = 0;
  auto mark = [&]() { if (sp.dbg && tid == 0) sp.dbg[stamp++] = wall_clock64(); };
  mark();
  // ---- dense corner
  const int rend = min(n, d);
  constexpr int kTJ = LEVELS ? kBackTJLevels : kBackTJ, kGl = kBackPre > 4 * kTJ * (kTJ + 1) ? kBackPre : 4 * kTJ * (kTJ + 1);
  double gl[kGl], xi[kBackInv], yv;        // gl: the gather operands of one block, or every block product of the block form
  // The kernel is ISSUE-bound (one workgroup, two waves per SIMD): every request below is a wave-uniform base (SALU) plus a 32-bit
  // per-lane byte offset, i.e. one VMEM instruction and no VALU address arithmetic, and the row tests are scalar branches -- with
  // 64-bit per-lane addresses and per-lane predicates issuing one block's 41 requests took 1.2-1.8 us of its 2.3-3.4.
  const int part_u = __builtin_amdgcn_readfirstlane(part);
  const unsigned c_off = 8u * (unsigned)c;
  // (no row tests either: k_prepare writes every entry of the padded corner, rows d.. meet x = 0, so the 8-row groups of the
  // 64 (nblk-1-kb) rows below a block are requested and multiplied whole)
  auto prefetch = [&](int kb) {
    const int r0 = kb * kNB, below = nblk - 1 - kb;
    const double* row = S + (size_t)(r0 + kNB + part_u) * ld + r0;
#pragma unroll
    for (int g = 0; g < kBackPre / 8; ++g)
      if (g < below) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gl[8 * g + j] = ld_off32(row + (size_t)(kBParts * (8 * g + j)) * ld, c_off);
      }
    const double* dv = Dinv + (size_t)kb * kNB * kNB + kBackInv * part_u;
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) xi[t] = ld_off32(dv + t, (unsigned)kNB * c_off);
    // the forward-substituted right-hand side: row d of the factor — a panel tile of S for every block but the last, whose part sits in
    // the factored DIAGONAL block (kept in the side buffer: chol_step_body)
    const double* yrow = (d / kNB == kb) ? A.Ldiag + (size_t)kb * kNB * kNB + (size_t)(d - r0) * kNB : S + (size_t)d * ld + r0;
    yv = (r0 + c < d) ? ld_off32(yrow, c_off) : 0.0;
  };
  prefetch(nblk - 1);
  // the stored L_bb^-1 and the node table go to LDS: ALL of a thread's requests are issued before the first LDS write (written as a
  // copy loop the compiler waits for every load in turn — eight dependent round trips at 50 keyframes, 4 of this kernel's 30 us)
  constexpr int kLinvPre = 8;
  if constexpr (LEVELS) {
  double lpre[kLinvPre];
  const int n_linv = sp.linv_in_lds ? 81 * sp.n_nodes : 0;
#pragma unroll
  for (int u = 0; u < kLinvPre; ++u) { const int i = tid + kBT * u; lpre[u] = i < n_linv ? ld_off32((const double*)sp.Linv, 8u * (unsigned)i) : 0.0; }
  SpNode ndpre = SpNode{0, 0, 0, 0};
  if (tid < sp.n_nodes) ndpre = sp.nodes[tid];
#pragma unroll
  for (int u = 0; u < kLinvPre; ++u) { const int i = tid + kBT * u; if (i < n_linv) linv[i] = lpre[u]; }
  for (int i = tid + kBT * kLinvPre; i < n_linv; i += kBT) linv[i] = sp.Linv[i];
  if (tid < sp.n_nodes) { snode[2 * tid] = ndpre.row_off; snode[2 * tid + 1] = ndpre.m; }
  for (int i = tid + kBT; i < sp.n_nodes; i += kBT) { const SpNode nd = sp.nodes[i]; snode[2 * i] = nd.row_off; snode[2 * i + 1] = nd.m; }
  asm volatile("" ::: "memory");
  }
  // block form: every link's share of T_kj, in the order the links run (k = j - 1, the one the next link waits for, first): all of it is in
  // flight while the first block is solved, and no link requests anything
  auto request_T = [&]() {
#pragma unroll
    for (int j = kTJ; j >= 1; --j)
      if (j < nblk) {
#pragma unroll
        for (int k = j - 1; k >= 0; --k) {
          const double* tb = Tb + ((size_t)k * nblk + j) * (kNB * kNB) + (size_t)(kBackInv * part_u) * kNB;
#pragma unroll
          for (int t = 0; t < kBackInv; ++t) gl[8 * (j * (j - 1) / 2 + k) + t] = ld_off32(tb + t * kNB, c_off);
        }
      }
  };
  if (blocks) request_T();
  // ---- requests for the sparse tail, AFTER the first dense prefetch: loads return in order, so the dense corner does not wait
  // for them and they land while it is being solved
  constexpr int kTailRegs = LEVELS ? kTailPre : 1;      // (the product form holds none of them)
  int tR[kTailRegs], tK[kTailRegs];
  double tW[kTailRegs][9];
#pragma unroll
  for (int u = 0; u < kTailRegs; ++u) {
    const int g = tid + kBT * u;
    const bool ok = LEVELS && g < sp.total_items;
    tR[u] = -1; tK[u] = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) tW[u][q] = 0.0;
    if (ok) {
      tR[u] = ld_off32((const int*)sp.rows, 4u * (unsigned)g);
      tK[u] = ld_off32((const int*)sp.owner, 4u * (unsigned)g);
#pragma unroll
      for (int q = 0; q < 9; ++q) tW[u][q] = ld_off32((const double*)sp.W, 8u * ((unsigned)q * (unsigned)sp.total_items + (unsigned)g));
    }
  }
  if (dv) return;                          // (every request above is in flight behind the flag's)
  for (int i = tid; i < sp.off + n; i += kBT) sm[i] = 0.0;
  lds_barrier();
  mark();
  const int kb_last = blocks ? nblk - 1 : 0;      // block form: the first solved block (its right-hand side sits in Ldiag) only
  for (int kb = nblk - 1; kb >= kb_last; --kb) {
    const int r0 = kb * kNB;
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < kBackPre / 8; ++g)
      if (g < nblk - 1 - kb) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += gl[8 * g + j] * x[r0 + kNB + part_u + kBParts * (8 * g + j)];
      }
    for (int r = r0 + kNB + part + kBParts * kBackPre; r < rend; r += kBParts) s += S[(size_t)r * ld + r0 + c] * x[r];
    partial[part * kNB + c] = s;
    double xc[kBackInv];
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) xc[t] = xi[t];
    const double yc = yv;
    if (kb > kb_last) prefetch(kb - 1);    // in flight during the reductions below
    lds_barrier();
    if (part == 0) {
      double a = yc;
#pragma unroll
      for (int pp = 0; pp < kBParts; ++pp) a -= partial[pp * kNB + c];
      rhs[c] = a;
    }
    lds_barrier();
    double t2 = 0.0;
#pragma unroll
    for (int t = 0; t < kBackInv; ++t) t2 += xc[t] * rhs[kBackInv * part + t];
    partial[part * kNB + c] = t2;
    lds_barrier();
    if (part == 0) {
      double a = 0.0;
#pragma unroll
      for (int pp = 0; pp < kBParts; ++pp) a += partial[pp * kNB + c];
      // (block form: the multiplier carries -1 at the augmented row d, which meets column d - r0 of T_k,last = -Dinv_k y_k)
      x[r0 + c] = (r0 + c < d) ? a : ((blocks && r0 + c == d) ? -1.0 : 0.0);
    }
    lds_barrier();
    mark();
  }
  if (blocks) {
    // x_k = sum_{j > k} T_kj x_j: once x_j is in LDS every thread adds its eight terms for EVERY k < j to running sums; only block j - 1 is
    // reduced across the parts now — one write, two barriers and eight multiply-adds on the critical link
    double acc[kTJ];
#pragma unroll
    for (int k = 0; k < kTJ; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = kTJ; j >= 1; --j)
      if (j < nblk) {
        double xv[kBackInv];
#pragma unroll
        for (int t = 0; t < kBackInv; ++t) xv[t] = x[j * kNB + kBackInv * part_u + t];
#pragma unroll
        for (int k = j - 1; k >= 0; --k) {
#pragma unroll
          for (int t = 0; t < kBackInv; ++t) acc[k] += gl[8 * (j * (j - 1) / 2 + k) + t] * xv[t];
        }
        partial[part * kNB + c] = acc[j - 1];
        lds_barrier();
        if (part == 0) {
          double a = 0.0;
#pragma unroll
          for (int pp = 0; pp < kBParts; ++pp) a += partial[pp * kNB + c];
          x[(j - 1) * kNB + c] = a;
        }
        lds_barrier();
        mark();
      }
  }
  if (A.pose_ready) {
    // the pose increments are final (every pose row lives in the dense corner): out they go, so that the landmark back-substitution — which
    // reads nothing else of the step — runs in the sibling workgroups of this launch WHILE the sparse levels below are solved here
    // The increments and the flag travel as agent-scope ATOMICS (written through to the coherence point, read there by the consumers): an
    // agent-scope release / acquire FENCE pair instead writes this XCD's dirty L2 lines back and makes every consumer invalidate its L2 —
    // measured: 6 us on this workgroup's path and the landmark pass twice as long (320 workgroups flushing the E rows out of each other's
    // L2).  pose_fenced (LVF_CHAIN_FENCE=2) adds the fences back for A/B.
    {
      int last = -1;
      if constexpr (LEVELS) {
        for (int i = tid; i < A.n_pose; i += kBT) { __hip_atomic_store(xout + i, sm[sp.perm[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = i; }
      } else {
        // every unknown that lives in the dense corner: the poses and the (v, ba, bg) blocks the plan left there
        for (int i = tid; i < sp.d_total; i += kBT) {
          const int pi = sp.perm[i];
          if (pi >= sp.off) { __hip_atomic_store(xout + i, sm[pi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); last = i; }
        }
      }
      // (a store is acknowledged to the wave before it is necessarily performed; a load of the same address is ordered behind it and RETURNS:
      // once it is back — the s_waitcnt below — the store is where the consumers read.  Round 3 met the same with returnless atomic adds.)
      if (last >= 0) { const double chk = __hip_atomic_load(xout + last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); asm volatile("" ::"v"(chk)); }
    }
    if (A.pose_fenced) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");          // every wave's stores have been performed before the flag goes up
    if (tid == 0) __hip_atomic_store((int*)A.pose_ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (!LEVELS) {
    mark();
    if (sp.dbg && tid == 0) sp.dbg[63] = (unsigned long long)stamp;
    return;
  }
  // ---- sparse levels, last eliminated first
  for (int lv = sp.lv.n - 1; lv >= 0; --lv) {
    const int first = sp.lv.first[lv], count = sp.lv.count[lv], item0 = sp.item0[lv], item1 = item0 + sp.items[lv];
    const bool staged = sp.items[lv] <= sp.prod_items;
    if (staged) {
      // (1) products -W x_r of every (block, row) item into LDS (stride 9 doubles: conflict-free)
#pragma unroll
      for (int u = 0; u < kTailRegs; ++u) {
        const int g = tid + kBT * u;
        if (g >= item0 && g < item1) {
          const double xr = (tR[u] == sp.aug) ? -1.0 : sm[tR[u]];          // the rhs row carries y_b itself
#pragma unroll
          for (int q = 0; q < 9; ++q) prod[9 * (g - item0) + q] = -tW[u][q] * xr;
        }
      }
      for (int g = max(item0, kBT * kTailPre) + tid; g < item1; g += kBT) {   // items beyond the register window (large windows only)
        const int R = sp.rows[g];
        const double xr = (R == sp.aug) ? -1.0 : sm[R];
#pragma unroll
        for (int q = 0; q < 9; ++q) prod[9 * (g - item0) + q] = -sp.W[(size_t)q * sp.total_items + g] * xr;
      }
      lds_barrier();
      // (2) thread (block k, component q, part j of J) sums its share of the block's rows; (3) thread (k, q) adds the J parts
      int J = 1;
      while (2 * J * 9 * count <= kBT && J < 32) J *= 2;
      if (tid < 9 * count * J) {
        const int j = tid % J, kq = tid / J, q = kq % 9, k = kq / 9;
        const int base = snode[2 * (first + k)] - item0, m = snode[2 * (first + k) + 1];
        double a = 0.0;
        for (int r = j; r < m; r += J) a += prod[9 * (base + r) + q];
        part1[tid] = a;
      }
      lds_barrier();
      if (tid < 9 * count) {
        double a = 0.0;
        for (int j = 0; j < J; ++j) a += part1[tid * J + j];
        accs[tid] = a;
      }
    } else {                                   // no LDS room for the products: LDS atomics (slow under contention, but general)
      for (int i = tid; i < 9 * count; i += kBT) accs[i] = 0.0;
      lds_barrier();
      for (int g = item0 + tid; g < item1; g += kBT) {
        const int R = sp.rows[g], k = sp.owner[g] - first;
        const double xr = (R == sp.aug) ? -1.0 : sm[R];
#pragma unroll
        for (int q = 0; q < 9; ++q) atomicAdd(&accs[9 * k + q], -sp.W[(size_t)q * sp.total_items + g] * xr);
      }
    }
    lds_barrier();
    for (int idx = tid; idx < 9 * count; idx += kBT) {
      const int kk = idx / 9, qq = idx - 9 * kk;
      double v = 0.0;                                       // x_q = sum_{t >= q} (L^-1)[t][q] acc_t
      if (sp.linv_in_lds) { const double* Li = linv + (size_t)(first + kk) * 81; for (int t = qq; t < 9; ++t) v += Li[t * 9 + qq] * accs[9 * kk + t]; }
      else { const double* Li = sp.Linv + (size_t)(first + kk) * 81; for (int t = qq; t < 9; ++t) v += Li[t * 9 + qq] * accs[9 * kk + t]; }
      sm[9 * (first + kk) + qq] = v;                        // block `first + kk` owns S columns 9 (first + kk) ..
    }
    lds_barrier();
    mark();
  }
  for (int i = tid; i < sp.d_total; i += kBT) xout[i] = sm[sp.perm[i]];
  mark();
  if (sp.dbg && tid == 0) sp.dbg[63] = (unsigned long long)stamp;
}
__global__ __launch_bounds__(kBT) void k_chol_backsolve(BackArgs a) { chol_backsolve_body(a); }
__global__ __launch_bounds__(kBT) void k_chol_backsolve_b(const BackArgs* __restrict__ t) { chol_backsolve_body(t[blockIdx.y]); }

// ------------------------------------------------------------------------------------------------ step pieces
// landmark back-substitution: dl = (-gr - e_l . dx_pose) / Cd ; model terms and norms
// (on DENSE rows one thread per landmark beat a wave per landmark, 25.6 vs 29.9 us; with the row limited to the landmark's track
// a per-thread walk diverges (41-54 us) and 16 lanes per landmark is the right shape)
// COH_DX: the pose increments were published by a sibling workgroup of THIS launch as agent-scope atomic stores: read past the non-coherent cache levels
// PRE > 0 (the landmark workgroups of k_backsolve_tail, which spend the dense solve waiting for the pose increments): nothing but the step
// depends on it, so the operands of the workgroup's first PRE passes are requested BEFORE `wait` (the bounded wait for the increments) — the
// track limits, then per lane a window of kLmEPre entries of the E band (16 lanes: 128 entries less the alignment slack, 18 keyframes; the
// tracks of synthetic.config4_window are geometric with mean 10) and gr / Cd / C / inv_depth.  Behind the wait these passes are the step
// into LDS, multiply-adds from registers, row16_sum and the stores; the rest of a longer band and any further pass are read as before.
// Two passes of 32 landmarks over 224 workgroups hold 14 336 landmarks: the 10 000 of the headline window need nothing else.
// (What is requested early is NOT __restrict__ then: LLVM would sink the requests past the wait to their uses, as in chol_backsolve_body.)
struct NoWait { __device__ __forceinline__ void operator()() const {} };
template <bool R, typename T> struct RestrictIf { typedef T* __restrict__ type; };
template <typename T> struct RestrictIf<false, T> { typedef T* type; };
template <int NT = kT, bool COH_DX = false, int PRE = 0, typename Wait = NoWait>
__device__ __forceinline__ void landmark_back_body(const int vb, const int nwg, int n_lm, int dp, int ldE, typename RestrictIf<PRE == 0, const double>::type E,
                                                   typename RestrictIf<PRE == 0, const double>::type C, typename RestrictIf<PRE == 0, const double>::type Cd,
                                                   typename RestrictIf<PRE == 0, const double>::type gr,
                                                   const double* __restrict__ dxc, typename RestrictIf<PRE == 0, const double>::type inv_depth,
                                                   double* __restrict__ dxl, double* __restrict__ invd2, double* __restrict__ scal,
                                                   typename RestrictIf<PRE == 0, const int>::type kmin, typename RestrictIf<PRE == 0, const int>::type kmax,
                                                   const Wait wait = Wait()) {
  extern __shared__ double sdx[];
  const int q = threadIdx.x & 15;
  constexpr int kP = PRE > 0 ? PRE : 1;
  int pb[kP], pi1[kP];
  double pe[kP][kLmEPre], pg[kP], pcd[kP], pc[kP], pid[kP];
  if constexpr (PRE > 0) {
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
      const int l = vb * (NT / 16) + (threadIdx.x >> 4) + p * nwg * (NT / 16);
      const bool ok = l < n_lm;
      const int i0 = (ok && kmin) ? 6 * min(kmin[l], dp / 6) : 0;
      pi1[p] = ok ? (kmin ? 6 * (kmax[l] + 1) : dp) : 0;
      pb[p] = (i0 & ~15) + q;
      const double* e = E + (size_t)(ok ? l : 0) * ldE + pb[p];
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) pe[p][u] = pb[p] + 16 * u < pi1[p] ? e[16 * u] : 0.0;
      pg[p] = ok ? gr[l] : 0.0; pcd[p] = ok ? Cd[l] : 1.0; pc[p] = ok ? C[l] : 0.0; pid[p] = ok ? inv_depth[l] : 0.0;
    }
    // the values are consumed HERE, ahead of the wait: whatever the optimiser makes of the pointers, the requests cannot sink behind it
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) asm volatile("" ::"v"(pe[p][u]));
      asm volatile("" ::"v"(pg[p]), "v"(pcd[p]), "v"(pc[p]), "v"(pid[p]));
    }
    wait();
  }
  for (int i = threadIdx.x; i < dp; i += NT) sdx[i] = COH_DX ? __hip_atomic_load(dxc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : dxc[i];
  __syncthreads();
  // 16 lanes per landmark: the band of a row is a few 128-byte runs, read coalesced and reduced with four shuffles; the grid is
  // capped and strides over the landmarks so that the three scalar sums cost one atomic per WORKGROUP (thousands of per-wave
  // atomics on the 32 striped slots were most of this kernel's time)
  double m = 0.0, n2 = 0.0, x2 = 0.0, gmx = 0.0;
  if constexpr (PRE > 0) {
#pragma unroll
    for (int p = 0; p < PRE; ++p) {
      const int l = vb * (NT / 16) + (threadIdx.x >> 4) + p * nwg * (NT / 16);
      double ed = 0.0;
#pragma unroll
      for (int u = 0; u < kLmEPre; ++u) if (pb[p] + 16 * u < pi1[p]) ed += pe[p][u] * sdx[pb[p] + 16 * u];
      if (pb[p] + 16 * kLmEPre < pi1[p]) {        // the rest of a band longer than the window
        const double* e = E + (size_t)l * ldE;
        for (int i = pb[p] + 16 * kLmEPre; i < pi1[p]; i += 16) ed += e[i] * sdx[i];
      }
      ed = row16_sum(ed);
      if (q == 0 && l < n_lm) {
        const double g_l = pg[p];
        const double dl = (-g_l - ed) / pcd[p];
        gmx = fmax(gmx, fabs(g_l));
        dxl[l] = dl;
        invd2[l] = pid[p] + dl;
        m += -0.5 * dl * ((pcd[p] - pc[p]) * dl - g_l);
        n2 += dl * dl; x2 += pid[p] * pid[p];
      }
    }
  }
  for (int l = vb * (NT / 16) + (threadIdx.x >> 4) + PRE * nwg * (NT / 16); l < n_lm; l += nwg * (NT / 16)) {
    const double* e = E + (size_t)l * ldE;
    double ed = 0.0;
    const int i0 = kmin ? 6 * min(kmin[l], dp / 6) : 0, i1 = kmin ? 6 * (kmax[l] + 1) : dp;   // the row is zero outside the landmark's track
    for (int i = (i0 & ~15) + q; i < i1; i += 16) ed += e[i] * sdx[i];
    ed = row16_sum(ed);
    if (q == 0) {
      const double g_l = gr[l];
      const double dl = (-g_l - ed) / Cd[l];
      gmx = fmax(gmx, fabs(g_l));                   // Ceres' gradient_max_norm runs over every unknown, the inverse depths included
      dxl[l] = dl;
      invd2[l] = inv_depth[l] + dl;                 // the candidate inverse depth (was a second pass in k_apply_step)
      m += -0.5 * dl * ((Cd[l] - C[l]) * dl - g_l);
      n2 += dl * dl; x2 += inv_depth[l] * inv_depth[l];
    }
  }
  __shared__ double red[4][NT / 64];
  m = wave_sum(m); n2 = wave_sum(n2); x2 = wave_sum(x2);
  for (int o = 32; o > 0; o >>= 1) gmx = fmax(gmx, __shfl_down(gmx, o));
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = m; red[1][threadIdx.x >> 6] = n2; red[2][threadIdx.x >> 6] = x2; red[3][threadIdx.x >> 6] = gmx; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int k = 0; k < NT / 64; ++k) v += red[threadIdx.x][k];
    double* dst = scal + (threadIdx.x == 0 ? SC_MODEL : (threadIdx.x == 1 ? SC_DXNORM : SC_XNORM));
    if (v != 0.0) atomicAdd(dst + (vb & (kStripes - 1)), v);
  } else if (threadIdx.x == 3) {
    double v = 0.0;
    for (int k = 0; k < NT / 64; ++k) v = fmax(v, red[3][k]);
    // (non-negative doubles order like their bit patterns; striped like the sums: hundreds of workgroups hitting ONE address serialise,
    // measured +4 us on this launch)
    if (v != 0.0) atomicMax(reinterpret_cast<unsigned long long*>(scal + SC_GMAX + (vb & (kStripes - 1))), (unsigned long long)__double_as_longlong(v));
  }
}
// Model cost change without a pass over H:  (H + D) dx = -g  =>  -dx^T (g + H dx / 2) = 1/2 sum_i dx_i (D_i dx_i - g_i).
// Camera part in k_apply_step (D_i = clamp(B_ii)/radius), landmark part in k_landmark_back.  SC_MODEL accumulates the NEGATED value
// (host flips the sign), keeping the convention model = -SC_MODEL.
// x_new = x [+] dx  (EigenQuaternionParameterization::Plus on the quaternion, plain add elsewhere)
// ... fused with the camera part of the model cost change (k_model_cam's body; d <= 15 n_kf threads of the same grid)
// PARTS: bit 0 = the pose unknowns (sums over [0, 6 n_kf), candidate poses), bit 1 = the (v, ba, bg) unknowns (sums over [6 n_kf, d), candidate
// velocities / biases); 3 = everything (k_step_tail).  k_backsolve_tail runs the two parts in different workgroups at different times.
// What apply_step_body reads for thread i (unknown i, keyframe i) that does not depend on the step: the pose workgroup of k_backsolve_tail
// requests it before it waits for the increments (the pointers are not __restrict__: the requests must stay where they are written).
struct StepOps { double h, h0d, gci, p[7]; int frozen, cm_kf; };
template <int PARTS>
__device__ __forceinline__ StepOps step_ops_load(const int i, int n_kf, StateP s, int d, int ld, const double* B, const double* gc,
                                                 const unsigned char* pose_const, const JacobiDev jac) {
  StepOps o{};
  if (i < d && ((PARTS & 1) || i >= 6 * n_kf) && ((PARTS & 2) || i < 6 * n_kf)) {
    o.h = B[(size_t)i * ld + i]; o.h0d = jac.h0[i]; o.gci = gc[i]; o.frozen = *jac.frozen;
  }
  o.cm_kf = (i < n_kf && pose_const) ? pose_const[i] : 0;      // bit 0: pose, bits 1..3: v, ba, bg held constant
  if (i < n_kf && (PARTS & 1)) {
    const double* sp = s.poses;
#pragma unroll
    for (int c = 0; c < 7; ++c) o.p[c] = sp[7 * i + c];
  }
  return o;
}
template <int NT = kT, int PARTS = 3>
__device__ __forceinline__ void apply_step_ops(const int vb, int n_kf, int n_lm, StateP s, const double* __restrict__ dxc, const double* __restrict__ dxl,
                                               double* __restrict__ poses2, double* __restrict__ vel2, double* __restrict__ ba2,
                                               double* __restrict__ bg2, double* __restrict__ invd2, double* __restrict__ scal, int d, double inv_radius,
                                               const StepOps& ops) {
  const int i = vb * NT + threadIdx.x;
  // step_norm / x_norm as Ceres takes them (trust_region_minimizer.cc): |x - x_plus_delta| and |x| over the AMBIENT parameter vector of the
  // reduced program — the quaternion's four coefficients, not its three tangent increments; constant pose blocks are not part of it
  double m = 0.0, n2 = 0.0, g = 0.0, x2 = 0.0;
  if (i < d && ((PARTS & 1) || i >= 6 * n_kf) && ((PARTS & 2) || i < 6 * n_kf)) {
    const double dx = dxc[i];
    const double h = ops.h, h0d = ops.h0d;
    m = -0.5 * dx * (lm_damping(h, ops.frozen ? h0d : h) * inv_radius * dx - ops.gci);      // (first pass: H0 = H, being recorded by the assembly)
    const bool rot = i < 6 * n_kf && (i % 6) < 3;           // rotation increments enter through the quaternion difference below
    n2 = rot ? 0.0 : dx * dx;
    g = fabs(ops.gci);
  }
  const int cm_kf = ops.cm_kf;
  if (i < n_kf && (PARTS & 1)) {
    const double* p = ops.p; const double* dlt = dxc + 6 * i;
    const double nrm = sqrt(dlt[0] * dlt[0] + dlt[1] * dlt[1] + dlt[2] * dlt[2]);
    double* o = poses2 + 7 * i;
    if (nrm > 0.0) {
      const double sn = sin(nrm) / nrm, cw = cos(nrm);
      const double dx = sn * dlt[0], dy = sn * dlt[1], dz = sn * dlt[2];
      const double xw = p[3], xx = p[0], xy = p[1], xz = p[2];   // q_delta (x) x, Hamilton [w,x,y,z]
      o[3] = cw * xw - dx * xx - dy * xy - dz * xz;
      o[0] = cw * xx + dx * xw + dy * xz - dz * xy;
      o[1] = cw * xy - dx * xz + dy * xw + dz * xx;
      o[2] = cw * xz + dx * xy - dy * xx + dz * xw;
    } else { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3]; }
    for (int c = 0; c < 3; ++c) o[4 + c] = p[4 + c] + dlt[3 + c];
    for (int c = 0; c < 4; ++c) n2 += (o[c] - p[c]) * (o[c] - p[c]);
    if (!(cm_kf & 1)) for (int c = 0; c < 7; ++c) x2 += p[c] * p[c];
  }
  if (i < n_kf && (PARTS & 2)) {
    const int cm = cm_kf;
    const double* dv = dxc + 6 * n_kf + 9 * i;
    for (int c = 0; c < 3; ++c) { vel2[3 * i + c] = s.vel[3 * i + c] + dv[c]; ba2[3 * i + c] = s.ba[3 * i + c] + dv[3 + c]; bg2[3 * i + c] = s.bg[3 * i + c] + dv[6 + c]; }
    for (int c = 0; c < 3; ++c)
      x2 += ((cm & 2) ? 0.0 : s.vel[3 * i + c] * s.vel[3 * i + c]) + ((cm & 4) ? 0.0 : s.ba[3 * i + c] * s.ba[3 * i + c]) + ((cm & 8) ? 0.0 : s.bg[3 * i + c] * s.bg[3 * i + c]);
  }
  if (i < n_lm) invd2[i] = s.inv_depth[i] + dxl[i];
  if (vb * NT < d) {      // block-uniform
    block_add(m, scal + SC_MODEL); block_add(n2, scal + SC_DXNORM);
    for (int o = 32; o > 0; o >>= 1) g = fmax(g, __shfl_down(g, o));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned long long*>(scal + SC_GMAX + (vb & (kStripes - 1))), (unsigned long long)__double_as_longlong(g));
  }
  block_add(x2, scal + SC_XNORM);
}
template <int NT = kT, int PARTS = 3>
__device__ __forceinline__ void apply_step_body(const int vb, int n_kf, int n_lm, StateP s, const double* __restrict__ dxc, const double* __restrict__ dxl,
                                                double* __restrict__ poses2, double* __restrict__ vel2, double* __restrict__ ba2,
                                                double* __restrict__ bg2, double* __restrict__ invd2, double* __restrict__ scal, int d, int ld,
                                                const double* __restrict__ B, const double* __restrict__ gc, double inv_radius,
                                                const unsigned char* __restrict__ pose_const, const JacobiDev jac) {
  const StepOps ops = step_ops_load<PARTS>(vb * NT + threadIdx.x, n_kf, s, d, ld, B, gc, pose_const, jac);
  apply_step_ops<NT, PARTS>(vb, n_kf, n_lm, s, dxc, dxl, poses2, vel2, ba2, bg2, invd2, scal, d, inv_radius, ops);
}

// landmark back-substitution and the camera-side step / model terms as ONE launch: workgroups [0, g_lm) walk the landmarks,
// the rest apply dx to the keyframe states (independent of the landmark results)
template <bool SEL = true> __device__ __forceinline__ const double* tail_E(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.E : (const double*)A.E; }
template <bool SEL = true> __device__ __forceinline__ const double* tail_B(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.B : (const double*)A.B; }
template <bool SEL = true> __device__ __forceinline__ const double* tail_gc(const TailArgs& A) { return acc_set_t<SEL>(A.acc) ? (const double*)A.acc.gc : (const double*)A.gc; }
template <bool SEL>
__device__ __forceinline__ void step_tail_body(const int bx, const TailArgs& A) {
  if (bx >= A.nblocks || (A.done && *A.done)) return;
  if (bx < A.g_lm) landmark_back_body(bx, A.g_lm, A.n_lm, A.dp, A.ldE, tail_E<SEL>(A), A.C, A.Cd, A.gr, A.dxc, A.s.inv_depth, A.dxl, A.invd2, A.scal, A.kmin, A.kmax);
  else apply_step_body(bx - A.g_lm, A.n_kf, 0, A.s, A.dxc, A.dxl, A.poses2, A.vel2, A.ba2, A.bg2, A.invd2, A.scal, A.d, A.ld, tail_B<SEL>(A), tail_gc<SEL>(A), 1.0 / *A.radius, A.pose_const, A.jac);
}
__global__ __launch_bounds__(kT) void k_step_tail(TailArgs a) { step_tail_body<true>(blockIdx.x, a); }
__global__ __launch_bounds__(kT) void k_step_tail_b(const TailArgs* __restrict__ t) { step_tail_body<false>(blockIdx.x, t[blockIdx.y]); }
__global__ __launch_bounds__(kT) void k_step_tail_bt(const TailArgs* __restrict__ t) { step_tail_body<false>(blockIdx.y, t[blockIdx.x]); }

// The back substitution and the step tail as ONE launch (single-window chain).  The landmark back-substitution needs the POSE part of the
// step only, and the poses are solved first (dense corner, 16 of the back substitution's 28 us); the sparse levels behind it (the
// velocities' and biases' increments, 11 us in one workgroup) and the landmark pass (10 us in hundreds of workgroups) have nothing to do
// with each other, yet as two launches they ran one after the other.  Here workgroup 0 is the back substitution — it publishes the pose
// increments as soon as the dense corner is done, goes on with the sparse levels and finally applies the step to the keyframe states
// (apply_step_body) — and workgroups 1.. are the landmark pass: they wait for the pose increments inside the launch (bounded, like the
// chained sparse levels: on a time-out the hand-over flag is raised, the pass is not judged and the host re-runs it with the two launches
// of old; SpSrc has the rules) and then walk the landmarks.  One launch boundary less and the two tails overlap: 39 -> 29 us at configs[3].
// Product form (g_prod > 0, Chain::back_product): workgroup 0 solves the dense corner only and publishes all of it; the (v, ba, bg) part of
// the step no longer runs behind it as five sequential levels but in g_prod further sibling workgroups, each owning kpw keyframes: they
// wait for the same flag as the landmark workgroups, take one product with their rows of G (formed under the dense factorisation:
// back_product_ride) and apply the (v, ba, bg) part of the step for their keyframes.  The launch then ends at flag + max(landmark pass,
// product) instead of flag + levels.
// the bounded wait of the consumers of pose_ready (SpSrc has the rules)
__device__ __forceinline__ void wait_pose_ready(const BackTailArgs& a) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load((int*)a.back.pose_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      __builtin_amdgcn_s_sleep(16);
      if (wall_clock64() - t0 > (unsigned long long)a.timeout_ticks) { atomicMax(a.fail, kFailHandover + 90000); break; }
    }
  }
  __syncthreads();
  if (a.fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// G workgroup vb: keyframes [vb kpw, vb kpw + kpw).  Row (keyframe k, component c) is natural unknown dp + 9 k + c and S column perm[..]:
// below `off` it is G row perm[..] (an eliminated node), otherwise the block stayed in the dense corner and its increment is read from the
// published solution — either way it is applied here, exactly once.  16 lanes per row, 32 rows per pass; a lane's share of the first pass
// is requested into a fixed register window BEFORE the wait (what does not fit, and further passes, are read from memory afterwards).
constexpr int kGPre = 24, kLmPre = 2;      // kLmPre: passes of a landmark workgroup whose operands are requested before the wait (landmark_back_body)
__device__ __forceinline__ void back_product_body(const int vb, const BackTailArgs& a) {
  const TailArgs& T = a.tail; const SpBack& sp = a.back.sp;
  extern __shared__ double gsm[];          // xd[ldG]: [x_dense ; -1 ; 0 ..] | xs[9 kpw]: this workgroup's rows of the step
  double* xd = gsm; double* xs = gsm + a.ldG;
  const int tid = threadIdx.x, q = tid & 15, row = tid >> 4, ldG = a.ldG, nu = ldG >> 4;
  const int k0 = vb * a.kpw, nrows = 9 * min(a.kpw, T.n_kf - k0), i0 = T.dp + 9 * k0;      // the rows' natural unknowns are contiguous from i0
  unsigned long long* dbg = (sp.dbg && vb == 0 && tid == 0) ? sp.dbg + 40 : nullptr;
  if (dbg) dbg[0] = wall_clock64();
  // ---- requests: nothing below depends on the step
  const int scol = row < nrows ? sp.perm[i0 + row] : -1;
  const bool in_g = scol >= 0 && scol < sp.off;
  const double* grow = a.G + (size_t)(in_g ? scol : 0) * ldG + q;
  double g[kGPre];
#pragma unroll
  for (int u = 0; u < kGPre; ++u) g[u] = (in_g && u < nu) ? grow[16 * u] : 0.0;
  const int ip0 = tid < ldG ? a.iperm[sp.off + tid] : -1;
  // the operands of this thread's unknown (thread t < nrows applies row t)
  const bool mine = tid < nrows;
  const int ui = i0 + (mine ? tid : 0), uk = k0 + (mine ? tid / 9 : 0), uc = mine ? tid % 9 : 0;
  const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
  const double* sv = uc < 3 ? (const double*)T.s.vel : (uc < 6 ? (const double*)T.s.ba : (const double*)T.s.bg);
  double* cv = uc < 3 ? (double*)T.vel2 : (uc < 6 ? (double*)T.ba2 : (double*)T.bg2);
  const double h = mine ? Bt[(size_t)ui * T.ld + ui] : 0.0, h0d = mine ? T.jac.h0[ui] : 0.0, gci = mine ? gct[ui] : 0.0;
  const double sval = mine ? sv[3 * uk + uc % 3] : 0.0;
  const int cm = (mine && T.pose_const) ? T.pose_const[uk] : 0;      // bit 0: pose, bits 1..3: v, ba, bg held constant
  const int frozen = *T.jac.frozen;
  const double inv_radius = 1.0 / *T.radius;
  wait_pose_ready(a);
  if (dbg) dbg[1] = wall_clock64();
  // ---- the dense solution, read at the coherence point
  for (int j = tid; j < ldG; j += kBT) {
    const int ip = j == tid ? ip0 : a.iperm[sp.off + j];
    xd[j] = ip >= 0 ? __hip_atomic_load(T.dxc + ip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (ip == -2 ? -1.0 : 0.0);      // (-2: the augmented column)
  }
  __syncthreads();
  if (dbg) dbg[2] = wall_clock64();
  // ---- rows of x
  {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < kGPre; ++u) if (u < nu) s += g[u] * xd[q + 16 * u];
    if (in_g) for (int u = kGPre; u < nu; ++u) s += grow[16 * u] * xd[q + 16 * u];
    s = row16_sum(s);
    if (q == 0 && row < nrows) {
      if (in_g) { xs[row] = s; a.back.xout[i0 + row] = s; }      // (a block of the dense corner was written out by workgroup 0)
      else xs[row] = xd[scol - sp.off];
    }
  }
  for (int r0 = kBT / 16; r0 < nrows; r0 += kBT / 16) {             // further passes (more than 3 keyframes per workgroup)
    const int rw = r0 + row;
    const int sc = rw < nrows ? sp.perm[i0 + rw] : -1;
    const bool ing = sc >= 0 && sc < sp.off;
    double s = 0.0;
    if (ing) { const double* gr = a.G + (size_t)sc * ldG + q; for (int u = 0; u < nu; ++u) s += gr[16 * u] * xd[q + 16 * u]; }
    s = row16_sum(s);
    if (q == 0 && rw < nrows) {
      if (ing) { xs[rw] = s; a.back.xout[i0 + rw] = s; }
      else xs[rw] = xd[sc - sp.off];
    }
  }
  __syncthreads();
  if (dbg) dbg[3] = wall_clock64();
  // ---- the (v, ba, bg) part of the step for these keyframes: candidate state and the unknowns' share of the model cost change, the norms
  // and the gradient's max norm (apply_step_body's PARTS bit 1, one thread per unknown)
  double m = 0.0, n2 = 0.0, gm = 0.0, x2 = 0.0;
  if (mine) {
    const double dx = xs[tid];
    cv[3 * uk + uc % 3] = sval + dx;
    m = -0.5 * dx * (lm_damping(h, frozen ? h0d : h) * inv_radius * dx - gci);
    n2 = dx * dx;
    gm = fabs(gci);
    x2 = (cm & (2 << (uc / 3))) ? 0.0 : sval * sval;
  }
  block_add(m, T.scal + SC_MODEL); block_add(n2, T.scal + SC_DXNORM); block_add(x2, T.scal + SC_XNORM);
  for (int o = 32; o > 0; o >>= 1) gm = fmax(gm, __shfl_down(gm, o));
  if ((tid & 63) == 0 && gm != 0.0) atomicMax(reinterpret_cast<unsigned long long*>(T.scal + SC_GMAX + (blockIdx.x & (kStripes - 1))), (unsigned long long)__double_as_longlong(gm));
  if (dbg) dbg[4] = wall_clock64();
}
__global__ __launch_bounds__(kBT) void k_backsolve_tail(BackTailArgs a) {
  if (a.back.done && *a.back.done) return;                      // (every workgroup tests the same flag: nobody waits for a producer that has left)
  const TailArgs& T = a.tail;
  if (blockIdx.x == 0 && a.g_prod > 0) {
    chol_backsolve_body<false>(a.back);
    if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[55] = wall_clock64();      // LVF_BACK_TIMING: workgroup 0 is done
    return;
  }
  if ((int)blockIdx.x >= 2 + a.g_lm) { back_product_body((int)blockIdx.x - 2 - a.g_lm, a); return; }
  if (blockIdx.x == 0) {
    chol_backsolve_body(a.back);
    // the whole step is in xout (this workgroup wrote it): the velocities' and biases' part is applied here, with its share of the model cost
    // change.  (Requesting what that part reads — B's diagonal, the gradient, the states — ahead of the back substitution was measured
    // SLOWER: 36.1 vs 33.1 us for the launch; the registers it holds across the solve cost more than the three round trips it saves.)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    const double inv_radius = 1.0 / *T.radius;
    const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
    for (int vb = 0; vb * kBT < max(T.d, T.n_kf); ++vb)
      apply_step_body<kBT, 2>(vb, T.n_kf, 0, T.s, T.dxc, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, T.ld, Bt, gct, inv_radius, T.pose_const, T.jac);
    if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[55] = wall_clock64();      // LVF_BACK_TIMING: the step is applied
    return;
  }
  unsigned long long* ldbg = (a.back.sp.dbg && (blockIdx.x == 2 || (int)blockIdx.x == 1 + a.g_lm) && threadIdx.x == 0) ? a.back.sp.dbg + (blockIdx.x == 2 ? 56 : 59) : nullptr;
  if (ldbg) ldbg[0] = wall_clock64();
  if (blockIdx.x == 1) {
    // the pose part of the step: candidate poses and the pose unknowns' share of the model cost change / step norm (the increments are read
    // at the coherence point into LDS; apply_step_ops takes them from there).  What the first 512 unknowns / keyframes read beside the
    // increments — B's diagonal, h0, the gradient, the poses, the constant flags, the radius — is requested and consumed before the wait
    // (a.early; LVF_BACK_EARLY=0: behind it, as it was).
    extern __shared__ double sdx_pose[];
    const double* const Bt = tail_B(T); const double* const gct = tail_gc(T);
    StepOps ops{}; double radius = 0.0;
    if (a.early) {
      ops = step_ops_load<1>(threadIdx.x, T.n_kf, T.s, T.d, T.ld, Bt, gct, T.pose_const, T.jac);
      radius = *T.radius;
      asm volatile("" ::"v"(ops.h), "v"(ops.h0d), "v"(ops.gci), "v"(ops.frozen), "v"(ops.cm_kf), "v"(radius));
#pragma unroll
      for (int c = 0; c < 7; ++c) asm volatile("" ::"v"(ops.p[c]));
    }
    wait_pose_ready(a);
    for (int i = threadIdx.x; i < T.dp; i += kBT) sdx_pose[i] = __hip_atomic_load(T.dxc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (!a.early) { ops = step_ops_load<1>(threadIdx.x, T.n_kf, T.s, T.d, T.ld, Bt, gct, T.pose_const, T.jac); radius = *T.radius; }
    const double inv_radius = 1.0 / radius;
    apply_step_ops<kBT, 1>(0, T.n_kf, 0, T.s, sdx_pose, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, inv_radius, ops);
    for (int vb = 1; vb * kBT < max(T.dp, T.n_kf); ++vb)
      apply_step_body<kBT, 1>(vb, T.n_kf, 0, T.s, sdx_pose, T.dxl, T.poses2, T.vel2, T.ba2, T.bg2, T.invd2, T.scal, T.d, T.ld, Bt, gct, inv_radius, T.pose_const, T.jac);
    if (a.back.sp.dbg && threadIdx.x == 0) a.back.sp.dbg[62] = wall_clock64();      // LVF_BACK_TIMING: the pose part is applied
    return;
  }
  if (a.early)
    landmark_back_body<kBT, true, kLmPre>((int)blockIdx.x - 2, a.g_lm, T.n_lm, T.dp, T.ldE, tail_E(T), T.C, T.Cd, T.gr, T.dxc, T.s.inv_depth, T.dxl, T.invd2, T.scal, T.kmin, T.kmax,
                                          [&]() { wait_pose_ready(a); if (ldbg) ldbg[1] = wall_clock64(); });
  else {
    wait_pose_ready(a);
    if (ldbg) ldbg[1] = wall_clock64();
    landmark_back_body<kBT, true>((int)blockIdx.x - 2, a.g_lm, T.n_lm, T.dp, T.ldE, tail_E(T), T.C, T.Cd, T.gr, T.dxc, T.s.inv_depth, T.dxl, T.invd2, T.scal, T.kmin, T.kmax);
  }
  if (ldbg) ldbg[2] = wall_clock64();
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
    // the fields of the control block are read up front (independent requests, one wait) and written back once at the end: read and
    // written where the logic uses them they were 1.2 us of dependent traffic.  (A whole-struct copy goes through a scratch segment.)
    struct { double radius, decrease, last_radius, cost, initial_cost, cost_before, cost_after, model, dxnorm, xnorm, gmax;
             double function_tol, gradient_tol, parameter_tol, min_rel_decrease; int max_iters, iter, successes, invalid_run, accepted, solved, done, termination, why, rejected; } lc;
    lc.radius = c->radius; lc.decrease = c->decrease; lc.cost = c->cost; lc.initial_cost = c->initial_cost;
    lc.function_tol = c->function_tol; lc.gradient_tol = c->gradient_tol; lc.parameter_tol = c->parameter_tol; lc.min_rel_decrease = c->min_rel_decrease;
    lc.max_iters = c->max_iters; lc.iter = c->iter; lc.successes = c->successes; lc.invalid_run = c->invalid_run; lc.done = c->done; lc.termination = c->termination; lc.why = c->why; lc.rejected = c->rejected;
    const int hfail = *reinterpret_cast<const int*>(A.scal + SC_FAIL);
    const double cost_before = s_sum[SC_COST / kStripes], cost_new = s_sum[SC_COST_NEW / kStripes], model = -s_sum[SC_MODEL / kStripes];
    const double dxnorm = sqrt(s_sum[SC_DXNORM / kStripes]), xnorm = sqrt(s_sum[SC_XNORM / kStripes]);
    const double gmax = s_sum[SC_GMAX / kStripes];             // a max over the stripes (the stored bit patterns are the doubles')
    const bool solved = hfail == 0 && isfinite(cost_new) && isfinite(model);
    const int it = lc.iter;
    if (it == 0) { lc.initial_cost = cost_before; lc.cost = cost_before; }
    lc.cost_before = cost_before; lc.model = model; lc.dxnorm = dxnorm; lc.xnorm = xnorm; lc.gmax = gmax; lc.solved = solved ? 1 : 0;
    lc.last_radius = lc.radius;
    bool accepted = false, done = false;
    int termination = 1, why = LVF_WHY_MAX_ITERATIONS;
    // ceres::Solve's TrustRegionMinimizer, in its order (declared semantics + citations: oracle/lm.h lm_solve).
    // Top of the loop (FinalizeIterationAndCheckIfMinimizerCanContinue): the gradient at the point this pass linearised — it ends the
    // solve before a step is taken, so the pass is NOT an iteration; the smallest trust region likewise.
    // a chained sparse level gave up waiting for the level below (SpSrc): nothing about this step is judged — the loop stops where it is
    // (state, radius and counters untouched) and the host re-runs the iteration with un-chained launches
    if (hfail >= kFailHandover) { done = true; termination = 2; why = LVF_WHY_HANDOVER; }
    else if (gmax <= lc.gradient_tol) { done = true; termination = 0; why = LVF_WHY_GRADIENT; }
    else if (lc.radius < 1e-32) { done = true; termination = 0; why = LVF_WHY_MIN_RADIUS; }
    else {
      // (num_iterations = what Ceres records in Summary::iterations: accepted, rejected and invalid steps; a trial step that ends the solve
      // through the parameter / function tolerance returns before it is recorded)
      const bool valid = solved && model > 0.0;      // ComputeTrustRegionStep: solver failure or model_cost_change <= 0 = INVALID step
      if (!valid) {
        lc.iter = it + 1;
        lc.rejected += 1;
        lc.invalid_run += 1;
        if (lc.invalid_run >= 5) { done = true; termination = 2; why = LVF_WHY_INVALID_STEPS; }      // max_num_consecutive_invalid_steps
        else lc.radius *= 0.5;                       // LevenbergMarquardtStrategy::StepIsInvalid (decrease factor untouched)
      } else {
        lc.invalid_run = 0;
        // parameter tolerance, then function tolerance: both BEFORE the step-quality test, and neither takes the candidate
        if (dxnorm <= lc.parameter_tol * (xnorm + lc.parameter_tol)) { done = true; termination = 0; why = LVF_WHY_PARAMETER; }
        else if (fabs(cost_before - cost_new) <= lc.function_tol * cost_before) { done = true; termination = 0; why = LVF_WHY_FUNCTION; }
        else {
          lc.iter = it + 1;
          const double rho = (cost_before - cost_new) / model;
          if (rho > lc.min_rel_decrease) {
            accepted = true;
            const double t = 2.0 * rho - 1.0;
            lc.radius = fmin(lc.radius / fmax(1.0 / 3.0, 1.0 - t * t * t), 1e16);
            lc.decrease = 2.0;
            lc.successes += 1;
            lc.cost = cost_new;
          } else {
            lc.radius = lc.radius / lc.decrease;
            lc.decrease *= 2.0;
            lc.rejected += 1;
          }
        }
      }
      // after the step, Finalize's order again: the iteration cap first, then the smallest trust region (the gradient at an accepted point is
      // only known to the next pass)
      if (!done && lc.iter >= lc.max_iters) { done = true; termination = 1; why = LVF_WHY_MAX_ITERATIONS; }
      else if (!done && lc.radius < 1e-32) { done = true; termination = 0; why = LVF_WHY_MIN_RADIUS; }
    }
    lc.cost_after = accepted ? cost_new : (solved ? cost_new : cost_before);
    lc.accepted = accepted ? 1 : 0;
    if (done) { lc.termination = termination; lc.why = why; lc.done = 1; }
    s_commit = accepted ? 1 : 0;
    c->radius = lc.radius; c->decrease = lc.decrease; c->last_radius = lc.last_radius; c->cost = lc.cost; c->initial_cost = lc.initial_cost;
    c->cost_before = lc.cost_before; c->cost_after = lc.cost_after; c->model = lc.model; c->dxnorm = lc.dxnorm; c->xnorm = lc.xnorm; c->gmax = lc.gmax;
    c->iter = lc.iter; c->successes = lc.successes; c->invalid_run = lc.invalid_run; c->accepted = lc.accepted; c->solved = lc.solved;
    c->done = lc.done; c->termination = lc.termination; c->why = lc.why; c->rejected = lc.rejected;
    if (hfail < kFailHandover) c->jfrozen = 1;      // the Jacobi scaling of this solve is the first pass's (a pass that is re-run after a hand-over time-out takes it again)
    if (A.fused) {
      // the candidate pass linearised x + dx into the standby set: accepted, that set becomes the active one, its TwoFrame slabs still to be
      // reduced (k_tf_reduce); rejected, the active set keeps the linearisation at x, already reduced
      c->lin_pending = accepted ? 1 : 0;
      if (accepted) c->aset = c->aset ^ 1;
    }
    s_iter = lc.iter; s_done = lc.done;
    if (A.hist) {                                      // diagnostic: what this pass decided on
      double* h = A.hist + 8 * (it & 63);
      h[0] = (double)it; h[1] = cost_before; h[2] = cost_new; h[3] = model; h[4] = accepted ? 1.0 : 0.0; h[5] = (double)hfail; h[6] = lc.last_radius; h[7] = gmax;
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
__global__ __launch_bounds__(kDT) void k_lm_decide_b(const DecideArgs* __restrict__ t) { lm_decide_body(t[blockIdx.y]); }

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
