// solver_dev.hpp — the device helpers that kernels of more than one translation unit of the LM iteration call.
// used by: solver_kernels.hip (block_add, acc_set, zero_lower, zero_list_share, reset_step_scalars; LmState of lm_rule.hpp: lm_decide_body)
// used by: solver_assemble.hip (done_flag_issue, acc_set*, zero_list_share, reset_step_scalars, lm_damping_fast, fmac_row_bcast, double4_t)
// used by: solver_chol.hip (chol_step_body, back_product_ride, back_block_ride and what they call: k_chol_step*)
// used by: solver_back.hip (done_flag_issue, block_add, acc_set_t, lm_damping_fast; chol_step_body, back_product_ride, back_block_ride:
//          k_chol_backsolve_tail runs the last block step and the back substitution as one launch)
#pragma once
#include "lm_rule.hpp"
#include "lvf_internal.hpp"
#include "solver_args.hpp"

namespace lvf {

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

// rows of a lower-triangular matrix (leading dimension ld, even): one wave per row, columns [0, end of the row's 64-column block)
__device__ __forceinline__ void zero_lower(double* __restrict__ p, const int ld, const unsigned long long wave, const unsigned long long n_waves) {
  const int lane = threadIdx.x & 63;
  for (unsigned long long r = wave; r < (unsigned long long)ld; r += n_waves) {
    double2* row = reinterpret_cast<double2*>(p + r * (unsigned long long)ld);
    const int end2 = min(ld, (((int)r | 63) + 1)) / 2;
    for (int c = lane; c < end2; c += 64) row[c] = make_double2(0.0, 0.0);
  }
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

__device__ __forceinline__ void reset_step_scalars(double* scal) {
  for (int k = SC_COST_NEW + threadIdx.x; k < SC_N; k += kT) scal[k] = 0.0;
  if (threadIdx.x == 0) { *reinterpret_cast<int*>(scal + SC_FAIL) = 0; *reinterpret_cast<int*>(scal + SC_TICKET) = 0; }
}

// (the fp64 square root and two divisions of the literal form cost k_prepare / k_tf_reduce / k_step_tail 6.6 us per iteration between them
// when every diagonal entry took them — profiles/r05_a; they are only needed where the clamp can act:  s^2 h >= 1e-6  <=  h >= 2e-6 (1 + h0),
// because (1 + sqrt(h0))^2 <= 2 (1 + h0); there clamp(s^2 h) / s^2 = h up to one rounding.  A column that was empty at iteration 0 has s = 1.)
// Not the literal form (lm_rule.hpp lm_damping) to the bit where the short cut is taken; the fall-through is the literal form.
__device__ __forceinline__ double lm_damping_fast(double h, double h0) {
  if (h >= 2e-6 * (1.0 + h0) && h < 1e32) return h;
  if (h0 == 0.0) return fmin(fmax(h, 1e-6), 1e32);
  return lm_damping(h, h0);
}

// acc += (lane N of each 16-lane row of lv) * m: the DPP row_newbcast operand of v_fmac_f64 hands a row-uniform value to all 16 lanes
// inside the multiply-add itself (no LDS broadcast read, no v_readlane + SGPR operand)
template <int N>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double lv, double m) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(lv), "v"(m), "n"(N));
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
// XLAST (the sub-block sweep of the LAST block step inside k_chol_backsolve_tail): the inverse workgroup publishes the solution's last block
// (XLast) as soon as its sweep is over, ahead of its stores
template <bool SUB, bool XLAST = false>
__device__ __forceinline__ void chol_step_body(const int bx, const CholArgs& A, const int kb, const XLast xl = XLast()) {
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
  if constexpr (SUB && XLAST) {
    if (inverse_wg && kb == A.nb - 1 && xl.flag) {    // (workgroup-uniform)
      // x_last = L_kk^-T y_last with the arithmetic of the first-block solve of chol_backsolve_body: thread (c, part) takes eight terms of
      // row c, part 0 adds the eight parts.  L_kk^-T is complete in Pi (the panel waves put every row of their columns back).  y is row
      // dr = d - 64 kb of the factored diagonal block, columns [0, dr): the diagonal waves keep their finished columns in a[] for every row
      // (Pj lacks the diagonal tiles), so lane dr of each hands its 16 entries over; columns from dr on meet 0, as rows d.. do there.
      // Scratch: Pj, which nobody reads behind the last stage's barrier (the stores below take a[]).
      // It publishes also when a pivot was bad: the NaN flows into a step the failure flag rejects, and nobody is left waiting.
      const int dr = ncols - 1, xc = tid & 63, part = tid >> 6;
      double* ys = Pj; double* partial = Pj + kNB;
      if (!panel_wave && r == dr) {
#pragma unroll
        for (int c = 0; c < 16; ++c) ys[16 * q + c] = (16 * q + c < dr) ? a[c] : 0.0;
      }
      __syncthreads();
      double t2 = 0.0;
#pragma unroll
      for (int t = 0; t < kNB / 8; ++t) t2 += Pi[xc * kLd + (kNB / 8) * part + t] * ys[(kNB / 8) * part + t];
      partial[part * kNB + xc] = t2;
      __syncthreads();
      if (part == 0) {
        double s = 0.0;
#pragma unroll
        for (int pp = 0; pp < 8; ++pp) s += partial[pp * kNB + xc];
        const double xv = xc < dr ? s : (xc == dr ? -1.0 : 0.0);      // (-1 at the augmented row d: it meets column d - 64 kb of T_k,last)
        // one wave stores all 64 values: its own s_waitcnt orders them before the flag (no workgroup barrier).  As in chol_backsolve_body a
        // returning load of the same address stands behind the store: once it is back the value is where the consumer reads
        __hip_atomic_store((double*)xl.x + xc, xv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double chk = __hip_atomic_load((double*)xl.x + xc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(chk));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (xc == 0) __hip_atomic_store((int*)xl.flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
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
// ARRIVE (the riders of k_chol_backsolve_tail, whose rows are multiplied by sibling workgroups of the SAME launch): the rows leave as agent-scope
// atomic stores, confirmed by a returning load, and the workgroup then arrives at *arrive — the hand-over of the pose increments
// (chol_backsolve_body), with a counter for the flag
template <bool ARRIVE = false>
__device__ __forceinline__ void back_product_ride(const int vb, const GRide& R, int* arrive = nullptr) {
  if (vb >= R.n) return;
  if (R.done && *R.done) return;
  const int b = R.first + vb;
  const SpNode nd = R.nodes[b];
  const int* rows = R.rows + nd.row_off;
  const double* W = R.W + nd.row_off;                  // component t of the node's row r: W[t * wstride + r]
  const double* Li = R.Linv + (size_t)b * 81;
  double* G = R.G;
  double* last = nullptr;
  int ms = 0;
  // ARRIVE: sibling workgroups of the launch wait for these rows, so the dependent round trips are cut down — the first kRidePre row numbers are
  // requested together, and per column the neighbours' G entries, the map entry and the node's own W entries are all in flight before the first
  // multiply-add (same terms in the same order as the plain form below, which hides under a block step and stays as it was)
  constexpr int kRidePre = 4;
  int rw[kRidePre];
  if constexpr (ARRIVE) {
#pragma unroll
    for (int i = 0; i < kRidePre; ++i) rw[i] = i < nd.m ? rows[i] : R.off;
#pragma unroll
    for (int i = 0; i < kRidePre; ++i) if (ms == i && rw[i] < R.off) ms = i + 1;
    if (ms == kRidePre) while (ms < nd.m && rows[ms] < R.off) ++ms;
  } else {
    while (ms < nd.m && rows[ms] < R.off) ++ms;        // the sparse neighbours' rows
  }
  for (int j = threadIdx.x; j < R.ldG; j += kCT) {
    double T[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) T[t] = 0.0;
    if constexpr (ARRIVE) {
      const int g = R.map[(size_t)b * R.ldG + j];      // (global item index: already includes row_off)
      double xg[kRidePre], wo[9];
#pragma unroll
      for (int i = 0; i < kRidePre; ++i) xg[i] = i < ms ? G[(size_t)rw[i] * R.ldG + j] : 0.0;
#pragma unroll
      for (int t = 0; t < 9; ++t) wo[t] = g >= 0 ? R.W[(size_t)t * R.wstride + g] : 0.0;
#pragma unroll
      for (int i = 0; i < kRidePre; ++i)
        if (i < ms) {
#pragma unroll
          for (int t = 0; t < 9; ++t) T[t] -= W[(size_t)t * R.wstride + i] * xg[i];
        }
      for (int r = kRidePre; r < ms; ++r) {
        const double x = G[(size_t)rows[r] * R.ldG + j];
#pragma unroll
        for (int t = 0; t < 9; ++t) T[t] -= W[(size_t)t * R.wstride + r] * x;
      }
      if (g >= 0) {
#pragma unroll
        for (int t = 0; t < 9; ++t) T[t] -= wo[t];
      }
    } else {
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
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      double v = 0.0;
#pragma unroll
      for (int t = q; t < 9; ++t) v += Li[t * 9 + q] * T[t];
      if constexpr (ARRIVE) { last = G + (size_t)(9 * b + q) * R.ldG + j; __hip_atomic_store(last, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      else G[(size_t)(9 * b + q) * R.ldG + j] = v;
    }
  }
  if constexpr (ARRIVE) {
    if (last) { const double chk = __hip_atomic_load(last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); asm volatile("" ::"v"(chk)); }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave's stores have been performed before the workgroup arrives
    if (threadIdx.x == 0) __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace lvf
