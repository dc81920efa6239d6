// solver_dev.hpp — the device helpers that kernels of more than one translation unit of the LM iteration call.
// used by: solver_kernels.hip (block_add, acc_set, zero_lower, zero_list_share, reset_step_scalars)
// used by: solver_assemble.hip (done_flag_issue, acc_set*, zero_list_share, reset_step_scalars, lm_damping, fmac_row_bcast, double4_t)
// used by: solver_chol.hip (done_flag_issue, fmac_row_bcast, double4_t)
// used by: solver_back.hip (done_flag_issue, block_add, acc_set_t, lm_damping)
#pragma once
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
__device__ __forceinline__ double lm_damping(double h, double h0) {
  if (h >= 2e-6 * (1.0 + h0) && h < 1e32) return h;
  if (h0 == 0.0) return fmin(fmax(h, 1e-6), 1e32);
  const double sj = 1.0 / (1.0 + sqrt(h0)), s2 = sj * sj;
  return fmin(fmax(h * s2, 1e-6), 1e32) / s2;
}

// acc += (lane N of each 16-lane row of lv) * m: the DPP row_newbcast operand of v_fmac_f64 hands a row-uniform value to all 16 lanes
// inside the multiply-add itself (no LDS broadcast read, no v_readlane + SGPR operand)
template <int N>
__device__ __forceinline__ void fmac_row_bcast(double& acc, double lv, double m) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(lv), "v"(m), "n"(N));
}

}  // namespace lvf
