// debug_taps.hip — device code of the test taps, kept out of the translation units of the hot path so that their code objects do not
// change with it.
#include <hip/hip_runtime.h>

#include "lvf_internal.hpp"

namespace lvf {
constexpr int kTapT = 256;
// Test tap: the caller's system over the assembled one.  Natural unknowns (i, j <= i) sit at S row max(perm[i], perm[j]), column min(..);
// rhs[j] in the augmented row `aug`, column perm[j].  The triangle of the d + 1 rows (row d = the rhs) is dealt one entry per thread.
__global__ __launch_bounds__(kTapT) void k_override_reduced(int d, int ld, int aug, const int* __restrict__ perm, const double* __restrict__ Sov,
                                                         const double* __restrict__ rhs, double* __restrict__ S) {
  const int i = blockIdx.y, j = blockIdx.x * kTapT + threadIdx.x;
  if (i > d || j >= d || (i < d && j > i)) return;
  const int pj = perm[j];
  if (i == d) { S[(size_t)aug * ld + pj] = rhs[j]; return; }
  const int pi = perm[i];
  S[(size_t)max(pi, pj) * ld + min(pi, pj)] = Sov[(size_t)i * d + j];
}

// (a plain launch: a test-only copy is no stage of lvf_problem_stage_times)
int launch_override_reduced(hipStream_t q, int d, int ld, int aug, const int* perm, const double* Sov, const double* rhs, double* S) {
  hipLaunchKernelGGL(k_override_reduced, dim3((d + kTapT - 1) / kTapT, d + 1), dim3(kTapT), 0, q, d, ld, aug, perm, Sov, rhs, S);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}
}  // namespace lvf
