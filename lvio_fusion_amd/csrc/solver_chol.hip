// solver_chol.hip — LM iteration, stage 3: blocked dense Cholesky of the reduced camera system's pose corner, one launch per block step,
// with the riders that build the back substitution's products under it.  Device code only (solver_args.hpp: argument blocks, constants,
// prototypes).  The kernels of the block steps are defined here; their bodies (chol_step_body, back_product_ride, back_block_ride) live in
// solver_dev.hpp, because the merged last launch of solver_back.hip (k_chol_backsolve_tail) runs them too.
#include "solver_dev.hpp"

namespace lvf {

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

}  // namespace lvf
