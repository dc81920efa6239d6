// lm_rule.hpp — the declared Ceres trust-region rule, stated ONCE for every Levenberg-Marquardt loop on the device: LmState.  The solves that run
// whole inside one launch call it from their loop (lm_small, small_lm.hpp; k_pose_chain, pose_chain_kernels.hip); the two whose iteration is split
// over launches around a device-resident control block load that block into an LmState, call the members and write the fields back once:
// lm_decide_body (solver_kernels.hip, LmCtl: the window solver) and icp_step / icp_decide (icp_kernels.hip, IcpDev: every scan-to-map solve,
// scan_match's chain included).  With it the literal form of the damping term.  A header of its own, because small_lm.hpp brings the workgroup
// of kLT threads and its sums with it, which neither of the split solves has.  Declared semantics: oracle/lm.h lm_solve (the order of the
// tests), oracle/robust.h (the damping).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/lvf.h"

namespace lvf {

struct LmOpts { int max_iters; double function_tol, gradient_tol, parameter_tol, min_rel_decrease, radius0; };
struct LmRec { double initial_cost, final_cost; int iters, successes, termination, why, contractions, pad; };

// The trust-region rule of ceres::Solve's TrustRegionMinimizer: one member per decision point of oracle/lm.h lm_solve; `true` from a test ends
// the solve, termination and why set.  Scalars in, scalars out: how the sums are formed, how the step is solved and how x (+) dx and the norms
// are formed is the caller's, and so is the order of the tests where a caller's iteration does not begin and end where lm_solve's does.  In a
// workgroup that runs a whole loop every thread holds one and takes the same decisions.
struct LmState {
  double radius, decrease = 2.0, cost = 0.0, initial_cost = 0.0;
  int iters = 0, successes = 0, invalid_run = 0, termination = 0, why = LVF_WHY_NONE;      // (what a problem without unknowns ends with)
  bool first = true;                                 // no linearisation yet
  __device__ __forceinline__ explicit LmState(double radius0) : radius(radius0) {}
  __device__ __forceinline__ bool end(int t, int w) { termination = t; why = w; return true; }
  // the cost of a linearisation; true at the first one (iteration 0: the caller freezes its Jacobi scaling there)
  __device__ __forceinline__ bool linearized(double c) { const bool f = first; cost = c; if (f) initial_cost = c; first = false; return f; }
  // the three tests at the top of the loop, and the top of lm_solve's loop: them in its order.  A loop whose iteration is split over launches
  // calls the single tests where its split puts them.
  __device__ __forceinline__ bool cap(const LmOpts& o) { return iters >= o.max_iters && end(1, LVF_WHY_MAX_ITERATIONS); }
  __device__ __forceinline__ bool gradient(const LmOpts& o, double gnorm) { return gnorm <= o.gradient_tol && end(0, LVF_WHY_GRADIENT); }
  __device__ __forceinline__ bool min_radius() { return radius < 1e-32 && end(0, LVF_WHY_MIN_RADIUS); }
  __device__ __forceinline__ bool top(const LmOpts& o, double gnorm) { return cap(o) || gradient(o, gnorm) || min_radius(); }
  // the step as solved: valid if the factorisation went through and the model decreases; that ends a run of invalid ones
  __device__ __forceinline__ bool valid_step(bool solved, double model) { const bool v = solved && model > 0.0; if (v) invalid_run = 0; return v; }
  // an invalid step is counted; five in a row end the solve, else the radius is halved and the caller linearises again
  __device__ __forceinline__ bool invalid_step() {
    ++iters;
    if (++invalid_run >= 5) return end(2, LVF_WHY_INVALID_STEPS);
    radius *= 0.5; return false;
  }
  // parameter tolerance on the squared norms of the step and of x, then function tolerance on the candidate's cost
  __device__ __forceinline__ bool parameter_tol(const LmOpts& o, double sn2, double xn2) { return sqrt(sn2) <= o.parameter_tol * (sqrt(xn2) + o.parameter_tol) && end(0, LVF_WHY_PARAMETER); }
  __device__ __forceinline__ bool function_tol(const LmOpts& o, double cand) { return fabs(cost - cand) <= o.function_tol * cost && end(0, LVF_WHY_FUNCTION); }
  // step quality against the model decrease and the radius update of either outcome; true: the caller takes the candidate
  __device__ __forceinline__ bool accept(const LmOpts& o, double cand, double model) {
    ++iters;
    const double rho = (cost - cand) / model;
    if (!(rho > o.min_rel_decrease)) { radius /= decrease; decrease *= 2.0; return false; }
    cost = cand; ++successes;
    const double t = 2.0 * rho - 1.0;
    radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - t * t * t), 1e16); decrease = 2.0;
    return true;
  }
  // the ending: true is a FAILURE, and the caller puts the parameters back where they were (fail soft); then the record
  __device__ __forceinline__ bool failed() { const bool f = termination == 2 || !isfinite(cost); if (f) { termination = 2; cost = initial_cost; } return f; }
  __device__ __forceinline__ void fill(LmRec& rec) const {
    rec.initial_cost = initial_cost; rec.final_cost = cost; rec.iters = iters; rec.successes = successes; rec.termination = termination; rec.why = why;
    rec.contractions = 0; rec.pad = 0;
  }
};

// the damping of one unknown under Ceres' Jacobi scaling, unscaled, not yet over the radius (oracle/robust.h lm_damping): h = H_jj, h0 = H_jj at iteration 0
__device__ __forceinline__ double lm_damping(double h, double h0) {
  const double sj = 1.0 / (1.0 + sqrt(h0)), s2 = sj * sj;
  return fmin(fmax(h * s2, 1e-6), 1e32) / s2;
}

}  // namespace lvf
