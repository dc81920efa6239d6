// small_lm.hpp — the declared Ceres trust-region loop for the solves that run whole inside ONE launch of one workgroup.  The rule is stated once,
// in LmState.  lm_small runs it for a compile-time number of unknowns: the GNSS alignment (navsat_kernels.hip), Relocator::UpdateNewSubmap's
// rotation (loop_kernels.hip), the pose-only refinement of the visual relocalisation (reloc_kernels.hip); k_pose_chain (pose_chain_kernels.hip)
// for a run-time number of poses.  Three restatements stay outside, their decision being split over launches around a device-resident control
// block: lm_decide_body (solver_kernels.hip), icp_step / icp_decide (icp_kernels.hip) and scan_match.  Declared semantics: oracle/lm.h lm_solve (the
// order of the tests), oracle/robust.h (the loss, the damping); the box bounds: DESIGN.md "GNSS alignment".  Device code only; every array is
// indexed statically once the loops are unrolled (no scratch segment).
#pragma once
#include <cfloat>
#include <cmath>

#include "loop_dev.hpp"

namespace lvf {

struct LmOpts { int max_iters; double function_tol, gradient_tol, parameter_tol, min_rel_decrease, radius0; };
struct LmRec { double initial_cost, final_cost; int iters, successes, termination, why, contractions, pad; };

// The trust-region rule of ceres::Solve's TrustRegionMinimizer: one member per decision point of oracle/lm.h lm_solve, in its order; `true`
// from a test ends the solve, termination and why set.  Scalars in, scalars out: how the sums are formed, how the step is solved and how
// x (+) dx and the norms are formed is the caller's.  Every thread of the workgroup holds one and takes the same decisions.
struct LmState {
  double radius, decrease = 2.0, cost = 0.0, initial_cost = 0.0;
  int iters = 0, successes = 0, invalid_run = 0, termination = 0, why = LVF_WHY_NONE;      // (what a problem without unknowns ends with)
  bool first = true;                                 // no linearisation yet
  __device__ __forceinline__ explicit LmState(double radius0) : radius(radius0) {}
  __device__ __forceinline__ bool end(int t, int w) { termination = t; why = w; return true; }
  // the cost of a linearisation; true at the first one (iteration 0: the caller freezes its Jacobi scaling there)
  __device__ __forceinline__ bool linearized(double c) { const bool f = first; cost = c; if (f) initial_cost = c; first = false; return f; }
  // top of the loop: iteration cap, gradient, smallest radius
  __device__ __forceinline__ bool top(const LmOpts& o, double gnorm) {
    if (iters >= o.max_iters) return end(1, LVF_WHY_MAX_ITERATIONS);
    if (gnorm <= o.gradient_tol) return end(0, LVF_WHY_GRADIENT);
    return radius < 1e-32 && end(0, LVF_WHY_MIN_RADIUS);
  }
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

// HuberLoss::Evaluate (rho, rho') at s = |r|^2; a <= 0: no loss function.  Ceres' form: rho' = max(DBL_MIN, a / r), which differs from the
// plain a / r only where that quotient underflows to zero.
__device__ __forceinline__ void huber_eval(double a, double s, double& rho0, double& rho1) {
  if (a > 0.0 && s > a * a) {
    const double r = sqrt(s);
    rho0 = 2.0 * a * r - a * a; rho1 = fmax(DBL_MIN, a / r);
  } else { rho0 = s; rho1 = 1.0; }
}

// sums K per-thread values over the workgroup of kLT threads in place, every thread getting all K totals: wave_sum per value, one
// tile[kLT / 64][K], two barriers, the waves added in wave order (the values K calls of wg_sum give, up to the sign of a zero)
template <int K>
__device__ __forceinline__ void wg_sum_n(double acc[K], double* tile) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double sum = wave_sum(acc[k]);
    if (lane == 0) tile[wave * K + k] = sum;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = ((tile[k] + tile[K + k]) + tile[2 * K + k]) + tile[3 * K + k];
}
static_assert(kLT / 64 == 4, "wg_sum_n adds four waves");
// doubles of LDS the loop needs for N unknowns: the tile of wg_sum_n (its first kLT / 64 words also serve wg_sum)
constexpr int lm_tile_doubles(int N) { return (kLT / 64) * (N * (N + 1) / 2 + N + 1); }

// the damping of one unknown under Ceres' Jacobi scaling, unscaled, not yet over the radius (oracle/robust.h lm_damping): h = H_jj, h0 = H_jj at iteration 0
__device__ __forceinline__ double lm_damping(double h, double h0) {
  const double sj = 1.0 / (1.0 + sqrt(h0)), s2 = sj * sj;
  return fmin(fmax(h * s2, 1e-6), 1e32) / s2;
}

// One Levenberg-Marquardt step of the N x N system (H, g): Jacobi scaling s from h0 (the diagonal at iteration 0), the damping term clamped
// on the scaled system and divided by the radius, Cholesky, both triangular solves, and the model decrease -dx.(g + H dx / 2).  The system stays
// N x N whatever is constant: a slot outside free_mask gets a unit diagonal and a zero gradient entry, so that its step is exactly 0 and the
// factor of the free columns is, operation for operation, the factor of the reduced system.  false: the damped matrix is not positive definite
// (dx = 0).
template <int N>
__device__ __forceinline__ bool lm_damped_step(const double (&H)[N][N], const double (&g)[N], const double (&h0)[N], double radius, unsigned free_mask,
                                               double (&dx)[N], double& model) {
  double L[N][N];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool fr = (free_mask >> j) & 1u;
    double d = 1.0;
    if (fr) d = H[j][j] + lm_damping(H[j][j], h0[j]) / radius;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && (d > 0.0);
    const double l = sqrt(d);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = (fr && ((free_mask >> i) & 1u)) ? H[i][j] : 0.0;
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
#pragma unroll
  for (int c = 0; c < N; ++c) dx[c] = 0.0;
  if (ok) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = ((free_mask >> i) & 1u) ? -g[i] : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < N; ++k) s -= L[k][i] * dx[k];
      dx[i] = s / L[i][i];
    }
  }
  model = 0.0;
#pragma unroll
  for (int u = 0; u < N; ++u) {
    if (!((free_mask >> u) & 1u)) continue;
    double hd = 0.0;
#pragma unroll
    for (int v = 0; v < N; ++v)
      if ((free_mask >> v) & 1u) hd += H[u][v] * dx[v];
    model -= dx[u] * (g[u] + 0.5 * hd);
  }
  return ok;
}

template <bool PAR, class P>
__device__ __forceinline__ double lm_cost(const P& p, const double* x, double* tile) {
  const double c = p.cost_part(x);
  return PAR ? wg_sum(c, tile) : c;
}
template <class P>
__device__ __forceinline__ double box_clamp(const P& p, int c, double v) {
  if constexpr (P::kBox) return fmin(fmax(v, p.lo[c]), p.hi[c]);
  else return v;
}
template <int N, class P>
__device__ __forceinline__ void project_box(const P& p, double x[N], unsigned bound_mask) {
#pragma unroll
  for (int c = 0; c < N; ++c)
    if ((bound_mask >> c) & 1u) x[c] = box_clamp(p, c, x[c]);
}

// ceres::Solve's TrustRegionMinimizer loop (order of tests: oracle/lm.h lm_solve) on M ambient coordinates x and N tangent unknowns, of which
// those in free_mask are unknowns.  x is updated in place; a FAILURE leaves it as it came.  The problem P supplies what differs:
//   accumulate(x, free_mask, acc)   this thread's share, added into acc: the lower triangle of J^T J (row-major, entry u (u + 1) / 2 + v), then
//                                   J^T r (N entries), then the cost 1/2 sum rho — the loss already applied
//   cost_part(x)                    this thread's share of the cost
//   plus(x, dx, xc)                 xc = x (+) dx
//   norm_mask(free_mask)            the ambient coordinates that enter the step and parameter norms
//   kBox                            compile-time: box bounds bound_mask / lo[] / hi[] on the coordinates (then M == N and plus is addition):
//                                   projection, projected gradient, projected Armijo search
// PAR: the shares are summed over the workgroup through `tile` (lm_tile_doubles(N) doubles of LDS); else every thread holds the whole sums.
// Either way every thread of the workgroup takes the same decisions.
template <int N, int M, bool PAR, class P>
__device__ __forceinline__ void lm_small(const P& p, int n_active, double (&x)[M], unsigned free_mask, const LmOpts& o, LmRec& rec, double* tile) {
  constexpr int T = N * (N + 1) / 2, K = T + N + 1;
  static_assert(!P::kBox || N == M, "box bounds sit on coordinates that are their own tangent");
  LmState s(o.radius0);
  if (n_active == 0 || free_mask == 0u) {            // no residual block: Ceres drops the unused parameter blocks, nothing moves; or every block
    if (n_active != 0) s.linearized(lm_cost<PAR>(p, x, tile));      // constant: the problem has a cost and no unknown
    s.fill(rec);
    return;
  }
  unsigned bound_mask = 0u;
  if constexpr (P::kBox) bound_mask = p.bound_mask & free_mask;
  const bool bounded = bound_mask != 0u;
  const unsigned norm_mask = p.norm_mask(free_mask);
  double x0[M];
#pragma unroll
  for (int c = 0; c < M; ++c) x0[c] = x[c];
  if (bounded) project_box<M>(p, x, bound_mask);
  int contractions = 0;
  double h0[N];
#pragma unroll
  for (int c = 0; c < N; ++c) h0[c] = 0.0;
  for (;;) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    p.accumulate(x, free_mask, acc);
    if (PAR) wg_sum_n<K>(acc, tile);
    double H[N][N], g[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
      g[u] = acc[T + u];
#pragma unroll
      for (int v = 0; v <= u; ++v) { H[u][v] = acc[u * (u + 1) / 2 + v]; H[v][u] = H[u][v]; }
    }
    if (s.linearized(acc[T + N])) {                  // Jacobi scaling: iteration 0, frozen
#pragma unroll
      for (int c = 0; c < N; ++c) h0[c] = H[c][c];
    }
    double gnorm = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (!((free_mask >> c) & 1u)) continue;
      double e = g[c];
      if ((bound_mask >> c) & 1u) e = x[c] - box_clamp(p, c, x[c] - g[c]);      // projected gradient: x - P(x - g)
      gnorm = fmax(gnorm, fabs(e));
    }
    if (s.top(o, gnorm)) break;
    double dx[N], model;
    const bool ok = lm_damped_step<N>(H, g, h0, s.radius, free_mask, dx, model);
    if (!s.valid_step(ok, model)) { if (s.invalid_step()) break; continue; }
    double xc[M];
    if constexpr (P::kBox) {
      if (bounded) {
        // projected Armijo search along dx: f(P(x + t dx)) <= f(x) + 1e-4 t g.dx, t = 1 first; quadratic-interpolation contraction
        // clamped to [1e-3, 0.6] of the last step size; 20 samples, minimum step size 1e-9.  A failed search leaves dx as it is.
        double gd = 0.0;
#pragma unroll
        for (int c = 0; c < N; ++c)
          if ((free_mask >> c) & 1u) gd += g[c] * dx[c];
        if (gd < 0.0) {
          double t = 1.0;
          bool found = false;
          for (int sample = 0; sample < 20; ++sample) {
#pragma unroll
            for (int c = 0; c < N; ++c) xc[c] = x[c] + t * dx[c];
            project_box<N>(p, xc, bound_mask);
            const double ft = lm_cost<PAR>(p, xc, tile);
            if (ft <= s.cost + 1e-4 * t * gd) { found = true; break; }
            double tn = -gd * t * t / (2.0 * (ft - s.cost - gd * t));
            tn = fmin(fmax(tn, 1e-3 * t), 0.6 * t);
            ++contractions;
            if (tn < 1e-9) break;
            t = tn;
          }
          if (found) {
#pragma unroll
            for (int c = 0; c < N; ++c) dx[c] *= t;
          }
        }
      }
    }
    p.plus(x, dx, xc);
    if (bounded) project_box<M>(p, xc, bound_mask);
    double sn2 = 0.0, xn2 = 0.0;
#pragma unroll
    for (int c = 0; c < M; ++c) {
      if (!((norm_mask >> c) & 1u)) continue;
      sn2 += (xc[c] - x[c]) * (xc[c] - x[c]); xn2 += x[c] * x[c];
    }
    if (s.parameter_tol(o, sn2, xn2)) break;
    const double cand = lm_cost<PAR>(p, xc, tile);
    if (s.function_tol(o, cand)) break;
    if (s.accept(o, cand, model)) {
#pragma unroll
      for (int c = 0; c < M; ++c) x[c] = xc[c];
    }
  }
  if (s.failed()) {                                  // fail soft: the parameters stay where they were
#pragma unroll
    for (int c = 0; c < M; ++c) x[c] = x0[c];
  }
  s.fill(rec);
  rec.contractions = contractions;
}

}  // namespace lvf
