// small_lm.hpp — the declared Ceres trust-region loop for the solves that run whole inside ONE launch of one workgroup.  The rule itself is
// LmState (lm_rule.hpp), the one statement every device LM loop goes through; here are the loop around it and what the loop needs.  lm_small
// runs it for a compile-time number of unknowns: the GNSS alignment (navsat_kernels.hip), Relocator::UpdateNewSubmap's rotation
// (loop_kernels.hip), the pose-only refinement of the visual relocalisation (reloc_kernels.hip); k_pose_chain (pose_chain_kernels.hip) for a
// run-time number of poses.  Declared semantics: oracle/lm.h lm_solve (the order of the tests), oracle/robust.h (the loss, the damping); the box
// bounds: DESIGN.md "GNSS alignment".  Device code only; every array is indexed statically once the loops are unrolled (no scratch segment).
#pragma once
#include <cfloat>
#include <cmath>

#include "lm_rule.hpp"
#include "loop_dev.hpp"

namespace lvf {

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
