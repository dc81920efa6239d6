// pose_chain_kernels.hip — a chain of poses between two constant ends, solved on device (DESIGN.md "Pose chain"):
//
//   Navsat::OptimizeAB                                   src/lvio_fusion/src/navsat.cpp:271-307
//   the chain of PoseGraph::BuildProblem                 src/lvio_fusion/src/pose_graph.cpp:163-196
//   PoseGraphError <6,7,7>, RError <4,7>                 pose_error.hpp:10-53, :88-110  (prior_eval.hpp: the same code the window solver runs)
//   TError <3,7>                                         pose_error.hpp:112-130
//
// n poses, pose 0 and pose n-1 constant, m = n - 2 free poses of 6 tangent unknowns each (EigenQuaternionParameterization (+) Identity(3)).
// The normal equations are block tridiagonal: D_i (6 x 6) on the diagonal, O_i = the block in block-row i+1, block-column i.  The whole
// ceres::Solve is ONE launch of one workgroup of kLT threads over the trust-region rule of small_lm.hpp (LmState, the one lm_small runs; the
// restatements left outside it are named there).  What the chain brings: the sums, the block-tridiagonal solve, x (+) dx and the norms over
// a run-time m; Jacobi scaling frozen at iteration 0, a FAILURE leaves the poses as they came.  tests/pose_chain_ref.py restates it on the host.
//
// The linear solve is odd-even block cyclic reduction: level l (stride s = 2^l) eliminates the rows e = (2j+1) s - 1 at once — they are
// independent of one another — into their neighbours e - s and e + s, which form the next level's chain.  Operation for operation this is
// the Cholesky factorisation of the odd-even permuted matrix, so the reduced chains stay positive definite; depth floor(log2 m) + 1.
// A row of the working set is kRowW doubles: D | CL | CR | r.  An eliminated row keeps what the back substitution needs in place: the
// factor L of its pivot in D, L^-1 A[e][e-s] in CL, (L^-1 A[e][e+s])^T in CR, L^-1 r in r (then its solution).  A coupling always joins a
// row that is eliminated at this level to one that is kept, and is stored with the eliminated one; the coupling a level creates between two
// kept rows goes to whichever of them the next level eliminates, whose slots are still unused.  No floating-point atomics anywhere: every
// sum has one owner thread and a fixed order, so two runs are bit-equal.
#include "prior_eval.hpp"
#include "small_lm.hpp"

namespace lvf {

constexpr int kChainCapacity = 1022;                 // free poses
constexpr int kRowW = 114;                           // D 36 | CL 36 | CR 36 | r 6
constexpr int kChainLdsRows = 120;                   // the working set stays in LDS up to here (120 * 114 * 8 = 109440 bytes), else the workspace
constexpr int kEdgeW = 120;                          // J_a^T J_a 36 | J_b^T J_b 36 | J_b^T J_a 36 | J_a^T r 6 | J_b^T r 6
constexpr int kRowsPerRound = kLT / 6;               // six threads per eliminated row, a row never split between two rounds

struct ChainRec { LmRec lm; double model; int fail, pad; };

struct ChainArgs {
  int n, m;
  int mode;                  // 0: the solve; 1: one linearisation + one damped solve at `radius`; 2: one linearisation
  int targets_from_poses;    // edge targets = PoseGraphError(last_pose, pose) of the poses as they come
  int navsat;                // Navsat::OptimizeAB's set-up: weights, fix z interpolated, last edge from relative_B
  double huber_a, radius;
  LmOpts o;
  const double* in;          // [n][7]
  double *X, *XC;            // [n][7] the iterate and the candidate
  double *tg, *ew, *ev;      // edges: [n-1][6], [n-1], [n-1]
  int* kind;                 // [n]
  double *ut, *uw;           // unaries: [n][4], [n]
  const double *stamps, *relB;
  double *E;                 // [n-1][kEdgeW]
  double *D, *O, *g;         // the undamped system: [m][36], [m][36] (m - 1 used), [6 m]
  double *h0, *dx;           // [6 m]; [6 m]: the step of mode 1
  double* W;                 // [m][kRowW] when the working set is not in LDS
  ChainRec* rec;
};

// rows [6][7] of an ambient Jacobian -> [6][6] local: the quaternion columns through the plus-Jacobian at q, the translation columns as they are
__device__ __forceinline__ void rows_to_local(const double* J7, const double* q, double* L) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    quat_row_to_local(J7 + 7 * r, q, L + 6 * r);
    L[6 * r + 3] = J7[7 * r + 4]; L[6 * r + 4] = J7[7 * r + 5]; L[6 * r + 5] = J7[7 * r + 6];
  }
}

// the unary block of pose p: adds its J^T J into Dl, J^T r into gl (rho' applied) and returns 1/2 rho
template <bool WITH_J>
__device__ __forceinline__ double chain_unary(const ChainArgs& a, const double* X, int p, double* Dl, double* gl) {
  const int kind = a.kind[p];
  const double w = a.uw[p];
  if (kind == LVF_CHAIN_T) {
    double r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = w * (X[7 * p + 4 + k] - a.ut[4 * p + k]);
    double rho0, rho1;
    huber_eval(a.huber_a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho0, rho1);
    if (WITH_J) {
      const double sc = sqrt(rho1), l = sc * w;      // Corrector, rho'' <= 0
#pragma unroll
      for (int k = 0; k < 3; ++k) { Dl[7 * (3 + k)] += l * l; gl[3 + k] += l * (sc * r[k]); }
    }
    return 0.5 * rho0;
  }
  if (kind == LVF_CHAIN_R) {
    double res[6], ja[42], jb[42];
    pose_prior_eval<WITH_J>(-2, p, a.ut + 4 * p, w, 0.0, X, res, ja, jb);
    if (WITH_J) {
      double l3[4][3];
#pragma unroll
      for (int r = 0; r < 4; ++r) quat_row_to_local(jb + 7 * r, X + 7 * p, l3[r]);
#pragma unroll
      for (int u = 0; u < 3; ++u) {
#pragma unroll
        for (int v = 0; v < 3; ++v) Dl[6 * u + v] += ((l3[0][u] * l3[0][v] + l3[1][u] * l3[1][v]) + l3[2][u] * l3[2][v]) + l3[3][u] * l3[3][v];
        gl[u] += ((l3[0][u] * res[0] + l3[1][u] * res[1]) + l3[2][u] * res[2]) + l3[3][u] * res[3];
      }
    }
    return 0.5 * (((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]) + res[3] * res[3]);
  }
  return 0.0;
}

// 1/2 sum rho at the poses X: every thread sums the blocks it owns (edges first, then unaries), then the workgroup
__device__ __forceinline__ double chain_cost(const ChainArgs& a, const double* X, double* tile) {
  double c = 0.0;
  for (int k = threadIdx.x; k < a.n - 1; k += kLT) {
    double res[6];
    pose_prior_eval<false>(k, k + 1, a.tg + 6 * k, a.ew[k], a.ev[k], X, res, nullptr, nullptr);
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += res[r] * res[r];
    c += 0.5 * s;
  }
  for (int f = threadIdx.x; f < a.m; f += kLT) c += chain_unary<false>(a, X, f + 1, nullptr, nullptr);
  return wg_sum(c, tile);
}

// One linearisation at X.  One thread per edge leaves the five products of its projected Jacobians; then one thread per free pose forms
// D_f = unary + edge(p-1).bb + edge(p).aa, O_f = edge(p).ba and g_f likewise (p = f + 1), in that order, keeps them (the model decrease uses the
// undamped blocks) and writes its row of the working set while it holds them: D + the clamped damping term (on the Jacobi-scaled diagonal,
// divided by the radius), r = -g, and, for the rows level 0 eliminates (the even ones), the couplings with both neighbours.  `first`: the
// Jacobi scaling h0 is this linearisation's diagonal.  Returns the cost; gnorm = max |g|.
__device__ __forceinline__ double chain_linearize(const ChainArgs& a, const double* X, double* W, double radius, bool first, double* tile, double& gnorm) {
  double cost = 0.0, gn = 0.0;
  for (int k = threadIdx.x; k < a.n - 1; k += kLT) {
    double res[6], La[36], Lb[36];
    {
      double ja[42], jb[42];
      pose_prior_eval<true>(k, k + 1, a.tg + 6 * k, a.ew[k], a.ev[k], X, res, ja, jb);
      rows_to_local(ja, X + 7 * k, La);
      rows_to_local(jb, X + 7 * (k + 1), Lb);
    }
    double* e = a.E + (size_t)kEdgeW * k;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
#pragma unroll
      for (int v = 0; v < 6; ++v) {
        double saa = 0.0, sbb = 0.0, sba = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) { saa += La[6 * r + u] * La[6 * r + v]; sbb += Lb[6 * r + u] * Lb[6 * r + v]; sba += Lb[6 * r + u] * La[6 * r + v]; }
        e[6 * u + v] = saa; e[36 + 6 * u + v] = sbb; e[72 + 6 * u + v] = sba;
      }
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) { sa += La[6 * r + u] * res[r]; sb += Lb[6 * r + u] * res[r]; }
      e[108 + u] = sa; e[114 + u] = sb;
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += res[r] * res[r];
    cost += 0.5 * s;
  }
  __syncthreads();
  const int m = a.m;
  for (int f = threadIdx.x; f < m; f += kLT) {
    const int p = f + 1;
    double Dl[36], gl[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) Dl[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) gl[i] = 0.0;
    cost += chain_unary<true>(a, X, p, Dl, gl);
    const double* eb = a.E + (size_t)kEdgeW * (p - 1);      // pose p is the edge's second pose
    const double* ea = a.E + (size_t)kEdgeW * p;            // pose p is the edge's first pose
    double* row = W + (size_t)kRowW * f;
    const bool elim = !(f & 1), left = elim && f >= 1, right = elim && f + 1 < m;
#pragma unroll
    for (int i = 0; i < 36; ++i) {
      Dl[i] = (Dl[i] + eb[36 + i]) + ea[i];
      a.D[36 * (size_t)f + i] = Dl[i];
      const double o = ea[72 + i];
      if (f + 1 < m) a.O[36 * (size_t)f + i] = o;
      row[36 + i] = left ? eb[72 + i] : 0.0;               // A[f][f-1]
      row[72 + i] = right ? o : 0.0;                       // A[f+1][f]
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double g = (gl[c] + eb[114 + c]) + ea[108 + c];
      a.g[6 * f + c] = g;
      gn = fmax(gn, fabs(g));
      row[108 + c] = -g;
      double h = Dl[7 * c];
      if (first) a.h0[6 * f + c] = h;
      else h = a.h0[6 * f + c];
      Dl[7 * c] += lm_damping(Dl[7 * c], h) / radius;
    }
#pragma unroll
    for (int i = 0; i < 36; ++i) row[i] = Dl[i];
  }
  gnorm = wg_max(gn, tile);
  return wg_sum(cost, tile);
}

// Factorisation and both substitutions on the working set.  *fail is raised when a pivot is not positive (or is NaN): the caller then takes
// dx = 0.  Nothing traps: the arithmetic runs on and its result is not used.
__device__ __forceinline__ void chain_reduce(int m, double* W, int* fail) {
  const int tid = threadIdx.x;
  int s = 1;
  for (; s <= m; s <<= 1) {
    const int nE = (m / s + 1) / 2, nK = (m / s) / 2;
    // the eliminated rows: thread (row, c) factors the pivot and solves column c against both couplings; thread (row, 0) also the right-hand side
    for (int base = 0; base < nE; base += kRowsPerRound) {
      const int j = base + tid / 6, c = tid % 6;
      const bool act = tid < 6 * kRowsPerRound && j < nE;
      double* row = W + (size_t)kRowW * (act ? (2 * j + 1) * s - 1 : 0);
      double L[21], u[6], w[6], y[6];
      if (act) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int k = 0; k <= i; ++k) L[i * (i + 1) / 2 + k] = row[6 * i + k];
          u[i] = row[36 + 6 * i + c]; w[i] = row[72 + 6 * c + i]; y[i] = row[108 + i];
        }
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) {
          double d = L[jj * (jj + 1) / 2 + jj];
#pragma unroll
          for (int k = 0; k < jj; ++k) d -= L[jj * (jj + 1) / 2 + k] * L[jj * (jj + 1) / 2 + k];
          ok = ok && (d > 0.0);
          const double l = sqrt(d);
          L[jj * (jj + 1) / 2 + jj] = l;
#pragma unroll
          for (int i = jj + 1; i < 6; ++i) {
            double t = L[i * (i + 1) / 2 + jj];
#pragma unroll
            for (int k = 0; k < jj; ++k) t -= L[i * (i + 1) / 2 + k] * L[jj * (jj + 1) / 2 + k];
            L[i * (i + 1) / 2 + jj] = t / l;
          }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double tu = u[i], tw = w[i], ty = y[i];
#pragma unroll
          for (int k = 0; k < i; ++k) { tu -= L[i * (i + 1) / 2 + k] * u[k]; tw -= L[i * (i + 1) / 2 + k] * w[k]; ty -= L[i * (i + 1) / 2 + k] * y[k]; }
          u[i] = tu / L[i * (i + 1) / 2 + i]; w[i] = tw / L[i * (i + 1) / 2 + i]; y[i] = ty / L[i * (i + 1) / 2 + i];
        }
        if (!ok) *fail = 1;
      }
      __syncthreads();                               // every thread of the row has read D, r and its part of the couplings
      if (act) {
#pragma unroll
        for (int i = 0; i < 6; ++i) { row[36 + 6 * i + c] = u[i]; row[72 + 6 * c + i] = w[i]; }
        if (c == 0) {
#pragma unroll
          for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int k = 0; k <= i; ++k) row[6 * i + k] = L[i * (i + 1) / 2 + k];
            row[108 + i] = y[i];
          }
        }
      }
    }
    __syncthreads();
    // the kept rows: thread (row, c) takes column c of the Schur updates from the left neighbour, then the right one, and of the new coupling
    for (int idx = tid; idx < 6 * nK; idx += kLT) {
      const int j = idx / 6, c = idx - 6 * j, k = (2 * j + 2) * s - 1;
      double* row = W + (size_t)kRowW * k;
      const double* rl = W + (size_t)kRowW * (k - s);
      double dl[6], rc = row[108 + c];
#pragma unroll
      for (int i = 0; i < 6; ++i) dl[i] = row[6 * i + c];
      {
        double uc[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) uc[q] = rl[72 + 6 * c + q];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) t += rl[72 + 6 * i + q] * uc[q];
          dl[i] -= t;
        }
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) t += uc[q] * rl[108 + q];
        rc -= t;
      }
      if (k + s < m) {
        const double* rr = W + (size_t)kRowW * (k + s);
        double uc[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) uc[q] = rr[36 + 6 * q + c];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) t += rr[36 + 6 * q + i] * uc[q];
          dl[i] -= t;
        }
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) t += uc[q] * rr[108 + q];
        rc -= t;
        if (k + 2 * s < m) {                         // A[k+2s][k] = -(L^-1 A[e][k+2s])^T (L^-1 A[e][k]), stored with the row the next level eliminates
          double* dst = (((k + 1) / (2 * s)) & 1) ? row + 72 : W + (size_t)kRowW * (k + 2 * s) + 36;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            double t2 = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) t2 += rr[72 + 6 * i + q] * uc[q];
            dst[6 * i + c] = -t2;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) row[6 * i + c] = dl[i];
      row[108 + c] = rc;
    }
    __syncthreads();
  }
  // back substitution, level by level in reverse: x_e = L^-T (y_e - U_left x_{e-s} - U_right x_{e+s}), one thread per row
  for (s >>= 1; s >= 1; s >>= 1) {
    const int nE = (m / s + 1) / 2;
    for (int j = tid; j < nE; j += kLT) {
      const int e = (2 * j + 1) * s - 1;
      double* row = W + (size_t)kRowW * e;
      double t[6], x[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) t[i] = row[108 + i];
      if (e - s >= 0) {
        const double* xp = W + (size_t)kRowW * (e - s) + 108;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int q = 0; q < 6; ++q) t[i] -= row[36 + 6 * i + q] * xp[q];
        }
      }
      if (e + s < m) {
        const double* xq = W + (size_t)kRowW * (e + s) + 108;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int q = 0; q < 6; ++q) t[i] -= row[72 + 6 * q + i] * xq[q];
        }
      }
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double v = t[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= row[6 * k + i] * x[k];
        x[i] = v / row[6 * i + i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) row[108 + i] = x[i];
    }
    __syncthreads();
  }
}

// -dx.(g + H dx / 2) on the undamped blocks; dx is where the back substitution left it (the r slots)
__device__ __forceinline__ double chain_model(const ChainArgs& a, const double* W, double* tile) {
  double part = 0.0;
  for (int f = threadIdx.x; f < a.m; f += kLT) {
    const double* D = a.D + 36 * (size_t)f;
    double x[6], hd[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = W[(size_t)kRowW * f + 108 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) t += D[6 * i + q] * x[q];
      hd[i] = t;
    }
    if (f >= 1) {
      const double* O = a.O + 36 * (size_t)(f - 1);
      const double* xl = W + (size_t)kRowW * (f - 1) + 108;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int q = 0; q < 6; ++q) hd[i] += O[6 * i + q] * xl[q];
      }
    }
    if (f + 1 < a.m) {
      const double* O = a.O + 36 * (size_t)f;
      const double* xr = W + (size_t)kRowW * (f + 1) + 108;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int q = 0; q < 6; ++q) hd[i] += O[6 * q + i] * xr[q];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) part -= x[i] * (a.g[6 * f + i] + 0.5 * hd[i]);
  }
  return wg_sum(part, tile);
}

// The damped solve of the system chain_linearize left in W, and the model decrease of its step; `failed`: a pivot was not positive, dx = 0
__device__ __forceinline__ double chain_step(const ChainArgs& a, double* W, int* s_fail, double* tile, int& failed) {
  chain_reduce(a.m, W, s_fail);
  failed = *s_fail;
  __syncthreads();                                   // every thread has read the flag
  if (threadIdx.x == 0) *s_fail = 0;
  return failed ? 0.0 : chain_model(a, W, tile);
}

template <bool IN_LDS>
__global__ __launch_bounds__(kLT) void k_pose_chain(ChainArgs a) {
  extern __shared__ double chain_lds[];
  __shared__ double tile[kLT / 64];
  __shared__ int s_fail;
  const int tid = threadIdx.x, n = a.n, m = a.m;
  double* W = IN_LDS ? chain_lds : a.W;
  // ---- set-up ----
  for (int i = tid; i < 7 * n; i += kLT) { const double v = a.in[i]; a.X[i] = v; a.XC[i] = v; }
  if (a.navsat) {
    const double tA = a.stamps[0], tB = a.stamps[n - 1], zA = a.in[6], zB = a.in[7 * (n - 1) + 6];
    for (int i = tid; i < n; i += kLT) {
      const bool fr = i >= 1 && i + 1 < n;
      a.kind[i] = fr ? LVF_CHAIN_T : LVF_CHAIN_NONE;
      a.uw[i] = 1.0;
      if (fr) {
        const double al = (a.stamps[i] - tA) / (tB - tA);
        a.ut[4 * i + 2] = al * zB + (1.0 - al) * zA;                        // navsat.cpp:288-290
      }
      if (i + 1 < n) { a.ew[i] = i + 2 < n ? 1.0 : 10.0; a.ev[i] = 20.0; }    // navsat.cpp:294, :300
    }
  }
  if (a.targets_from_poses) {
    typedef DJet<1> S;                               // (the value path of the dual-number helpers)
    for (int k = tid; k < n - 1; k += kLT) {
      S rel[7], rp[6];
      if (a.navsat && k == n - 2) {
#pragma unroll
        for (int c = 0; c < 7; ++c) rel[c] = S(a.relB[c]);
      } else {
        S T1[7], T2[7], inv1[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) { T1[c] = S(a.in[7 * k + c]); T2[c] = S(a.in[7 * (k + 1) + c]); }
        se3_inverse(T1, inv1);
        se3_product(inv1, T2, rel);
      }
      se3_to_rpyxyz(rel, rp);
#pragma unroll
      for (int c = 0; c < 6; ++c) a.tg[6 * k + c] = rp[c].a;
    }
  }
  if (tid == 0) s_fail = 0;
  __syncthreads();

  // mode 2 is one linearisation, mode 1 one linearisation and one damped solve at a.radius, mode 0 the loop; all three end the same way
  const LmOpts& o = a.o;
  LmState s(a.mode == 1 ? a.radius : o.radius0);
  double model = 0.0, gn;
  int failed = 0;
  double *Xp = a.X, *Xc = a.XC;
  if (m == 0) s.linearized(chain_cost(a, a.X, tile));       // no free pose: the problem has a cost and no unknown
  else if (a.mode != 0) {
    s.linearized(chain_linearize(a, Xp, W, s.radius, true, tile, gn));
    if (a.mode == 1) {
      model = chain_step(a, W, &s_fail, tile, failed);
      for (int f = tid; f < m; f += kLT) {
#pragma unroll
        for (int c = 0; c < 6; ++c) a.dx[6 * f + c] = failed ? 0.0 : W[(size_t)kRowW * f + 108 + c];
      }
    }
  } else for (;;) {
    s.linearized(chain_linearize(a, Xp, W, s.radius, s.first, tile, gn));      // (Jacobi scaling: iteration 0, frozen)
    if (s.top(o, gn)) break;
    model = chain_step(a, W, &s_fail, tile, failed);
    if (!s.valid_step(!failed, model)) { if (s.invalid_step()) break; continue; }
    double sn2 = 0.0, xn2 = 0.0;                     // over the ambient coordinates of the free poses
    for (int f = tid; f < m; f += kLT) {
      const double* x = Xp + 7 * (f + 1);
      double dl[6], xc[7];
#pragma unroll
      for (int c = 0; c < 6; ++c) dl[c] = W[(size_t)kRowW * f + 108 + c];
      pose_plus(x, dl, xc);
#pragma unroll
      for (int c = 0; c < 7; ++c) { Xc[7 * (f + 1) + c] = xc[c]; sn2 += (xc[c] - x[c]) * (xc[c] - x[c]); xn2 += x[c] * x[c]; }
    }
    sn2 = wg_sum(sn2, tile); xn2 = wg_sum(xn2, tile);
    if (s.parameter_tol(o, sn2, xn2)) break;
    const double cand = chain_cost(a, Xc, tile);
    if (s.function_tol(o, cand)) break;
    if (s.accept(o, cand, model)) { double* t2 = Xp; Xp = Xc; Xc = t2; }      // the candidate becomes the iterate (the constant ends are in both)
  }
  const double* out = s.failed() ? a.in : Xp;        // fail soft: the poses stay as they came
  if (out != a.X) {                                  // the host reads a.X
    for (int i = tid; i < n; i += kLT) {
#pragma unroll
      for (int c = 0; c < 7; ++c) a.X[7 * i + c] = out[7 * i + c];
    }
  }
  if (tid == 0) {
    s.fill(a.rec->lm);
    a.rec->model = model; a.rec->fail = failed; a.rec->pad = 0;
  }
}

}  // namespace lvf

using namespace lvf;

namespace {

struct ChainProblem {
  int n;
  const double *poses, *tg, *ew, *ev, *ut, *uw;
  const int32_t* kind;
  const double *stamps, *fix, *relB;      // Navsat::OptimizeAB's inputs (then tg .. kind are null)
  double huber_a;
};

// device buffers of one call; everything a launch reads or writes
struct ChainRun {
  DevBuf<double> in, work;
  DevBuf<int> kind;
  DevBuf<ChainRec> rec;
  ChainArgs a{};
};

int chain_check(const char* who, lvf_ctx* ctx, const ChainProblem& p) {
  LVF_REQUIRE(ctx && p.poses, "%s: null argument", who);
  LVF_REQUIRE(p.n >= 2, "%s: a chain has at least its two constant ends (n = %d)", who, p.n);
  LVF_REQUIRE(p.n - 2 <= kChainCapacity, "%s: %d free poses, the capacity is %d (lvf_pose_chain_capacity)", who, p.n - 2, kChainCapacity);
  if (p.stamps) {
    LVF_REQUIRE(p.fix && p.relB, "%s: null argument", who);
    LVF_REQUIRE(p.n == 2 || p.stamps[p.n - 1] != p.stamps[0], "%s: A and B have the same stamp", who);
  } else {
    LVF_REQUIRE(p.ew && p.ev, "%s: null edge arrays", who);
    LVF_REQUIRE(p.n == 2 || (p.kind && p.ut && p.uw), "%s: null unary arrays", who);
    for (int i = 1; i + 1 < p.n; ++i)
      LVF_REQUIRE(p.kind[i] >= LVF_CHAIN_NONE && p.kind[i] <= LVF_CHAIN_R, "%s: unary_kind[%d] = %d", who, i, p.kind[i]);
  }
  for (int i = 0; i < p.n; ++i) {
    const double* q = p.poses + (size_t)7 * i;
    LVF_REQUIRE(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0, "%s: zero quaternion (pose %d)", who, i);
  }
  return LVF_OK;
}

// uploads the problem, lays out the workspace and launches; the caller downloads what it wants and waits
int chain_launch(lvf_ctx* ctx, const ChainProblem& p, int mode, double radius, const lvf_solver_options* o, ChainRun& run) {
  const int n = p.n, m = n - 2;
  hipStream_t s = ctx->stream;
  ChainArgs& a = run.a;
  a.n = n; a.m = m; a.mode = mode; a.targets_from_poses = p.stamps || !p.tg; a.navsat = p.stamps != nullptr; a.huber_a = p.huber_a; a.radius = radius;
  if (o) a.o = LmOpts{o->max_num_iterations, o->function_tolerance, o->gradient_tolerance, o->parameter_tolerance, o->min_relative_decrease, o->initial_trust_region_radius};
  else a.o = LmOpts{0, 0.0, 0.0, 0.0, 0.0, radius};
  // inputs, one upload: poses 7n | targets 6(n-1) | ew n-1 | ev n-1 | ut 4n | uw n | stamps n | relative_B 7
  const size_t o_tg = (size_t)7 * n, o_ew = o_tg + (size_t)6 * (n - 1), o_ev = o_ew + (n - 1), o_ut = o_ev + (n - 1), o_uw = o_ut + (size_t)4 * n, o_st = o_uw + n,
               o_rb = o_st + n, n_in = o_rb + 7;
  std::vector<double> h(n_in, 0.0);
  std::memcpy(h.data(), p.poses, sizeof(double) * 7 * n);
  std::vector<int32_t> hk(n, LVF_CHAIN_NONE);
  if (p.stamps) {
    for (int i = 1; i + 1 < n; ++i) std::memcpy(h.data() + o_ut + 4 * i, p.fix + 3 * i, sizeof(double) * 3);
    std::memcpy(h.data() + o_st, p.stamps, sizeof(double) * n);
    std::memcpy(h.data() + o_rb, p.relB, sizeof(double) * 7);
  } else {
    if (p.tg) std::memcpy(h.data() + o_tg, p.tg, sizeof(double) * 6 * (n - 1));
    std::memcpy(h.data() + o_ew, p.ew, sizeof(double) * (n - 1));
    std::memcpy(h.data() + o_ev, p.ev, sizeof(double) * (n - 1));
    for (int i = 1; i + 1 < n; ++i) {
      hk[i] = p.kind[i];
      if (hk[i] != LVF_CHAIN_NONE) { std::memcpy(h.data() + o_ut + 4 * i, p.ut + 4 * i, sizeof(double) * 4); h[o_uw + i] = p.uw[i]; }
    }
  }
  LVF_TRY(run.in.upload(h.data(), n_in, s));
  LVF_TRY(run.kind.upload(hk.data(), (size_t)n, s));
  LVF_TRY(run.rec.alloc(1));
  const bool in_lds = m <= kChainLdsRows;
  // workspace: X 7n | XC 7n | E | D 36m | O 36m | g 6m | h0 6m | dx 6m | W
  const size_t mm = (size_t)std::max(m, 1);
  const size_t w_x = 0, w_xc = w_x + (size_t)7 * n, w_e = w_xc + (size_t)7 * n, w_d = w_e + (size_t)kEdgeW * (n - 1), w_o = w_d + 36 * mm, w_g = w_o + 36 * mm,
               w_h = w_g + 6 * mm, w_dx = w_h + 6 * mm, w_w = w_dx + 6 * mm, n_work = w_w + (in_lds ? 0 : (size_t)kRowW * mm);
  LVF_TRY(run.work.alloc(n_work));
  double *I = run.in.p, *Wk = run.work.p;
  a.in = I; a.tg = I + o_tg; a.ew = I + o_ew; a.ev = I + o_ev; a.ut = I + o_ut; a.uw = I + o_uw; a.stamps = I + o_st; a.relB = I + o_rb; a.kind = run.kind.p;
  a.X = Wk + w_x; a.XC = Wk + w_xc; a.E = Wk + w_e; a.D = Wk + w_d; a.O = Wk + w_o; a.g = Wk + w_g; a.h0 = Wk + w_h; a.dx = Wk + w_dx;
  a.W = in_lds ? nullptr : Wk + w_w;
  a.rec = run.rec.p;
  if (in_lds) {
    const size_t lds = sizeof(double) * kRowW * mm;
    if (lds > 48 * 1024) LVF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pose_chain<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_pose_chain<true>, dim3(1), dim3(kLT), lds, s, a);
  } else {
    hipLaunchKernelGGL(k_pose_chain<false>, dim3(1), dim3(kLT), 0, s, a);
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

int chain_blocks(const ChainProblem& p) {
  int nb = p.n - 1;
  for (int i = 1; i + 1 < p.n; ++i) nb += p.stamps ? 1 : p.kind[i] != LVF_CHAIN_NONE;
  return nb;
}

int chain_solve(const char* who, lvf_ctx* ctx, const ChainProblem& p, double* poses7, const lvf_solver_options* o, lvf_solver_summary* summary) {
  LVF_REQUIRE(o && summary, "%s: null argument", who);
  LVF_TRY(chain_check(who, ctx, p));
  LVF_TRY(lvf::enter(ctx));
  ChainRun run;
  LVF_TRY(chain_launch(ctx, p, 0, 0.0, o, run));
  LVF_HIP(hipMemcpyAsync(poses7, run.a.X, sizeof(double) * 7 * p.n, hipMemcpyDeviceToHost, ctx->stream));      // one download: the poses and the record
  ChainRec h;
  LVF_TRY(lvf::read_back(ctx, &h, run.rec.p, sizeof(h)));
  std::memset(summary, 0, sizeof(*summary));
  summary->initial_cost = h.lm.initial_cost; summary->final_cost = h.lm.final_cost; summary->num_iterations = h.lm.iters;
  summary->num_successful_steps = h.lm.successes; summary->num_unsuccessful_steps = h.lm.iters - h.lm.successes; summary->num_residual_blocks = chain_blocks(p);
  summary->termination = h.lm.termination; summary->termination_reason = h.lm.why;
  return LVF_OK;
}

}  // namespace

extern "C" {

int lvf_pose_chain_capacity(void) { return kChainCapacity; }

int lvf_pose_chain_solve(lvf_ctx* ctx, int n, double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v, const int32_t* unary_kind,
                         const double* unary_target4, const double* unary_weight, double huber_a, const lvf_solver_options* o, lvf_solver_summary* summary) {
  const ChainProblem p{n, poses7, edge_target6, edge_weight, edge_v, unary_target4, unary_weight, unary_kind, nullptr, nullptr, nullptr, huber_a};
  return chain_solve("lvf_pose_chain_solve", ctx, p, poses7, o, summary);
}

int lvf_navsat_optimize_ab(lvf_ctx* ctx, int n, double* poses7, const double* stamps, const double* fix_point, const double* relative_B7, double huber_a,
                           const lvf_solver_options* o, lvf_solver_summary* summary) {
  LVF_REQUIRE(stamps, "lvf_navsat_optimize_ab: null argument");
  const ChainProblem p{n, poses7, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stamps, fix_point, relative_B7, huber_a};
  return chain_solve("lvf_navsat_optimize_ab", ctx, p, poses7, o, summary);
}

int lvf_pose_chain_debug_step(lvf_ctx* ctx, int n, const double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v,
                              const int32_t* unary_kind, const double* unary_target4, const double* unary_weight, double huber_a, double radius, double* dx,
                              double* model, double* cost, int32_t* fail) {
  const ChainProblem p{n, poses7, edge_target6, edge_weight, edge_v, unary_target4, unary_weight, unary_kind, nullptr, nullptr, nullptr, huber_a};
  LVF_REQUIRE(model && cost && fail && (n <= 2 || dx), "lvf_pose_chain_debug_step: null argument");
  LVF_REQUIRE(radius > 0.0, "lvf_pose_chain_debug_step: radius must be > 0");
  LVF_TRY(chain_check("lvf_pose_chain_debug_step", ctx, p));
  LVF_TRY(lvf::enter(ctx));
  ChainRun run;
  LVF_TRY(chain_launch(ctx, p, 1, radius, nullptr, run));
  if (n > 2) LVF_HIP(hipMemcpyAsync(dx, run.a.dx, sizeof(double) * 6 * (n - 2), hipMemcpyDeviceToHost, ctx->stream));
  ChainRec h;
  LVF_TRY(lvf::read_back(ctx, &h, run.rec.p, sizeof(h)));
  *model = h.model; *cost = h.lm.final_cost; *fail = h.fail;
  return LVF_OK;
}

int lvf_pose_chain_debug_system(lvf_ctx* ctx, int n, const double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v,
                                const int32_t* unary_kind, const double* unary_target4, const double* unary_weight, double huber_a, double* D, double* O,
                                double* g) {
  const ChainProblem p{n, poses7, edge_target6, edge_weight, edge_v, unary_target4, unary_weight, unary_kind, nullptr, nullptr, nullptr, huber_a};
  LVF_REQUIRE(n <= 2 || (D && g && (n == 3 || O)), "lvf_pose_chain_debug_system: null argument");
  LVF_TRY(chain_check("lvf_pose_chain_debug_system", ctx, p));
  LVF_TRY(lvf::enter(ctx));
  ChainRun run;
  LVF_TRY(chain_launch(ctx, p, 2, 1.0, nullptr, run));
  const int m = n - 2;
  if (m > 0) {
    LVF_HIP(hipMemcpyAsync(D, run.a.D, sizeof(double) * 36 * m, hipMemcpyDeviceToHost, ctx->stream));
    LVF_HIP(hipMemcpyAsync(g, run.a.g, sizeof(double) * 6 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (m > 1) LVF_HIP(hipMemcpyAsync(O, run.a.O, sizeof(double) * 36 * (m - 1), hipMemcpyDeviceToHost, ctx->stream));
  }
  LVF_HIP(hipStreamSynchronize(ctx->stream));
  return LVF_OK;
}

}  // extern "C"
