// marginal_kernels.hip — marginal information and covariance of a few selected unknowns of a reduced (Schur) system S over the keyframe
// unknowns (lvf_marginal_dense, lvf_problem_marginal; lvf_window_marginal in window.hip calls the latter):
//     info = S_ss - S_sr S_rr^-1 S_rs,     cov = info^-1 = (S^-1)_ss          (s = the selection, r = the rest)
// No right-hand sides are solved.  The unknowns are ordered [rest | padding to a multiple of 64 | selection] in a workspace of the call's
// own, the production block step (k_chol_step, solver_chol.hip: nothing of it is changed) eliminates the rest one 64-column launch at a time,
// and what is left in the trailing block is `info`; one workgroup then factors that block in LDS, inverts the triangle and forms L^-T L^-1.
//
// Absent unknowns (an identically zero Jacobian column: a constant pose, a (v, ba, bg) block no ImuError factor touches; detected EXACTLY, as a
// zero on the undamped diagonal) stay where the order puts them but as identity rows, like the padding: they take no part in anything and
// their rows / columns of both outputs are zero (ceres::Covariance's convention for constant blocks).
//
// The block step's trailing update lags its panel by one launch (chol_step_body: launch kb applies the update of column kb - 1), so after
// the last launch the update of the LAST rest column onto the selected block is still pending: k_marg_tail_update applies it with the same
// tile product (chol_update_tile).  A non-positive or NaN pivot raises the failure flag (1 + kb, atomicMax); the flag is also every launch's
// `done` gate, so whatever is enqueued behind a failed step returns at once.  Nothing here waits on another workgroup.
//
// lvf_problem_marginal_prior carries the reduced right-hand side along as one more row behind the selection — [rest | padding | selection |
// rhs] — so the same block steps leave, beside `info`, the information vector eta = g_s - H_sr H_rr^-1 g_r in that row and -g_r^T H_rr^-1 g_r
// on its diagonal (gathered as 0: the 1e300 the production system keeps there would swallow it).  No covariance is formed there, so a
// singular selected block is no failure (k_marg_prior_finish).
#include <vector>

#include "solver_dev.hpp"
#include "solver_host.hpp"

namespace lvf {

constexpr int kMargT = 256, kMargFT = 512, kMargMaxSel = 120;
constexpr double kMargRadius = 1e300;     // "undamped": see lvf_problem_marginal

// ---- gather: workspace W [ld x ld] (lower triangle; the rest is cleared) = S through the order `src` (workspace row -> natural unknown, -1 =
// padding).  S is read at row rowmap[u] (null: u) with leading dimension lds, lower triangle only; unknown u is absent iff diag[u * dstride] == 0.
// Kept aside per workspace row: the diagonal as gathered (diag0, for the pivot ratios) and the presence flag.  One workgroup per row.
struct MargGather {
  GP<const double> S; int lds; GP<const int> rowmap; GP<const double> diag; size_t dstride;
  GP<const int> src; int ld; GP<double> W, diag0; GP<int> pres, fail;
  int aug_row;      // src == -2: the right-hand-side row, read from row aug_row of S (lvf_problem_marginal_prior)
};
__global__ __launch_bounds__(kMargT) void k_marg_gather(MargGather a) {
  const int r = blockIdx.x;
  const int ua = a.src[r];
  const bool rhs = ua == -2;
  const bool pa = rhs || (ua >= 0 && a.diag[(size_t)ua * a.dstride] != 0.0);      // (a NaN diagonal is present: its pivot then fails)
  const size_t ra = rhs ? (size_t)a.aug_row : pa ? (size_t)(a.rowmap ? a.rowmap[ua] : ua) : 0;
  double* row = a.W + (size_t)r * a.ld;
  for (int c = threadIdx.x; c < a.ld; c += kMargT) {
    double v = 0.0;
    if (c == r) {
      v = rhs ? 0.0 : pa ? a.S[ra * a.lds + ra] : 1.0;
      a.diag0[r] = v; a.pres[r] = (pa && !rhs) ? 1 : 0;
    } else if (c < r && pa) {
      const int ub = a.src[c];
      if (ub >= 0 && a.diag[(size_t)ub * a.dstride] != 0.0) {
        const size_t rb = (size_t)(a.rowmap ? a.rowmap[ub] : ub);
        v = a.S[max(ra, rb) * a.lds + min(ra, rb)];
      }
    }
    row[c] = v;
  }
  if (r == 0 && threadIdx.x == 0) *a.fail = 0;
}

// ---- the pending update of the last rest column (block nr - 1) onto the tiles of the selected block, lower tiles only: one workgroup per tile
__global__ __launch_bounds__(kCT) void k_marg_tail_update(GP<double> W, int ld, int nr, GP<const int> fail) {
  if (done_flag_issue(fail)) return;                  // (workgroup-uniform)
  int t = blockIdx.x, ii = 0;
  while (t >= ii + 1) { t -= ii + 1; ++ii; }
  const PanelLds PL = panel_lds();
  chol_update_tile(W, ld, nr - 1, nr + ii, nr + t, PL.Pi, PL.Pj);
}

// ---- finish: ONE workgroup.  The m x m trailing block (rows / columns from R = 64 nr) is `info`; it is factored in LDS (right-looking, one
// column per step), the triangle inverted in place row by row, cov = L^-T L^-1 formed from it.  Row i of both outputs belongs to sel[i] (the
// selection sits in the workspace in the caller's order).  out = info [m x m] | cov [m x m] | {fail, n_present, n_absent, min_pivot_ratio}.
struct MargFinish {
  GP<const double> W; int ld, R, nr, m, d; GP<const int> pres; GP<const double> diag0, Ldiag; GP<const int> fail; GP<double> out;
};
__device__ __forceinline__ double marg_block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kMargFT / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double marg_block_min(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kMargFT / 64; ++w) s = fmin(s, red[w]);
  __syncthreads();
  return s;
}
__global__ __launch_bounds__(kMargFT) void k_marg_finish(MargFinish a) {
  extern __shared__ double A[];                       // info, then its factor L, then L^-1: lower triangle, row stride ldm (odd: no bank conflicts down a column)
  __shared__ double rowb[128];
  __shared__ double red[kMargFT / 64];
  const int tid = threadIdx.x, m = a.m, ldm = m | 1, R = a.R;
  double* const stats = a.out + 2 * (size_t)m * m;
  int np = 0;
  for (int p = tid; p < a.ld; p += kMargFT) np += a.pres[p];
  const double n_present = marg_block_sum((double)np, red);
  const int f0 = done_flag_issue(a.fail);
  if (f0) {                                           // the elimination failed: the trailing block holds nothing of use
    if (tid == 0) { stats[0] = (double)f0; stats[1] = n_present; stats[2] = (double)a.d - n_present; stats[3] = 0.0; }
    return;
  }
  const double* T = a.W + (size_t)R * a.ld + R;
  double* const info = a.out; double* const cov = a.out + (size_t)m * m;
  for (int idx = tid; idx < m * m; idx += kMargFT) {
    const int i = idx / m, j = idx - i * m;
    if (j > i) continue;
    const double v = T[(size_t)i * a.ld + j];
    A[i * ldm + j] = v;
    const double o = (a.pres[R + i] && a.pres[R + j]) ? v : 0.0;
    info[i * m + j] = o; info[j * m + i] = o;
  }
  bool bad = false;
  for (int j = 0; j < m; ++j) {
    __syncthreads();
    const double djj = A[j * ldm + j];                // (every thread reads the same value: the exit below is uniform)
    if (!(djj > 0.0)) { bad = true; break; }
    const double l = sqrt(djj);
    for (int i = j + 1 + tid; i < m; i += kMargFT) A[i * ldm + j] /= l;
    __syncthreads();
    if (tid == 0) A[j * ldm + j] = l;                 // (nothing below reads the pivot's own entry)
    const int i = j + 1 + (tid & 127), part = tid >> 7;      // four threads per row, `part` uniform over a wave
    if (i < m) {
      const double lij = A[i * ldm + j];
      for (int k = j + 1 + part; k <= i; k += 4) A[i * ldm + k] = fma(-lij, A[k * ldm + j], A[i * ldm + k]);
    }
  }
  __syncthreads();
  if (bad) {                                          // one past the last elimination step
    if (tid == 0) { stats[0] = (double)(1 + a.nr); stats[1] = n_present; stats[2] = (double)a.d - n_present; stats[3] = 0.0; }
    return;
  }
  // min L_jj^2 / S_jj over the present unknowns: the selection's pivots from LDS, the rest's from the block steps' factored diagonal blocks
  double mn = 1.0;
  for (int j = tid; j < m; j += kMargFT)
    if (a.pres[R + j]) { const double l = A[j * ldm + j]; mn = fmin(mn, l * l / a.diag0[R + j]); }
  for (int p = tid; p < R; p += kMargFT)
    if (a.pres[p]) { const double l = a.Ldiag[(size_t)(p >> 6) * kNB * kNB + (size_t)(p & 63) * (kNB + 1)]; mn = fmin(mn, l * l / a.diag0[p]); }
  mn = marg_block_min(mn, red);
  // W = L^-1 in place, rows ascending: W_ij = -(sum_{k = j .. i-1} L_ik W_kj) / L_ii, W_ii = 1 / L_ii; row i of L waits in rowb while the
  // row is overwritten.  Thread (j, part) = (tid / 4, tid % 4) takes every fourth term of column j.
  for (int i = 0; i < m; ++i) {
    __syncthreads();
    if (tid <= i) rowb[tid] = A[i * ldm + tid];
    __syncthreads();
    const int j = tid >> 2, part = tid & 3;
    double s = 0.0;
    if (j < i) for (int k = j + part; k < i; k += 4) s = fma(rowb[k], A[k * ldm + j], s);
    s = quad_sum(s);
    if (part == 0) {
      if (j < i) A[i * ldm + j] = -s / rowb[i];
      else if (j == i) A[i * ldm + i] = 1.0 / rowb[i];
    }
  }
  __syncthreads();
  // cov = W^T W: cov_rc = sum_{k >= r} W_kr W_kc for c <= r, mirrored; absent rows / columns are zero
  for (int idx = tid; idx < m * m; idx += kMargFT) {
    const int r = idx / m, c = idx - r * m;
    if (c > r) continue;
    double s = 0.0;
    for (int k = r; k < m; ++k) s = fma(A[k * ldm + r], A[k * ldm + c], s);
    const double o = (a.pres[R + r] && a.pres[R + c]) ? s : 0.0;
    cov[r * m + c] = o; cov[c * m + r] = o;
  }
  if (tid == 0) { stats[0] = 0.0; stats[1] = n_present; stats[2] = (double)a.d - n_present; stats[3] = mn; }
}

// ---- finish of lvf_problem_marginal_prior: ONE workgroup.  Trailing block rows R .. R + m - 1 = info, row R + m = -(eta) with
// -g_r^T H_rr^-1 g_r on its diagonal.  c0 = cost - 1/2 sum_l g_l^2 / Cd_l (the landmarks' share, from what k_prepare left in E's extra
// column and Cd) + 1/2 of that diagonal.  out = info [m x m] | eta [m] | c0 | {fail, n_present, n_absent, min_pivot_ratio over the rest}.
struct MargPriorFinish {
  GP<const double> W; int ld, R, nr, m, d; GP<const int> pres; GP<const double> diag0, Ldiag; GP<const int> fail; GP<double> out;
  GP<const double> cost; int n_lm, ldE, dp; GP<const double> E, Cd;
};
__global__ __launch_bounds__(kMargFT) void k_marg_prior_finish(MargPriorFinish a) {
  __shared__ double red[kMargFT / 64];
  const int tid = threadIdx.x, m = a.m, R = a.R;
  double* const info = a.out; double* const eta = a.out + (size_t)m * m; double* const stats = eta + m + 1;
  int np = 0;
  for (int p = tid; p < a.ld; p += kMargFT) np += a.pres[p];
  const double n_present = marg_block_sum((double)np, red);
  const int f0 = done_flag_issue(a.fail);
  if (f0) {
    if (tid == 0) { stats[0] = (double)f0; stats[1] = n_present; stats[2] = (double)a.d - n_present; stats[3] = 0.0; }
    return;
  }
  const double* T = a.W + (size_t)R * a.ld + R;
  for (int idx = tid; idx < m * m; idx += kMargFT) {
    const int i = idx / m, j = idx - i * m;
    if (j > i) continue;
    const double o = (a.pres[R + i] && a.pres[R + j]) ? T[(size_t)i * a.ld + j] : 0.0;
    info[i * m + j] = o; info[j * m + i] = o;
  }
  for (int j = tid; j < m; j += kMargFT) eta[j] = a.pres[R + j] ? -T[(size_t)m * a.ld + j] : 0.0;
  double lm = 0.0;
  for (int l = tid; l < a.n_lm; l += kMargFT) { const double g = a.E[(size_t)l * a.ldE + a.dp], cd = a.Cd[l]; if (cd > 0.0) lm += g * g / cd; }      // (a landmark no block observes: g = 0, and Cd may be 0)
  lm = marg_block_sum(lm, red);
  double c = tid < kStripes ? a.cost[tid] : 0.0;
  c = marg_block_sum(c, red);
  double mn = 1.0;
  for (int p = tid; p < R; p += kMargFT)
    if (a.pres[p]) { const double l = a.Ldiag[(size_t)(p >> 6) * kNB * kNB + (size_t)(p & 63) * (kNB + 1)]; mn = fmin(mn, l * l / a.diag0[p]); }
  mn = marg_block_min(mn, red);
  if (tid == 0) {
    eta[m] = c - 0.5 * lm + 0.5 * T[(size_t)m * a.ld + m];
    stats[0] = 0.0; stats[1] = n_present; stats[2] = (double)a.d - n_present; stats[3] = mn;
  }
}

// checks a selection of unknowns: 1 <= m <= 120, distinct, in range
static int check_selection(const char* who, int d, const int* sel, int m) {
  LVF_REQUIRE(d >= 1 && d <= 32768, "%s: %d unknowns (1 .. 32768)", who, d);
  LVF_REQUIRE(m >= 1 && m <= kMargMaxSel && m <= d, "%s: %d selected unknowns (1 .. %d, at most all %d)", who, m, kMargMaxSel, d);
  std::vector<char> seen((size_t)d, 0);
  for (int i = 0; i < m; ++i) {
    LVF_REQUIRE(sel[i] >= 0 && sel[i] < d, "%s: selected unknown %d out of range (%d unknowns)", who, sel[i], d);
    LVF_REQUIRE(!seen[sel[i]], "%s: unknown %d selected twice", who, sel[i]);
    seen[sel[i]] = 1;
  }
  return LVF_OK;
}

// The device path on a system that is already on the device: S (leading dimension lds, lower triangle) read through rowmap, absence from
// diag.  Enqueues gather, one block step per 64 rest columns, the tail update and the finish, waits ONCE and downloads 2 m^2 + 4 doubles.
// The selection has been checked (check_selection).  A numeric failure leaves info / cov untouched.
// `rhs` (lvf_problem_marginal_prior): the right-hand-side row rides behind the selection and the outputs are info, eta, c0 (no covariance).
struct MargRhs { int aug_row; const double* cost; int n_lm, ldE, dp; const double *E, *Cd; double *eta, *c0; };
static int marginal_run(lvf_ctx* ctx, const double* S, int lds, const int* rowmap, const double* diag, size_t dstride, int d, const int* sel, int m,
                        double* info, double* cov, lvf_marginal_stats* stats, const MargRhs* rhs = nullptr) {
  hipStream_t q = ctx->stream;
  const int nrest = d - m, nr = (nrest + kNB - 1) / kNB, R = kNB * nr, ns = (m + (rhs ? 1 : 0) + kNB - 1) / kNB, nb = nr + ns, ld = kNB * nb;
  std::vector<int> src((size_t)ld, -1);
  if (rhs) src[(size_t)R + m] = -2;
  {
    std::vector<char> is_sel((size_t)d, 0);
    for (int i = 0; i < m; ++i) { is_sel[sel[i]] = 1; src[(size_t)R + i] = sel[i]; }
    int at = 0;
    for (int u = 0; u < d; ++u) if (!is_sel[u]) src[at++] = u;
  }
  DevBuf<int> srcd, pres, fail;
  DevBuf<double> W, Dinv, Ldiag, diag0, out;
  LVF_TRY(srcd.assign(src.data(), src.size(), q));
  LVF_TRY(W.alloc((size_t)ld * ld)); LVF_TRY(Dinv.alloc((size_t)std::max(nr, 1) * kNB * kNB)); LVF_TRY(Ldiag.alloc((size_t)std::max(nr, 1) * kNB * kNB));
  LVF_TRY(diag0.alloc(ld)); LVF_TRY(pres.alloc(ld)); LVF_TRY(fail.alloc(1));
  const size_t n_out = rhs ? (size_t)m * m + m + 1 + 4 : 2 * (size_t)m * m + 4;
  LVF_TRY(out.alloc(n_out));
  StreamWaitGuard guard(q);                           // (the buffers above go back to the context's pool only once the stream is idle, on every path out)
  MargGather ga{};
  ga.S = S; ga.lds = lds; ga.rowmap = rowmap; ga.diag = diag; ga.dstride = dstride; ga.src = srcd.p; ga.ld = ld; ga.W = W.p; ga.diag0 = diag0.p; ga.pres = pres.p; ga.fail = fail.p;
  ga.aug_row = rhs ? rhs->aug_row : -1;
  hipLaunchKernelGGL(k_marg_gather, dim3(ld), dim3(kMargT), 0, q, ga);
  CholArgs ca{};
  ca.Sd = W.p; ca.ld = ld; ca.nb = nb; ca.fail = fail.p; ca.Dinv = Dinv.p; ca.done = fail.p; ca.dbg = nullptr; ca.last_cols = 0; ca.Ldiag = Ldiag.p;
  GRide gr{}; gr.n = 0;
  TRide tr{}; tr.n = 0;
  for (int kb = 0; kb < nr; ++kb) hipLaunchKernelGGL(k_chol_step, dim3(chol_step_grid(nb, kb)), dim3(kCT), 0, q, ca, kb, gr, tr);
  if (nr > 0) hipLaunchKernelGGL(k_marg_tail_update, dim3(ns * (ns + 1) / 2), dim3(kCT), 0, q, GP<double>(W.p), ld, nr, GP<const int>(fail.p));
  if (rhs) {
    MargPriorFinish fp{};
    fp.W = W.p; fp.ld = ld; fp.R = R; fp.nr = nr; fp.m = m; fp.d = d; fp.pres = pres.p; fp.diag0 = diag0.p; fp.Ldiag = Ldiag.p; fp.fail = fail.p; fp.out = out.p;
    fp.cost = rhs->cost; fp.n_lm = rhs->n_lm; fp.ldE = rhs->ldE; fp.dp = rhs->dp; fp.E = rhs->E; fp.Cd = rhs->Cd;
    hipLaunchKernelGGL(k_marg_prior_finish, dim3(1), dim3(kMargFT), 0, q, fp);
    LVF_HIP(hipGetLastError());
    std::vector<double> h(n_out);
    LVF_TRY(copy_down_wait(ctx, h.data(), out.p, n_out * sizeof(double)));
    guard.dismiss();
    const double* st = h.data() + (size_t)m * m + m + 1;
    stats->fail = (int)st[0]; stats->n_present = (int)st[1]; stats->n_absent = (int)st[2]; stats->min_pivot_ratio = st[3];
    if (stats->fail == 0) {
      if (info) std::memcpy(info, h.data(), (size_t)m * m * sizeof(double));
      if (rhs->eta) std::memcpy(rhs->eta, h.data() + (size_t)m * m, (size_t)m * sizeof(double));
      if (rhs->c0) *rhs->c0 = h[(size_t)m * m + m];
    }
    return LVF_OK;
  }
  MargFinish fa{};
  fa.W = W.p; fa.ld = ld; fa.R = R; fa.nr = nr; fa.m = m; fa.d = d; fa.pres = pres.p; fa.diag0 = diag0.p; fa.Ldiag = Ldiag.p; fa.fail = fail.p; fa.out = out.p;
  const size_t lds_bytes = (size_t)m * (m | 1) * sizeof(double);
  static const bool big_lds = hipFuncSetAttribute(reinterpret_cast<const void*>(k_marg_finish), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)((size_t)kMargMaxSel * (kMargMaxSel | 1) * sizeof(double))) == hipSuccess;
  LVF_REQUIRE(big_lds || lds_bytes <= 48 * 1024, "marginal: the device refuses %zu bytes of LDS", lds_bytes);
  hipLaunchKernelGGL(k_marg_finish, dim3(1), dim3(kMargFT), lds_bytes, q, fa);
  LVF_HIP(hipGetLastError());
  std::vector<double> h(n_out);
  LVF_TRY(copy_down_wait(ctx, h.data(), out.p, n_out * sizeof(double)));
  guard.dismiss();
  const double* st = h.data() + 2 * (size_t)m * m;
  stats->fail = (int)st[0]; stats->n_present = (int)st[1]; stats->n_absent = (int)st[2]; stats->min_pivot_ratio = st[3];
  if (stats->fail == 0) {
    if (info) std::memcpy(info, h.data(), (size_t)m * m * sizeof(double));
    if (cov) std::memcpy(cov, h.data() + (size_t)m * m, (size_t)m * m * sizeof(double));
  }
  return LVF_OK;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_marginal_dense(lvf_ctx* ctx, const double* S, int d, const int* sel, int m, double* info, double* cov, lvf_marginal_stats* stats) {
  LVF_REQUIRE(ctx && S && sel && stats, "lvf_marginal_dense: null argument");
  LVF_REQUIRE(info || cov, "lvf_marginal_dense: info and cov are both NULL");
  LVF_TRY(check_selection("lvf_marginal_dense", d, sel, m));
  LVF_TRY(lvf::enter(ctx));
  DevBuf<double> Sd;
  LVF_TRY(Sd.alloc((size_t)d * d));
  StreamWaitGuard guard(ctx->stream);
  LVF_HIP(hipMemcpyAsync(Sd.p, S, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int rc = marginal_run(ctx, Sd.p, d, nullptr, Sd.p, (size_t)d + 1, d, sel, m, info, cov, stats);
  if (rc == LVF_OK) guard.dismiss();                  // (waited for inside)
  return rc;
}

// The undamped reduced system of the problem at its current state, assembled the way the parity tap (lvf_problem_download_reduced) does — the
// classic k_prepare and the Schur complement alone, nothing eliminated — at a trust-region radius of 1e300: the production assembly adds
// D_jj / radius to every diagonal entry (D_jj <= 1e32), which is below half an ulp of any H_jj > 1e-252, and an unobserved landmark keeps a
// non-zero Cd instead of 0 / 0.  The absence mask comes from the undamped accumulator B's own diagonal.
int lvf_problem_marginal(lvf_problem* p, const lvf_solver_options* o, const int* kfs, int n_sel, double* info, double* cov, lvf_marginal_stats* stats) {
  LVF_REQUIRE(p && o && kfs && stats, "lvf_problem_marginal: null argument");
  LVF_REQUIRE(info || cov, "lvf_problem_marginal: info and cov are both NULL");
  LVF_REQUIRE(n_sel >= 1 && n_sel <= kMargMaxSel / 15, "lvf_problem_marginal: %d keyframes selected (1 .. %d)", n_sel, kMargMaxSel / 15);
  std::vector<int> sel;
  for (int i = 0; i < n_sel; ++i) {
    const int k = kfs[i];
    LVF_REQUIRE(k >= 0 && k < p->n_kf, "lvf_problem_marginal: keyframe %d out of range (%d keyframes)", k, p->n_kf);
    for (int t = 0; t < 6; ++t) sel.push_back(6 * k + t);
    for (int t = 0; t < 9; ++t) sel.push_back(p->dp + 9 * k + t);
  }
  LVF_TRY(check_selection("lvf_problem_marginal", p->d, sel.data(), (int)sel.size()));      // (a keyframe listed twice)
  LVF_TRY(lvf::enter(p->ctx));
  // the control block only lends the assembly its radius slot and a cleared Jacobi-scaling flag: every iteration entry point uploads its own,
  // and the radius of the last iteration (what lvf_problem_download_reduced rebuilds with) is carried over
  LmCtl c;
  ctl_from_options(o, kMargRadius, 2.0, 1, false, &c);
  if (p->last_radius > 0.0) c.last_radius = p->last_radius;
  LVF_TRY(upload_ctl(p, c));
  LVF_TRY(enqueue_linearize(p, o->huber_a, false));                                        // (marks the accumulators dirty)
  LVF_TRY(enqueue_reduced_system(p, &p->ctl.p->radius, false, false, nullptr));            // (marks S dirty where the chain would add into it)
  return marginal_run(p->ctx, p->S.p, p->ld, p->perm.p, p->B.p, (size_t)p->dpad + 1, p->d, sel.data(), (int)sel.size(), info, cov, stats);
}

// The same assembly; the right-hand-side row of S (-(gc - E^T Cd^-1 g_rho)) rides behind the selection, the cost comes from the
// linearisation's stripes (cleared with the accumulators, which the linearisation above finds dirty or clears itself)
int lvf_problem_marginal_prior(lvf_problem* p, const lvf_solver_options* o, const int* kfs, int n_sel, double* info, double* eta, double* c0,
                               lvf_marginal_stats* stats) {
  LVF_REQUIRE(p && o && kfs && stats, "lvf_problem_marginal_prior: null argument");
  LVF_REQUIRE(n_sel >= 1 && n_sel <= kMargMaxSel / 15, "lvf_problem_marginal_prior: %d keyframes selected (1 .. %d)", n_sel, kMargMaxSel / 15);
  std::vector<int> sel;
  for (int i = 0; i < n_sel; ++i) {
    const int k = kfs[i];
    LVF_REQUIRE(k >= 0 && k < p->n_kf, "lvf_problem_marginal_prior: keyframe %d out of range (%d keyframes)", k, p->n_kf);
    for (int t = 0; t < 6; ++t) sel.push_back(6 * k + t);
    for (int t = 0; t < 9; ++t) sel.push_back(p->dp + 9 * k + t);
  }
  LVF_TRY(check_selection("lvf_problem_marginal_prior", p->d, sel.data(), (int)sel.size()));
  LVF_TRY(lvf::enter(p->ctx));
  LmCtl c;
  ctl_from_options(o, kMargRadius, 2.0, 1, false, &c);
  if (p->last_radius > 0.0) c.last_radius = p->last_radius;
  LVF_TRY(upload_ctl(p, c));
  // (the cost stripes start from zero: cleared with the accumulators, or left so by whatever left the accumulators clean)
  LVF_TRY(enqueue_linearize(p, o->huber_a, false));
  LVF_TRY(enqueue_reduced_system(p, &p->ctl.p->radius, false, false, nullptr));
  const MargRhs rhs{p->aug, p->scal.p + SC_COST, p->n_lm, p->ldE, p->dp, p->E.p, p->Cd.p, eta, c0};
  return marginal_run(p->ctx, p->S.p, p->ld, p->perm.p, p->B.p, (size_t)p->dpad + 1, p->d, sel.data(), (int)sel.size(), info, nullptr, stats, &rhs);      // (the accumulators and the stripes are left dirty and marked so)
}

}  // extern "C"
