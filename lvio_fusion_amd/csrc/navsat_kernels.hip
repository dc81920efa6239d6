// navsat_kernels.hip — GNSS (NavSat) alignment on device (DESIGN.md "GNSS alignment"):
//
//   NavsatInitError / NavsatRXError / NavsatRError      src/lvio_fusion/include/lvio_fusion/ceres/navsat_error.hpp:9-120  (navsat_eval.hpp)
//   Navsat::Initialize                                   src/lvio_fusion/src/navsat.cpp:100-133
//   Navsat::OptimizeBC                                   src/lvio_fusion/src/navsat.cpp:192-269
//   the per-keyframe loop of Navsat::Optimize / QuickFix src/lvio_fusion/src/navsat.cpp:150-155, :171-176
//
// Every solve is a ceres::Solve(DENSE_QR) of at most six scalar parameter blocks: like Relocator::UpdateNewSubmap's rotation solve
// (loop_kernels.hip) the whole Levenberg-Marquardt loop is ONE launch of one workgroup and the host reads one record.  The loop is lm_small
// (small_lm.hpp); what these problems bring to it is below: the block lists, and Blocks3, which makes a list of 3-vector blocks the loop's
// problem — a loss function (HuberLoss, Corrector scale sqrt(rho')), constant parameter blocks (a constant slot gets no dual seed: a zero
// Jacobian column) and box bounds (SetParameterLowerBound / UpperBound).
// Declared solver semantics: oracle/lm.h (header), oracle/robust.h; the bounds: DESIGN.md, and tests/navsat_ref.py restates the whole loop.
#include "navsat_eval.hpp"
#include "small_lm.hpp"

namespace lvf {

// A list F of 3-vector residual blocks over N slots as lm_small's problem: 1/2 sum rho(|r_b|^2), plus is addition, the norms run over the
// free slots.  PAR: the blocks are dealt over the workgroup; else every thread walks all of them.  BOX: the slots in bound_mask are boxed.
template <int N, bool PAR, class F, bool BOX = false>
struct Blocks3 {
  static constexpr bool kBox = BOX;
  const F& f;
  int nb;
  double huber_a;
  unsigned bound_mask;
  double lo[N], hi[N];
  __device__ __forceinline__ void accumulate(const double* x, unsigned free_mask, double* acc) const {
    constexpr int T = N * (N + 1) / 2;
    for (int i = PAR ? (int)threadIdx.x : 0; i < nb; i += PAR ? kLT : 1) {
      if (!f.has(i)) continue;
      double r[3], J[3 * N];
      f.template eval<true>(i, x, free_mask, r, J);
      double rho0, rho1;
      huber_eval(huber_a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho0, rho1);
      acc[T + N] += 0.5 * rho0;
      const double sc = sqrt(rho1);                  // Corrector, rho'' <= 0
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double rk = sc * r[k];
        double l[N];
#pragma unroll
        for (int c = 0; c < N; ++c) l[c] = sc * J[N * k + c];
#pragma unroll
        for (int u = 0; u < N; ++u) {
          acc[T + u] += l[u] * rk;
#pragma unroll
          for (int v = 0; v <= u; ++v) acc[u * (u + 1) / 2 + v] += l[u] * l[v];
        }
      }
    }
  }
  __device__ __forceinline__ double cost_part(const double* x) const {
    double c = 0.0;
    for (int i = PAR ? (int)threadIdx.x : 0; i < nb; i += PAR ? kLT : 1) {
      if (!f.has(i)) continue;
      double r[3], J[3 * N];
      f.template eval<false>(i, x, 0u, r, J);
      double rho0, rho1;
      huber_eval(huber_a, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], rho0, rho1);
      c += 0.5 * rho0;
    }
    return c;
  }
  __device__ __forceinline__ void plus(const double* x, const double* dx, double* xc) const {
#pragma unroll
    for (int c = 0; c < N; ++c) xc[c] = x[c] + dx[c];
  }
  __device__ __forceinline__ unsigned norm_mask(unsigned free_mask) const { return free_mask; }
};

// ---- the block lists ---------------------------------------------------------------------------------------------------------------
// NavsatInitError blocks; slots (yaw, x, y) in the order Navsat::Initialize adds the parameter blocks (navsat.cpp:106-108)
struct InitBlocks {
  const double *p0, *p1, *cov;
  __device__ __forceinline__ bool has(int) const { return true; }
  template <bool WITH_J>
  __device__ __forceinline__ void eval(int i, const double x[3], unsigned free_mask, double r[3], double J[9]) const {
    typedef DJet<3> T;
    T p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (WITH_J && ((free_mask >> c) & 1u)) ? T(x[c], c) : T(x[c]);
    const double sq[3] = {cov2sqrt_info(cov[3 * i]), cov2sqrt_info(cov[3 * i + 1]), cov2sqrt_info(cov[3 * i + 2])};
    T rr[3];
    navsat_init_functor<3>(p0 + 3 * i, p1 + 3 * i, sq, p[0], p[1], p[2], rr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = rr[k].a;
#pragma unroll
      for (int c = 0; c < 3; ++c) J[3 * k + c] = rr[k].v[c];
    }
  }
};

// NavsatRXError blocks of one frame; slots (z, y, x, roll, pitch, yaw) = para[5 - slot], the order Navsat::OptimizeBC adds the parameter
// blocks (navsat.cpp:204-209)
struct RxBlocks {
  const double *fix, *p1, *cov;
  const int* has_fix;
  double pose[7];
  __device__ __forceinline__ bool has(int i) const { return has_fix[i] != 0; }
  template <bool WITH_J>
  __device__ __forceinline__ void eval(int i, const double x[6], unsigned free_mask, double r[3], double J[18]) const {
    typedef DJet<6> T;
    T rp[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) rp[p] = (WITH_J && ((free_mask >> (5 - p)) & 1u)) ? T(x[5 - p], 5 - p) : T(x[5 - p]);
    const double sq[3] = {cov2sqrt_info(cov[3 * i]), cov2sqrt_info(cov[3 * i + 1]), cov2sqrt_info(cov[3 * i + 2])};
    T rr[3];
    navsat_rx_functor<6>(fix + 3 * i, p1 + 3 * i, pose, sq, rp, rr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[k] = rr[k].a;
#pragma unroll
      for (int c = 0; c < 6; ++c) J[6 * k + c] = rr[k].v[c];
    }
  }
};

// one NavsatRXError block with only x free (mode 0b110111), everything in registers: the chain's step
struct RxOne {
  double fix[3], p1[3], sq[3], pose[7];
  __device__ __forceinline__ bool has(int) const { return true; }
  template <bool WITH_J>
  __device__ __forceinline__ void eval(int, const double x[1], unsigned, double r[3], double J[3]) const {
    typedef DJet<1> T;
    const T rp[6] = {T(0.0), T(0.0), T(0.0), WITH_J ? T(x[0], 0) : T(x[0]), T(0.0), T(0.0)};
    T rr[3];
    navsat_rx_functor<1>(fix, p1, pose, sq, rp, rr);
#pragma unroll
    for (int k = 0; k < 3; ++k) { r[k] = rr[k].a; J[k] = rr[k].v[0]; }
  }
};

// the single NavsatRError block of the roll pre-solve (a 1-vector: rows 1 and 2 stay zero); block 0 only
struct ROne {
  double y[3], pose[7];
  __device__ __forceinline__ bool has(int) const { return true; }
  template <bool WITH_J>
  __device__ __forceinline__ void eval(int, const double x[1], unsigned, double r[3], double J[3]) const {
    typedef DJet<1> T;
    const T rr = navsat_r_functor<1>(y, pose, WITH_J ? T(x[0], 0) : T(x[0]));
    r[0] = rr.a; r[1] = 0.0; r[2] = 0.0; J[0] = rr.v[0]; J[1] = 0.0; J[2] = 0.0;
  }
};

// ---- batched functor evaluation: one thread, one block ---------------------------------------------------------------------------------
template <bool WITH_J>
__global__ __launch_bounds__(kLT) void k_navsat_init_eval(int n, const double* __restrict__ p0, const double* __restrict__ p1, const double* __restrict__ cov,
                                                           const double* __restrict__ x3, double* __restrict__ res, double* __restrict__ jac) {
  const int i = blockIdx.x * kLT + threadIdx.x;
  if (i >= n) return;
  const InitBlocks b{p0, p1, cov};
  const double x[3] = {x3[0], x3[1], x3[2]};
  double r[3], J[9];
  b.eval<WITH_J>(i, x, 7u, r, J);
#pragma unroll
  for (int k = 0; k < 3; ++k) res[3 * i + k] = r[k];
  if (WITH_J) {
#pragma unroll
    for (int k = 0; k < 9; ++k) jac[9 * i + k] = J[k];
  }
}

template <bool WITH_J>
__global__ __launch_bounds__(kLT) void k_navsat_rx_eval(int n, const double* __restrict__ p0, const double* __restrict__ p1, const double* __restrict__ pose7,
                                                         const double* __restrict__ cov, const double* __restrict__ x6, double* __restrict__ res,
                                                         double* __restrict__ jac) {
  const int i = blockIdx.x * kLT + threadIdx.x;
  if (i >= n) return;
  RxBlocks b{p0, p1, cov, nullptr, {pose7[0], pose7[1], pose7[2], pose7[3], pose7[4], pose7[5], pose7[6]}};
  const double x[6] = {x6[5], x6[4], x6[3], x6[2], x6[1], x6[0]};      // slots
  double r[3], J[18];
  b.eval<WITH_J>(i, x, 63u, r, J);
#pragma unroll
  for (int k = 0; k < 3; ++k) res[3 * i + k] = r[k];
  if (WITH_J) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int p = 0; p < 6; ++p) jac[18 * i + 6 * k + p] = J[6 * k + (5 - p)];      // columns back in (yaw, pitch, roll, x, y, z)
    }
  }
}

__global__ __launch_bounds__(64) void k_navsat_r_eval(const double* __restrict__ y3, const double* __restrict__ pose7, double roll, double* __restrict__ out2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const ROne b{{y3[0], y3[1], y3[2]}, {pose7[0], pose7[1], pose7[2], pose7[3], pose7[4], pose7[5], pose7[6]}};
  const double x[1] = {roll};
  double r[3], J[3];
  b.eval<true>(0, x, 1u, r, J);
  out2[0] = r[0]; out2[1] = J[0];
}

// ---- Navsat::Initialize: both stages in one launch ---------------------------------------------------------------------------------------
struct InitRecord { double para[6], extrinsic[7]; LmRec stage1, stage2; };

__global__ __launch_bounds__(kLT) void k_navsat_initialize(int n, const double* __restrict__ position, const double* __restrict__ raw, const double* __restrict__ cov,
                                                            LmOpts o, InitRecord* __restrict__ out) {
  __shared__ double tile[lm_tile_doubles(3)];
  const InitBlocks b{position, raw, cov};
  const Blocks3<3, true, InitBlocks> p{b, n, 0.0};
  double x[3] = {0.0, 0.0, 0.0};
  LmRec r1, r2;
  lm_small<3, 3, true>(p, n, x, 1u, o, r1, tile);      // x, y constant (navsat.cpp:109-110)
  lm_small<3, 3, true>(p, n, x, 7u, o, r2, tile);      // all three (navsat.cpp:127-129)
  if (threadIdx.x == 0) {
    const double para[6] = {x[0], 0.0, 0.0, x[1], x[2], 0.0};
    double e[7];
    rpyxyz_to_se3(para, e);
#pragma unroll
    for (int k = 0; k < 6; ++k) out->para[k] = para[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) out->extrinsic[k] = e[k];
    out->stage1 = r1; out->stage2 = r2;
  }
}

// ---- Navsat::OptimizeBC --------------------------------------------------------------------------------------------------------------------
struct BcArgs {
  int n, n_total;            // active keyframes (frame first), all poses (active + update-only)
  int n_fix;                 // keyframes with a fix
  unsigned free_mask;        // slots (z, y, x, roll, pitch, yaw) free in the main solve
  int roll_presolve, z_bounded;
  double z_lower, z_upper, huber_a;
  LmOpts o;
};
struct BcRecord { double para[6], transform[7]; LmRec roll, main; };

__global__ __launch_bounds__(kLT) void k_navsat_optimize_bc(BcArgs a, double* __restrict__ poses, const int* __restrict__ has_fix, const double* __restrict__ fix,
                                                             const double* __restrict__ cov, double* __restrict__ p1, BcRecord* __restrict__ out) {
  __shared__ double tile[lm_tile_doubles(6)];
  const int tid = threadIdx.x;
  double frame[7], inv[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) frame[k] = poses[k];
  sophus_inverse(frame, inv);
  // frame^-1 * t_i (navsat.cpp:256) and, for the roll pre-solve, sum_i (frame^-1.so3 * pose_i.so3) * UnitY (navsat.cpp:220-225)
  double ys[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < a.n; i += kLT) {
    const double* p = poses + (size_t)7 * i;
    double q[3];
    sophus_transform_point(inv, p[4], p[5], p[6], q);
    p1[3 * i] = q[0]; p1[3 * i + 1] = q[1]; p1[3 * i + 2] = q[2];
    if (a.roll_presolve) {
      double rel[7], yv[3];
      forward_update_pose(inv, p, rel);
      quat_transform_vector(rel[0], rel[1], rel[2], rel[3], 0.0, 1.0, 0.0, yv);
      ys[0] += yv[0]; ys[1] += yv[1]; ys[2] += yv[2];
    }
  }
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // slots (z, y, x, roll, pitch, yaw)
  LmRec rr{}, rm;                                    // (LVF_WHY_NONE is 0)
  if (a.roll_presolve) {
    ROne rb;
#pragma unroll
    for (int k = 0; k < 3; ++k) rb.y[k] = wg_sum(ys[k], tile);
#pragma unroll
    for (int k = 0; k < 7; ++k) rb.pose[k] = frame[k];
    double xr[1] = {0.0};
    lm_small<1, 1, false>(Blocks3<1, false, ROne>{rb, 1, 0.0}, 1, xr, 1u, a.o, rr, nullptr);      // every thread solves the same 1 x 1 problem
    x[3] = xr[0];
  }
  __syncthreads();                                   // p1 is complete
  const RxBlocks b{fix, p1, cov, has_fix, {frame[0], frame[1], frame[2], frame[3], frame[4], frame[5], frame[6]}};
  const Blocks3<6, true, RxBlocks, true> p{b, a.n, a.huber_a, a.z_bounded ? 1u : 0u, {a.z_lower}, {a.z_upper}};
  lm_small<6, 6, true>(p, a.n_fix, x, a.free_mask, a.o, rm, tile);
  // frame <- frame * rpyxyz2se3(para); every later pose <- (new * old^-1) * pose (navsat.cpp:265-268)
  const double para[6] = {x[5], x[4], x[3], x[2], x[1], x[0]};
  double rel[7], fresh[7], T[7];
  rpyxyz_to_se3(para, rel);
  forward_update_pose(frame, rel, fresh);
  forward_update_pose(fresh, inv, T);
  for (int i = 1 + tid; i < a.n_total; i += kLT) {
    double* p = poses + (size_t)7 * i;
    forward_update_pose(T, p, p);
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) { poses[k] = fresh[k]; out->transform[k] = T[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) out->para[k] = para[k];
    out->roll = rr; out->main = rm;
  }
}

// ---- the per-keyframe loop of Navsat::Optimize / QuickFix: the whole chain in one launch -------------------------------------------------
struct ChainRecord { double initial_cost, final_cost; int iters, successes, termination, pad; };

// P: the n poses the steps work on — LDS (IN_LDS, n <= kChainLdsPoses) or a device buffer; pose k is final once step k has run and goes
// straight to `out`, so nothing ever re-reads a slot another thread is writing between two barriers.
constexpr int kChainLdsPoses = 2048;
template <bool IN_LDS>
__global__ __launch_bounds__(kLT) void k_navsat_fix_chain(int n, const double* __restrict__ in, double* __restrict__ work, double* __restrict__ out,
                                                           const int* __restrict__ has_fix, const double* __restrict__ fix, const double* __restrict__ cov,
                                                           double huber_a, LmOpts o, double* __restrict__ x_out, int* __restrict__ iters_out,
                                                           ChainRecord* __restrict__ rec) {
  extern __shared__ double lds_poses[];
  const int tid = threadIdx.x;
  double* P = IN_LDS ? lds_poses : work;
  for (int i = tid; i < 7 * n; i += kLT) P[i] = in[i];
  __syncthreads();
  double sum_c0 = 0.0, sum_c1 = 0.0;
  int sum_it = 0, sum_ok = 0, worst = 0;
  for (int k = 0; k + 1 < n; ++k) {
    RxOne b;
#pragma unroll
    for (int c = 0; c < 7; ++c) b.pose[c] = P[(size_t)7 * k + c];      // the same words for every thread (broadcast)
    double inv[7];
    sophus_inverse(b.pose, inv);
    double xs[1] = {0.0};
    LmRec r{};
    if (has_fix[k]) {
      sophus_transform_point(inv, b.pose[4], b.pose[5], b.pose[6], b.p1);      // frame^-1 * t_frame (navsat.cpp:256)
#pragma unroll
      for (int c = 0; c < 3; ++c) { b.fix[c] = fix[3 * k + c]; b.sq[c] = cov2sqrt_info(cov[3 * k + c]); }
      lm_small<1, 1, false>(Blocks3<1, false, RxOne>{b, 1, huber_a}, 1, xs, 1u, o, r, nullptr);
    }
    const double para[6] = {0.0, 0.0, 0.0, xs[0], 0.0, 0.0};
    double rel[7], fresh[7], T[7];
    rpyxyz_to_se3(para, rel);
    forward_update_pose(b.pose, rel, fresh);
    forward_update_pose(fresh, inv, T);
    for (int j = k + 1 + ((tid - (k + 1)) & (kLT - 1)); j < n; j += kLT) {      // the poses this thread owns (j % kLT == tid) after k
      double* p = P + (size_t)7 * j;
      forward_update_pose(T, p, p);
    }
    if (tid == (k & (kLT - 1))) {
#pragma unroll
      for (int c = 0; c < 7; ++c) out[(size_t)7 * k + c] = fresh[c];
      x_out[k] = xs[0]; iters_out[k] = r.iters;
    }
    sum_c0 += r.initial_cost; sum_c1 += r.final_cost; sum_it += r.iters; sum_ok += r.successes; worst = max(worst, r.termination);
    __syncthreads();
  }
  if (n > 0 && tid == ((n - 1) & (kLT - 1))) {
#pragma unroll
    for (int c = 0; c < 7; ++c) out[(size_t)7 * (n - 1) + c] = P[(size_t)7 * (n - 1) + c];
  }
  if (tid == 0) { rec->initial_cost = sum_c0; rec->final_cost = sum_c1; rec->iters = sum_it; rec->successes = sum_ok; rec->termination = worst; rec->pad = 0; }
}

}  // namespace lvf

using namespace lvf;

namespace {

LmOpts lm_opts(const lvf_solver_options* o) {
  return LmOpts{o->max_num_iterations, o->function_tolerance, o->gradient_tolerance, o->parameter_tolerance, o->min_relative_decrease, o->initial_trust_region_radius};
}
void fill_summary(const LmRec& r, int blocks, lvf_solver_summary* s) {
  std::memset(s, 0, sizeof(*s));
  s->initial_cost = r.initial_cost; s->final_cost = r.final_cost; s->num_iterations = r.iters; s->num_successful_steps = r.successes;
  s->num_unsuccessful_steps = r.iters - r.successes; s->num_residual_blocks = blocks; s->termination = r.termination; s->termination_reason = r.why;
}
bool all_positive(const double* cov, const int* has, int n) {
  for (int i = 0; i < n; ++i) {
    if (has && !has[i]) continue;
    for (int k = 0; k < 3; ++k)
      if (!(cov[3 * i + k] > 0.0) || !std::isfinite(cov[3 * i + k])) return false;
  }
  return true;
}
bool quats_nonzero(const double* poses, int n) {
  for (int i = 0; i < n; ++i) {
    const double* q = poses + (size_t)7 * i;
    if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return false;
  }
  return true;
}

}  // namespace

extern "C" {

int lvf_navsat_init_evaluate(lvf_ctx* ctx, int n, const double* p0, const double* p1, const double* cov, const double* x3, double* residuals, double* jacobians) {
  LVF_REQUIRE(ctx && x3, "lvf_navsat_init_evaluate: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || (p0 && p1 && cov && residuals)), "lvf_navsat_init_evaluate: bad block arrays");
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(all_positive(cov, nullptr, n), "lvf_navsat_init_evaluate: covariance must be > 0");
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> a, b, c, x, r, J;
  LVF_TRY(a.upload(p0, (size_t)3 * n, s)); LVF_TRY(b.upload(p1, (size_t)3 * n, s)); LVF_TRY(c.upload(cov, (size_t)3 * n, s)); LVF_TRY(x.upload(x3, 3, s));
  LVF_TRY(r.alloc((size_t)3 * n));
  const dim3 grid((n + kLT - 1) / kLT), block(kLT);
  if (jacobians) {
    LVF_TRY(J.alloc((size_t)9 * n));
    hipLaunchKernelGGL(k_navsat_init_eval<true>, grid, block, 0, s, n, a.p, b.p, c.p, x.p, r.p, J.p);
  } else {
    hipLaunchKernelGGL(k_navsat_init_eval<false>, grid, block, 0, s, n, a.p, b.p, c.p, x.p, r.p, (double*)nullptr);
  }
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(residuals, r.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  if (jacobians) LVF_HIP(hipMemcpyAsync(jacobians, J.p, (size_t)9 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_navsat_rx_evaluate(lvf_ctx* ctx, int n, const double* p0, const double* p1, const double* pose7, const double* cov, const double* x6, double* residuals,
                           double* jacobians) {
  LVF_REQUIRE(ctx && pose7 && x6, "lvf_navsat_rx_evaluate: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || (p0 && p1 && cov && residuals)), "lvf_navsat_rx_evaluate: bad block arrays");
  LVF_REQUIRE(quats_nonzero(pose7, 1), "lvf_navsat_rx_evaluate: zero quaternion");
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(all_positive(cov, nullptr, n), "lvf_navsat_rx_evaluate: covariance must be > 0");
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> a, b, c, P, x, r, J;
  LVF_TRY(a.upload(p0, (size_t)3 * n, s)); LVF_TRY(b.upload(p1, (size_t)3 * n, s)); LVF_TRY(c.upload(cov, (size_t)3 * n, s)); LVF_TRY(P.upload(pose7, 7, s));
  LVF_TRY(x.upload(x6, 6, s)); LVF_TRY(r.alloc((size_t)3 * n));
  const dim3 grid((n + kLT - 1) / kLT), block(kLT);
  if (jacobians) {
    LVF_TRY(J.alloc((size_t)18 * n));
    hipLaunchKernelGGL(k_navsat_rx_eval<true>, grid, block, 0, s, n, a.p, b.p, P.p, c.p, x.p, r.p, J.p);
  } else {
    hipLaunchKernelGGL(k_navsat_rx_eval<false>, grid, block, 0, s, n, a.p, b.p, P.p, c.p, x.p, r.p, (double*)nullptr);
  }
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(residuals, r.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  if (jacobians) LVF_HIP(hipMemcpyAsync(jacobians, J.p, (size_t)18 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_navsat_r_evaluate(lvf_ctx* ctx, const double* y3, const double* pose7, double roll, double* residual, double* jacobian) {
  LVF_REQUIRE(ctx && y3 && pose7 && residual, "lvf_navsat_r_evaluate: null argument");
  LVF_REQUIRE(quats_nonzero(pose7, 1), "lvf_navsat_r_evaluate: zero quaternion");
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> y, P, out;
  LVF_TRY(y.upload(y3, 3, s)); LVF_TRY(P.upload(pose7, 7, s)); LVF_TRY(out.alloc(2));
  hipLaunchKernelGGL(k_navsat_r_eval, dim3(1), dim3(64), 0, s, y.p, P.p, roll, out.p);
  LVF_HIP(hipGetLastError());
  double h[2];
  LVF_TRY(lvf::read_back(ctx, h, out.p, sizeof(h)));
  *residual = h[0];
  if (jacobian) *jacobian = h[1];
  return LVF_OK;
}

int lvf_navsat_initialize(lvf_ctx* ctx, int n, const double* position, const double* raw, const double* cov, const lvf_solver_options* o, double* para6,
                          double* extrinsic7, lvf_solver_summary* stage1, lvf_solver_summary* stage2) {
  LVF_REQUIRE(ctx && o && para6 && extrinsic7 && stage1 && stage2, "lvf_navsat_initialize: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || (position && raw && cov)), "lvf_navsat_initialize: bad block arrays");
  LVF_REQUIRE(n == 0 || all_positive(cov, nullptr, n), "lvf_navsat_initialize: covariance must be > 0");
  std::memset(stage1, 0, sizeof(*stage1)); std::memset(stage2, 0, sizeof(*stage2));
  for (int k = 0; k < 6; ++k) para6[k] = 0.0;
  for (int k = 0; k < 7; ++k) extrinsic7[k] = k == 3 ? 1.0 : 0.0;
  if (n == 0) return LVF_OK;                         // no keyframe has a fix: para stays 0, extrinsic = identity
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> a, b, c;
  DevBuf<InitRecord> rec;
  LVF_TRY(a.upload(position, (size_t)3 * n, s)); LVF_TRY(b.upload(raw, (size_t)3 * n, s)); LVF_TRY(c.upload(cov, (size_t)3 * n, s)); LVF_TRY(rec.alloc(1));
  hipLaunchKernelGGL(k_navsat_initialize, dim3(1), dim3(kLT), 0, s, n, a.p, b.p, c.p, lm_opts(o), rec.p);
  LVF_HIP(hipGetLastError());
  InitRecord h;
  LVF_TRY(lvf::read_back(ctx, &h, rec.p, sizeof(h)));
  std::memcpy(para6, h.para, sizeof(h.para)); std::memcpy(extrinsic7, h.extrinsic, sizeof(h.extrinsic));
  fill_summary(h.stage1, n, stage1); fill_summary(h.stage2, n, stage2);
  return LVF_OK;
}

void lvf_navsat_bc_options_default(lvf_navsat_bc_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->mode = 0; o->distance = 0.0; o->trust_distance_yaw = 20.0; o->trust_distance_pitch = 10.0; o->z_lower = -5.0; o->z_upper = 5.0; o->huber_a = 0.1;
  lvf_solver_options_default(&o->solver);
}

int lvf_navsat_optimize_bc(lvf_ctx* ctx, int n, int n_update, double* poses, const int32_t* has_fix, const double* fix_point, const double* cov,
                           const lvf_navsat_bc_options* opt, lvf_navsat_bc_result* result) {
  LVF_REQUIRE(ctx && opt && result, "lvf_navsat_optimize_bc: null argument");
  LVF_REQUIRE(n >= 0 && n_update >= 0 && (n > 0 || n_update == 0), "lvf_navsat_optimize_bc: bad counts (n %d, n_update %d)", n, n_update);
  LVF_REQUIRE(n == 0 || (poses && has_fix && fix_point && cov), "lvf_navsat_optimize_bc: bad arrays");
  LVF_REQUIRE(opt->mode >= 0 && opt->mode < 64, "lvf_navsat_optimize_bc: mode %d is not a 6-bit mask", opt->mode);
  std::memset(result, 0, sizeof(*result));
  result->transform[3] = 1.0;
  // rotation's optimisation needs a longer path (navsat.cpp:195-197)
  if (n == 0 || ((opt->mode & 7) != 7 && opt->distance < opt->trust_distance_yaw)) { result->skipped = 1; return LVF_OK; }
  LVF_REQUIRE(quats_nonzero(poses, n + n_update), "lvf_navsat_optimize_bc: zero quaternion");
  LVF_REQUIRE(all_positive(cov, has_fix, n), "lvf_navsat_optimize_bc: covariance must be > 0");
  unsigned constant = (unsigned)opt->mode;           // bit i: para[i] constant, para = (yaw, pitch, roll, x, y, z)
  BcArgs a{};
  a.n = n; a.n_total = n + n_update;
  for (int i = 0; i < n; ++i) a.n_fix += has_fix[i] != 0;
  if (!(constant & 4u)) {                            // roll free: pre-solve it on a long path, then hold it (navsat.cpp:216-234)
    a.roll_presolve = opt->distance > opt->trust_distance_yaw;
    constant |= 4u;
  }
  if (!(constant & 2u) && opt->distance < opt->trust_distance_pitch) constant |= 2u;      // navsat.cpp:236-240
  a.z_bounded = !(constant & 32u);                   // navsat.cpp:242-247
  a.z_lower = opt->z_lower; a.z_upper = opt->z_upper; a.huber_a = opt->huber_a;
  LVF_REQUIRE(!a.z_bounded || opt->z_lower <= opt->z_upper, "lvf_navsat_optimize_bc: z_lower > z_upper");
  a.free_mask = 0u;
  for (int p = 0; p < 6; ++p)
    if (!((constant >> p) & 1u)) a.free_mask |= 1u << (5 - p);
  a.o = lm_opts(&opt->solver);
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> P, F, C, p1;
  DevBuf<int> H;
  DevBuf<BcRecord> rec;
  LVF_TRY(P.upload(poses, (size_t)7 * a.n_total, s)); LVF_TRY(F.upload(fix_point, (size_t)3 * n, s)); LVF_TRY(C.upload(cov, (size_t)3 * n, s));
  LVF_TRY(H.upload(has_fix, (size_t)n, s)); LVF_TRY(p1.alloc((size_t)3 * n)); LVF_TRY(rec.alloc(1));
  hipLaunchKernelGGL(k_navsat_optimize_bc, dim3(1), dim3(kLT), 0, s, a, P.p, H.p, F.p, C.p, p1.p, rec.p);
  LVF_HIP(hipGetLastError());
  BcRecord h;
  LVF_HIP(hipMemcpyAsync(poses, P.p, (size_t)7 * a.n_total * 8, hipMemcpyDeviceToHost, s));
  LVF_TRY(lvf::read_back(ctx, &h, rec.p, sizeof(h)));
  std::memcpy(result->para, h.para, sizeof(h.para)); std::memcpy(result->transform, h.transform, sizeof(h.transform));
  fill_summary(h.roll, a.roll_presolve ? 1 : 0, &result->roll); fill_summary(h.main, a.n_fix, &result->main);
  result->line_search_contractions = h.main.contractions;
  return LVF_OK;
}

int lvf_navsat_fix_chain(lvf_ctx* ctx, int n, double* poses, const int32_t* has_fix, const double* fix_point, const double* cov, double huber_a,
                         const lvf_solver_options* o, double* x, int32_t* iterations, lvf_solver_summary* summary) {
  LVF_REQUIRE(ctx && o && summary, "lvf_navsat_fix_chain: null argument");
  LVF_REQUIRE(n >= 0 && (n < 2 || (poses && has_fix && fix_point && cov)), "lvf_navsat_fix_chain: bad arrays");
  std::memset(summary, 0, sizeof(*summary));
  if (n < 2) return LVF_OK;                          // no keyframe strictly between B and C
  LVF_REQUIRE(quats_nonzero(poses, n), "lvf_navsat_fix_chain: zero quaternion");
  LVF_REQUIRE(all_positive(cov, has_fix, n - 1), "lvf_navsat_fix_chain: covariance must be > 0");
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  const int steps = n - 1;
  DevBuf<double> In, Work, Out, F, C, X;
  DevBuf<int> H, It;
  DevBuf<ChainRecord> rec;
  LVF_TRY(In.upload(poses, (size_t)7 * n, s)); LVF_TRY(Out.alloc((size_t)7 * n)); LVF_TRY(F.upload(fix_point, (size_t)3 * steps, s));
  LVF_TRY(C.upload(cov, (size_t)3 * steps, s)); LVF_TRY(H.upload(has_fix, (size_t)steps, s)); LVF_TRY(X.alloc(steps)); LVF_TRY(It.alloc(steps)); LVF_TRY(rec.alloc(1));
  for (int i = 0; i < steps; ++i) summary->num_residual_blocks += has_fix[i] != 0;
  if (n <= kChainLdsPoses) {
    const size_t lds = (size_t)7 * n * sizeof(double);
    if (lds > 48 * 1024) LVF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_navsat_fix_chain<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_navsat_fix_chain<true>, dim3(1), dim3(kLT), lds, s, n, In.p, (double*)nullptr, Out.p, H.p, F.p, C.p, huber_a, lm_opts(o), X.p, It.p, rec.p);
  } else {
    LVF_TRY(Work.alloc((size_t)7 * n));
    hipLaunchKernelGGL(k_navsat_fix_chain<false>, dim3(1), dim3(kLT), 0, s, n, In.p, Work.p, Out.p, H.p, F.p, C.p, huber_a, lm_opts(o), X.p, It.p, rec.p);
  }
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(poses, Out.p, (size_t)7 * n * 8, hipMemcpyDeviceToHost, s));
  if (x) LVF_HIP(hipMemcpyAsync(x, X.p, (size_t)steps * 8, hipMemcpyDeviceToHost, s));
  if (iterations) LVF_HIP(hipMemcpyAsync(iterations, It.p, (size_t)steps * 4, hipMemcpyDeviceToHost, s));
  ChainRecord h;
  LVF_TRY(lvf::read_back(ctx, &h, rec.p, sizeof(h)));
  summary->initial_cost = h.initial_cost; summary->final_cost = h.final_cost; summary->num_iterations = h.iters; summary->num_successful_steps = h.successes;
  summary->num_unsuccessful_steps = h.iters - h.successes; summary->termination = h.termination;
  return LVF_OK;
}

}  // extern "C"
