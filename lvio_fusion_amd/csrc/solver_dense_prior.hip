// solver_dense_prior.hip — a dense prior on the 15 tangent unknowns of up to eight keyframes, as a block of the sliding-window problem:
// what marginalising departed keyframes leaves on the ones that stay (lvf_problem_marginal_prior makes one, marginal_kernels.hip).
//
//     cost(x) = c0 + eta^T e + 1/2 e^T info e,      e = x [-] x0      (declared semantics: tests/dense_prior_ref.py)
//
// e is the local coordinate of x at x0 in the solver's own parameterisation (pose_plus, lvf_math.hpp): for the rotation, with u = q/|q|,
// u0 = q0/|q0| and d = u (x) u0^-1 (negated if d.w < 0), delta = atan2(|d.v|, d.w) d.v/|d.v|, so that Plus(q0, delta) = q; plain differences
// for the other twelve entries of a keyframe.  No loss function, no first-estimate Jacobians: e is re-evaluated at every state.
//
// Derivatives follow the convention of every pose factor here (the ambient derivative, projected by quat_row_to_local), which for this
// factor has a closed form: Plus(q, eps) = exp(eps) (x) q turns d into exp(eps) (x) d whatever |q| is, so the tangent Jacobian of e is block
// diagonal, the identity except for one 3 x 3 block per keyframe,
//     T_rot = d log(exp(eps) (x) d) / d eps = I - [delta]x + (1 - theta cot theta) / theta^2 [delta]x^2,     theta = |delta| <= pi/2,
// the inverse left Jacobian of the rotation by 2 theta.  Gradient T^T (info e + eta), Gauss-Newton matrix T^T info T, zero columns for a
// constant block (pose_const bit 0: the pose's six, bits 1 .. 3: v, ba, bg).
//
// One workgroup does all of it: m <= 120, so info is 113 KB at most and is read twice from L2; every entry of T^T info T is a sum of at most
// nine products.  The terms go into the LOWER triangle of B in the natural order, cross blocks between the prior's keyframes included —
// which is why the elimination plan keeps those keyframes' (v, ba, bg) blocks in the dense corner (solver_plan.hip).
#include <cmath>

#include "solver_dev.hpp"
#include "solver_host.hpp"

namespace lvf {

constexpr int kDpM = 15 * kDensePriorMaxKf;

struct DensePriorLds {
  double e[kDpM], y[kDpM], cm[kDpM], T[9 * kDensePriorMaxKf], red[kDensePriorT / 64];
  int nat[kDpM];
};

// e and T_rot of keyframe slot j (one thread each); the column mask and the natural-order rows of its 15 unknowns
__device__ __forceinline__ void dense_prior_local(const DensePriorArgs& P, const int j, const int n_kf, const StateP& s, const uint8_t* __restrict__ pose_const,
                                                  DensePriorLds& L) {
  const int k = P.kf[j];
  const double* x0 = P.x0 + 16 * j;
  const double* q = s.poses + 7 * (size_t)k;
  double* e = L.e + 15 * j;
  {
    const double n = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double n0 = 1.0 / sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2] + x0[3] * x0[3]);
    const double ax = n * q[0], ay = n * q[1], az = n * q[2], aw = n * q[3];
    const double bx = -n0 * x0[0], by = -n0 * x0[1], bz = -n0 * x0[2], bw = n0 * x0[3];      // u0^-1
    double dx = aw * bx + ax * bw + ay * bz - az * by, dy = aw * by - ax * bz + ay * bw + az * bx, dz = aw * bz + ax * by - ay * bx + az * bw;
    double dw = aw * bw - ax * bx - ay * by - az * bz;
    if (dw < 0.0) { dx = -dx; dy = -dy; dz = -dz; dw = -dw; }
    const double nv = sqrt(dx * dx + dy * dy + dz * dz);
    double* T = L.T + 9 * j;
    if (nv == 0.0) {
      e[0] = e[1] = e[2] = 0.0;
      T[0] = T[4] = T[8] = 1.0; T[1] = T[2] = T[3] = T[5] = T[6] = T[7] = 0.0;
    } else {
      const double th = atan2(nv, dw), f = th / nv;
      const double a = f * dx, b = f * dy, c = f * dz, th2 = th * th;
      e[0] = a; e[1] = b; e[2] = c;
      // (1 - theta cot theta) / theta^2: the series below 1e-4 rad, where the closed form loses its digits (1/3 + theta^2/45 + O(theta^4))
      const double g = th2 < 1e-8 ? 1.0 / 3.0 + th2 / 45.0 : (1.0 - th * dw / nv) / th2;
      // I - K + g K^2 with K = [delta]x:  K^2 = delta delta^T - theta^2 I
      T[0] = 1.0 + g * (a * a - th2); T[1] = c + g * a * b;           T[2] = -b + g * a * c;
      T[3] = -c + g * a * b;          T[4] = 1.0 + g * (b * b - th2); T[5] = a + g * b * c;
      T[6] = b + g * a * c;           T[7] = -a + g * b * c;          T[8] = 1.0 + g * (c * c - th2);
    }
  }
  for (int c = 0; c < 3; ++c) {
    e[3 + c] = q[4 + c] - x0[4 + c];
    e[6 + c] = s.vel[3 * (size_t)k + c] - x0[7 + c];
    e[9 + c] = s.ba[3 * (size_t)k + c] - x0[10 + c];
    e[12 + c] = s.bg[3 * (size_t)k + c] - x0[13 + c];
  }
  const int bits = pose_const ? pose_const[k] : 0;
  for (int c = 0; c < 15; ++c) {
    L.cm[15 * j + c] = (c < 6 ? (bits & 1) : (bits & (2 << ((c - 6) / 3)))) ? 0.0 : 1.0;
    L.nat[15 * j + c] = c < 6 ? 6 * k + c : 6 * n_kf + 9 * k + (c - 6);
  }
}

// y = info e + eta into LDS and the cost c0 + 1/2 e^T (y + eta), returned to every thread
__device__ __forceinline__ double dense_prior_y_cost(const DensePriorArgs& P, DensePriorLds& L) {
  const int i = threadIdx.x, m = P.m;
  double part = 0.0;
  if (i < m) {
    const double* info = P.info;
    double acc = 0.0;
    for (int j = 0; j < m; ++j) acc = fma(info[(size_t)max(i, j) * m + min(i, j)], L.e[j], acc);
    const double eta = P.eta[i];
    L.y[i] = acc + eta;
    part = 0.5 * L.e[i] * (acc + 2.0 * eta);
  }
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) L.red[threadIdx.x >> 6] = part;
  __syncthreads();
  double c = P.c0;
  for (int w = 0; w < kDensePriorT / 64; ++w) c += L.red[w];
  return c;
}

__global__ __launch_bounds__(kDensePriorT) void k_dense_prior_cost(DensePriorArgs P, StateP s, double* __restrict__ cost) {
  __shared__ DensePriorLds L;
  if ((int)threadIdx.x < P.n_sel) dense_prior_local(P, threadIdx.x, 0, s, nullptr, L);
  __syncthreads();
  const double c = dense_prior_y_cost(P, L);
  if (threadIdx.x == 0) atomicAdd(cost, c);
}

__global__ __launch_bounds__(kDensePriorT) void k_dense_prior_lin(DensePriorArgs P, int n_kf, StateP s, const uint8_t* __restrict__ pose_const,
                                                                  double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost,
                                                                  double* __restrict__ gout, double* __restrict__ Hout) {
  __shared__ DensePriorLds L;
  const int tid = threadIdx.x, m = P.m;
  if (tid < P.n_sel) dense_prior_local(P, tid, n_kf, s, pose_const, L);
  __syncthreads();
  const double c = dense_prior_y_cost(P, L);
  if (tid == 0) atomicAdd(cost, c);
  // row i of T^T: the three rotation rows of its keyframe for a rotation unknown, itself otherwise
  if (tid < m) {
    const int kj = tid / 15, ci = tid - 15 * kj;
    double g = L.y[tid];
    if (ci < 3) { const double* T = L.T + 9 * kj; const double* y = L.y + 15 * kj; g = T[ci] * y[0] + T[3 + ci] * y[1] + T[6 + ci] * y[2]; }
    g *= L.cm[tid];
    if (gout) gout[tid] = g;
    else if (g != 0.0) atomicAdd(&gc[L.nat[tid]], g);
  }
  const double* info = P.info;
  for (int idx = tid; idx < m * m; idx += kDensePriorT) {
    const int i = idx / m, j = idx - i * m;
    if (j > i) continue;
    const int ki = i / 15, ci = i - 15 * ki, kj = j / 15, cj = j - 15 * kj;
    const int na = ci < 3 ? 3 : 1, nb = cj < 3 ? 3 : 1;
    const int a0 = ci < 3 ? 15 * ki : i, b0 = cj < 3 ? 15 * kj : j;
    double h = 0.0;
    for (int a = 0; a < na; ++a) {
      const double ta = ci < 3 ? L.T[9 * ki + 3 * a + ci] : 1.0;
      const int ra = a0 + a;
      double r = 0.0;
      for (int b = 0; b < nb; ++b) {
        const double tb = cj < 3 ? L.T[9 * kj + 3 * b + cj] : 1.0;
        const int rb = b0 + b;
        r = fma(info[(size_t)max(ra, rb) * m + min(ra, rb)], tb, r);
      }
      h = fma(ta, r, h);
    }
    h *= L.cm[i] * L.cm[j];
    if (Hout) { Hout[(size_t)i * m + j] = h; Hout[(size_t)j * m + i] = h; }
    else if (h != 0.0) {
      const int r = L.nat[i], cc = L.nat[j];
      atomicAdd(&B[(size_t)max(r, cc) * ld + min(r, cc)], h);
    }
  }
}

// fills (creating it first if *dp is null) a prior from checked host arrays; grow-only buffers, so a window re-fills its one object
int dense_prior_assign(lvf_ctx* ctx, lvf_dense_prior** dp, int n_sel, const int32_t* kf, const double* x0, const double* info, const double* eta, double c0) {
  const bool fresh = *dp == nullptr;
  lvf_dense_prior* d = fresh ? new lvf_dense_prior() : *dp;
  const int m = 15 * n_sel;
  d->ctx = ctx; d->n_sel = n_sel; d->m = m; d->c0 = c0;
  d->kf_h.assign(kf, kf + n_sel);
  hipStream_t q = ctx->stream;
  const std::vector<double> zeros((size_t)m, 0.0);
  int rc;
  if ((rc = d->kf.assign(d->kf_h.data(), (size_t)n_sel, q)) || (rc = d->x0.assign(x0, (size_t)16 * n_sel, q)) || (rc = d->info.assign(info, (size_t)m * m, q)) ||
      (rc = d->eta.assign(eta ? eta : zeros.data(), (size_t)m, q))) { (void)hipStreamSynchronize(q); if (fresh) delete d; return rc; }
  const hipError_t e = hipStreamSynchronize(q);      // (the caller's arrays are read until here)
  if (e != hipSuccess) { if (fresh) delete d; return hip_fail(e, "dense prior upload", __FILE__, __LINE__); }
  *dp = d;
  return LVF_OK;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_dense_prior_create(lvf_ctx* ctx, int n_sel, const int32_t* kf_idx, const double* x0, const double* info, const double* eta, double c0,
                           lvf_dense_prior** out) {
  LVF_REQUIRE(ctx && out, "lvf_dense_prior_create: null argument");
  LVF_REQUIRE(n_sel >= 1 && n_sel <= kDensePriorMaxKf, "lvf_dense_prior_create: %d keyframes (1 .. %d)", n_sel, kDensePriorMaxKf);
  LVF_REQUIRE(kf_idx && x0 && info, "lvf_dense_prior_create: null input array");
  const int m = 15 * n_sel;
  for (int i = 0; i < n_sel; ++i) {
    LVF_REQUIRE(kf_idx[i] >= 0, "lvf_dense_prior_create: kf_idx[%d] = %d is negative", i, kf_idx[i]);
    for (int j = 0; j < i; ++j) LVF_REQUIRE(kf_idx[j] != kf_idx[i], "lvf_dense_prior_create: keyframe %d listed twice", kf_idx[i]);
    double n2 = 0.0;
    for (int c = 0; c < 16; ++c) LVF_REQUIRE(std::isfinite(x0[16 * i + c]), "lvf_dense_prior_create: x0 of keyframe slot %d is not finite", i);
    for (int c = 0; c < 4; ++c) n2 += x0[16 * i + c] * x0[16 * i + c];
    LVF_REQUIRE(n2 > 0.0, "lvf_dense_prior_create: x0 of keyframe slot %d has a zero quaternion", i);
  }
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j <= i; ++j) LVF_REQUIRE(std::isfinite(info[(size_t)i * m + j]), "lvf_dense_prior_create: info[%d][%d] is not finite", i, j);
    LVF_REQUIRE(!eta || std::isfinite(eta[i]), "lvf_dense_prior_create: eta[%d] is not finite", i);
  }
  LVF_REQUIRE(std::isfinite(c0), "lvf_dense_prior_create: c0 is not finite");
  LVF_TRY(lvf::enter(ctx));
  lvf_dense_prior* d = nullptr;
  LVF_TRY(dense_prior_assign(ctx, &d, n_sel, kf_idx, x0, info, eta, c0));
  *out = d;
  return LVF_OK;
}

int lvf_dense_prior_destroy(lvf_dense_prior* d) { delete d; return LVF_OK; }

int lvf_dense_prior_size(const lvf_dense_prior* d) { return d ? d->n_sel : -1; }

int lvf_dense_prior_download(lvf_dense_prior* d, int32_t* kf_idx, double* x0, double* info, double* eta, double* c0) {
  LVF_REQUIRE(d, "lvf_dense_prior_download: null prior");
  LVF_TRY(lvf::enter(d->ctx));
  hipStream_t q = d->ctx->stream;
  if (kf_idx) std::copy(d->kf_h.begin(), d->kf_h.end(), kf_idx);
  if (x0) LVF_HIP(hipMemcpyAsync(x0, d->x0.p, (size_t)16 * d->n_sel * 8, hipMemcpyDeviceToHost, q));
  if (info) LVF_HIP(hipMemcpyAsync(info, d->info.p, (size_t)d->m * d->m * 8, hipMemcpyDeviceToHost, q));
  if (eta) LVF_HIP(hipMemcpyAsync(eta, d->eta.p, (size_t)d->m * 8, hipMemcpyDeviceToHost, q));
  LVF_HIP(hipStreamSynchronize(q));
  if (c0) *c0 = d->c0;
  return LVF_OK;
}

int lvf_dense_prior_evaluate(lvf_dense_prior* d, const lvf_state* st, const uint8_t* const_bits, double* cost, double* gradient, double* matrix) {
  LVF_REQUIRE(d && st, "lvf_dense_prior_evaluate: null argument");
  LVF_REQUIRE(st->ctx == d->ctx, "lvf_dense_prior_evaluate: state belongs to another context");
  for (int i = 0; i < d->n_sel; ++i)
    LVF_REQUIRE(d->kf_h[i] < st->n_kf, "lvf_dense_prior_evaluate: the prior references keyframe %d but the state has %d", d->kf_h[i], st->n_kf);
  LVF_TRY(lvf::enter(d->ctx));
  hipStream_t q = d->ctx->stream;
  const size_t m = (size_t)d->m, n_out = m + m * m + kStripes;
  LVF_TRY(d->out.ensure(n_out));
  DevBuf<uint8_t> cb;
  StreamWaitGuard guard(q);
  if (const_bits) LVF_TRY(cb.upload(const_bits, (size_t)st->n_kf, q));
  double* costd = d->out.p + m + m * m;
  LVF_HIP(hipMemsetAsync(costd, 0, kStripes * 8, q));
  hipLaunchKernelGGL(k_dense_prior_lin, dim3(1), dim3(kDensePriorT), 0, q, dense_prior_args(d), st->n_kf, state_ptrs(st), const_bits ? (const uint8_t*)cb.p : nullptr,
                     (double*)nullptr, 0, (double*)nullptr, costd, d->out.p, d->out.p + m);
  LVF_HIP(hipGetLastError());
  std::vector<double> h(n_out);
  LVF_TRY(copy_down_wait(d->ctx, h.data(), d->out.p, n_out * 8));
  guard.dismiss();
  if (cost) *cost = h[m + m * m];
  if (gradient) std::copy(h.begin(), h.begin() + m, gradient);
  if (matrix) std::copy(h.begin() + m, h.begin() + m + m * m, matrix);
  return LVF_OK;
}

int lvf_problem_set_dense_prior(lvf_problem* p, lvf_dense_prior* prior) {
  LVF_REQUIRE(p, "lvf_problem_set_dense_prior: null problem");
  if (prior) {
    LVF_REQUIRE(prior->ctx == p->ctx, "lvf_problem_set_dense_prior: the prior belongs to another context");
    for (int i = 0; i < prior->n_sel; ++i)
      LVF_REQUIRE(prior->kf_h[i] < p->st->n_kf, "lvf_problem_set_dense_prior: the prior references keyframe %d but the window has %d", prior->kf_h[i], p->st->n_kf);
  }
  LVF_TRY(lvf::enter(p->ctx));
  return problem_set_dense_prior(p, prior);
}

}  // extern "C"
