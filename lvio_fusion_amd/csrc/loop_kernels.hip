// loop_kernels.hip — the loop-correction tail after the multi-GPU candidate gather, on device:
//
//   RelocateRError <7,4>                           src/lvio_fusion/include/lvio_fusion/ceres/pose_error.hpp:192-222
//   Relocator::UpdateNewSubmap's rotation solve    src/lvio_fusion/src/relocator.cpp:247-268
//       one quaternion parameter r under EigenQuaternionParameterization, one RelocateRError(relocated_i, unrelocated_i) per keyframe
//       of the new submap, no loss function, ceres::Solve(DENSE_QR) with default options;
//   PoseGraph::ForwardUpdate                       src/lvio_fusion/src/pose_graph.cpp:245-252   (also Backend::UpdateFrontend, backend.cpp:256)
//       pose <- transform * pose, Vw <- transform.unit_quaternion() * Vw for every keyframe after the corrected section.
//
// RelocateRError goes through SE3Product of the UN-normalised parameter quaternion (the rotation of the translation normalises it,
// the quaternion product does not), so its ambient 7x4 Jacobian is taken exactly as the reference's autodiff does: dual numbers
// (djet.hpp).  The problem has 3 tangent unknowns and a few dozen blocks: the whole LM loop (lm_small, small_lm.hpp: linearise, damped
// 3x3 solve, candidate cost, accept / reject, trust-region update, termination tests) is ONE launch of one workgroup; the host reads one
// record.
#include "lvf_internal.hpp"
#include "se3_jet.hpp"
#include "small_lm.hpp"

namespace lvf {

// residual r[7] (+ ambient J[7][4], row-major) of one block at quaternion q (x,y,z,w)
template <bool WITH_J>
__device__ __forceinline__ void relocate_r_eval(const double* __restrict__ relocated, const double* __restrict__ unrelocated, const double q[4], double r[7],
                                                double J[28]) {
  typedef DJet<4> T;
  T R[7], U[7], RU[7];
#pragma unroll
  for (int k = 0; k < 4; ++k) R[k] = WITH_J ? T(q[k], k) : T(q[k]);
  R[4] = T(0.0); R[5] = T(0.0); R[6] = T(0.0);
#pragma unroll
  for (int k = 0; k < 7; ++k) U[k] = T(unrelocated[k]);
  se3_product(R, U, RU);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    r[k] = relocated[k] - RU[k].a;
    if (WITH_J) {
#pragma unroll
      for (int c = 0; c < 4; ++c) J[4 * k + c] = -RU[k].v[c];
    }
  }
}

template <bool WITH_J>
__global__ __launch_bounds__(64) void k_relocate_r(int n, const double* __restrict__ relocated, const double* __restrict__ unrelocated,
                                                   const double* __restrict__ q4, double* __restrict__ res, double* __restrict__ jac) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double q[4] = {q4[0], q4[1], q4[2], q4[3]};
  double r[7], J[28];
  relocate_r_eval<WITH_J>(relocated + 7 * i, unrelocated + 7 * i, q, r, J);
#pragma unroll
  for (int k = 0; k < 7; ++k) res[7 * i + k] = r[k];
  if (WITH_J) {
#pragma unroll
    for (int k = 0; k < 28; ++k) jac[28 * i + k] = J[k];
  }
}

// lm_small's problem (small_lm.hpp): the RelocateRError blocks on one quaternion, 4 ambient coordinates and 3 tangent unknowns, no loss function
struct RelocateR {
  static constexpr bool kBox = false;
  int n;
  const double *relocated, *unrelocated;
  __device__ __forceinline__ void accumulate(const double* q, unsigned, double* acc) const {
    // EigenQuaternionParameterization::ComputeJacobian at q
    const double P[12] = {q[3], q[2], -q[1], -q[2], q[3], q[0], q[1], -q[0], q[3], -q[0], -q[1], -q[2]};
    for (int i = threadIdx.x; i < n; i += kLT) {
      double r[7], J[28];
      relocate_r_eval<true>(relocated + 7 * i, unrelocated + 7 * i, q, r, J);
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        acc[9] += 0.5 * r[k] * r[k];
        double l[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) l[x] = J[4 * k] * P[x] + J[4 * k + 1] * P[3 + x] + J[4 * k + 2] * P[6 + x] + J[4 * k + 3] * P[9 + x];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          acc[6 + u] += l[u] * r[k];
#pragma unroll
          for (int v = 0; v <= u; ++v) acc[u * (u + 1) / 2 + v] += l[u] * l[v];
        }
      }
    }
  }
  __device__ __forceinline__ double cost_part(const double* q) const {
    double c = 0.0;
    for (int i = threadIdx.x; i < n; i += kLT) {
      double r[7], J[28];
      relocate_r_eval<false>(relocated + 7 * i, unrelocated + 7 * i, q, r, J);
#pragma unroll
      for (int k = 0; k < 7; ++k) c += 0.5 * r[k] * r[k];
    }
    return c;
  }
  // EigenQuaternionParameterization::Plus
  __device__ __forceinline__ void plus(const double* q, const double* dx, double* qc) const {
    qc[0] = q[0]; qc[1] = q[1]; qc[2] = q[2]; qc[3] = q[3];
    const double dn = sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
    if (dn > 0.0) {
      const double sn = sin(dn) / dn, cw = cos(dn);
      const double ax = sn * dx[0], ay = sn * dx[1], az = sn * dx[2];
      qc[3] = cw * q[3] - ax * q[0] - ay * q[1] - az * q[2];
      qc[0] = cw * q[0] + ax * q[3] + ay * q[2] - az * q[1];
      qc[1] = cw * q[1] - ax * q[2] + ay * q[3] + az * q[0];
      qc[2] = cw * q[2] + ax * q[1] - ay * q[0] + az * q[3];
    }
  }
  __device__ __forceinline__ unsigned norm_mask(unsigned) const { return 15u; }
};

struct RelocRecord { double q[4]; LmRec lm; };

// Jacobi scaling frozen at iteration 0 is Ceres' default jacobi_scaling: relocator.cpp:259 solves with default options.  This problem's
// restatement: oracle/loop.h.
__global__ __launch_bounds__(kLT) void k_relocate_solve(int n, const double* __restrict__ relocated, const double* __restrict__ unrelocated,
                                                        const double* __restrict__ q_in, LmOpts o, RelocRecord* __restrict__ out) {
  __shared__ double tile[lm_tile_doubles(3)];
  double q[4] = {q_in[0], q_in[1], q_in[2], q_in[3]};
  LmRec rec;
  lm_small<3, 4, true>(RelocateR{n, relocated, unrelocated}, n, q, 7u, o, rec, tile);
  if (threadIdx.x == 0) {
    out->q[0] = q[0]; out->q[1] = q[1]; out->q[2] = q[2]; out->q[3] = q[3];
    out->lm = rec;
  }
}

// PoseGraph::ForwardUpdate: Sophus SE3 product (Hamilton product re-normalised; translation through Eigen's _transformVector): loop_dev.hpp
__global__ __launch_bounds__(kLT) void k_forward_update(int n, const double* __restrict__ T, double* __restrict__ poses, double* __restrict__ vw) {
  const int i = blockIdx.x * kLT + threadIdx.x;
  if (i >= n) return;
  double* p = poses + (size_t)7 * i;
  forward_update_pose(T, p, p);
  if (vw) forward_update_velocity(T, vw + (size_t)3 * i);
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_relocate_r_evaluate(lvf_ctx* ctx, int n, const double* relocated, const double* unrelocated, const double* q4, double* residuals, double* jacobians) {
  LVF_REQUIRE(ctx && q4 && residuals, "lvf_relocate_r_evaluate: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || (relocated && unrelocated)), "lvf_relocate_r_evaluate: bad block arrays");
  if (n == 0) return LVF_OK;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> a, b, q, r, J;
  LVF_TRY(a.upload(relocated, (size_t)7 * n, s)); LVF_TRY(b.upload(unrelocated, (size_t)7 * n, s)); LVF_TRY(q.upload(q4, 4, s));
  LVF_TRY(r.alloc((size_t)7 * n));
  if (jacobians) {
    LVF_TRY(J.alloc((size_t)28 * n));
    hipLaunchKernelGGL(k_relocate_r<true>, dim3((n + 63) / 64), dim3(64), 0, s, n, a.p, b.p, q.p, r.p, J.p);
  } else {
    hipLaunchKernelGGL(k_relocate_r<false>, dim3((n + 63) / 64), dim3(64), 0, s, n, a.p, b.p, q.p, r.p, (double*)nullptr);
  }
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(residuals, r.p, (size_t)7 * n * 8, hipMemcpyDeviceToHost, s));
  if (jacobians) LVF_HIP(hipMemcpyAsync(jacobians, J.p, (size_t)28 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_relocate_rotation_solve(lvf_ctx* ctx, int n, const double* relocated, const double* unrelocated, double* q4, const lvf_solver_options* o,
                                lvf_solver_summary* summary) {
  LVF_REQUIRE(ctx && q4 && o && summary, "lvf_relocate_rotation_solve: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || (relocated && unrelocated)), "lvf_relocate_rotation_solve: bad block arrays");
  LVF_REQUIRE(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3] > 0.0, "lvf_relocate_rotation_solve: zero quaternion");
  std::memset(summary, 0, sizeof(*summary));
  summary->num_residual_blocks = n;
  if (n == 0) return LVF_OK;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> a, b, q;
  DevBuf<RelocRecord> rec;
  LVF_TRY(a.upload(relocated, (size_t)7 * n, s)); LVF_TRY(b.upload(unrelocated, (size_t)7 * n, s)); LVF_TRY(q.upload(q4, 4, s)); LVF_TRY(rec.alloc(1));
  const LmOpts lo{o->max_num_iterations, o->function_tolerance, o->gradient_tolerance, o->parameter_tolerance, o->min_relative_decrease,
                  o->initial_trust_region_radius};
  hipLaunchKernelGGL(k_relocate_solve, dim3(1), dim3(kLT), 0, s, n, a.p, b.p, q.p, lo, rec.p);
  LVF_HIP(hipGetLastError());
  RelocRecord h;
  LVF_HIP(hipMemcpyAsync(&h, rec.p, sizeof(h), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  const LmRec& r = h.lm;
  if (r.termination == 2 || !std::isfinite(r.final_cost)) { summary->termination = 2; summary->initial_cost = r.initial_cost; summary->final_cost = r.initial_cost; return LVF_OK; }   // fail soft: q4 untouched
  std::memcpy(q4, h.q, 32);
  summary->initial_cost = r.initial_cost; summary->final_cost = r.final_cost; summary->num_iterations = r.iters; summary->num_successful_steps = r.successes;
  summary->termination = r.termination; summary->num_unsuccessful_steps = r.iters - r.successes;
  return LVF_OK;
}

int lvf_forward_update(lvf_ctx* ctx, const double* transform7, int n, double* poses, double* vw) {
  LVF_REQUIRE(ctx && transform7, "lvf_forward_update: null argument");
  LVF_REQUIRE(n >= 0 && (n == 0 || poses), "lvf_forward_update: bad pose array");
  LVF_REQUIRE(transform7[0] * transform7[0] + transform7[1] * transform7[1] + transform7[2] * transform7[2] + transform7[3] * transform7[3] > 0.0,
              "lvf_forward_update: zero quaternion");
  if (n == 0) return LVF_OK;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> T, P, V;
  LVF_TRY(T.upload(transform7, 7, s)); LVF_TRY(P.upload(poses, (size_t)7 * n, s));
  if (vw) LVF_TRY(V.upload(vw, (size_t)3 * n, s));
  hipLaunchKernelGGL(k_forward_update, dim3((n + kLT - 1) / kLT), dim3(kLT), 0, s, n, T.p, P.p, vw ? V.p : (double*)nullptr);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(poses, P.p, (size_t)7 * n * 8, hipMemcpyDeviceToHost, s));
  if (vw) LVF_HIP(hipMemcpyAsync(vw, V.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_state_forward_update(lvf_state* st, const double* transform7, int first_kf) {
  LVF_REQUIRE(st && transform7, "lvf_state_forward_update: null argument");
  LVF_REQUIRE(first_kf >= 0 && first_kf <= st->n_kf, "lvf_state_forward_update: first_kf %d out of range [0,%d]", first_kf, st->n_kf);
  LVF_REQUIRE(transform7[0] * transform7[0] + transform7[1] * transform7[1] + transform7[2] * transform7[2] + transform7[3] * transform7[3] > 0.0,
              "lvf_state_forward_update: zero quaternion");
  const int n = st->n_kf - first_kf;
  if (n == 0) return LVF_OK;
  LVF_TRY(lvf::enter(st->ctx));
  hipStream_t s = st->ctx->stream;
  DevBuf<double> T;
  LVF_TRY(T.upload(transform7, 7, s));
  hipLaunchKernelGGL(k_forward_update, dim3((n + kLT - 1) / kLT), dim3(kLT), 0, s, n, T.p, st->poses.p + (size_t)7 * first_kf, st->vel.p + (size_t)3 * first_kf);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipStreamSynchronize(s));     // T is released on return
  return LVF_OK;
}

}  // extern "C"
