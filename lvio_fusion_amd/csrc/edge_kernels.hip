// edge_kernels.hip — the point-to-line factor evaluated stand-alone, and one frame's scan-to-map update with lines.
//
// LidarEdgeErrorYXY / LidarEdgeErrorRPZ <3,1,1,1>: r = w P (Twc2 p - c), Twc2 = Twc1 * RpyxyzToSE3(rpyxyz) formed as LidarPlaneErrorYXY / RPZ
// form it (src/lvio_fusion/include/lvio_fusion/ceres/lidar_error.hpp:42-110).  The reference declares edge clouds (lidar/feature.h:23-24) and
// has no edge functor at this commit: the factor is DECLARED (tests/edge_ref.py).  Row k is the plane residual with normal P[k,:] and anchor
// c, so the device math is lidar_point (lidar_eval.hpp) three times.  The association lives with the 3-NN (knn_kernels.hip), the solve with
// the 3-DoF LM (icp_kernels.hip).
#include <cmath>
#include "host_se3.hpp"
#include "lidar_eval.hpp"
#include "lvf_internal.hpp"

namespace lvf {

constexpr int kET = 256;

// one thread per block; Twc2 and its derivatives are derived once per workgroup into LDS
template <bool WANT_J>
__global__ __launch_bounds__(kET) void k_lidar_edge_eval(int n, const double* __restrict__ p, const double* __restrict__ c, const double* __restrict__ proj,
                                                         const LidarArgs a, double* __restrict__ res, double* __restrict__ jac) {
  __shared__ LidarU U;
  if (threadIdx.x == 0) derive_lidar(a, U);
  __syncthreads();
  const int i = blockIdx.x * kET + threadIdx.x;
  if (i >= n) return;
  const double pp[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]}, cc[3] = {c[3 * (size_t)i], c[3 * (size_t)i + 1], c[3 * (size_t)i + 2]};
  double pr[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) pr[k] = proj[6 * (size_t)i + k];
  double r[3], J[3][3];
  lidar_edge_block(U, a.mode, pp, cc, pr, r, J);
#pragma unroll
  for (int k = 0; k < 3; ++k) res[3 * (size_t)i + k] = r[k];
  if (WANT_J) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) jac[9 * (size_t)i + 3 * k + j] = J[k][j];
  }
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_lidar_edge_evaluate(lvf_ctx* ctx, int mode, int n, const double* p, const double* c, const double* proj6, const double* Twc1, const double* rpyxyz,
                            double weight, double* residuals, double* jacobians) {
  LVF_REQUIRE(ctx && Twc1 && rpyxyz, "lvf_lidar_edge_evaluate: null argument");
  LVF_REQUIRE(mode == 0 || mode == 1, "lvf_lidar_edge_evaluate: mode must be 0 (RPZ) or 1 (YXY)");
  LVF_REQUIRE(n >= 0 && (n == 0 || (p && c && proj6 && residuals)), "lvf_lidar_edge_evaluate: bad block arrays");
  LVF_REQUIRE(Twc1[0] * Twc1[0] + Twc1[1] * Twc1[1] + Twc1[2] * Twc1[2] + Twc1[3] * Twc1[3] > 0.0, "lvf_lidar_edge_evaluate: zero quaternion");
  if (n == 0) return LVF_OK;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<double> dp, dc, dpr, r, J;
  LVF_TRY(dp.upload(p, (size_t)3 * n, s)); LVF_TRY(dc.upload(c, (size_t)3 * n, s)); LVF_TRY(dpr.upload(proj6, (size_t)6 * n, s));
  LVF_TRY(r.alloc((size_t)3 * n));
  LidarArgs a;
  std::memcpy(a.Twc1, Twc1, sizeof(a.Twc1)); std::memcpy(a.rpyxyz, rpyxyz, sizeof(a.rpyxyz));
  a.weight = weight; a.mode = mode;
  const dim3 grid((n + kET - 1) / kET), block(kET);
  if (jacobians) {
    LVF_TRY(J.alloc((size_t)9 * n));
    hipLaunchKernelGGL(k_lidar_edge_eval<true>, grid, block, 0, s, n, dp.p, dc.p, dpr.p, a, r.p, J.p);
  } else {
    hipLaunchKernelGGL(k_lidar_edge_eval<false>, grid, block, 0, s, n, dp.p, dc.p, dpr.p, a, r.p, (double*)nullptr);
  }
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(residuals, r.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  if (jacobians) LVF_HIP(hipMemcpyAsync(jacobians, J.p, (size_t)9 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

// Mapping::Optimize's per-frame body / Mapping::Relocate (mapping.cpp:147-178, :251-300) with planes AND lines in the (yaw, x, y) sub-problem.
// A single-frame chain: the pose is composed on the host between the sub-problems (host_se3.hpp), one wait per sub-problem.
int lvf_scan_match_edges(lvf_map* map_ground, lvf_scan* scan_ground, lvf_map* map_surf, lvf_scan* scan_surf, lvf_map* map_edge, lvf_scan* scan_edge,
                         const double* map_pose, const double* frame_pose, const double* last_pose, const lvf_scan_match_options* opt,
                         const lvf_edge_icp_options* edge_opt, lvf_scan_match_result* out) {
  LVF_REQUIRE((map_edge != nullptr) == (scan_edge != nullptr), "lvf_scan_match_edges: a map and its scan must be given together");
  if (!map_edge) return lvf_scan_match(map_ground, scan_ground, map_surf, scan_surf, map_pose, frame_pose, last_pose, opt, out);
  LVF_REQUIRE(map_pose && frame_pose && opt && edge_opt && out, "lvf_scan_match_edges: null argument");
  LVF_REQUIRE((map_ground != nullptr) == (scan_ground != nullptr) && (map_surf != nullptr) == (scan_surf != nullptr),
              "lvf_scan_match_edges: a map and its scan must be given together");
  LVF_REQUIRE(opt->outer_iterations >= 1 && opt->max_num_iterations >= 0, "lvf_scan_match_edges: bad options");
  const bool has_ground = map_ground && map_ground->M > 0;
  const bool has_surf = map_surf && map_surf->M > 0;            // (an empty map: the reference skips that cloud)
  double pose[7], minv[7];
  std::memcpy(pose, frame_pose, sizeof(pose));
  hse3::inv(map_pose, minv);
  std::memset(out, 0, sizeof(*out));
  double score[2] = {0.0, 0.0};
  const double cap[2] = {20.0, 30.0};                            // mapping.cpp:279, :293
  for (int it = 0; it < opt->outer_iterations; ++it) {
    double rel[7], rpyxyz[6], dT[7];
    hse3::mul(minv, pose, rel);
    hse3::to_rpyxyz(rel, rpyxyz);                                // mapping.cpp:154, :264-266
    for (int m = 0; m < 2; ++m) {
      if (m == 0 && !has_ground) continue;
      lvf_icp_options o;
      o.mode = m; o.thr = m == 0 ? opt->thr_ground : opt->thr_surf; o.weight = m == 0 ? opt->weight_ground : opt->weight_surf;
      o.huber_a = m == 0 ? 0.0 : opt->huber_surf; o.prior_weight = opt->prior_weight; o.max_num_iterations = opt->max_num_iterations;
      lvf_icp_summary& s = m == 0 ? out->ground : out->surf;
      if (m == 0) LVF_TRY(lvf_icp_solve(map_ground, scan_ground, map_pose, pose, rpyxyz, &o, &s));
      else LVF_TRY(lvf_icp_solve_edges(has_surf ? map_surf : nullptr, has_surf ? scan_surf : nullptr, map_edge, scan_edge, map_pose, pose, rpyxyz, &o, edge_opt, &s));
      hse3::from_rpyxyz(rpyxyz, dT);
      hse3::mul(map_pose, dT, pose);                             // frame->pose = map_frame->pose * rpyxyz2se3(rpyxyz)
      const int nr = s.num_residual_blocks;
      score[m] = std::fmin((double)nr / 10, cap[m]) - (nr > 0 ? 2 * s.final_cost / nr : 0.0);
    }
  }
  std::memcpy(out->pose, pose, sizeof(pose));
  if (last_pose) { double linv[7]; hse3::inv(last_pose, linv); hse3::mul(linv, pose, out->relative_o_c); }
  else std::memcpy(out->relative_o_c, pose, sizeof(pose));
  out->score_ground = score[0]; out->score_surf = score[1];
  out->score = (int)(score[0] + score[1]);
  return LVF_OK;
}

}  // extern "C"
