// loop_dev.hpp — device pieces shared by the loop-correction tail (loop_kernels.hip), the GNSS alignment (navsat_kernels.hip) and the visual
// relocalisation (reloc_kernels.hip), which all reach it through small_lm.hpp: the workgroup sum of one value (the candidate cost and the
// line search of lm_small, the roll pre-solve's vector sum, the inlier count) and its maximum (the pose chain's gradient norm), the body of PoseGraph::ForwardUpdate
// (src/lvio_fusion/src/pose_graph.cpp:245-252) and the Sophus SE3 operations built from the same arithmetic (Hamilton product re-normalised;
// vectors through Eigen's _transformVector).
#pragma once
#include "lvf_internal.hpp"

namespace lvf {

constexpr int kLT = 256;

// sums `v` over the workgroup of kLT threads; every thread returns the total (two barriers)
__device__ __forceinline__ double wg_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kLT / 64; ++k) s += red[k];
  return s;
}

// the largest `v` of the workgroup of kLT threads; every thread returns it (two barriers)
__device__ __forceinline__ double wg_max(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// Eigen QuaternionBase::_transformVector with the quaternion (ux, uy, uz, uw) taken as it is: uv = 2 u x v ; v + w uv + u x uv
__device__ __forceinline__ void quat_transform_vector(double ux, double uy, double uz, double uw, double v0, double v1, double v2, double o[3]) {
  const double cx = 2.0 * (uy * v2 - uz * v1), cy = 2.0 * (uz * v0 - ux * v2), cz = 2.0 * (ux * v1 - uy * v0);
  o[0] = v0 + uw * cx + (uy * cz - uz * cy); o[1] = v1 + uw * cy + (uz * cx - ux * cz); o[2] = v2 + uw * cz + (ux * cy - uy * cx);
}

// pose <- T * pose (Sophus SE3 product: T's quaternion normalised, Hamilton product re-normalised, t_T + R(q_T) t).  `in` and `out` may be the
// same seven words.
__device__ __forceinline__ void forward_update_pose(const double* T, const double* in, double* out) {
  const double qn = sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]);
  const double ux = T[0] / qn, uy = T[1] / qn, uz = T[2] / qn, uw = T[3] / qn;
  const double bx = in[0], by = in[1], bz = in[2], bw = in[3];
  const double w = uw * bw - ux * bx - uy * by - uz * bz, x = uw * bx + ux * bw + uy * bz - uz * by, y = uw * by + uy * bw + uz * bx - ux * bz,
               z = uw * bz + uz * bw + ux * by - uy * bx;
  const double nn = sqrt(w * w + x * x + y * y + z * z);
  {
    const double v0 = in[4], v1 = in[5], v2 = in[6];
    const double cx = 2.0 * (uy * v2 - uz * v1), cy = 2.0 * (uz * v0 - ux * v2), cz = 2.0 * (ux * v1 - uy * v0);
    out[4] = T[4] + (v0 + uw * cx + (uy * cz - uz * cy)); out[5] = T[5] + (v1 + uw * cy + (uz * cx - ux * cz)); out[6] = T[6] + (v2 + uw * cz + (ux * cy - uy * cx));
  }
  out[0] = x / nn; out[1] = y / nn; out[2] = z / nn; out[3] = w / nn;
}
// Vw <- R(q_T) Vw, in place
__device__ __forceinline__ void forward_update_velocity(const double* T, double* v) {
  const double qn = sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]);
  const double ux = T[0] / qn, uy = T[1] / qn, uz = T[2] / qn, uw = T[3] / qn;
  const double v0 = v[0], v1 = v[1], v2 = v[2];
  const double cx = 2.0 * (uy * v2 - uz * v1), cy = 2.0 * (uz * v0 - ux * v2), cz = 2.0 * (ux * v1 - uy * v0);
  v[0] = v0 + uw * cx + (uy * cz - uz * cy); v[1] = v1 + uw * cy + (uz * cx - ux * cz); v[2] = v2 + uw * cz + (ux * cy - uy * cx);
}

// Sophus SE3::inverse(): (q*, q* (-t)), the quaternion normalised first like the transform of forward_update_pose
__device__ __forceinline__ void sophus_inverse(const double* a, double* inv) {
  const double qn = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
  const double ux = -(a[0] / qn), uy = -(a[1] / qn), uz = -(a[2] / qn), uw = a[3] / qn;
  double t[3];
  quat_transform_vector(ux, uy, uz, uw, -a[4], -a[5], -a[6], t);
  inv[0] = ux; inv[1] = uy; inv[2] = uz; inv[3] = uw; inv[4] = t[0]; inv[5] = t[1]; inv[6] = t[2];
}
// Sophus SE3 * point: R(q) p + t, q as stored
__device__ __forceinline__ void sophus_transform_point(const double* a, double p0, double p1, double p2, double o[3]) {
  double r[3];
  quat_transform_vector(a[0], a[1], a[2], a[3], p0, p1, p2, r);
  o[0] = r[0] + a[4]; o[1] = r[1] + a[5]; o[2] = r[2] + a[6];
}

}  // namespace lvf
