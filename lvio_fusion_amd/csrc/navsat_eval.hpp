// navsat_eval.hpp — the GNSS alignment functors of src/lvio_fusion/include/lvio_fusion/ceres/navsat_error.hpp:9-120 on the device dual
// number DJet<N> (djet.hpp), in the operation order of the functor text, so that the Jacobians are the exact derivatives of the code as
// written, like the reference's AutoDiffCostFunction:
//   NavsatInitError <3,1,1,1>        (yaw, x, y)                          :17-51
//   NavsatRXError   <3,1,1,1,1,1,1>  (yaw, pitch, roll, x, y, z)          :53-91
//   NavsatRError    <1,1>            (roll)                               :93-120
//   cov2sqrt_info                                                          :9-15
// cov2sqrt_info is only ever handed a diagonal covariance: sqrt_info_k = sqrt(1.0 / cov_k) here.  The reference goes through Eigen's 3x3
// inverse() (cofactors over the determinant) and LLT; on a diagonal matrix those compute the same numbers up to the LAST BIT (the
// determinant product and its division round differently from 1.0 / cov_k).  Declared, not pinned.
#pragma once
#include "se3_jet.hpp"

namespace lvf {

__device__ __forceinline__ double jsin(double x) { return sin(x); }
__device__ __forceinline__ double jcos(double x) { return cos(x); }
template <int N>
__device__ __forceinline__ DJet<N> jsin(const DJet<N>& x) {
  DJet<N> r;
  r.a = sin(x.a);
  const double d = cos(x.a);
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = d * x.v[i];
  return r;
}
template <int N>
__device__ __forceinline__ DJet<N> jcos(const DJet<N>& x) {
  DJet<N> r;
  r.a = cos(x.a);
  const double d = -sin(x.a);
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = d * x.v[i];
  return r;
}

// base.hpp:110-132  RPYToEigenQuaternion: rpy[0] = yaw (Z), rpy[1] = pitch (Y), rpy[2] = roll (X); out x,y,z,w
template <typename T>
__device__ __forceinline__ void rpy_to_eigen_quat(const T rpy[3], T eq[4]) {
  const T z = rpy[0] / T(2.0), y = rpy[1] / T(2.0), x = rpy[2] / T(2.0);
  const T c_z = jcos(z), s_z = jsin(z), c_y = jcos(y), s_y = jsin(y), c_x = jcos(x), s_x = jsin(x);
  eq[3] = c_z * c_y * c_x + s_z * s_y * s_x;
  eq[0] = c_z * c_y * s_x - s_z * s_y * c_x;
  eq[1] = c_z * s_y * c_x + s_z * c_y * s_x;
  eq[2] = s_z * c_y * c_x - c_z * s_y * s_x;
}
// base.hpp:143-150
template <typename T>
__device__ __forceinline__ void rpyxyz_to_se3(const T rpyxyz[6], T out[7]) {
  rpy_to_eigen_quat(rpyxyz, out);
  out[4] = rpyxyz[3]; out[5] = rpyxyz[4]; out[6] = rpyxyz[5];
}
// base.hpp:33-38
template <typename T>
__device__ __forceinline__ void se3_transform_point(const T se3[7], const T pt[3], T out[3]) {
  eigen_quat_rotate(se3, pt, out);
  out[0] = out[0] + se3[4]; out[1] = out[1] + se3[5]; out[2] = out[2] + se3[6];
}

__device__ __forceinline__ double cov2sqrt_info(double cov) { return sqrt(1.0 / cov); }

// navsat_error.hpp:27-40
template <int N>
__device__ __forceinline__ void navsat_init_functor(const double p0[3], const double p1[3], const double sqrt_info[3], const DJet<N>& yaw,
                                                    const DJet<N>& x, const DJet<N>& y, DJet<N> r[3]) {
  typedef DJet<N> T;
  T tf[7];
  const T rpyxyz[6] = {yaw, T(0.0), T(0.0), x, y, T(0.0)};
  rpyxyz_to_se3(rpyxyz, tf);
  const T q1[3] = {T(p1[0]), T(p1[1]), T(p1[2])};
  T tf_p1[3];
  se3_transform_point(tf, q1, tf_p1);
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = T(sqrt_info[k]) * (T(p0[k]) - tf_p1[k]);
}

// navsat_error.hpp:64-79   rpyxyz = (yaw, pitch, roll, x, y, z)
template <int N>
__device__ __forceinline__ void navsat_rx_functor(const double p0[3], const double p1[3], const double pose7[7], const double sqrt_info[3],
                                                  const DJet<N> rpyxyz[6], DJet<N> r[3]) {
  typedef DJet<N> T;
  T pose[7], tf[7], relative_pose[7];
  rpyxyz_to_se3(rpyxyz, relative_pose);
#pragma unroll
  for (int k = 0; k < 7; ++k) pose[k] = T(pose7[k]);
  se3_product(pose, relative_pose, tf);
  const T q1[3] = {T(p1[0]), T(p1[1]), T(p1[2])};
  T tf_p1[3];
  se3_transform_point(tf, q1, tf_p1);
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = T(sqrt_info[k]) * (T(p0[k]) - tf_p1[k]);
}

// navsat_error.hpp:98-110
template <int N>
__device__ __forceinline__ DJet<N> navsat_r_functor(const double y3[3], const double pose7[7], const DJet<N>& roll) {
  typedef DJet<N> T;
  const T rpy[3] = {T(0.0), T(0.0), roll};
  T relative_pose[4], pose[4], y[3], tf_y[3];
  rpy_to_eigen_quat(rpy, relative_pose);
#pragma unroll
  for (int k = 0; k < 4; ++k) pose[k] = T(pose7[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = T(y3[k]);
  const T z[4] = {pose[3], pose[0], pose[1], pose[2]}, w[4] = {relative_pose[3], relative_pose[0], relative_pose[1], relative_pose[2]};
  T zw[4];
  quat_product_wxyz(z, w, zw);
  const T pb[4] = {zw[1], zw[2], zw[3], zw[0]};
  eigen_quat_rotate(pb, y, tf_y);
  return tf_y[2];
}

}  // namespace lvf
