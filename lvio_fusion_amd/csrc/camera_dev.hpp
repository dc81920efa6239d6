// camera_dev.hpp — the rigid camera model of the reference (sensor.h:16-44, camera.h:38-57), stated ONCE for the device and once for the host
// (DESIGN 13).  Every front-end kernel that moves a point between pixel, sensor, robot and world takes these structs and calls these chains.
// The expression forms are the ones the bit-equal Python restatements state (tests/lidar_depth_ref.py): left-to-right sums, one operation each.
// Contraction follows the INCLUDING unit: a unit whose semantics forbid FMA says `#pragma clang fp contract(off)` ahead of its includes.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#include "../../include/lvf.h"

namespace lvf {

struct Rigid { double R[9], t[3]; };                        // p -> R p + t, R row-major; each use says what it maps (body -> world, ...)
struct Pinhole { double fx, fy, cx, cy, R[9], t[3]; };      // R, t: sensor -> robot (the extrinsic)

// Camera::Pixel2Sensor (camera.h:51-57)
__device__ __forceinline__ void pixel2sensor(const Pinhole& c, double u, double v, double depth, double ps[3]) {
  ps[0] = (u - c.cx) * depth / c.fx; ps[1] = (v - c.cy) * depth / c.fy; ps[2] = depth;
}
// Sensor::Sensor2Robot (sensor.h:31-34)
__device__ __forceinline__ void sensor2robot(const Pinhole& c, const double ps[3], double pb[3]) {
  pb[0] = c.R[0] * ps[0] + c.R[1] * ps[1] + c.R[2] * ps[2] + c.t[0];
  pb[1] = c.R[3] * ps[0] + c.R[4] * ps[1] + c.R[5] * ps[2] + c.t[1];
  pb[2] = c.R[6] * ps[0] + c.R[7] * ps[1] + c.R[8] * ps[2] + c.t[2];
}
// p -> R^T (p - t): the inverse of a rigid map, from its rotation and translation
__device__ __forceinline__ void rigid_inverse_apply(const double R[9], const double t[3], const double p[3], double o[3]) {
  const double d[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};
  o[0] = R[0] * d[0] + R[3] * d[1] + R[6] * d[2];
  o[1] = R[1] * d[0] + R[4] * d[1] + R[7] * d[2];
  o[2] = R[2] * d[0] + R[5] * d[1] + R[8] * d[2];
}
// Sensor::Robot2Sensor (sensor.h:36-39)
__device__ __forceinline__ void robot2sensor(const Pinhole& c, const double pb[3], double pc[3]) { rigid_inverse_apply(c.R, c.t, pb, pc); }
// Sensor::World2Robot (sensor.h:26-29); T: body -> world
__device__ __forceinline__ void world2robot(const Rigid& T, const double pw[3], double pb[3]) { rigid_inverse_apply(T.R, T.t, pw, pb); }
// Camera::Sensor2Pixel (camera.h:43-49), rounded to the float pair a keypoint is
__device__ __forceinline__ float2 sensor2pixel(const Pinhole& c, const double pc[3]) {
  return make_float2((float)(c.fx * pc[0] / pc[2] + c.cx), (float)(c.fy * pc[1] / pc[2] + c.cy));
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
inline void unit_quat_matrix(double x, double y, double z, double w, double R[9]) {      // (x, y, z, w) is taken as it comes
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
inline void rot_of_quat(const double q[4], double R[9]) {      // of q / |q|, as Sophus holds it
  const double inv = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  unit_quat_matrix(q[0] * inv, q[1] * inv, q[2] * inv, q[3] * inv, R);
}
inline Pinhole make_pinhole(const lvf_camera& c) {
  Pinhole k;
  k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy;
  rot_of_quat(c.extrinsic, k.R);
  for (int i = 0; i < 3; ++i) k.t[i] = c.extrinsic[4 + i];
  return k;
}
inline Rigid make_rigid(const double pose7[7]) {               // pose7 = [qx, qy, qz, qw, tx, ty, tz]
  Rigid T;
  rot_of_quat(pose7, T.R);
  for (int i = 0; i < 3; ++i) T.t[i] = pose7[4 + i];
  return T;
}

}  // namespace lvf
