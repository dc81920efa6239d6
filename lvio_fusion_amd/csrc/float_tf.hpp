// float_tf.hpp — the bit-exact float32 SE3 transform and the ordered-uint float encoding, shared by knn_kernels.hip and cloud_kernels.hip.
// ONLY for translation units that are contraction-free THROUGHOUT: the including file states `#pragma clang fp contract(off)` at its top,
// before its first function.  In a unit compiled with the default -ffp-contract=fast, code that inlines these functions could still fuse
// what it does with their results, and the bit-exact results (the transform, d2) would no longer round after every multiply and add.
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>

// (stated here as well, before the first function: HIP's own __fmul_rn/__fadd_rn are plain operators compiled with the `contract` flag and
// DO get fused after inlining — checked in the ISA — so the primitives are declared under the pragma)
#pragma clang fp contract(off)

namespace lvf {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }

struct TfArg { float v[7]; };   // a pose as a kernel argument: quaternion xyzw, translation
static inline TfArg tf_arg(const double* pose) {   // Sophus SE3d::cast<float>()  association.cpp:287, mapping.cpp:195
  TfArg tf;
  for (int k = 0; k < 7; ++k) tf.v[k] = (float)pose[k];
  return tf;
}

struct Tf32 { float a[9]; float t[3]; };   // out = 2*((a0 p0 + a1 p1) + a2 p2) + p0 + t0 ...

// float instantiation of ceres::QuaternionRotatePoint (1.x): normalise, then the expanded polynomial (oracle/se3_ops.h UnitQuatRotate_wxyz,
// oracle/knn.h::transform_query_f32), RN ops only
__device__ __forceinline__ Tf32 make_tf32(const float tf[7]) {
  const float q0 = tf[3], q1 = tf[0], q2 = tf[1], q3 = tf[2];
  const float ss = add_rn(add_rn(add_rn(mul_rn(q0, q0), mul_rn(q1, q1)), mul_rn(q2, q2)), mul_rn(q3, q3));
  const float scale = div_rn(1.0f, sqrt_rn(ss));
  const float u0 = mul_rn(scale, q0), u1 = mul_rn(scale, q1), u2 = mul_rn(scale, q2), u3 = mul_rn(scale, q3);
  const float t2 = mul_rn(u0, u1), t3 = mul_rn(u0, u2), t4 = mul_rn(u0, u3);
  const float t5 = mul_rn(-u1, u1), t6 = mul_rn(u1, u2), t7 = mul_rn(u1, u3);
  const float t8 = mul_rn(-u2, u2), t9 = mul_rn(u2, u3), t1 = mul_rn(-u3, u3);
  Tf32 T;
  T.a[0] = add_rn(t8, t1); T.a[1] = sub_rn(t6, t4); T.a[2] = add_rn(t3, t7);
  T.a[3] = add_rn(t4, t6); T.a[4] = add_rn(t5, t1); T.a[5] = sub_rn(t9, t2);
  T.a[6] = sub_rn(t7, t3); T.a[7] = add_rn(t2, t9); T.a[8] = add_rn(t5, t8);
  T.t[0] = tf[4]; T.t[1] = tf[5]; T.t[2] = tf[6];
  return T;
}
__device__ __forceinline__ float tf_row(const float* a, float p0, float p1, float p2, float pk, float t) {
  const float s = add_rn(add_rn(mul_rn(a[0], p0), mul_rn(a[1], p1)), mul_rn(a[2], p2));
  return add_rn(add_rn(mul_rn(2.0f, s), pk), t);
}

// floats as unsigned ints of the same order (bounding boxes reduce with integer atomicMin / atomicMax)
__device__ __forceinline__ unsigned f2ord(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float ord2f(unsigned u) {
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f; memcpy(&f, &u, 4); return f;
}

}  // namespace lvf
