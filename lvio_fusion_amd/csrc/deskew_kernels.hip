// deskew_kernels.hip — motion compensation of a LiDAR sweep on the device: the step the reference declares four times and never
// calls — the `deskew` key of its configs (estimator.cpp:152), FeatureAssociation::deskew_ (association.h:22,65), the `//TODO:deskew` of
// AdjustDistortion (association.cpp:142-145) and the implementation written for it:
//   Map::ComputePose (map.cpp:92-102)                                              -> pose_between + the bracket search, lvf_trajectory_compute_pose
//   FeatureAssociation::UndistortPoint / UndistortPointCloud (association.cpp:65-83) -> k_deskew, lvf_cloud_deskew
//   Lidar::Sensor2World / World2Sensor (sensor.h:16-24)                              -> the two rigid maps around the interpolated pose
// The semantics are the DECLARED ones of tests/deskew_ref.py, which restates those lines and names two deviations: the bracket is
// (last stamp <= t, the next one) with s NOT clamped (the reference's lower_bound / upper_bound pair names one keyframe twice), and the time
// offset is I - floorf(I + 0.5f) (the reference's I - int(I) is one second off for a negative offset on ring >= 1).
//
// One thread per point: a float4 load, the point's time in float / double as declared, the bracket, Eigen's slerp and the lerp in double,
// p2 = A (T(t) (E p)) with E the extrinsic and A = E^-1 T_f^-1 composed on the host, a float4 store: 32 bytes per point.  The trajectory is
// ONE device array of 8 doubles per knot (stamp, q, t).  The host narrows it to the knots that bracket the sweep (+- a quarter cycle: the
// offset's range is about [-0.25, 1.25] cycle); at most kFastKnots of them are staged in LDS per workgroup and a point whose time lies in the
// narrowed window counts stamps there.  Any other point — and every point of a sweep that spans more knots than the stage holds — takes a
// binary search over the whole array: the bracket is the same, so is every operation after it.  The point count may live on the device
// (n_dev: the extraction's picks), the launch then covers the capacity.
#pragma clang fp contract(off)      // ahead of the includes: the unit's semantics are contraction-free, shared inline chains included

#include "host_se3.hpp"
#include "lvf_internal.hpp"

#include <cfloat>
#include <cmath>

struct lvf_trajectory {
  lvf_ctx* ctx = nullptr;
  std::vector<double> knots;         // [n][8]: stamp, qx, qy, qz, qw (unit), tx, ty, tz — the host copy narrows the sweep
  lvf::DevBuf<double> dev;           // the same on the device
  int n = 0;
};

namespace lvf {

constexpr int kD = 256;

// clamp(#{stamps <= t} - 1, 0, n - 2) by bisection over knots[n][8]; n >= 2.  A NaN time counts no stamp.
__host__ __device__ inline int bracket_search(const double* __restrict__ knots, int n, double t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (knots[(size_t)mid * 8] <= t) lo = mid + 1; else hi = mid;
  }
  const int i = lo - 1;
  return i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
}

// Map::ComputePose between two knots a, b ([8] each): s = (t - stamp_a) / (stamp_b - stamp_a), not clamped; Eigen's Quaternion::slerp, the
// SE3d(q, t) constructor's normalisation, the translation's lerp
__host__ __device__ inline void pose_between(const double* a, const double* b, double t, double q[4], double p[3]) {
  const double s = (t - a[0]) / (b[0] - a[0]);
  const double d = ((a[1] * b[1] + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4];
  const double ad = fabs(d);
  double w0, w1;
  if (ad >= 1.0 - DBL_EPSILON) { w0 = 1.0 - s; w1 = s; }
  else {
    const double th = acos(ad), sn = sin(th);
    w0 = sin((1.0 - s) * th) / sn; w1 = sin(s * th) / sn;
  }
  if (d < 0.0) w1 = -w1;
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = w0 * a[1 + k] + w1 * b[1 + k];
  const double inv = 1.0 / sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = r[k] * inv;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = (1.0 - s) * a[5 + k] + s * b[5 + k];
}

// lvf_trajectory_compute_pose: one thread per time, the bracket by bisection
__global__ __launch_bounds__(kD) void k_traj_pose(int m, const double* __restrict__ times, const double* __restrict__ knots, int n, double* __restrict__ out) {
  const int i = blockIdx.x * kD + threadIdx.x;
  if (i >= m) return;
  double q[4], p[3];
  if (n == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = knots[1 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = knots[5 + k];
  } else {
    const double t = times[i];
    const int b = bracket_search(knots, n, t);
    pose_between(knots + (size_t)b * 8, knots + (size_t)b * 8 + 8, t, q, p);
  }
  double* o = out + (size_t)i * 7;
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = p[0]; o[5] = p[1]; o[6] = p[2];
}

__device__ __forceinline__ void rt_apply(const Rigid& M, const double v[3], double o[3]) {
  o[0] = ((M.R[0] * v[0] + M.R[1] * v[1]) + M.R[2] * v[2]) + M.t[0];
  o[1] = ((M.R[3] * v[0] + M.R[4] * v[1]) + M.R[5] * v[2]) + M.t[1];
  o[2] = ((M.R[6] * v[0] + M.R[7] * v[1]) + M.R[8] * v[2]) + M.t[2];
}

// UndistortPointCloud.  in == out is allowed (a thread reads and writes its own point only).
__global__ __launch_bounds__(kD) void k_deskew(int cap, const int* __restrict__ n_dev, const float4* in, float4* out, const DeskewP P) {
  __shared__ double s_knots[kDeskewFastKnots * 8];
  int n = cap;
  if (n_dev) n = min(n, *n_dev);
  if ((long long)blockIdx.x * kD >= (long long)n) return;                 // (the whole workgroup: nobody is left behind at the barrier)
  if ((int)threadIdx.x < P.nk * 8) s_knots[threadIdx.x] = P.knots[(size_t)P.k0 * 8 + threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * kD + threadIdx.x;
  if (i >= n) return;
  const float4 pt = in[i];
  if (!(isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z) && isfinite(pt.w))) { out[i] = pt; return; }
  // the point's time: float arithmetic as the reference's, the ring taken by rounding (association.cpp:67-68)
  const float ring = floorf(pt.w + 0.5f);
  const float delta = pt.w - ring;
  const double t = P.t0 + (double)delta;
  double q[4], tr[3];
  if (P.nk > 0 && t >= P.t_lo && t <= P.t_hi) {
    int cnt = 0;
    for (int k = 0; k < P.nk; ++k) cnt += s_knots[k * 8] <= t ? 1 : 0;
    const int b = min(max(cnt - 1, 0), P.nk - 2);
    pose_between(s_knots + b * 8, s_knots + b * 8 + 8, t, q, tr);
  } else {
    const int b = bracket_search(P.knots, P.n, t);
    pose_between(P.knots + (size_t)b * 8, P.knots + (size_t)b * 8 + 8, t, q, tr);
  }
  // p1 = T(t) (E p)   Lidar::Sensor2World;   p2 = E^-1 (T_f^-1 p1)   Lidar::World2Sensor
  const double v[3] = {(double)pt.x, (double)pt.y, (double)pt.z};
  double pb[3], p1[3], p2[3];
  rt_apply(P.E, v, pb);
  {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double cx = y * pb[2] - z * pb[1], cy = z * pb[0] - x * pb[2], cz = x * pb[1] - y * pb[0];
    const double dx = y * cz - z * cy, dy = z * cx - x * cz, dz = x * cy - y * cx;
    p1[0] = (pb[0] + 2.0 * (w * cx + dx)) + tr[0]; p1[1] = (pb[1] + 2.0 * (w * cy + dy)) + tr[1]; p1[2] = (pb[2] + 2.0 * (w * cz + dz)) + tr[2];
  }
  rt_apply(P.A, p1, p2);
  out[i] = make_float4((float)p2[0], (float)p2[1], (float)p2[2], pt.w);
}

namespace {

// the matrix form of a pose whose quaternion hse3 has ALREADY normalised: normalising again (make_rigid) would move the last bit
Rigid rigid_of_unit(const double T[7]) {
  Rigid M;
  unit_quat_matrix(T[0], T[1], T[2], T[3], M.R);
  for (int k = 0; k < 3; ++k) M.t[k] = T[4 + k];
  return M;
}
// the knot's row goes up; the device array grows by re-uploading the host copy (contents are not preserved across a growth)
int upload_knots(lvf_trajectory* tr, int first, int count) {
  lvf_ctx* ctx = tr->ctx;
  if ((size_t)tr->n * 8 > tr->dev.cap || !tr->dev.p) {
    LVF_TRY(tr->dev.ensure((size_t)tr->n * 8));
    first = 0; count = tr->n;
  }
  tr->dev.n = (size_t)tr->n * 8;
  return copy_up_wait(ctx, tr->dev.p + (size_t)first * 8, tr->knots.data() + (size_t)first * 8, (size_t)count * 8 * sizeof(double));
}

}  // namespace

int deskew_prepare(const char* who, lvf_ctx* ctx, const lvf_trajectory* tr, double frame_time, const double* frame_pose7, double cycle_time, const double* extrinsic7,
                   DeskewP* P, bool* active) {
  LVF_REQUIRE(tr && frame_pose7 && extrinsic7, "%s: null trajectory, frame pose or extrinsic", who);
  LVF_REQUIRE(tr->ctx == ctx, "%s: the trajectory belongs to another context", who);
  LVF_REQUIRE(std::isfinite(frame_time), "%s: non-finite frame time", who);
  // (the offset cycle_time * rel_time, rel_time in about [-0.25, 1.25], must stay inside (-0.5, 0.5) for the ring to be recoverable by rounding)
  LVF_REQUIRE(cycle_time > 0.0 && cycle_time < 0.4, "%s: cycle_time %g outside (0, 0.4)", who, cycle_time);
  double E[7], Tf[7];
  LVF_TRY(check_pose(who, "the frame pose", frame_pose7, Tf));
  LVF_TRY(check_pose(who, "the extrinsic", extrinsic7, E));
  *active = tr->n >= 2;            // one pose: ComputePose is constant, the caller copies
  if (!*active) return LVF_OK;
  double Ei[7], Tfi[7], A[7];
  hse3::inv(E, Ei); hse3::inv(Tf, Tfi); hse3::mul(Ei, Tfi, A);
  P->E = rigid_of_unit(E); P->A = rigid_of_unit(A);
  P->knots = tr->dev.p; P->n = tr->n;
  P->t0 = frame_time - 0.5 * cycle_time;
  P->t_lo = frame_time - 0.75 * cycle_time; P->t_hi = frame_time + 0.75 * cycle_time;
  const int b_lo = bracket_search(tr->knots.data(), tr->n, P->t_lo), b_hi = bracket_search(tr->knots.data(), tr->n, P->t_hi);
  const int nk = b_hi - b_lo + 2;
  P->k0 = b_lo; P->nk = nk <= kDeskewFastKnots ? nk : 0;
  return LVF_OK;
}

int deskew_launch(hipStream_t q, int cap, const int* n_dev, const float4* in, float4* out, const DeskewP& P) {
  if (cap <= 0) return LVF_OK;
  hipLaunchKernelGGL(k_deskew, dim3((cap + kD - 1) / kD), dim3(kD), 0, q, cap, n_dev, in, out, P);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_trajectory_create(lvf_ctx* ctx, const double* stamps, const double* poses7, int n, lvf_trajectory** out) {
  LVF_REQUIRE(ctx && out && stamps && poses7, "lvf_trajectory_create: null argument");
  LVF_REQUIRE(n >= 1, "lvf_trajectory_create: a trajectory has at least one pose (n = %d)", n);
  std::unique_ptr<lvf_trajectory> tr(new lvf_trajectory());
  tr->ctx = ctx; tr->n = n;
  tr->knots.resize((size_t)n * 8);
  for (int k = 0; k < n; ++k) {
    LVF_REQUIRE(std::isfinite(stamps[k]), "lvf_trajectory_create: stamp %d is not finite", k);
    LVF_REQUIRE(k == 0 || stamps[k] > stamps[k - 1], "lvf_trajectory_create: stamps must increase strictly (stamp %d = %.9f after %.9f)", k, stamps[k], stamps[k - 1]);
    tr->knots[(size_t)k * 8] = stamps[k];
    LVF_TRY(check_pose("lvf_trajectory_create", "a pose", poses7 + (size_t)k * 7, tr->knots.data() + (size_t)k * 8 + 1));
  }
  LVF_TRY(lvf::enter(ctx));
  LVF_TRY(upload_knots(tr.get(), 0, n));
  *out = tr.release();
  return LVF_OK;
}

int lvf_trajectory_append(lvf_trajectory* tr, double stamp, const double* pose7) {
  LVF_REQUIRE(tr && pose7, "lvf_trajectory_append: null argument");
  LVF_REQUIRE(std::isfinite(stamp) && stamp > tr->knots[(size_t)(tr->n - 1) * 8], "lvf_trajectory_append: stamp %.9f does not lie after the last one (%.9f)", stamp,
              tr->knots[(size_t)(tr->n - 1) * 8]);
  double row[8];
  row[0] = stamp;
  LVF_TRY(check_pose("lvf_trajectory_append", "the pose", pose7, row + 1));
  LVF_TRY(lvf::enter(tr->ctx));
  tr->knots.insert(tr->knots.end(), row, row + 8);
  tr->n += 1;
  const int rc = upload_knots(tr, tr->n - 1, 1);
  if (rc != LVF_OK) { tr->knots.resize(tr->knots.size() - 8); tr->n -= 1; }
  return rc;
}

int lvf_trajectory_set_pose(lvf_trajectory* tr, int i, const double* pose7) {
  LVF_REQUIRE(tr && pose7, "lvf_trajectory_set_pose: null argument");
  LVF_REQUIRE(i >= 0 && i < tr->n, "lvf_trajectory_set_pose: index %d outside [0, %d)", i, tr->n);
  double row[7];
  LVF_TRY(check_pose("lvf_trajectory_set_pose", "the pose", pose7, row));
  LVF_TRY(lvf::enter(tr->ctx));
  std::memcpy(tr->knots.data() + (size_t)i * 8 + 1, row, sizeof(row));
  return upload_knots(tr, i, 1);
}

int lvf_trajectory_size(const lvf_trajectory* tr) { return tr ? tr->n : -1; }
int lvf_trajectory_destroy(lvf_trajectory* tr) { delete tr; return LVF_OK; }

int lvf_trajectory_compute_pose(const lvf_trajectory* tr, const double* times, int m, double* poses7_out) {
  LVF_REQUIRE(tr && m >= 0 && (m == 0 || (times && poses7_out)), "lvf_trajectory_compute_pose: null argument or m < 0");
  if (m == 0) return LVF_OK;
  lvf_ctx* ctx = tr->ctx;
  LVF_TRY(lvf::enter(ctx));
  DevBuf<double> d_t, d_o;
  StreamWaitGuard wait(ctx->stream);      // (the caller's array feeds the copy)
  LVF_TRY(d_t.upload(times, m, ctx->stream)); LVF_TRY(d_o.alloc((size_t)m * 7));
  hipLaunchKernelGGL(k_traj_pose, dim3((m + kD - 1) / kD), dim3(kD), 0, ctx->stream, m, d_t.p, tr->dev.p, tr->n, d_o.p);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(poses7_out, d_o.p, (size_t)m * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LVF_HIP(hipStreamSynchronize(ctx->stream));
  wait.dismiss();
  return LVF_OK;
}

int lvf_cloud_deskew(const lvf_cloud* in, const lvf_trajectory* traj, double frame_time, const double* frame_pose7, double cycle_time, const double* extrinsic7,
                     lvf_cloud** out) {
  LVF_REQUIRE(in && out, "lvf_cloud_deskew: null argument");
  DeskewP P;
  bool active = false;
  LVF_TRY(deskew_prepare("lvf_cloud_deskew", in->ctx, traj, frame_time, frame_pose7, cycle_time, extrinsic7, &P, &active));
  LVF_TRY(lvf::enter(in->ctx));
  std::unique_ptr<lvf_cloud> c(new lvf_cloud());
  c->ctx = in->ctx; c->n = in->n;
  LVF_TRY(c->pts.alloc((size_t)in->n));
  if (in->n && !active) LVF_HIP(hipMemcpyAsync(c->pts.p, in->pts.p, (size_t)in->n * sizeof(float4), hipMemcpyDeviceToDevice, in->ctx->stream));
  if (in->n && active) LVF_TRY(deskew_launch(in->ctx->stream, in->n, nullptr, in->pts.p, c->pts.p, P));
  *out = c.release();
  return LVF_OK;
}

}  // extern "C"
