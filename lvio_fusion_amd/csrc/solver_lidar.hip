// solver_lidar.hip — LiDAR point-to-plane factors on full keyframe poses, as blocks of the sliding-window problem.
//
// The factor is LidarPlaneError<1,7> (src/lvio_fusion/include/lvio_fusion/ceres/lidar_error.hpp:10-40), which the reference declares and never
// adds to a problem:  r = n . (R(q/|q|) p + t - pa),  n the unit normal of (pa - pb) x (pa - pc), p in the keyframe's body frame, pa, pb, pc in
// the world frame.  Declared semantics: tests/lidar_window_ref.py.  The one deviation from the functor is a per-block weight w (r is scaled by
// it) and a per-block Huber a (<= 0: no loss), so that a ground sweep (w = 1, no loss) and a surf sweep (w = 0.01, a = 0.1) share a batch.
//
// A block is unary and rank one: it touches its keyframe's diagonal 6 x 6 block of B and 6 entries of gc, the places k_lin_po writes, and
// the chain launches k_lidar_lin / k_lidar_cost where it launches the pose-prior passes (solver_chain.hip).  About 90 B are read per block:
// the passes are latency- and atomic-bound, so the sums follow lin_po_body's scheme and nothing here uses the matrix cores.
#include <cmath>

#include "factor_eval.hpp"
#include "lidar_eval.hpp"
#include "solver_dev.hpp"

namespace lvf {

// ------------------------------------------------------------------------------------------------ building a batch
// One out-of-line copy, its nine inputs and three outputs in registers: the host-fed and the device-built batch then run the same
// instructions on the same three points and hold the same bits (tests/test_gpu_lidar_window.py compares them bit for bit).  That equality
// rests on the compiler honouring __noinline__, not on the language: were the routine inlined, each kernel could contract its multiplies and
// adds differently and the two batches would agree to rounding only.
__device__ __noinline__ double3 lidar_pose_normal(double3 a, double3 b, double3 c) {
  const double pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z}, pc[3] = {c.x, c.y, c.z};
  double n[3];
  plane_normal(pa, pb, pc, n);
  return make_double3(n[0], n[1], n[2]);
}

__global__ __launch_bounds__(kT) void k_lidar_pose_normals(int n, const double* __restrict__ pa, const double* __restrict__ pb, const double* __restrict__ pc,
                                                           double* __restrict__ nrm) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const double3 nn = lidar_pose_normal(make_double3(pa[i], pa[n + i], pa[2 * n + i]), make_double3(pb[i], pb[n + i], pb[2 * n + i]),
                                       make_double3(pc[i], pc[n + i], pc[2 * n + i]));
  nrm[i] = nn.x; nrm[n + i] = nn.y; nrm[2 * n + i] = nn.z;
}

// The correspondences lvf_knn3 left in up to kGatherScans scans -> blocks [off, off + Q) of a batch of N blocks (blockIdx.y = scan).  The
// floats are widened as association.cpp:303-314 does.  A query that failed the gate keeps its point and becomes a block of weight 0 with a
// zero anchor and normal: nothing is compacted, so nothing is counted before the launch and the host waits for nothing.
constexpr int kGatherScans = 16;
struct GatherJob { const float4* pts; const int* idx; const uint8_t* valid; const float4* map_raw; int Q, M, off, kf; double w, a; };
struct GatherJobs { GatherJob j[kGatherScans]; };
struct LidarPoseOut { double *p, *pa, *nrm; int* kf; double *w, *a; int* n_valid; int N; };

__global__ __launch_bounds__(kT) void k_lidar_pose_gather(GatherJobs jobs, LidarPoseOut o) {
  GatherJob J = jobs.j[0];
  // (static indices only: a run-time index into the by-value table would put it in scratch memory)
#pragma unroll
  for (int k = 1; k < kGatherScans; ++k) if ((int)blockIdx.y == k) J = jobs.j[k];
  const int q = blockIdx.x * kT + threadIdx.x;
  bool ok = false;
  if (q < J.Q) {
    const float4 s = J.pts[q];
    const int i0 = J.idx[3 * q], i1 = J.idx[3 * q + 1], i2 = J.idx[3 * q + 2];
    ok = J.valid[q] != 0 && i0 >= 0 && i0 < J.M && i1 >= 0 && i1 < J.M && i2 >= 0 && i2 < J.M;
    double pa[3] = {0.0, 0.0, 0.0}, nn[3] = {0.0, 0.0, 0.0};
    if (ok) {
      const float4 a = J.map_raw[i0], b = J.map_raw[i1], c = J.map_raw[i2];
      pa[0] = (double)a.x; pa[1] = (double)a.y; pa[2] = (double)a.z;
      const double3 n3 = lidar_pose_normal(make_double3(pa[0], pa[1], pa[2]), make_double3((double)b.x, (double)b.y, (double)b.z),
                                           make_double3((double)c.x, (double)c.y, (double)c.z));
      nn[0] = n3.x; nn[1] = n3.y; nn[2] = n3.z;
    }
    const size_t i = (size_t)J.off + q, N = (size_t)o.N;
    o.p[i] = (double)s.x; o.p[N + i] = (double)s.y; o.p[2 * N + i] = (double)s.z;
    o.pa[i] = pa[0]; o.pa[N + i] = pa[1]; o.pa[2 * N + i] = pa[2];
    o.nrm[i] = nn[0]; o.nrm[N + i] = nn[1]; o.nrm[2 * N + i] = nn[2];
    o.kf[i] = J.kf; o.w[i] = ok ? J.w : 0.0; o.a[i] = J.a;
    ok = ok && J.w > 0.0;
  }
  const int cnt = __popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(o.n_valid, cnt);
}

// blocks of one batch -> blocks [off, off + L.n) of another with N blocks, all on keyframe `kf` (the window's per-keyframe segments)
__global__ __launch_bounds__(kT) void k_lidar_pose_concat(LidarPoseArgs L, LidarPoseOut o, int off, int kf) {
  const int q = blockIdx.x * kT + threadIdx.x;
  if (q >= L.n) return;
  const size_t i = (size_t)off + q, N = (size_t)o.N, n = (size_t)L.n;
#pragma unroll
  for (int c = 0; c < 3; ++c) { o.p[c * N + i] = L.p[c * n + q]; o.pa[c * N + i] = L.pa[c * n + q]; o.nrm[c * N + i] = L.nrm[c * n + q]; }
  o.kf[i] = kf; o.w[i] = L.w[q]; o.a[i] = L.a[q];
}

// ------------------------------------------------------------------------------------------------ the factor
struct LidarBlock { double p[3], pa[3], nn[3], w, a; int k; };
__device__ __forceinline__ LidarBlock lidar_load(const LidarPoseArgs& L, int i) {
  LidarBlock b;
  const size_t n = (size_t)L.n;
  b.k = L.kf[i]; b.w = L.w[i]; b.a = L.a[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) { b.p[c] = L.p[c * n + i]; b.pa[c] = L.pa[c * n + i]; b.nn[c] = L.nrm[c * n + i]; }
  return b;
}
// w n . (R p + t - pa); rp = R p
__device__ __forceinline__ double lidar_residual(const LidarBlock& b, const PoseD& P, double rp[3]) {
  mat3_mul_vec(P.R, b.p, rp);
  return b.w * (b.nn[0] * (rp[0] + P.t[0] - b.pa[0]) + b.nn[1] * (rp[1] + P.t[1] - b.pa[1]) + b.nn[2] * (rp[2] + P.t[2] - b.pa[2]));
}

// lvf_batch_evaluate: the raw residual [n] and the 1 x 7 ambient Jacobian [n][7] (Ceres' layout, the projector of the quaternion's
// normalisation included: row_times_drot_dq)
template <bool WITH_J>
__global__ __launch_bounds__(kT) void k_lidar_pose_eval(LidarPoseArgs L, const double* __restrict__ poses, double* __restrict__ res, double* __restrict__ jac) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= L.n) return;
  const LidarBlock b = lidar_load(L, i);
  PoseD P;
  derive_pose(poses + 7 * b.k, P);
  double rp[3];
  res[i] = lidar_residual(b, P, rp);
  if (WITH_J) {
    const double fmp[3] = {rp[0] - b.p[0], rp[1] - b.p[1], rp[2] - b.p[2]};
    double g[4];
    row_times_drot_dq<false>(b.nn, P.u, P.inv_n, b.p, fmp, g);
    double* J = jac + (size_t)7 * i;
    J[0] = b.w * g[0]; J[1] = b.w * g[1]; J[2] = b.w * g[2]; J[3] = b.w * g[3];
    J[4] = b.w * b.nn[0]; J[5] = b.w * b.nn[1]; J[6] = b.w * b.nn[2];
  }
}

// One thread per block.  The block is rank one: the thread holds l = sqrt(rho') J_local (1 x 6, zero for a constant pose) and sqrt(rho') r,
// and the 21 + 6 sums of l^T l and l^T r go where lin_po_body's go — wave_sum when the wave shares one keyframe, a per-workgroup LDS table
// [n_kf][27] whose non-zero entries are flushed with atomics when n_kf <= kMaxStagedKf, global atomics otherwise.
template <bool COST_ONLY>
__device__ __forceinline__ void lidar_body(const LidarPoseArgs& L, int n_kf, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const,
                                           double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost) {
  __shared__ PoseD s_pose[kMaxStagedKf];
  stage_poses<kT>(s_pose, poses, n_kf);
  const int i = blockIdx.x * kT + threadIdx.x;
  double c = 0.0;
  int k = -1;
  double l[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  if (i < L.n) {
    const LidarBlock b = lidar_load(L, i);
    k = b.k;
    const PoseD P = fetch_pose(s_pose, poses, n_kf, k);
    double rp[3];
    const double res = lidar_residual(b, P, rp);
    double rho;
    const double sc = robust_scale(b.a, res * res, rho);
    c = 0.5 * rho;
    if (!COST_ONLY) {
      // d(n . R p) / d delta = 2 (R p) x n for the left perturbation of EigenQuaternionParameterization (factor_eval.hpp), d / dt = n
      const double sl = (pose_const[k] & 1) ? 0.0 : sc * b.w;
      cross2(rp, b.nn, l[0], l[1], l[2]);
      l[0] *= sl; l[1] *= sl; l[2] *= sl; l[3] = sl * b.nn[0]; l[4] = sl * b.nn[1]; l[5] = sl * b.nn[2];
      r = sc * res;
    }
  }
  if (!COST_ONLY) {
    __shared__ double s_acc[kMaxStagedKf * 27];
    const bool lds_path = n_kf <= kMaxStagedKf;
    if (lds_path) {
      for (int e = threadIdx.x; e < n_kf * 27; e += kT) s_acc[e] = 0.0;
      __syncthreads();
    }
    double v[27];
    {
      int q = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) v[q++] = l[a] * l[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[21 + a] = l[a] * r;
    }
    const int k0 = __shfl(k, 0);
    const bool uniform = __all(k == k0) && k0 >= 0;
    if (uniform) {
#pragma unroll
      for (int q = 0; q < 27; ++q) v[q] = wave_sum(v[q]);
      if ((threadIdx.x & 63) == 0) {
        if (lds_path) { for (int q = 0; q < 27; ++q) atomicAdd(&s_acc[k0 * 27 + q], v[q]); }
        else {
          int q = 0;
          for (int a = 0; a < 6; ++a) for (int b = 0; b <= a; ++b, ++q) if (v[q] != 0.0) atomicAdd(&B[(size_t)(6 * k0 + a) * ld + 6 * k0 + b], v[q]);
          for (int a = 0; a < 6; ++a) if (v[21 + a] != 0.0) atomicAdd(&gc[6 * k0 + a], v[21 + a]);
        }
      }
    } else if (k >= 0) {
      if (lds_path) { for (int q = 0; q < 27; ++q) if (v[q] != 0.0) atomicAdd(&s_acc[k * 27 + q], v[q]); }
      else {
        int q = 0;
        for (int a = 0; a < 6; ++a) for (int b = 0; b <= a; ++b, ++q) if (v[q] != 0.0) atomicAdd(&B[(size_t)(6 * k + a) * ld + 6 * k + b], v[q]);
        for (int a = 0; a < 6; ++a) if (v[21 + a] != 0.0) atomicAdd(&gc[6 * k + a], v[21 + a]);
      }
    }
    if (lds_path) {
      __syncthreads();
      for (int e = threadIdx.x; e < n_kf * 27; e += kT) {
        const double val = s_acc[e];
        if (val == 0.0) continue;
        const int kk = e / 27, slot = e - kk * 27;
        if (slot < 21) {
          int x = 0, rem = slot;
          while (rem > x) { rem -= x + 1; ++x; }
          atomicAdd(&B[(size_t)(6 * kk + x) * ld + 6 * kk + rem], val);
        } else atomicAdd(&gc[6 * kk + slot - 21], val);
      }
    }
  }
  block_add(c, cost);
}
__global__ __launch_bounds__(kT) void k_lidar_lin(LidarPoseArgs L, int n_kf, const double* __restrict__ poses, const uint8_t* __restrict__ pose_const,
                                                  double* __restrict__ B, int ld, double* __restrict__ gc, double* __restrict__ cost) {
  lidar_body<false>(L, n_kf, poses, pose_const, B, ld, gc, cost);
}
// the same loads, 1/2 rho only, into the given (striped) cost slot
__global__ __launch_bounds__(kT) void k_lidar_cost(LidarPoseArgs L, int n_kf, const double* __restrict__ poses, double* __restrict__ cost) {
  lidar_body<true>(L, n_kf, poses, nullptr, nullptr, 0, nullptr, cost);
}

int launch_lidar_pose(lvf_batch* b, const lvf_state* st, bool want_j) {
  if (b->n == 0) return LVF_OK;
  LVF_TRY(b->res.ensure((size_t)b->n));
  if (want_j) LVF_TRY(b->jac[0].ensure((size_t)7 * b->n));
  const LidarPoseArgs L = lidar_pose_args(b);
  const dim3 g((b->n + kT - 1) / kT), blk(kT);
  if (want_j) hipLaunchKernelGGL(k_lidar_pose_eval<true>, g, blk, 0, b->ctx->stream, L, st->poses.p, b->res.p, b->jac[0].p);
  else hipLaunchKernelGGL(k_lidar_pose_eval<false>, g, blk, 0, b->ctx->stream, L, st->poses.p, b->res.p, (double*)nullptr);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

static lvf_batch* new_lidar_pose_batch(lvf_ctx* ctx) {
  auto* b = new lvf_batch();
  b->ctx = ctx; b->kind = LVF_K_LIDAR_POSE; b->n_res = 1; b->n_blocks = 1; b->block_size[0] = 7;
  return b;
}
// the buffers of a batch of n blocks (grow-only: the window re-fills its batch every time its segments change)
static int lidar_pose_reserve(lvf_batch* b, int n) {
  const size_t m = (size_t)n;
  LVF_TRY(b->lp.ensure(3 * m)); LVF_TRY(b->lpa.ensure(3 * m)); LVF_TRY(b->lnrm.ensure(3 * m)); LVF_TRY(b->idx_a.ensure(m));
  LVF_TRY(b->ob_a.ensure(m)); LVF_TRY(b->ob_b.ensure(m)); LVF_TRY(b->n_valid_dev.ensure(1));      // (res / jac: by the first lvf_batch_evaluate)
  b->n = n; b->evaluated = false; b->have_jac = false;
  return LVF_OK;
}
static LidarPoseOut lidar_pose_out(lvf_batch* b) { return LidarPoseOut{b->lp.p, b->lpa.p, b->lnrm.p, b->idx_a.p, b->ob_a.p, b->ob_b.p, b->n_valid_dev.p, b->n}; }

static int gather_scans(lvf_batch* b, int n_scans, lvf_map* const* maps, lvf_scan* const* scans, const int32_t* kf_idx, const double* weight, const double* huber_a) {
  hipStream_t s = b->ctx->stream;
  LVF_HIP(hipMemsetAsync(b->n_valid_dev.p, 0, sizeof(int), s));
  const LidarPoseOut o = lidar_pose_out(b);
  int off = 0;
  for (int first = 0; first < n_scans; first += kGatherScans) {
    GatherJobs jobs{};
    const int cnt = std::min(kGatherScans, n_scans - first);
    int max_q = 0;
    for (int k = 0; k < cnt; ++k) {
      const lvf_scan* sc = scans[first + k];
      jobs.j[k] = GatherJob{sc->pts.p, sc->idx.p, sc->valid.p, maps[first + k]->raw.p, sc->Q, maps[first + k]->M, off, kf_idx[first + k],
                            weight ? weight[first + k] : 1.0, huber_a ? huber_a[first + k] : 0.0};
      off += sc->Q; max_q = std::max(max_q, sc->Q);
    }
    if (max_q > 0) hipLaunchKernelGGL(k_lidar_pose_gather, dim3((max_q + kT - 1) / kT, cnt), dim3(kT), 0, s, jobs, o);
  }
  LVF_HIP(hipGetLastError());
  b->n_valid = -1;
  return LVF_OK;
}

static int check_scans(const char* who, lvf_ctx* ctx, int n_scans, lvf_map* const* maps, lvf_scan* const* scans, const int32_t* kf_idx, const double* weight,
                       const double* huber_a, long long* total) {
  *total = 0;
  for (int k = 0; k < n_scans; ++k) {
    LVF_REQUIRE(maps[k] && scans[k], "%s: scan or map %d is null", who, k);
    LVF_REQUIRE(maps[k]->ctx == ctx && scans[k]->ctx == ctx, "%s: scan or map %d belongs to another context", who, k);
    LVF_REQUIRE(scans[k]->searched || scans[k]->Q == 0, "%s: scan %d was not searched (lvf_knn3 first)", who, k);      // (an empty scan has nothing to search)
    LVF_REQUIRE(kf_idx[k] >= 0, "%s: kf_idx[%d] = %d is negative", who, k, kf_idx[k]);
    LVF_REQUIRE(k == 0 || kf_idx[k] >= kf_idx[k - 1], "%s: scans must come in keyframe order (kf_idx[%d] = %d after %d)", who, k, kf_idx[k], kf_idx[k - 1]);
    LVF_REQUIRE(!weight || (std::isfinite(weight[k]) && weight[k] >= 0.0), "%s: weight[%d] is negative or not finite", who, k);
    LVF_REQUIRE(!huber_a || std::isfinite(huber_a[k]), "%s: huber_a[%d] is not finite", who, k);
    *total += scans[k]->Q;
  }
  LVF_REQUIRE(*total < (1ll << 30), "%s: too many blocks", who);
  return LVF_OK;
}

// The window's batch: the per-keyframe segments `seg[k]` (null: none) of the keyframes at positions 0 .. n_kf - 1, concatenated in that
// order into `dst` (created on first use).  Sorted by construction.
int lidar_pose_assemble(lvf_ctx* ctx, int n_kf, lvf_batch* const* seg, lvf_batch** dst) {
  if (!*dst) *dst = new_lidar_pose_batch(ctx);
  lvf_batch* b = *dst;
  long long total = 0;
  int last = -1;
  for (int k = 0; k < n_kf; ++k) if (seg[k] && seg[k]->n) { total += seg[k]->n; last = k; }
  LVF_REQUIRE(total < (1ll << 30), "lidar planes: too many blocks");
  LVF_TRY(lidar_pose_reserve(b, (int)total));
  b->min_n_kf = last + 1; b->sorted_by_kf = true;      // (the window keeps this batch to itself: nobody asks it for its valid count)
  const LidarPoseOut o = lidar_pose_out(b);
  int off = 0;
  for (int k = 0; k < n_kf; ++k) {
    if (!(seg[k] && seg[k]->n)) continue;
    hipLaunchKernelGGL(k_lidar_pose_concat, dim3((seg[k]->n + kT - 1) / kT), dim3(kT), 0, ctx->stream, lidar_pose_args(seg[k]), o, off, k);
    off += seg[k]->n;
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

int lvf_lidar_pose_create(lvf_ctx* ctx, int n, const double* p, const double* pa, const double* pb, const double* pc, const int32_t* kf_idx,
                          const double* weight, const double* huber_a, lvf_batch** out) {
  LVF_REQUIRE(ctx && out, "lvf_lidar_pose_create: null argument");
  LVF_REQUIRE(n >= 0, "lvf_lidar_pose_create: negative size");
  LVF_REQUIRE(n == 0 || (p && pa && pb && pc && kf_idx), "lvf_lidar_pose_create: null input array");
  int mx = -1, n_valid = 0;
  bool sorted = true;
  for (int i = 0; i < n; ++i) {
    LVF_REQUIRE(kf_idx[i] >= 0, "lvf_lidar_pose_create: kf_idx[%d] = %d is negative", i, kf_idx[i]);
    for (int c = 0; c < 3; ++c)
      LVF_REQUIRE(std::isfinite(p[3 * i + c]) && std::isfinite(pa[3 * i + c]) && std::isfinite(pb[3 * i + c]) && std::isfinite(pc[3 * i + c]),
                  "lvf_lidar_pose_create: block %d has a point that is not finite", i);
    LVF_REQUIRE(!weight || (std::isfinite(weight[i]) && weight[i] >= 0.0), "lvf_lidar_pose_create: weight[%d] is negative or not finite", i);
    LVF_REQUIRE(!huber_a || std::isfinite(huber_a[i]), "lvf_lidar_pose_create: huber_a[%d] is not finite", i);
    if (i > 0 && kf_idx[i] < kf_idx[i - 1]) sorted = false;
    mx = std::max(mx, kf_idx[i]);
    if (!weight || weight[i] > 0.0) ++n_valid;
  }
  LVF_TRY(lvf::enter(ctx));
  lvf_batch* b = new_lidar_pose_batch(ctx);
  hipStream_t s = ctx->stream;
  std::vector<double> soa[4], w((size_t)n, 1.0), a((size_t)n, 0.0);
  const double* src[4] = {p, pa, pb, pc};
  for (int j = 0; j < 4; ++j) {
    soa[j].resize((size_t)3 * n);
    for (int i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) soa[j][(size_t)c * n + i] = src[j][3 * i + c];
  }
  if (weight) std::copy(weight, weight + n, w.begin());
  if (huber_a) std::copy(huber_a, huber_a + n, a.begin());
  DevBuf<double> dpb, dpc;
  const size_t m = (size_t)n;
  int rc;
  if ((rc = lidar_pose_reserve(b, n)) || (rc = b->lp.assign(soa[0].data(), 3 * m, s)) || (rc = b->lpa.assign(soa[1].data(), 3 * m, s)) ||
      (rc = dpb.upload(soa[2].data(), 3 * m, s)) || (rc = dpc.upload(soa[3].data(), 3 * m, s)) || (rc = b->idx_a.assign(kf_idx, m, s)) ||
      (rc = b->ob_a.assign(w.data(), m, s)) || (rc = b->ob_b.assign(a.data(), m, s))) { (void)hipStreamSynchronize(s); delete b; return rc; }
  if (n) hipLaunchKernelGGL(k_lidar_pose_normals, dim3((n + kT - 1) / kT), dim3(kT), 0, s, n, b->lpa.p, dpb.p, dpc.p, b->lnrm.p);
  hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(s);         // (the host arrays above are read until here)
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { delete b; return lvf::hip_fail(e, "lvf_lidar_pose_create", __FILE__, __LINE__); }
  b->min_n_kf = mx + 1; b->sorted_by_kf = sorted; b->n_valid = n_valid;
  *out = b;
  return LVF_OK;
}

int lvf_lidar_pose_from_scans(lvf_ctx* ctx, int n_scans, lvf_map* const* maps, lvf_scan* const* scans, const int32_t* kf_idx, const double* weight,
                              const double* huber_a, lvf_batch** out) {
  LVF_REQUIRE(ctx && out, "lvf_lidar_pose_from_scans: null argument");
  LVF_REQUIRE(n_scans >= 0, "lvf_lidar_pose_from_scans: negative size");
  LVF_REQUIRE(n_scans == 0 || (maps && scans && kf_idx), "lvf_lidar_pose_from_scans: null input array");
  long long total = 0;
  LVF_TRY(check_scans("lvf_lidar_pose_from_scans", ctx, n_scans, maps, scans, kf_idx, weight, huber_a, &total));
  LVF_TRY(lvf::enter(ctx));
  lvf_batch* b = new_lidar_pose_batch(ctx);
  int rc;
  if ((rc = lidar_pose_reserve(b, (int)total)) || (rc = gather_scans(b, n_scans, maps, scans, kf_idx, weight, huber_a))) { delete b; return rc; }
  b->min_n_kf = n_scans ? kf_idx[n_scans - 1] + 1 : 0; b->sorted_by_kf = true;
  *out = b;
  return LVF_OK;
}

int lvf_lidar_pose_download(lvf_batch* b, double* p, double* pa, int32_t* kf_idx, double* weight, double* huber_a) {
  LVF_REQUIRE(b, "lvf_lidar_pose_download: null batch");
  LVF_REQUIRE(b->kind == LVF_K_LIDAR_POSE, "lvf_lidar_pose_download: not a lidar-pose batch");
  LVF_TRY(lvf::enter(b->ctx));
  hipStream_t s = b->ctx->stream;
  const size_t n = (size_t)b->n;
  std::vector<double> sp(p ? 3 * n : 0), spa(pa ? 3 * n : 0);
  if (n) {
    if (p) LVF_HIP(hipMemcpyAsync(sp.data(), b->lp.p, 24 * n, hipMemcpyDeviceToHost, s));
    if (pa) LVF_HIP(hipMemcpyAsync(spa.data(), b->lpa.p, 24 * n, hipMemcpyDeviceToHost, s));
    if (kf_idx) LVF_HIP(hipMemcpyAsync(kf_idx, b->idx_a.p, 4 * n, hipMemcpyDeviceToHost, s));
    if (weight) LVF_HIP(hipMemcpyAsync(weight, b->ob_a.p, 8 * n, hipMemcpyDeviceToHost, s));
    if (huber_a) LVF_HIP(hipMemcpyAsync(huber_a, b->ob_b.p, 8 * n, hipMemcpyDeviceToHost, s));
  }
  LVF_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) { if (p) p[3 * i + c] = sp[c * n + i]; if (pa) pa[3 * i + c] = spa[c * n + i]; }
  return LVF_OK;
}

int lvf_lidar_pose_num_valid(lvf_batch* b, int* n) {
  LVF_REQUIRE(b && n, "lvf_lidar_pose_num_valid: null argument");
  LVF_REQUIRE(b->kind == LVF_K_LIDAR_POSE, "lvf_lidar_pose_num_valid: not a lidar-pose batch");
  if (b->n_valid < 0) {
    LVF_TRY(lvf::enter(b->ctx));
    int v = 0;
    LVF_TRY(read_back(b->ctx, &v, b->n_valid_dev.p, sizeof(int)));
    b->n_valid = v;
  }
  *n = b->n_valid;
  return LVF_OK;
}

}  // extern "C"
