// reloc_kernels.hip — visual relocalisation on device: the body Relocator::RelocateByImage declares and never builds
// (src/lvio_fusion/src/relocator.cpp:164-173).  Semantics are DECLARED; tests/reloc_ref.py is the statement of record.
//
//   k_orb_match     cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) in both directions, one wavefront per descriptor row
//   k_orb_gate      the gate of local_map.cpp:342-346 + the cross-check; k_match_list compacts the accepted pairs behind device_scan1
//   k_pnp_score     one wavefront per hypothesis: counter-based triple, P3P (Grunert's quartic by Ferrari's factorisation), inlier counts
//   k_pnp_refine    one workgroup, one launch: winner, then rounds of {classify, LocalMap::LocalBA's pose-only problem under the declared LM
//                   loop: lm_small, small_lm.hpp}
#include "factor_eval.hpp"
#include "small_lm.hpp"

namespace lvf {

constexpr int kRT = 256;
constexpr int kRelocMaxFeatures = 8192;
constexpr int kPnpMaxHypotheses = 4096;
constexpr int kPnpMaxDraws = 64;
constexpr unsigned long long kNoPair = ~0ull;

// ---- matching -------------------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  return (unsigned long long)__double_as_longlong(quad_perm<CTRL>(__longlong_as_double((long long)v)));
}
// the two smallest keys of two DISJOINT sets, each given by its two smallest
__device__ __forceinline__ void merge2(unsigned long long& b, unsigned long long& s, unsigned long long ob, unsigned long long os) {
  const unsigned long long lo = min(b, ob), hi = max(b, ob);
  b = lo; s = min(hi, min(s, os));
}
// wave-wide two smallest keys: a butterfly inside each 16-lane row on the DPP path (every step joins disjoint lane sets), then the four rows
// read as scalars.  Lane 0 (every lane, in fact) holds the result.
__device__ __forceinline__ void wave_min2(unsigned long long& b, unsigned long long& s) {
  merge2(b, s, dpp_u64<0xB1>(b), dpp_u64<0xB1>(s));
  merge2(b, s, dpp_u64<0x4E>(b), dpp_u64<0x4E>(s));
  merge2(b, s, dpp_u64<0x141>(b), dpp_u64<0x141>(s));
  merge2(b, s, dpp_u64<0x140>(b), dpp_u64<0x140>(s));
  const double bd = __longlong_as_double((long long)b), sd = __longlong_as_double((long long)s);
  unsigned long long rb = (unsigned long long)__double_as_longlong(lane_bcast(bd, 0)), rs = (unsigned long long)__double_as_longlong(lane_bcast(sd, 0));
#pragma unroll
  for (int r = 16; r < 64; r += 16)
    merge2(rb, rs, (unsigned long long)__double_as_longlong(lane_bcast(bd, r)), (unsigned long long)__double_as_longlong(lane_bcast(sd, r)));
  b = rb; s = rs;
}

// wave w < nq: query w against every train row -> qkey[2 w], qkey[2 w + 1]; wave nq + j: train j against every query -> tkey[j].
// key = distance << 32 | index of the other side: the tie rule (lower index) is part of the integer order.
__global__ void __launch_bounds__(kRT) k_orb_match(int nq, const unsigned long long* __restrict__ qd, int nt, const unsigned long long* __restrict__ td,
                                                   unsigned long long* __restrict__ qkey, unsigned long long* __restrict__ tkey) {
  const int w = blockIdx.x * (kRT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= nq + nt) return;
  const bool fwd = w < nq;
  const int row = fwd ? w : w - nq, n_other = fwd ? nt : nq;
  const unsigned long long* mine = (fwd ? qd : td) + 4 * (size_t)row;
  const unsigned long long* other = fwd ? td : qd;
  const unsigned long long q0 = mine[0], q1 = mine[1], q2 = mine[2], q3 = mine[3];
  unsigned long long b = kNoPair, s = kNoPair;
  for (int j = lane; j < n_other; j += 64) {
    const unsigned long long* t = other + 4 * (size_t)j;
    const int dist = __popcll(t[0] ^ q0) + __popcll(t[1] ^ q1) + __popcll(t[2] ^ q2) + __popcll(t[3] ^ q3);
    const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)j;
    if (key < b) { s = b; b = key; } else if (key < s) s = key;
  }
  wave_min2(b, s);
  if (lane == 0) {
    if (fwd) { qkey[2 * (size_t)row] = b; qkey[2 * (size_t)row + 1] = s; } else tkey[row] = b;
  }
}

struct MatchOpt { int max_distance; float ratio; int cross_check; };

__global__ void __launch_bounds__(kRT) k_orb_gate(int nq, int nt, const unsigned long long* __restrict__ qkey, const unsigned long long* __restrict__ tkey, MatchOpt o,
                                                  int* __restrict__ match, int* __restrict__ best, int* __restrict__ second, int* __restrict__ flag) {
  const int q = blockIdx.x * kRT + threadIdx.x;
  if (q >= nq) return;
  const unsigned long long b = qkey[2 * (size_t)q], s = qkey[2 * (size_t)q + 1];
  const int bd = b == kNoPair ? -1 : (int)(b >> 32), sd = s == kNoPair ? -1 : (int)(s >> 32);
  int m = -1;
  if (nt >= 2 && bd >= 0 && sd >= 0 && bd < o.max_distance && (float)bd < o.ratio * (float)sd) {
    const int j = (int)(b & 0xffffffffull);
    if (!o.cross_check || (int)(tkey[j] & 0xffffffffull) == q) m = j;
  }
  match[q] = m; best[q] = bd; second[q] = sd; flag[q] = m >= 0;
}

// the accepted pairs (query index, train index) in ascending query index: pos = the exclusive scan of the flags
__global__ void __launch_bounds__(kRT) k_match_list(int nq, const int* __restrict__ match, const int* __restrict__ pos, int2* __restrict__ list) {
  const int q = blockIdx.x * kRT + threadIdx.x;
  if (q >= nq) return;
  const int m = match[q];
  if (m >= 0) list[pos[q]] = make_int2(q, m);
}

// ---- hypotheses -----------------------------------------------------------------------------------------------------------------------------
struct PnpArgs {
  const int* n_dev;            // number of matches (written by the scan, or uploaded)
  const int2* list;            // (index into pt, index into pw)
  const double* pw;            // [.][3] world
  const float2* pt;            // [.] pixels
  CamD cam;
  int H, min_matches, have_init, have_old, rounds, iters, n_out;
  unsigned seed;
  double gate2, huber_a;
  double init[7], old[7];      // have_old: the initial pose is old * init and the result is also reported relative to old
};
struct PnpRec {
  double pose[7], rel[7], initial_cost, final_cost;
  int score, n_matches, winner, winner_count, iters, successes, termination, why, blocks, found;
};

__device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// squared PoseOnly residual norm at weight 1 (the World2Sensor / Sensor2Pixel chain of eval_pose_only) and the sensor-frame depth
__device__ __forceinline__ double reproj_raw(const PoseD& P, const CamD& cam, double obx, double oby, const double* __restrict__ pw, double& pcz) {
  const double d[3] = {pw[0] - P.t[0], pw[1] - P.t[1], pw[2] - P.t[2]};
  double pb[3];
  mat3t_mul_vec(P.R, d, pb);
  const double pcx = cam.E[0] * pb[0] + cam.E[1] * pb[1] + cam.E[2] * pb[2] + cam.c0[0];
  const double pcy = cam.E[3] * pb[0] + cam.E[4] * pb[1] + cam.E[5] * pb[2] + cam.c0[1];
  pcz = cam.E[6] * pb[0] + cam.E[7] * pb[1] + cam.E[8] * pb[2] + cam.c0[2];
  const double iz = 1.0 / pcz;
  const double rx = cam.fx * (pcx * iz) + cam.cx - obx, ry = cam.fy * (pcy * iz) + cam.cy - oby;
  return rx * rx + ry * ry;
}
// the classification error: +inf where the depth is <= 0
__device__ __forceinline__ double reproj_e2(const PoseD& P, const CamD& cam, double obx, double oby, const double* __restrict__ pw) {
  double pcz;
  const double e2 = reproj_raw(P, cam, obx, oby, pw, pcz);
  return pcz > 0.0 ? e2 : INFINITY;
}

// inliers of one pose over all matches; every lane of the wave returns the count
__device__ __forceinline__ int wave_count_inliers(const PnpArgs& a, int n, const double* pose7) {
  const int lane = threadIdx.x & 63;
  PoseD P;
  derive_pose(pose7, P);
  int cnt = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < n) {
      const int2 m = a.list[i];
      const float2 p = a.pt[m.x];
      in = reproj_e2(P, a.cam, (double)p.x, (double)p.y, a.pw + 3 * (size_t)m.y) < a.gate2;
    }
    cnt += __popcll(__ballot(in));
  }
  return cnt;
}

// largest real root of z^3 + A z^2 + B z + C: closed form, two Newton steps
__device__ __forceinline__ double cubic_largest_root(double A, double B, double C) {
  const double P = B - A * A / 3.0, Q = 2.0 * A * A * A / 27.0 - A * B / 3.0 + C;
  const double disc = Q * Q / 4.0 + P * P * P / 27.0;
  double t = 0.0;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    t = cbrt(-Q / 2.0 + sd) + cbrt(-Q / 2.0 - sd);
  } else if (P < 0.0) {
    const double arg = fmin(1.0, fmax(-1.0, 3.0 * Q / (2.0 * P) * sqrt(-3.0 / P)));
    t = 2.0 * sqrt(-P / 3.0) * cos(acos(arg) / 3.0);
  }
  double z = t - A / 3.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double f = ((z + A) * z + B) * z + C, fp = (3.0 * z + 2.0 * A) * z + B;
    if (fp != 0.0) z -= f / fp;
  }
  return z;
}

__device__ __forceinline__ void unit3(const double a[3], double o[3]) {
  const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  o[0] = a[0] / n; o[1] = a[1] / n; o[2] = a[2] / n;
}
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// the orthonormal frame a triangle spans: e1 along p2 - p1, e3 its normal, e2 = e3 x e1
__device__ __forceinline__ void tri_frame(const double p1[3], const double p2[3], const double p3[3], double e1[3], double e2[3], double e3[3]) {
  const double a[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]}, b[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
  unit3(a, e1);
  double c[3];
  cross3(e1, b, c);
  unit3(c, e3);
  cross3(e3, e1, e2);
}
// Shepperd's method, (x, y, z, w); R row-major
__device__ __forceinline__ void quat_of_rot(const double R[9], double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; q[3] = s / 4.0;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
    q[0] = s / 4.0; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; q[3] = (R[7] - R[5]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
    q[0] = (R[1] + R[3]) / s; q[1] = s / 4.0; q[2] = (R[5] + R[7]) / s; q[3] = (R[2] - R[6]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
    q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = s / 4.0; q[3] = (R[3] - R[1]) / s;
  }
}

__device__ __forceinline__ bool finite7(const double* p) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; ++k) ok = ok && isfinite(p[k]);
  return ok;
}

// hkey[h] = 0: no pose; else (count + 1) << 32 | ~(h + 1), h = -1 (slot H) being the caller's initial pose: the maximum is the largest count,
// ties to the initial pose, then to the lowest h.  htri[h] = (the triple, the number of poses).
__global__ void __launch_bounds__(kRT) k_pnp_score(PnpArgs a, unsigned long long* __restrict__ hkey, double* __restrict__ hpose, int4* __restrict__ htri) {
  const int h = blockIdx.x * (kRT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (h >= a.H + a.have_init) return;
  const int n = *a.n_dev;
  if (n < a.min_matches || n < 3) return;
  if (h == a.H) {                                          // the initial pose
    double p[7];
    if (a.have_old) forward_update_pose(a.old, a.init, p);
    else {
#pragma unroll
      for (int k = 0; k < 7; ++k) p[k] = a.init[k];
    }
    const int cnt = wave_count_inliers(a, n, p);
    if (lane == 0) {
      hkey[h] = ((unsigned long long)(cnt + 1) << 32) | 0xffffffffull;
#pragma unroll
      for (int k = 0; k < 7; ++k) hpose[7 * (size_t)h + k] = p[k];
    }
    return;
  }
  // the triple: draws equal to an earlier one are skipped
  int t0 = -1, t1 = -1, t2 = -1;
  for (int c = 0; c < kPnpMaxDraws && t2 < 0; ++c) {
    const int d = (int)(mix32(a.seed ^ mix32((unsigned)h * 0x9E3779B1u + (unsigned)c)) % (unsigned)n);
    if (t0 < 0) t0 = d;
    else if (t1 < 0) { if (d != t0) t1 = d; }
    else if (d != t0 && d != t1) t2 = d;
  }
  int n_poses = 0, best_cnt = -1;
  double best_pose[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  if (t2 >= 0) {
    const int2 m0 = a.list[t0], m1 = a.list[t1], m2 = a.list[t2];
    const double* Pw0 = a.pw + 3 * (size_t)m0.y; const double* Pw1 = a.pw + 3 * (size_t)m1.y; const double* Pw2 = a.pw + 3 * (size_t)m2.y;
    const double P0[3] = {Pw0[0], Pw0[1], Pw0[2]}, P1[3] = {Pw1[0], Pw1[1], Pw1[2]}, P2[3] = {Pw2[0], Pw2[1], Pw2[2]};
    const float2 x0 = a.pt[m0.x], x1 = a.pt[m1.x], x2 = a.pt[m2.x];
    const double r0[3] = {((double)x0.x - a.cam.cx) / a.cam.fx, ((double)x0.y - a.cam.cy) / a.cam.fy, 1.0};
    const double r1[3] = {((double)x1.x - a.cam.cx) / a.cam.fx, ((double)x1.y - a.cam.cy) / a.cam.fy, 1.0};
    const double r2[3] = {((double)x2.x - a.cam.cx) / a.cam.fx, ((double)x2.y - a.cam.cy) / a.cam.fy, 1.0};
    double f0[3], f1[3], f2[3];
    unit3(r0, f0); unit3(r1, f1); unit3(r2, f2);
    const double a2 = (P1[0] - P2[0]) * (P1[0] - P2[0]) + (P1[1] - P2[1]) * (P1[1] - P2[1]) + (P1[2] - P2[2]) * (P1[2] - P2[2]);
    const double b2 = (P0[0] - P2[0]) * (P0[0] - P2[0]) + (P0[1] - P2[1]) * (P0[1] - P2[1]) + (P0[2] - P2[2]) * (P0[2] - P2[2]);
    const double c2 = (P0[0] - P1[0]) * (P0[0] - P1[0]) + (P0[1] - P1[1]) * (P0[1] - P1[1]) + (P0[2] - P1[2]) * (P0[2] - P1[2]);
    const double ca = f1[0] * f2[0] + f1[1] * f2[1] + f1[2] * f2[2], cb = f0[0] * f2[0] + f0[1] * f2[1] + f0[2] * f2[2],
                 cg = f0[0] * f1[0] + f0[1] * f1[1] + f0[2] * f1[2];
    if (b2 > 0.0) {
      const double k = (a2 - c2) / b2, m = c2 / b2;
      const double n0 = 1.0 + k, n1 = -2.0 * k * cb, n2 = k - 1.0, d0 = 2.0 * cg, d1 = -2.0 * ca, q0 = 1.0 - m, q1 = 2.0 * m * cb, q2 = -m;
      const double A0 = n0 * n0 + d0 * d0 * q0 - 2.0 * cg * (n0 * d0);
      const double A1 = 2.0 * n0 * n1 + d0 * d0 * q1 + 2.0 * d0 * d1 * q0 - 2.0 * cg * (n0 * d1 + n1 * d0);
      const double A2 = n1 * n1 + 2.0 * n0 * n2 + d0 * d0 * q2 + 2.0 * d0 * d1 * q1 + d1 * d1 * q0 - 2.0 * cg * (n1 * d1 + n2 * d0);
      const double A3 = 2.0 * n1 * n2 + 2.0 * d0 * d1 * q2 + d1 * d1 * q1 - 2.0 * cg * (n2 * d1);
      const double A4 = n2 * n2 + d1 * d1 * q2;
      if (A4 != 0.0 && isfinite(A0) && isfinite(A1) && isfinite(A2) && isfinite(A3) && isfinite(A4)) {
        const double qa = A3 / A4, qb = A2 / A4, qc = A1 / A4, qd = A0 / A4;
        const double p = qb - 3.0 * qa * qa / 8.0, q = qc - qa * qb / 2.0 + qa * qa * qa / 8.0,
                     r = qd - qa * qc / 4.0 + qa * qa * qb / 16.0 - 3.0 * qa * qa * qa * qa / 256.0;
        const double z = cubic_largest_root(2.0 * p, p * p - 4.0 * r, -q * q);
        if (z > 0.0 && isfinite(z)) {
          const double s = sqrt(z);
          double w1[3], w2[3], w3[3];
          tri_frame(P0, P1, P2, w1, w2, w3);
#pragma unroll
          for (int slot = 0; slot < 4; ++slot) {           // first quadratic factor (+, -), second (+, -)
            const double sg = slot < 2 ? 1.0 : -1.0;
            const double u2 = slot < 2 ? (p + z - q / s) / 2.0 : (p + z + q / s) / 2.0;
            const double disc = z - 4.0 * u2;
            if (!(disc >= 0.0)) continue;
            const double sd = sqrt(disc);
            double v = ((slot & 1) ? (-sg * s - sd) / 2.0 : (-sg * s + sd) / 2.0) - qa / 4.0;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
              const double f = (((v + qa) * v + qb) * v + qc) * v + qd, fp = ((4.0 * v + 3.0 * qa) * v + 2.0 * qb) * v + qc;
              if (fp != 0.0) v -= f / fp;
            }
            const double D = d1 * v + d0, den = 1.0 + v * v - 2.0 * v * cb;
            if (D == 0.0 || !(den > 0.0)) continue;
            const double u = ((n2 * v + n1) * v + n0) / D;
            if (!(v > 0.0 && u > 0.0 && isfinite(u))) continue;
            const double s1 = sqrt(b2 / den), s2 = u * s1, s3 = v * s1;
            const double X0[3] = {s1 * f0[0], s1 * f0[1], s1 * f0[2]}, X1[3] = {s2 * f1[0], s2 * f1[1], s2 * f1[2]}, X2[3] = {s3 * f2[0], s3 * f2[1], s3 * f2[2]};
            double c1[3], c2v[3], c3[3];
            tri_frame(X0, X1, X2, c1, c2v, c3);
            double Rcw[9];                                 // X_cam = Rcw X_world + tcw
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
              for (int j = 0; j < 3; ++j) Rcw[3 * i + j] = c1[i] * w1[j] + c2v[i] * w2[j] + c3[i] * w3[j];
            }
            double rp[3];
            mat3_mul_vec(Rcw, P0, rp);
            const double tcw[3] = {X0[0] - rp[0], X0[1] - rp[1], X0[2] - rp[2]};
            // body pose: R_wb = (Re Rcw)^T, t_wb = -Rcw^T tcw - R_wb te
            double Rwb[9];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
              for (int j = 0; j < 3; ++j) Rwb[3 * j + i] = a.cam.Re[3 * i] * Rcw[j] + a.cam.Re[3 * i + 1] * Rcw[3 + j] + a.cam.Re[3 * i + 2] * Rcw[6 + j];
            }
            double twc[3], rte[3], pose[7];
            mat3t_mul_vec(Rcw, tcw, twc);
            mat3_mul_vec(Rwb, a.cam.te, rte);
            quat_of_rot(Rwb, pose);
            pose[4] = -twc[0] - rte[0]; pose[5] = -twc[1] - rte[1]; pose[6] = -twc[2] - rte[2];
            if (!finite7(pose)) continue;
            ++n_poses;
            const int cnt = wave_count_inliers(a, n, pose);
            if (cnt > best_cnt) {
              best_cnt = cnt;
#pragma unroll
              for (int kk = 0; kk < 7; ++kk) best_pose[kk] = pose[kk];
            }
          }
        }
      }
    }
  }
  if (lane == 0) {
    hkey[h] = n_poses > 0 ? (((unsigned long long)(best_cnt + 1) << 32) | (unsigned)~(unsigned)(h + 1)) : 0ull;
#pragma unroll
    for (int k = 0; k < 7; ++k) hpose[7 * (size_t)h + k] = best_pose[k];
    htri[h] = make_int4(t2 >= 0 ? t0 : -1, t2 >= 0 ? t1 : -1, t2, n_poses);
  }
}

// ---- selection and refinement ---------------------------------------------------------------------------------------------------------------
// lm_small's problem (small_lm.hpp): LocalMap::LocalBA's pose-only blocks on the matches the LDS mask s_in marks, 1/2 sum rho(|r|^2) under
// HuberLoss; 7 ambient coordinates, 6 tangent unknowns
struct PoseOnInliers {
  static constexpr bool kBox = false;
  const PnpArgs& a;
  int n;
  const uint8_t* s_in;
  __device__ __forceinline__ void accumulate(const double* x, unsigned, double* acc) const {
    PoseD P;
    derive_pose(x, P);
    for (int i = threadIdx.x; i < n; i += kRT) {
      if (!s_in[i]) continue;
      const int2 m = a.list[i];
      const float2 p = a.pt[m.x];
      double r[2], L[12];
      eval_pose_only_local(P, a.cam, (double)p.x, (double)p.y, a.pw + 3 * (size_t)m.y, 1.0, r, L);
      double rho0, rho1;
      huber_eval(a.huber_a, r[0] * r[0] + r[1] * r[1], rho0, rho1);
      acc[27] += 0.5 * rho0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
          const double lu = rho1 * L[6 * k + u];         // rho' J^T J and rho' J^T r: the rows scaled once by rho', not twice by its root
          acc[21 + u] += lu * r[k];
#pragma unroll
          for (int v = 0; v <= u; ++v) acc[u * (u + 1) / 2 + v] += lu * L[6 * k + v];
        }
      }
    }
  }
  __device__ __forceinline__ double cost_part(const double* x) const {
    PoseD P;
    derive_pose(x, P);
    double c = 0.0;
    for (int i = threadIdx.x; i < n; i += kRT) {
      if (!s_in[i]) continue;
      const int2 m = a.list[i];
      const float2 p = a.pt[m.x];
      double rho0, rho1, pcz;      // (the factor's own residual, as the linearisation has it: no depth test inside a solve)
      huber_eval(a.huber_a, reproj_raw(P, a.cam, (double)p.x, (double)p.y, a.pw + 3 * (size_t)m.y, pcz), rho0, rho1);
      c += 0.5 * rho0;
    }
    return c;
  }
  __device__ __forceinline__ void plus(const double* x, const double* dx, double* xc) const { pose_plus(x, dx, xc); }
  __device__ __forceinline__ unsigned norm_mask(unsigned) const { return 127u; }
};
static_assert(kRT == kLT, "lm_small sums over a workgroup of kLT threads");

__global__ void __launch_bounds__(kRT) k_pnp_refine(PnpArgs a, const unsigned long long* __restrict__ hkey, const double* __restrict__ hpose, PnpRec* __restrict__ rec,
                                                    uint8_t* __restrict__ inlier) {
  __shared__ uint8_t s_in[kRelocMaxFeatures];
  __shared__ double tile[lm_tile_doubles(6)];
  __shared__ unsigned long long kred[kRT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = *a.n_dev;
  for (int i = tid; i < a.n_out; i += kRT) inlier[i] = 0;
  // the winner
  unsigned long long key = 0ull;
  if (n >= a.min_matches && n >= 3)
    for (int h = tid; h < a.H + a.have_init; h += kRT) key = max(key, hkey[h]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) key = max(key, (unsigned long long)__shfl_xor(key, m));
  if (lane == 0) kred[wave] = key;
  __syncthreads();
  key = max(max(kred[0], kred[1]), max(kred[2], kred[3]));
  if (key == 0ull) {                                       // too few matches, or no hypothesis has a pose
    if (tid == 0) {
      PnpRec r{};
      r.pose[3] = 1.0; r.rel[3] = 1.0; r.n_matches = n; r.winner = -2;
      *rec = r;
    }
    return;
  }
  const int hw = (int)~(unsigned)(key & 0xffffffffull) - 1;   // -1: the initial pose
  const int slot = hw < 0 ? a.H : hw;
  double x[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) x[k] = hpose[7 * (size_t)slot + k];
  const double gate2 = a.gate2;
  const LmOpts o{a.iters, 1e-6, 1e-10, 1e-8, 1e-3, 1e4};     // function, gradient, parameter tolerance, min_relative_decrease, radius
  LmRec lm{};                                              // (LVF_WHY_NONE is 0)
  int blocks = 0;
  for (int round = 0; round <= a.rounds; ++round) {
    // classify at the current pose
    PoseD P;
    derive_pose(x, P);
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += kRT) {
      const int2 m = a.list[i];
      const float2 p = a.pt[m.x];
      const bool in = reproj_e2(P, a.cam, (double)p.x, (double)p.y, a.pw + 3 * (size_t)m.y) < gate2;
      s_in[i] = in; mine += in;
    }
    __syncthreads();
    const int n_in = (int)wg_sum((double)mine, tile);
    if (round == a.rounds) {                               // the final mask
      for (int i = tid; i < n; i += kRT)
        if (s_in[i]) inlier[a.list[i].x] = 1;
      if (tid == 0) {
        PnpRec r{};
#pragma unroll
        for (int k = 0; k < 7; ++k) { r.pose[k] = x[k]; r.rel[k] = x[k]; }
        if (a.have_old) { double inv[7]; sophus_inverse(a.old, inv); forward_update_pose(inv, x, r.rel); }
        r.initial_cost = lm.initial_cost; r.final_cost = lm.final_cost; r.score = n_in; r.n_matches = n; r.winner = hw; r.winner_count = (int)(key >> 32) - 1;
        r.iters = lm.iters; r.successes = lm.successes; r.termination = lm.termination; r.why = lm.why; r.blocks = blocks; r.found = 1;
        *rec = r;
      }
      break;
    }
    // LocalMap::LocalBA's problem on the inliers under the declared Ceres loop; a failed solve leaves the pose where the round found it
    blocks = n_in;
    lm_small<6, 7, true>(PoseOnInliers{a, n, s_in}, n_in, x, 63u, o, lm, tile);
  }
}

}  // namespace lvf

using namespace lvf;

namespace {

int check_match_options(const char* who, const lvf_match_options* o) {
  LVF_REQUIRE(o->max_distance >= 0 && o->max_distance <= 257, "%s: max_distance %d is outside 0 .. 257", who, o->max_distance);
  LVF_REQUIRE(std::isfinite(o->ratio) && o->ratio >= 0.f, "%s: bad ratio", who);
  LVF_REQUIRE(o->cross_check == 0 || o->cross_check == 1, "%s: cross_check is 0 or 1", who);
  return LVF_OK;
}
int check_pnp_options(const char* who, const lvf_pnp_options* o) {
  LVF_REQUIRE(o->num_hypotheses >= 1 && o->num_hypotheses <= kPnpMaxHypotheses, "%s: num_hypotheses %d is outside 1 .. %d", who, o->num_hypotheses, kPnpMaxHypotheses);
  LVF_REQUIRE(std::isfinite(o->max_reproj_px) && o->max_reproj_px > 0.0, "%s: max_reproj_px must be > 0", who);
  LVF_REQUIRE(o->min_matches >= 3, "%s: min_matches %d is below 3", who, o->min_matches);
  LVF_REQUIRE(o->refine_rounds >= 0 && o->refine_rounds <= 16 && o->refine_iterations >= 0, "%s: bad refine_rounds / refine_iterations", who);
  LVF_REQUIRE(std::isfinite(o->huber_a) && o->huber_a >= 0.0, "%s: bad huber_a", who);
  return LVF_OK;
}

// the match, the gate and the compaction, queued on the context's stream: match / best / second / flag are device arrays [nq], list [nq],
// pos [nq + 1] (pos[nq] = the number of pairs)
struct MatchBufs { DevBuf<unsigned long long> qd, td, qkey, tkey; DevBuf<int> flag, pos; DevBuf<int2> list; };
int queue_match(lvf_ctx* ctx, int nq, const uint8_t* query_desc, int nt, const uint8_t* train_desc, const lvf_match_options& o, MatchBufs& B, int* match_dev,
                int* best_dev, int* second_dev) {
  hipStream_t s = ctx->stream;
  LVF_TRY(B.qd.upload(reinterpret_cast<const unsigned long long*>(query_desc), (size_t)4 * nq, s));
  LVF_TRY(B.td.upload(reinterpret_cast<const unsigned long long*>(train_desc), (size_t)4 * nt, s));
  LVF_TRY(B.qkey.alloc((size_t)2 * nq)); LVF_TRY(B.tkey.alloc(nt)); LVF_TRY(B.flag.alloc(nq)); LVF_TRY(B.pos.alloc((size_t)nq + 1)); LVF_TRY(B.list.alloc(nq));
  hipLaunchKernelGGL(k_orb_match, dim3((nq + nt + 3) / 4), dim3(kRT), 0, s, nq, B.qd.p, nt, B.td.p, B.qkey.p, B.tkey.p);
  LVF_HIP(hipGetLastError());
  const MatchOpt mo{o.max_distance, o.ratio, o.cross_check};
  hipLaunchKernelGGL(k_orb_gate, dim3((nq + kRT - 1) / kRT), dim3(kRT), 0, s, nq, nt, B.qkey.p, B.tkey.p, mo, match_dev, best_dev, second_dev, B.flag.p);
  LVF_HIP(hipGetLastError());
  LVF_TRY(lvf::device_scan1(ctx, B.flag.p, nq, nullptr, B.pos.p, nullptr, nullptr, nullptr));
  hipLaunchKernelGGL(k_match_list, dim3((nq + kRT - 1) / kRT), dim3(kRT), 0, s, nq, match_dev, B.pos.p, B.list.p);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

// the one wait of a call that queued a device_scan1: the scan's sticky error word rides along (as lvf::read_back does), so that a tile that gave
// up fails THIS call instead of a later, unrelated read-back
int wait_checking_scan(lvf_ctx* ctx) {
  unsigned long long* const scan_err = ctx->scan_err;
  if (scan_err) {
    ctx->scan_err = nullptr;
    LVF_TRY(ctx->mailbox.reserve(4096 + 64));
    LVF_HIP(hipMemcpyAsync(ctx->mailbox.p + 4096, scan_err, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  }
  LVF_HIP(hipStreamSynchronize(ctx->stream));
  if (scan_err) {
    unsigned long long w = 0;
    std::memcpy(&w, ctx->mailbox.p + 4096, sizeof(w));
    if (w != 0) {
      (void)hipMemsetAsync(scan_err, 0, sizeof(unsigned long long), ctx->stream);
      lvf::set_error("device scan: tile %llu of launch %llu never published its sum", (w & 0xffffffffull) - 1, w >> 32);
      return LVF_ERR_STATE;
    }
  }
  return LVF_OK;
}

struct PnpBufs { DevBuf<unsigned long long> hkey; DevBuf<double> hpose; DevBuf<int4> htri; };
int queue_score(lvf_ctx* ctx, const PnpArgs& a, PnpBufs& B) {
  hipStream_t s = ctx->stream;
  const int slots = a.H + 1;
  LVF_TRY(B.hkey.alloc(slots)); LVF_TRY(B.hpose.alloc((size_t)7 * slots)); LVF_TRY(B.htri.alloc(slots));
  LVF_HIP(hipMemsetAsync(B.hkey.p, 0, (size_t)slots * sizeof(unsigned long long), s));
  LVF_HIP(hipMemsetAsync(B.htri.p, 0xff, (size_t)slots * sizeof(int4), s));
  hipLaunchKernelGGL(k_pnp_score, dim3((a.H + a.have_init + 3) / 4), dim3(kRT), 0, s, a, B.hkey.p, B.hpose.p, B.htri.p);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}
void fill_args(const lvf_camera* cam0, const lvf_pnp_options& o, PnpArgs* a) {
  std::memset(a, 0, sizeof(*a));
  lvf::make_camd(*cam0, a->cam);
  a->H = o.num_hypotheses; a->min_matches = o.min_matches; a->rounds = o.refine_rounds; a->iters = o.refine_iterations; a->seed = o.seed;
  a->gate2 = o.max_reproj_px * o.max_reproj_px; a->huber_a = o.huber_a;
  a->init[3] = 1.0; a->old[3] = 1.0;
}
void fill_pnp_summary(const PnpRec& r, lvf_solver_summary* s) {
  if (!s) return;
  std::memset(s, 0, sizeof(*s));
  s->initial_cost = r.initial_cost; s->final_cost = r.final_cost; s->num_iterations = r.iters; s->num_successful_steps = r.successes;
  s->num_unsuccessful_steps = r.iters - r.successes; s->num_residual_blocks = r.blocks; s->termination = r.termination; s->termination_reason = r.why;
}

}  // namespace

extern "C" {

void lvf_match_options_default(lvf_match_options* o) {
  if (!o) return;
  o->max_distance = 50; o->ratio = 0.8f; o->cross_check = 1;
}

void lvf_pnp_options_default(lvf_pnp_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->num_hypotheses = 512; o->seed = 0u; o->max_reproj_px = 3.0; o->min_matches = 21; o->refine_rounds = 2; o->refine_iterations = 10; o->huber_a = 1.0;
}

int lvf_orb_match(lvf_ctx* ctx, int nq, const uint8_t* query_desc, int nt, const uint8_t* train_desc, const lvf_match_options* opt, int32_t* match, int32_t* best,
                  int32_t* second) {
  LVF_REQUIRE(ctx && nq >= 0 && nt >= 0, "lvf_orb_match: bad argument");
  LVF_REQUIRE(nq <= kRelocMaxFeatures && nt <= kRelocMaxFeatures, "lvf_orb_match: %d x %d descriptors exceed the limit of %d a side", nq, nt, kRelocMaxFeatures);
  lvf_match_options o;
  if (opt) o = *opt; else lvf_match_options_default(&o);
  LVF_TRY(check_match_options("lvf_orb_match", &o));
  if (nq == 0) return LVF_OK;
  LVF_REQUIRE(match && query_desc && (nt == 0 || train_desc), "lvf_orb_match: null array");
  if (nt == 0) {
    for (int i = 0; i < nq; ++i) { match[i] = -1; if (best) best[i] = -1; if (second) second[i] = -1; }
    return LVF_OK;
  }
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  MatchBufs B;
  DevBuf<int> out;
  LVF_TRY(out.alloc((size_t)3 * nq));
  LVF_TRY(queue_match(ctx, nq, query_desc, nt, train_desc, o, B, out.p, out.p + nq, out.p + 2 * (size_t)nq));
  LVF_HIP(hipMemcpyAsync(match, out.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
  if (best) LVF_HIP(hipMemcpyAsync(best, out.p + nq, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
  if (second) LVF_HIP(hipMemcpyAsync(second, out.p + 2 * (size_t)nq, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, s));
  LVF_TRY(wait_checking_scan(ctx));
  return LVF_OK;
}

int lvf_pnp_ransac(lvf_ctx* ctx, const lvf_camera* cam0, int n, const double* pw, const float* pt, const double* init_pose7, const lvf_pnp_options* opt, double* pose7,
                   int32_t* score, uint8_t* inlier, lvf_solver_summary* summary) {
  LVF_REQUIRE(ctx && n >= 0 && score, "lvf_pnp_ransac: bad argument");
  LVF_REQUIRE(n <= kRelocMaxFeatures, "lvf_pnp_ransac: %d correspondences exceed the limit of %d", n, kRelocMaxFeatures);
  lvf_pnp_options o;
  if (opt) o = *opt; else lvf_pnp_options_default(&o);
  LVF_TRY(check_pnp_options("lvf_pnp_ransac", &o));
  LVF_TRY(check_camera("lvf_pnp_ransac", cam0));
  LVF_REQUIRE(n == 0 || (pw && pt), "lvf_pnp_ransac: null correspondence arrays");
  if (init_pose7) LVF_TRY(lvf::check_pose("lvf_pnp_ransac", "the initial pose", init_pose7, nullptr));
  LVF_REQUIRE(pose7 || n < o.min_matches, "lvf_pnp_ransac: null pose7");
  *score = 0;
  if (summary) std::memset(summary, 0, sizeof(*summary));
  if (inlier) std::memset(inlier, 0, (size_t)n);
  if (n < o.min_matches) return LVF_OK;                    // nothing is launched, pose7 stays as it came
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  std::vector<int2> ident(n);
  for (int i = 0; i < n; ++i) ident[i] = make_int2(i, i);
  DevBuf<int2> list; DevBuf<double> dpw; DevBuf<float2> dpt; DevBuf<int> nd; DevBuf<char> out;
  LVF_TRY(list.upload(ident.data(), n, s)); LVF_TRY(dpw.upload(pw, (size_t)3 * n, s)); LVF_TRY(dpt.upload(reinterpret_cast<const float2*>(pt), n, s));
  LVF_TRY(nd.upload(&n, 1, s)); LVF_TRY(out.alloc(sizeof(PnpRec) + (size_t)n));
  PnpArgs a;
  fill_args(cam0, o, &a);
  a.n_dev = nd.p; a.list = list.p; a.pw = dpw.p; a.pt = dpt.p; a.n_out = n;
  if (init_pose7) { a.have_init = 1; std::memcpy(a.init, init_pose7, sizeof(a.init)); }
  PnpBufs B;
  LVF_TRY(queue_score(ctx, a, B));
  hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(kRT), 0, s, a, B.hkey.p, B.hpose.p, reinterpret_cast<PnpRec*>(out.p), reinterpret_cast<uint8_t*>(out.p + sizeof(PnpRec)));
  LVF_HIP(hipGetLastError());
  std::vector<char> host(sizeof(PnpRec) + (size_t)n);
  LVF_HIP(hipMemcpyAsync(host.data(), out.p, host.size(), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  PnpRec r;
  std::memcpy(&r, host.data(), sizeof(r));
  if (!r.found) return LVF_OK;
  std::memcpy(pose7, r.pose, sizeof(r.pose));
  *score = r.score;
  if (inlier) std::memcpy(inlier, host.data() + sizeof(PnpRec), (size_t)n);
  fill_pnp_summary(r, summary);
  return LVF_OK;
}

int lvf_relocate_by_image(lvf_ctx* ctx, const lvf_camera* cam0, const double* old_pose7, int n_old, const double* old_pw, const uint8_t* old_desc, int n_cur,
                          const float* cur_pt, const uint8_t* cur_desc, const lvf_match_options* match_opt, const lvf_pnp_options* pnp_opt, double* relative_o_c7,
                          int32_t* score, int32_t* match, uint8_t* inlier, lvf_solver_summary* summary) {
  LVF_REQUIRE(ctx && n_old >= 0 && n_cur >= 0 && score && relative_o_c7 && old_pose7, "lvf_relocate_by_image: bad argument");
  LVF_REQUIRE(n_old <= kRelocMaxFeatures && n_cur <= kRelocMaxFeatures, "lvf_relocate_by_image: %d x %d features exceed the limit of %d a side", n_cur, n_old,
              kRelocMaxFeatures);
  lvf_match_options mo; lvf_pnp_options po;
  if (match_opt) mo = *match_opt; else lvf_match_options_default(&mo);
  if (pnp_opt) po = *pnp_opt; else lvf_pnp_options_default(&po);
  LVF_TRY(check_match_options("lvf_relocate_by_image", &mo));
  LVF_TRY(check_pnp_options("lvf_relocate_by_image", &po));
  LVF_TRY(check_camera("lvf_relocate_by_image", cam0));
  LVF_TRY(lvf::check_pose("lvf_relocate_by_image", "the old pose", old_pose7, nullptr));
  LVF_TRY(lvf::check_pose("lvf_relocate_by_image", "the relative pose", relative_o_c7, nullptr));
  LVF_REQUIRE((n_old == 0 || (old_pw && old_desc)) && (n_cur == 0 || (cur_pt && cur_desc)), "lvf_relocate_by_image: null feature arrays");
  *score = 0;
  if (summary) std::memset(summary, 0, sizeof(*summary));
  if (inlier) std::memset(inlier, 0, (size_t)n_cur);
  if (match) for (int i = 0; i < n_cur; ++i) match[i] = -1;
  if (n_cur == 0 || n_old == 0) return LVF_OK;             // nothing to match: no pair, as lvf_orb_match
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  // one buffer comes back: the record, match [n_cur], inlier [n_cur]
  const size_t off_match = sizeof(PnpRec), off_in = off_match + (size_t)n_cur * sizeof(int), total = off_in + (size_t)n_cur;
  DevBuf<char> out; DevBuf<int> bs; DevBuf<double> dpw; DevBuf<float2> dpt;
  LVF_TRY(out.alloc(total)); LVF_TRY(bs.alloc((size_t)2 * n_cur));
  LVF_TRY(dpw.upload(old_pw, (size_t)3 * n_old, s)); LVF_TRY(dpt.upload(reinterpret_cast<const float2*>(cur_pt), n_cur, s));
  MatchBufs MB;
  LVF_TRY(queue_match(ctx, n_cur, cur_desc, n_old, old_desc, mo, MB, reinterpret_cast<int*>(out.p + off_match), bs.p, bs.p + n_cur));
  PnpArgs a;
  fill_args(cam0, po, &a);
  a.n_dev = MB.pos.p + n_cur; a.list = MB.list.p; a.pw = dpw.p; a.pt = dpt.p; a.n_out = n_cur;
  a.have_init = 1; a.have_old = 1;
  std::memcpy(a.init, relative_o_c7, sizeof(a.init)); std::memcpy(a.old, old_pose7, sizeof(a.old));
  PnpBufs B;
  LVF_TRY(queue_score(ctx, a, B));
  hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(kRT), 0, s, a, B.hkey.p, B.hpose.p, reinterpret_cast<PnpRec*>(out.p), reinterpret_cast<uint8_t*>(out.p + off_in));
  LVF_HIP(hipGetLastError());
  std::vector<char> host(total);
  LVF_HIP(hipMemcpyAsync(host.data(), out.p, total, hipMemcpyDeviceToHost, s));
  LVF_TRY(wait_checking_scan(ctx));                        // the one wait
  PnpRec r;
  std::memcpy(&r, host.data(), sizeof(r));
  if (match) std::memcpy(match, host.data() + off_match, (size_t)n_cur * sizeof(int));
  if (!r.found) return LVF_OK;                             // fewer than min_matches pairs (the kernels returned at once), or no hypothesis has a pose
  std::memcpy(relative_o_c7, r.rel, sizeof(r.rel));
  *score = r.score;
  if (inlier) std::memcpy(inlier, host.data() + off_in, (size_t)n_cur);
  fill_pnp_summary(r, summary);
  return LVF_OK;
}

int lvf_pnp_debug_hypotheses(lvf_ctx* ctx, const lvf_camera* cam0, int n, const double* pw, const float* pt, const lvf_pnp_options* opt, int32_t* triples,
                             int32_t* n_poses, int32_t* count, double* poses) {
  LVF_REQUIRE(ctx && n >= 3 && n <= kRelocMaxFeatures && pw && pt && triples && n_poses && count, "lvf_pnp_debug_hypotheses: bad argument");
  lvf_pnp_options o;
  if (opt) o = *opt; else lvf_pnp_options_default(&o);
  LVF_TRY(check_pnp_options("lvf_pnp_debug_hypotheses", &o));
  LVF_TRY(check_camera("lvf_pnp_debug_hypotheses", cam0));
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  std::vector<int2> ident(n);
  for (int i = 0; i < n; ++i) ident[i] = make_int2(i, i);
  DevBuf<int2> list; DevBuf<double> dpw; DevBuf<float2> dpt; DevBuf<int> nd;
  LVF_TRY(list.upload(ident.data(), n, s)); LVF_TRY(dpw.upload(pw, (size_t)3 * n, s)); LVF_TRY(dpt.upload(reinterpret_cast<const float2*>(pt), n, s));
  LVF_TRY(nd.upload(&n, 1, s));
  PnpArgs a;
  fill_args(cam0, o, &a);
  a.min_matches = 3;                                       // (the tap scores whatever it is given)
  a.n_dev = nd.p; a.list = list.p; a.pw = dpw.p; a.pt = dpt.p; a.n_out = n;
  PnpBufs B;
  LVF_TRY(queue_score(ctx, a, B));
  const int H = a.H;
  std::vector<unsigned long long> key(H);
  std::vector<int4> tri(H);
  LVF_HIP(hipMemcpyAsync(key.data(), B.hkey.p, (size_t)H * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(tri.data(), B.htri.p, (size_t)H * sizeof(int4), hipMemcpyDeviceToHost, s));
  if (poses) LVF_HIP(hipMemcpyAsync(poses, B.hpose.p, (size_t)7 * H * sizeof(double), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  for (int h = 0; h < H; ++h) {
    triples[3 * h] = tri[h].x; triples[3 * h + 1] = tri[h].y; triples[3 * h + 2] = tri[h].z;
    n_poses[h] = tri[h].w; count[h] = key[h] ? (int)(key[h] >> 32) - 1 : 0;
  }
  return LVF_OK;
}

}  // extern "C"
