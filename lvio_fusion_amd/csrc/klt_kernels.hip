// klt_kernels.hip — the feature tracker on the device: image pyramids with Scharr derivatives, pyramidal Lucas-Kanade flow with the
// forward-backward gate (utility.cpp:55-89), the stereo triangulation (utility.cpp:7-18, local_map.cpp:233-269) and the numeric part of
// Frontend::TrackLastFrame (frontend.cpp:163-256).  The semantics are the declared ones of tests/klt_ref.py: the structure of
// cv::calcOpticalFlowPyrLK with floating-point interpolation, not a bit pin against OpenCV.
//
// Flow: ONE launch, one wavefront per feature.  The window's pixels (at most 21 x 21 = 441) are dealt 7 per lane; the template patch I and
// its derivative pair stay in registers for the whole level; the five sums of the normal equations are reduced by a __shfl_xor butterfly
// (a fixed order, no atomics: a feature's result depends on nothing but its own inputs, so runs and permutations are bit-identical).
// Every branch of the level / iteration control is taken on reduced values that all 64 lanes hold bit-equal, so a feature that converges,
// leaves the image or is lost stops its whole wave at once.  The J neighbourhood is gathered through the cache hierarchy (a level image is
// at most 466 KB at 1241 x 376 and stays in L2; the 22 x 22 bytes of one window stay in the CU's vector L1 across the iterations).
#include "lvf_internal.hpp"

#include <cmath>

namespace {
using lvf::DevBuf; using lvf::Pinhole; using lvf::Rigid; using lvf::grid_of; using lvf::refl101;

constexpr int kMaxLevels = 8;        // pyramid levels an image can hold (max_level <= 7)
constexpr int kMaxWin = 21;          // 7 pixels per lane x 64 lanes >= win^2
constexpr int kPerLane = 7;
constexpr int kFlowBlock = 256;      // 4 waves = 4 features per workgroup
constexpr int kT = 256;

struct KltLevel { const uint8_t* g; const short2* d; int w, h; };

}  // namespace

struct lvf_image {
  lvf_ctx* ctx = nullptr;
  int w = 0, h = 0, levels = 0;      // levels = max_level + 1
  int lw[kMaxLevels] = {0}, lh[kMaxLevels] = {0};
  size_t off[kMaxLevels] = {0};      // pixel offset of each level in gray / deriv
  DevBuf<uint8_t> gray;
  DevBuf<short2> deriv;              // (Sx, Sy) interleaved: one 4-byte load fetches the pair
  DevBuf<KltLevel> table;            // the level table the kernels read (wave-uniform loads)
  KltLevel host_table[kMaxLevels] = {};      // what `table` is copied from (lives as long as the copy may be in flight)
};

namespace {

// level L+1 from level L: separable [1 4 6 4 1] decimation, reflect-101, (sum + 128) >> 8
__global__ void __launch_bounds__(kT) k_klt_pyr_down(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= dw * dh) return;
  const int y = i / dw, x = i - y * dw;
  const int k[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) xs[t] = refl101(2 * x + t - 2, sw);
  int acc = 0;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const uint8_t* row = src + (size_t)refl101(2 * y + r - 2, sh) * sw;
    int s = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) s += k[t] * (int)row[xs[t]];
    acc += k[r] * s;
  }
  dst[i] = (uint8_t)((acc + 128) >> 8);
}

// unnormalised Scharr pair of one level, reflect-101 at the edge, exact in int16
__global__ void __launch_bounds__(kT) k_klt_scharr(const uint8_t* __restrict__ src, int w, int h, short2* __restrict__ dst) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i - y * w;
  const int xm = refl101(x - 1, w), xp = refl101(x + 1, w);
  const uint8_t* r0 = src + (size_t)refl101(y - 1, h) * w;
  const uint8_t* r1 = src + (size_t)y * w;
  const uint8_t* r2 = src + (size_t)refl101(y + 1, h) * w;
  const int sx = 3 * ((int)r0[xp] - (int)r0[xm]) + 10 * ((int)r1[xp] - (int)r1[xm]) + 3 * ((int)r2[xp] - (int)r2[xm]);
  const int sy = 3 * ((int)r2[xm] - (int)r0[xm]) + 10 * ((int)r2[x] - (int)r0[x]) + 3 * ((int)r2[xp] - (int)r0[xp]);
  dst[i] = make_short2((short)sx, (short)sy);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;      // the butterfly adds the same pairs in every lane: all 64 hold the same bits
}

__device__ __forceinline__ float gray_at(const KltLevel& lv, int x, int y, bool inside) {
  if (!inside) { x = refl101(x, lv.w); y = refl101(y, lv.h); }
  return (float)lv.g[(size_t)y * lv.w + x];
}

__device__ __forceinline__ float bilinear_gray(const KltLevel& lv, int x, int y, bool inside, float w00, float w01, float w10, float w11) {
  if (inside) {
    const uint8_t* p = lv.g + (size_t)y * lv.w + x;
    return w00 * (float)p[0] + w01 * (float)p[1] + w10 * (float)p[lv.w] + w11 * (float)p[lv.w + 1];
  }
  return w00 * gray_at(lv, x, y, false) + w01 * gray_at(lv, x + 1, y, false) + w10 * gray_at(lv, x, y + 1, false) + w11 * gray_at(lv, x + 1, y + 1, false);
}

__device__ __forceinline__ float2 deriv_at(const KltLevel& lv, int x, int y) {      // constant (zero) border
  if ((unsigned)x >= (unsigned)lv.w || (unsigned)y >= (unsigned)lv.h) return make_float2(0.f, 0.f);
  const short2 s = lv.d[(size_t)y * lv.w + x];
  return make_float2((float)s.x, (float)s.y);
}

__device__ __forceinline__ bool window_outside(int ix, int iy, int win, int cols, int rows) { return ix < -win || ix >= cols || iy < -win || iy >= rows; }

// One tracker pass of one feature by one wave (tests/klt_ref.py lk).  (nx, ny) enters as the initial flow and leaves as the result.
__device__ bool lk_pass(const KltLevel* __restrict__ A, const KltLevel* __restrict__ B, float px, float py, float& nx, float& ny, int win, int max_level,
                        int max_iter, float eps2, float min_eig, int lane) {
  bool st = true;
  const float half = (float)(win - 1) * 0.5f;
  const int npx = win * win;
  int ox[kPerLane], oy[kPerLane];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int p = lane + 64 * k;
    oy[k] = p / win;
    ox[k] = p - oy[k] * win;
  }
  for (int L = max_level; L >= 0; --L) {
    const KltLevel la = A[L], lb = B[L];
    const int cols = la.w, rows = la.h;
    const float scale = 1.0f / (float)(1 << L);
    const float pxl = px * scale - half, pyl = py * scale - half;
    if (L == max_level) { nx *= scale; ny *= scale; } else { nx *= 2.0f; ny *= 2.0f; }
    const int ipx = (int)floorf(pxl), ipy = (int)floorf(pyl);
    if (window_outside(ipx, ipy, win, cols, rows)) { if (L == 0) st = false; continue; }
    float I[kPerLane], Sx[kPerLane], Sy[kPerLane];
    float a11 = 0.f, a12 = 0.f, a22 = 0.f;
    {
      const float a = pxl - (float)ipx, b = pyl - (float)ipy;
      const float w00 = (1.f - a) * (1.f - b), w01 = a * (1.f - b), w10 = (1.f - a) * b, w11 = a * b;
      const bool inside = ipx >= 0 && ipy >= 0 && ipx + win < cols && ipy + win < rows;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        I[k] = 0.f; Sx[k] = 0.f; Sy[k] = 0.f;
        if (lane + 64 * k < npx) {
          const int x = ipx + ox[k], y = ipy + oy[k];
          I[k] = bilinear_gray(la, x, y, inside, w00, w01, w10, w11);
          const float2 d00 = deriv_at(la, x, y), d01 = deriv_at(la, x + 1, y), d10 = deriv_at(la, x, y + 1), d11 = deriv_at(la, x + 1, y + 1);
          Sx[k] = w00 * d00.x + w01 * d01.x + w10 * d10.x + w11 * d11.x;
          Sy[k] = w00 * d00.y + w01 * d01.y + w10 * d10.y + w11 * d11.y;
        }
        a11 += Sx[k] * Sx[k]; a12 += Sx[k] * Sy[k]; a22 += Sy[k] * Sy[k];
      }
    }
    const float kA = 1.0f / 1048576.0f, kB = 1.0f / 32768.0f;       // 2^-20, 2^-15
    const float A11 = wave_sum(a11) * kA, A12 = wave_sum(a12) * kA, A22 = wave_sum(a22) * kA;
    const float D = A11 * A22 - A12 * A12;
    const float me = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * npx);
    if (me < min_eig || D < 1.1920929e-07f) { if (L == 0) st = false; continue; }
    float qx = nx - half, qy = ny - half, dpx = 0.f, dpy = 0.f;
    for (int j = 0; j < max_iter; ++j) {
      const int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
      if (window_outside(iqx, iqy, win, cols, rows)) { if (L == 0) st = false; break; }
      const float a = qx - (float)iqx, b = qy - (float)iqy;
      const float w00 = (1.f - a) * (1.f - b), w01 = a * (1.f - b), w10 = (1.f - a) * b, w11 = a * b;
      const bool inside = iqx >= 0 && iqy >= 0 && iqx + win < cols && iqy + win < rows;
      float b1 = 0.f, b2 = 0.f;
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        if (lane + 64 * k < npx) {
          const float diff = bilinear_gray(lb, iqx + ox[k], iqy + oy[k], inside, w00, w01, w10, w11) - I[k];
          b1 += diff * Sx[k]; b2 += diff * Sy[k];
        }
      }
      b1 = wave_sum(b1) * kB; b2 = wave_sum(b2) * kB;
      const float dx = (A12 * b2 - A22 * b1) / D, dy = (A12 * b1 - A11 * b2) / D;
      qx += dx; qy += dy;
      nx = qx + half; ny = qy + half;
      if (dx * dx + dy * dy <= eps2) break;
      if (j > 0 && fabsf(dx + dpx) < 0.01f && fabsf(dy + dpy) < 0.01f) { nx -= dx * 0.5f; ny -= dy * 0.5f; break; }
      dpx = dx; dpy = dy;
    }
  }
  return st;
}

struct FlowP { int win, levels, bwin, blevels, max_iter; float eps2, min_eig; double fb_max; };

// optical_flow (utility.cpp:55-89) for n features: forward pass A -> B, backward pass B -> A started at prev, gate.
__global__ void __launch_bounds__(kFlowBlock) k_klt_flow(int n, const KltLevel* __restrict__ A, const KltLevel* __restrict__ B, const float2* __restrict__ prev,
                                                          float2* __restrict__ next, uint8_t* __restrict__ status, float* __restrict__ fb_out, FlowP P) {
  const int f = blockIdx.x * (kFlowBlock / 64) + (threadIdx.x >> 6);
  if (f >= n) return;
  const int lane = threadIdx.x & 63;
  const float2 p = prev[f];
  float2 q = next[f];
  const bool st = lk_pass(A, B, p.x, p.y, q.x, q.y, P.win, P.levels, P.max_iter, P.eps2, P.min_eig, lane);
  bool ok = false;
  float fb = INFINITY;
  if (st) {                                     // (a lost feature does not run the backward pass)
    float bx = p.x, by = p.y;
    if (lk_pass(B, A, q.x, q.y, bx, by, P.bwin, P.blevels, P.max_iter, P.eps2, P.min_eig, lane)) {
      const float dx = p.x - bx, dy = p.y - by;  // cv_distance: float differences, double norm (utility.cpp:20-25)
      const double d = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
      fb = (float)d;
      ok = d <= P.fb_max && q.x >= 0.f && q.x < (float)A[0].w && q.y >= 0.f && q.y < (float)A[0].h;
    }
  }
  if (lane == 0) {
    next[f] = q;
    status[f] = ok ? 1 : 0;
    if (fb_out) fb_out[f] = fb;
  }
}

// ---- geometry (fp64, one thread per feature; the camera chains are camera_dev.hpp's) ----------------------------------------------------------
// local_map.cpp:240-242: the left pixel at depth 50 * baseline, seen by camera 1
__global__ void __launch_bounds__(kT) k_klt_stereo_predict(int n, const float2* __restrict__ left, float2* __restrict__ right, Pinhole c0, Pinhole c1, double depth) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const float2 kp = left[i];
  double ps[3], pb[3], pc[3];
  pixel2sensor(c0, (double)kp.x, (double)kp.y, depth, ps);
  sensor2robot(c0, ps, pb);
  robot2sensor(c1, pb, pc);
  right[i] = sensor2pixel(c1, pc);
}

// one Hestenes rotation of columns P, Q of the 4x4 pair (A, V); column-major a[4 * col + row], all indices compile-time
template <int P, int Q>
__device__ __forceinline__ bool jacobi_rotate(double (&a)[16], double (&v)[16]) {
  double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) { alpha += a[4 * P + r] * a[4 * P + r]; beta += a[4 * Q + r] * a[4 * Q + r]; gamma += a[4 * P + r] * a[4 * Q + r]; }
  if (gamma == 0.0 || fabs(gamma) <= 4e-16 * sqrt(alpha * beta)) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double ap = a[4 * P + r], aq = a[4 * Q + r];
    a[4 * P + r] = c * ap - s * aq; a[4 * Q + r] = s * ap + c * aq;
    const double vp = v[4 * P + r], vq = v[4 * Q + r];
    v[4 * P + r] = c * vp - s * vq; v[4 * Q + r] = s * vp + c * vq;
  }
  return true;
}

// triangulate (utility.cpp:7-18) + the depth gate and inverse depth of local_map.cpp:256-258.  The right singular vector of the smallest
// singular value comes from a one-sided Jacobi SVD of the 4x4 DLT matrix itself (A^T A is never formed: it would square the condition number).
// status: in = the flow's (0 / 1); out = 0 lost, 1 accepted, 2 tracked but behind camera 0.
__global__ void __launch_bounds__(kT) k_klt_dlt(int n, const float2* __restrict__ left, const float2* __restrict__ right, uint8_t* __restrict__ status,
                                                 double* __restrict__ inv_depth, double* __restrict__ p_robot, Pinhole c0, Pinhole c1) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  double out_inv = 0.0, pb[3] = {0.0, 0.0, 0.0};
  uint8_t st = status[i];
  if (st) {
    const float2 kl = left[i], kr = right[i];
    double n0[3], n1[3];                                                                        // Pixel2Sensor, depth 1
    pixel2sensor(c0, (double)kl.x, (double)kl.y, 1.0, n0);
    pixel2sensor(c1, (double)kr.x, (double)kr.y, 1.0, n1);
    const double x0 = n0[0], y0 = n0[1], x1 = n1[0], y1 = n1[1];
    // P = extrinsic.inverse().matrix3x4() = [R^T | -R^T t]; row r of P: (R[r], R[3 + r], R[6 + r], m[r])
    const double m0[3] = {-(c0.R[0] * c0.t[0] + c0.R[3] * c0.t[1] + c0.R[6] * c0.t[2]), -(c0.R[1] * c0.t[0] + c0.R[4] * c0.t[1] + c0.R[7] * c0.t[2]),
                          -(c0.R[2] * c0.t[0] + c0.R[5] * c0.t[1] + c0.R[8] * c0.t[2])};
    const double m1[3] = {-(c1.R[0] * c1.t[0] + c1.R[3] * c1.t[1] + c1.R[6] * c1.t[2]), -(c1.R[1] * c1.t[0] + c1.R[4] * c1.t[1] + c1.R[7] * c1.t[2]),
                          -(c1.R[2] * c1.t[0] + c1.R[5] * c1.t[1] + c1.R[8] * c1.t[2])};
    const double P0[12] = {c0.R[0], c0.R[3], c0.R[6], m0[0], c0.R[1], c0.R[4], c0.R[7], m0[1], c0.R[2], c0.R[5], c0.R[8], m0[2]};
    const double P1[12] = {c1.R[0], c1.R[3], c1.R[6], m1[0], c1.R[1], c1.R[4], c1.R[7], m1[1], c1.R[2], c1.R[5], c1.R[8], m1[2]};
    double a[16], v[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[4 * c + 0] = x0 * P0[8 + c] - P0[c]; a[4 * c + 1] = y0 * P0[8 + c] - P0[4 + c];
      a[4 * c + 2] = x1 * P1[8 + c] - P1[c]; a[4 * c + 3] = y1 * P1[8 + c] - P1[4 + c];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * c + r] = r == c ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
      bool any = jacobi_rotate<0, 1>(a, v);
      any |= jacobi_rotate<0, 2>(a, v); any |= jacobi_rotate<0, 3>(a, v); any |= jacobi_rotate<1, 2>(a, v);
      any |= jacobi_rotate<1, 3>(a, v); any |= jacobi_rotate<2, 3>(a, v);
      if (!any) break;
    }
    double best = INFINITY, h[4] = {0, 0, 0, 1};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double s2 = a[4 * c] * a[4 * c] + a[4 * c + 1] * a[4 * c + 1] + a[4 * c + 2] * a[4 * c + 2] + a[4 * c + 3] * a[4 * c + 3];
      if (s2 < best) { best = s2; h[0] = v[4 * c]; h[1] = v[4 * c + 1]; h[2] = v[4 * c + 2]; h[3] = v[4 * c + 3]; }
    }
    pb[0] = h[0] / h[3]; pb[1] = h[1] / h[3]; pb[2] = h[2] / h[3];
    double s0[3], s1[3];
    robot2sensor(c0, pb, s0);
    robot2sensor(c1, pb, s1);
    st = s0[2] > 0 ? 1 : 2;                                  // local_map.cpp:256
    out_inv = 1.0 / s1[2];                                   // local_map.cpp:258: camera ONE, as the reference has it
  }
  status[i] = st;
  inv_depth[i] = out_inv;
  p_robot[3 * i] = pb[0]; p_robot[3 * i + 1] = pb[1]; p_robot[3 * i + 2] = pb[2];
}

// frontend.cpp:168-170: World2Pixel(pw, current pose); also the depth in camera 0 that Camera::Far tests (camera.h:38-41)
__global__ void __launch_bounds__(kT) k_klt_track_predict(int n, const double* __restrict__ pw, float2* __restrict__ pred, float2* __restrict__ cur, double* __restrict__ z,
                                                           Pinhole c0, Rigid T) {      // T: body -> world
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  double pb[3], pc[3];
  world2robot(T, pw + 3 * i, pb);
  robot2sensor(c0, pb, pc);
  const float2 px = sensor2pixel(c0, pc);
  pred[i] = px; cur[i] = px;                                 // kps_current = kps_perdict (frontend.cpp:188)
  z[i] = pc[2];
}

// frontend.cpp:195-256: mean deviation over the tracked points (fixed-order tree in fp64), class per point, number of good points.
// ONE workgroup.  cls: 0 lost, 1 far, 2 near, 3 moving.
__global__ void __launch_bounds__(kT) k_klt_track_classify(int n, const float2* __restrict__ pred, const float2* __restrict__ cur, const uint8_t* __restrict__ status,
                                                            const double* __restrict__ z, double far_depth, int remove_moving, int bad, uint8_t* __restrict__ cls,
                                                            int* __restrict__ n_good) {
  __shared__ double sx[kT], sy[kT];
  __shared__ int sc[kT];
  const int t = threadIdx.x;
  double ax = 0, ay = 0; int cnt = 0;
  for (int i = t; i < n; i += kT)
    if (status[i]) { ax += (double)(pred[i].x - cur[i].x); ay += (double)(pred[i].y - cur[i].y); ++cnt; }      // Point2f differences
  sx[t] = ax; sy[t] = ay; sc[t] = cnt;
  __syncthreads();
  for (int m = kT / 2; m >= 1; m >>= 1) {
    if (t < m) { sx[t] += sx[t + m]; sy[t] += sy[t + m]; sc[t] += sc[t + m]; }
    __syncthreads();
  }
  const int n_ok = sc[0];
  const double mx = sx[0] / (double)(n_ok > 1 ? n_ok : 1), my = sy[0] / (double)(n_ok > 1 ? n_ok : 1);
  __syncthreads();
  int good = 0;
  for (int i = t; i < n; i += kT) {
    uint8_t c = 0;
    if (status[i]) {
      const double dx = (double)(pred[i].x - cur[i].x) - mx, dy = (double)(pred[i].y - cur[i].y) - my;
      if (z[i] > far_depth) c = 1;
      else if (!remove_moving || sqrt(dx * dx + dy * dy) < 30.0) c = 2;
      else c = 3;
      good += c != 3;
    }
    cls[i] = c;
  }
  sc[t] = good;
  __syncthreads();
  for (int m = kT / 2; m >= 1; m >>= 1) {
    if (t < m) sc[t] += sc[t + m];
    __syncthreads();
  }
  if (t == 0) *n_good = sc[0] > bad ? sc[0] : 0;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
int check_flow(const char* who, const lvf_image* a, const lvf_image* b, int n, const lvf_flow_options* o) {
  LVF_REQUIRE(a && b, "%s: null image", who);
  LVF_REQUIRE(a->ctx == b->ctx, "%s: the images belong to different contexts", who);
  LVF_REQUIRE(a->w == b->w && a->h == b->h, "%s: image sizes differ (%d x %d vs %d x %d)", who, a->w, a->h, b->w, b->h);
  LVF_REQUIRE(n >= 0, "%s: negative point count", who);
  LVF_REQUIRE(o->win >= 1 && o->win <= kMaxWin && o->back_win >= 1 && o->back_win <= kMaxWin, "%s: window sizes must be in [1, %d]", who, kMaxWin);
  LVF_REQUIRE(o->max_level >= 0 && o->back_max_level >= 0, "%s: negative level count", who);
  const int need = std::max(o->max_level, o->back_max_level) + 1;
  LVF_REQUIRE(need <= a->levels && need <= b->levels, "%s: the options ask for %d pyramid levels, the images hold %d and %d", who, need, a->levels, b->levels);
  LVF_REQUIRE(o->max_iter >= 1 && o->eps >= 0.0 && o->fb_max >= 0.0, "%s: bad termination options", who);
  return LVF_OK;
}

// the flow launch on device arrays (next: in = initial flow, out = result)
void launch_flow(hipStream_t s, const lvf_image* a, const lvf_image* b, int n, const float2* prev, float2* next, uint8_t* status, float* fb, const lvf_flow_options* o) {
  FlowP P;
  P.win = o->win; P.levels = o->max_level; P.bwin = o->back_win; P.blevels = o->back_max_level; P.max_iter = o->max_iter;
  P.eps2 = (float)o->eps * (float)o->eps; P.min_eig = (float)o->min_eig; P.fb_max = o->fb_max;
  const int per = kFlowBlock / 64;
  hipLaunchKernelGGL(k_klt_flow, dim3((n + per - 1) / per), dim3(kFlowBlock), 0, s, n, a->table.p, b->table.p, prev, next, status, fb, P);
}

// lvf_stereo_triangulate and lvf_stereo_triangulate_lidar: the 50-baseline prediction, the flow and the DLT, then — with a projected sweep —
// the LiDAR query and the merge (lidar_depth_kernels.hip) behind them; the downloads and ONE wait.  depth == nullptr: no merge, no source.
int stereo_chain(const char* who, const lvf_image* left, const lvf_image* right, const lvf_camera* cam0, const lvf_camera* cam1, double baseline, int n,
                 const float* kps_left, float* kps_right, uint8_t* status, double* inv_depth, double* p_robot, const lvf_flow_options* opt, const lvf_lidar_depth* depth,
                 uint8_t* source) {
  lvf_flow_options o;
  if (opt) o = *opt; else lvf_flow_options_default(&o);
  LVF_TRY(check_flow(who, left, right, n, &o));
  LVF_TRY(lvf::check_camera(who, cam0));
  LVF_TRY(lvf::check_camera(who, cam1));
  LVF_REQUIRE(baseline > 0.0, "%s: baseline must be > 0", who);
  if (depth) LVF_TRY(lvf::lidar_depth_check(who, depth, left->ctx, cam0, cam1));
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(kps_left && kps_right && status && inv_depth && p_robot && (!depth || source), "%s: null point arrays", who);
  lvf_ctx* ctx = left->ctx;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  const Pinhole c0 = lvf::make_pinhole(*cam0), c1 = lvf::make_pinhole(*cam1);
  DevBuf<float2> p, q; DevBuf<uint8_t> st, src; DevBuf<double> inv, pb;
  lvf::StreamWaitGuard wait(s);                  // (an error below: what is queued ends before the buffers go)
  LVF_TRY(p.upload(reinterpret_cast<const float2*>(kps_left), n, s));
  LVF_TRY(q.alloc(n)); LVF_TRY(st.alloc(n)); LVF_TRY(inv.alloc(n)); LVF_TRY(pb.alloc((size_t)3 * n));
  if (depth) LVF_TRY(src.alloc(n));
  hipLaunchKernelGGL(k_klt_stereo_predict, dim3(grid_of(n)), dim3(kT), 0, s, n, p.p, q.p, c0, c1, baseline * 50);
  launch_flow(s, left, right, n, p.p, q.p, st.p, (float*)nullptr, &o);
  hipLaunchKernelGGL(k_klt_dlt, dim3(grid_of(n)), dim3(kT), 0, s, n, p.p, q.p, st.p, inv.p, pb.p, c0, c1);
  LVF_HIP(hipGetLastError());
  if (depth) LVF_TRY(lvf::lidar_depth_merge_queue(depth, c0, c1, baseline, n, p.p, q.p, st.p, inv.p, pb.p, src.p));
  LVF_HIP(hipMemcpyAsync(kps_right, q.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(status, st.p, (size_t)n, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(inv_depth, inv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(p_robot, pb.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  if (depth) LVF_HIP(hipMemcpyAsync(source, src.p, (size_t)n, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  wait.dismiss();
  return LVF_OK;
}

}  // namespace

const uint8_t* lvf::image_level0(const lvf_image* img, int* width, int* height, lvf_ctx** ctx) {
  *width = img->w; *height = img->h; *ctx = img->ctx;
  return img->gray.p;
}

int lvf::image_begin(const char* who, lvf_ctx* ctx, int width, int height, int max_level, lvf_image** out, uint8_t** level0) {
  LVF_REQUIRE(width >= 1 && height >= 1 && (size_t)width * height <= ((size_t)1 << 28), "%s: bad image size %d x %d", who, width, height);
  LVF_REQUIRE(max_level >= 0 && max_level < kMaxLevels, "%s: max_level must be in [0, %d]", who, kMaxLevels - 1);
  std::unique_ptr<lvf_image> im(new lvf_image());
  im->ctx = ctx; im->w = width; im->h = height; im->levels = max_level + 1;
  size_t total = 0;
  for (int L = 0, w = width, h = height; L <= max_level; ++L, w = (w + 1) / 2, h = (h + 1) / 2) {
    im->lw[L] = w; im->lh[L] = h; im->off[L] = total;
    total += ((size_t)w * h + 15) & ~(size_t)15;
  }
  LVF_TRY(im->gray.alloc(total));
  LVF_TRY(im->deriv.alloc(total));
  for (int L = 0; L <= max_level; ++L) im->host_table[L] = KltLevel{im->gray.p + im->off[L], im->deriv.p + im->off[L], im->lw[L], im->lh[L]};
  LVF_TRY(im->table.alloc(kMaxLevels));
  LVF_HIP(hipMemcpyAsync(im->table.p, im->host_table, sizeof(im->host_table), hipMemcpyHostToDevice, ctx->stream));
  *level0 = im->gray.p;
  *out = im.release();
  return LVF_OK;
}

int lvf::image_chain(lvf_image* im) {
  hipStream_t s = im->ctx->stream;
  for (int L = 0; L < im->levels; ++L) {
    const size_t npx = (size_t)im->lw[L] * im->lh[L];
    if (L > 0)
      hipLaunchKernelGGL(k_klt_pyr_down, dim3(grid_of(npx)), dim3(kT), 0, s, im->gray.p + im->off[L - 1], im->lw[L - 1], im->lh[L - 1], im->gray.p + im->off[L],
                         im->lw[L], im->lh[L]);
    hipLaunchKernelGGL(k_klt_scharr, dim3(grid_of(npx)), dim3(kT), 0, s, im->gray.p + im->off[L], im->lw[L], im->lh[L], im->deriv.p + im->off[L]);
  }
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

extern "C" {

int lvf_image_create(lvf_ctx* ctx, const uint8_t* data, int width, int height, size_t stride, int max_level, lvf_image** out) {
  LVF_REQUIRE(ctx && data && out, "lvf_image_create: null argument");
  LVF_REQUIRE(width >= 1 && height >= 1 && (size_t)width * height <= ((size_t)1 << 28), "lvf_image_create: bad image size %d x %d", width, height);
  LVF_REQUIRE(stride >= (size_t)width, "lvf_image_create: row stride %zu is smaller than the width %d", stride, width);
  LVF_REQUIRE(max_level >= 0 && max_level < kMaxLevels, "lvf_image_create: max_level must be in [0, %d]", kMaxLevels - 1);
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  lvf_image* raw_im = nullptr;
  uint8_t* level0 = nullptr;
  LVF_TRY(lvf::image_begin("lvf_image_create", ctx, width, height, max_level, &raw_im, &level0));
  std::unique_ptr<lvf_image> im(raw_im);
  lvf::StreamWaitGuard wait(s);            // (an error below: the queued copies end before the image goes)
  LVF_HIP(hipMemcpy2DAsync(level0, (size_t)width, data, stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice, s));
  LVF_TRY(lvf::image_chain(im.get()));
  LVF_HIP(hipStreamSynchronize(s));      // the caller's pixel buffer may go on return
  wait.dismiss();
  *out = im.release();
  return LVF_OK;
}

int lvf_image_destroy(lvf_image* img) { delete img; return LVF_OK; }

int lvf_image_size(const lvf_image* img, int* width, int* height, int* levels) {
  LVF_REQUIRE(img, "lvf_image_size: null image");
  if (width) *width = img->w;
  if (height) *height = img->h;
  if (levels) *levels = img->levels;
  return LVF_OK;
}

int lvf_image_download_level(const lvf_image* img, int level, int* width, int* height, uint8_t* gray, int16_t* deriv) {
  LVF_REQUIRE(img, "lvf_image_download_level: null image");
  LVF_REQUIRE(level >= 0 && level < img->levels, "lvf_image_download_level: level %d of %d", level, img->levels);
  LVF_TRY(lvf::enter(img->ctx));
  const size_t npx = (size_t)img->lw[level] * img->lh[level];
  hipStream_t s = img->ctx->stream;
  if (width) *width = img->lw[level];
  if (height) *height = img->lh[level];
  if (gray) LVF_HIP(hipMemcpyAsync(gray, img->gray.p + img->off[level], npx, hipMemcpyDeviceToHost, s));
  if (deriv) LVF_HIP(hipMemcpyAsync(deriv, img->deriv.p + img->off[level], npx * sizeof(short2), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

void lvf_flow_options_default(lvf_flow_options* o) {
  if (!o) return;
  o->win = 21; o->max_level = 3;                 // utility.cpp:64
  o->back_win = 3; o->back_max_level = 1;        // utility.cpp:71
  o->max_iter = 30; o->eps = 0.01;               // utility.cpp:65
  o->min_eig = 1e-4;                             // calcOpticalFlowPyrLK's default minEigThreshold
  o->fb_max = 0.5;                               // utility.cpp:79
}

int lvf_optical_flow(const lvf_image* prev_img, const lvf_image* next_img, int n, const float* prev_pts, float* next_pts, uint8_t* status, float* fb,
                     const lvf_flow_options* opt) {
  lvf_flow_options o;
  if (opt) o = *opt; else lvf_flow_options_default(&o);
  LVF_TRY(check_flow("lvf_optical_flow", prev_img, next_img, n, &o));
  if (n == 0) return LVF_OK;                     // utility.cpp:59-60
  LVF_REQUIRE(prev_pts && next_pts && status, "lvf_optical_flow: null point arrays");
  lvf_ctx* ctx = prev_img->ctx;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<float2> p, q; DevBuf<uint8_t> st; DevBuf<float> d;
  LVF_TRY(p.upload(reinterpret_cast<const float2*>(prev_pts), n, s));
  LVF_TRY(q.upload(reinterpret_cast<const float2*>(next_pts), n, s));
  LVF_TRY(st.alloc(n)); LVF_TRY(d.alloc(n));
  launch_flow(s, prev_img, next_img, n, p.p, q.p, st.p, d.p, &o);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(next_pts, q.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(status, st.p, (size_t)n, hipMemcpyDeviceToHost, s));
  if (fb) LVF_HIP(hipMemcpyAsync(fb, d.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_stereo_triangulate(const lvf_image* left, const lvf_image* right, const lvf_camera* cam0, const lvf_camera* cam1, double baseline, int n,
                           const float* kps_left, float* kps_right, uint8_t* status, double* inv_depth, double* p_robot, const lvf_flow_options* opt) {
  return stereo_chain("lvf_stereo_triangulate", left, right, cam0, cam1, baseline, n, kps_left, kps_right, status, inv_depth, p_robot, opt, nullptr, nullptr);
}

int lvf_stereo_triangulate_lidar(const lvf_image* left, const lvf_image* right, const lvf_camera* cam0, const lvf_camera* cam1, double baseline, int n,
                                 const float* kps_left, float* kps_right, uint8_t* status, double* inv_depth, double* p_robot, const lvf_flow_options* opt,
                                 const lvf_lidar_depth* depth, uint8_t* source) {
  LVF_REQUIRE(depth, "lvf_stereo_triangulate_lidar: null lvf_lidar_depth");
  return stereo_chain("lvf_stereo_triangulate_lidar", left, right, cam0, cam1, baseline, n, kps_left, kps_right, status, inv_depth, p_robot, opt, depth, source);
}

int lvf_track_last_frame(const lvf_image* last, const lvf_image* current, const lvf_camera* cam0, double baseline, const double* current_pose, int n,
                         const double* pw, const float* kps_last, int remove_moving_points, int num_features_tracking_bad, float* kps_current,
                         float* predictions, uint8_t* cls, int* num_good, const lvf_flow_options* opt) {
  lvf_flow_options o;
  if (opt) o = *opt; else lvf_flow_options_default(&o);
  LVF_TRY(check_flow("lvf_track_last_frame", last, current, n, &o));
  LVF_TRY(lvf::check_camera("lvf_track_last_frame", cam0));
  LVF_REQUIRE(baseline > 0.0 && current_pose && num_good, "lvf_track_last_frame: bad argument");
  LVF_TRY(lvf::check_pose("lvf_track_last_frame", "the current pose", current_pose, nullptr));
  if (n == 0) { *num_good = 0; return LVF_OK; }
  LVF_REQUIRE(pw && kps_last && kps_current && cls, "lvf_track_last_frame: null point arrays");
  lvf_ctx* ctx = last->ctx;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  const Pinhole c0 = lvf::make_pinhole(*cam0);
  const Rigid T = lvf::make_rigid(current_pose);      // body -> world
  DevBuf<float2> p, pred, q; DevBuf<uint8_t> st, cl; DevBuf<double> w, z; DevBuf<int> good;
  LVF_TRY(p.upload(reinterpret_cast<const float2*>(kps_last), n, s));
  LVF_TRY(w.upload(pw, (size_t)3 * n, s));
  LVF_TRY(pred.alloc(n)); LVF_TRY(q.alloc(n)); LVF_TRY(st.alloc(n)); LVF_TRY(cl.alloc(n)); LVF_TRY(z.alloc(n)); LVF_TRY(good.alloc(1));
  hipLaunchKernelGGL(k_klt_track_predict, dim3(grid_of(n)), dim3(kT), 0, s, n, w.p, pred.p, q.p, z.p, c0, T);
  launch_flow(s, last, current, n, p.p, q.p, st.p, (float*)nullptr, &o);
  hipLaunchKernelGGL(k_klt_track_classify, dim3(1), dim3(kT), 0, s, n, pred.p, q.p, st.p, z.p, baseline * 50, remove_moving_points, num_features_tracking_bad, cl.p,
                     good.p);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(kps_current, q.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s));
  if (predictions) LVF_HIP(hipMemcpyAsync(predictions, pred.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(cls, cl.p, (size_t)n, hipMemcpyDeviceToHost, s));
  int g = 0;
  LVF_TRY(lvf::read_back(ctx, &g, good.p, sizeof(int)));      // (waits for the stream: the copies above have landed)
  *num_good = g;
  return LVF_OK;
}

}  // extern "C"
