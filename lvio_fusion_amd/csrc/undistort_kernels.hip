// undistort_kernels.hip — image undistortion on the device: the cv::undistort of Estimator::InputImage (estimator.cpp:178-179) with the K, D of
// Camera (camera.h:22-26, 81-89).  The semantics are the declared ones of tests/undistort_ref.py: cv::undistort's structure (a
// fixed-point map with R = I and the new camera matrix = K, then a bilinear remap with a constant zero border), the map evaluated directly per
// pixel in fp64 and the weights exact integers; the device is bit equal to the restatement, nothing is pinned against OpenCV.
//
// The map is built ONCE per camera and size, on the host (fp64, no contraction: a device FMA must not be able to move a source pixel), and
// kept on the device as two arrays, 6 bytes per pixel: short2 (sx, sy) = the top-left tap, uint16 = b * 32 + a.  Both are indexed by the
// LINEAR output pixel, as level 0 of an lvf_image is (rows tightly packed at `width` bytes): a thread owns 4 consecutive linear pixels, so its
// map reads are one 16-byte and one 8-byte load and its store is one naturally aligned dword whatever width % 4 is (a group of 4 may straddle
// a row end: nothing in the remap depends on the output coordinate, only on the map entry).  The last (width * height) % 4 pixels of the image
// are the scalar tail.  The taps are gathered through the cache hierarchy: the staged raw image is at most 0.47 MB at 1241 x 376 and stays in
// L2, neighbouring outputs share three of their four taps, so a wave's 256 outputs touch a few rows of a few hundred bytes each.
#include "lvf_internal.hpp"

#include <climits>
#include <cmath>

namespace {
using lvf::DevBuf;

constexpr int kT = 256;
constexpr int kMaxSide = 4096;       // the limit lvf_orb_detect states

}  // namespace

struct lvf_undistort {
  lvf_ctx* ctx = nullptr;
  int w = 0, h = 0;
  DevBuf<short2> xy;                 // (sx, sy) per output pixel, saturated to int16
  DevBuf<uint16_t> frac;             // b * 32 + a
  DevBuf<uint8_t> raw;               // staging of the raw pixels, rows tightly packed
};

namespace {

// One output pixel: out = (p00 (32 - a)(32 - b) + p01 a (32 - b) + p10 (32 - a) b + p11 a b + 512) >> 10, the weights sum to 1024.
template <bool kChecked>
__device__ __forceinline__ unsigned remap_one(const uint8_t* __restrict__ raw, int w, int h, short2 m, unsigned f) {
  const int sx = m.x, sy = m.y;
  const int a = (int)(f & 31u), b = (int)((f >> 5) & 31u);
  int p00, p01, p10, p11;
  if (!kChecked) {
    const uint8_t* p = raw + sy * w + sx;
    p00 = p[0]; p01 = p[1]; p10 = p[w]; p11 = p[w + 1];
  } else {                                                   // constant zero border, per tap
    const bool x0 = (unsigned)sx < (unsigned)w, x1 = (unsigned)(sx + 1) < (unsigned)w;
    const bool y0 = (unsigned)sy < (unsigned)h, y1 = (unsigned)(sy + 1) < (unsigned)h;
    p00 = (x0 && y0) ? (int)raw[sy * w + sx] : 0;
    p01 = (x1 && y0) ? (int)raw[sy * w + sx + 1] : 0;
    p10 = (x0 && y1) ? (int)raw[(sy + 1) * w + sx] : 0;
    p11 = (x1 && y1) ? (int)raw[(sy + 1) * w + sx + 1] : 0;
  }
  const int wa = 32 - a, wb = 32 - b;
  return (unsigned)((p00 * (wa * wb) + p01 * (a * wb) + p10 * (wa * b) + p11 * (a * b) + 512) >> 10);
}

// remap(INTER_LINEAR, BORDER_CONSTANT 0) of the staged raw image through the map into level 0 of an lvf_image: n = w * h linear pixels, 4 per
// thread.  One wave-uniform test takes the path without bounds checks when all four taps of all the wave's pixels lie inside the image.
__global__ void __launch_bounds__(kT) k_undistort_remap(const uint8_t* __restrict__ raw, int w, int h, const short2* __restrict__ xy,
                                                         const uint16_t* __restrict__ frac, int n, uint8_t* __restrict__ dst) {
  const int i0 = 4 * (int)(blockIdx.x * kT + threadIdx.x);
  const int cnt = n - i0 >= 4 ? 4 : (n - i0 > 0 ? n - i0 : 0);
  short2 m[4];
  unsigned f[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { m[k] = make_short2(-1, -1); f[k] = 0; }          // (a pixel this thread does not own: all taps outside)
  if (cnt == 4) {
    const int4 q = *reinterpret_cast<const int4*>(xy + i0);                       // 16-byte aligned: i0 % 4 == 0
    const uint2 g = *reinterpret_cast<const uint2*>(frac + i0);
    const int qs[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = make_short2((short)(qs[k] & 0xffff), (short)(qs[k] >> 16));
    f[0] = g.x & 0xffffu; f[1] = g.x >> 16; f[2] = g.y & 0xffffu; f[3] = g.y >> 16;
  } else {                                                                        // the image's last (w * h) % 4 pixels
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < cnt) { m[k] = xy[i0 + k]; f[k] = frac[i0 + k]; }
  }
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < cnt) inside = inside && (unsigned)m[k].x < (unsigned)(w - 1) && (unsigned)m[k].y < (unsigned)(h - 1);
  unsigned r[4];
  if (__all(inside)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = k < cnt ? remap_one<false>(raw, w, h, m[k], f[k]) : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = remap_one<true>(raw, w, h, m[k], f[k]);
  }
  if (cnt == 4) {
    *reinterpret_cast<unsigned*>(dst + i0) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < cnt) dst[i0 + k] = (uint8_t)r[k];
  }
}

// rint(32 v), half to even, saturated to int32 (NaN: INT32_MIN, as the x86 conversion has it)
inline int fix5(double v) {
  const double r = std::nearbyint(32.0 * v);
  if (!(r == r)) return INT_MIN;
  if (r >= 2147483647.0) return INT_MAX;
  if (r <= -2147483648.0) return INT_MIN;
  return (int)r;
}
inline short sat16(int v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// initUndistortRectifyMap with R = I, new camera matrix = K, D = (k1, k2, p1, p2, 0), evaluated directly per pixel (tests/undistort_ref.py
// build_map): every operation separately rounded in fp64
void build_map(const lvf_camera& c, const lvf_distortion& d, int w, int h, short2* xy, uint16_t* frac) {
#pragma clang fp contract(off)
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy, k1 = d.k1, k2 = d.k2, p1 = d.p1, p2 = d.p2;
  for (int i = 0; i < h; ++i) {
    const double y = ((double)i - cy) / fy;
    for (int j = 0; j < w; ++j) {
      const double x = ((double)j - cx) / fx;
      const double r2 = x * x + y * y;
      const double kr = 1.0 + (k2 * r2 + k1) * r2;
      const double xy2 = 2.0 * x * y;
      const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * x * x);
      const double yd = y * kr + p1 * (r2 + 2.0 * y * y) + p2 * xy2;
      const double u = fx * xd + cx, v = fy * yd + cy;
      const int iu = fix5(u), iv = fix5(v);
      const size_t o = (size_t)i * w + j;
      xy[o] = make_short2(sat16(iu >> 5), sat16(iv >> 5));
      frac[o] = (uint16_t)(((iv & 31) << 5) | (iu & 31));
    }
  }
}

int check_frame(const char* who, const lvf_undistort* u, const uint8_t* raw, int width, int height, size_t stride) {
  LVF_REQUIRE(u && raw, "%s: null argument", who);
  LVF_REQUIRE(width == u->w && height == u->h, "%s: the image is %d x %d, the map was built for %d x %d", who, width, height, u->w, u->h);
  LVF_REQUIRE(stride >= (size_t)width, "%s: row stride %zu is smaller than the width %d", who, stride, width);
  return LVF_OK;
}

// upload of the raw pixels into the map's staging buffer (queued, not waited for)
int queue_upload(lvf_undistort* u, const uint8_t* raw, size_t stride) {
  LVF_HIP(hipMemcpy2DAsync(u->raw.p, (size_t)u->w, raw, stride, (size_t)u->w, (size_t)u->h, hipMemcpyHostToDevice, u->ctx->stream));
  return LVF_OK;
}

// the remap into level 0 of a new image and the image's pyramid / derivative chain (queued, not waited for)
int queue_image(lvf_undistort* u, const char* who, int max_level, lvf_image** out) {
  uint8_t* level0 = nullptr;
  LVF_TRY(lvf::image_begin(who, u->ctx, u->w, u->h, max_level, out, &level0));
  const int n = u->w * u->h;
  hipLaunchKernelGGL(k_undistort_remap, dim3((n + 4 * kT - 1) / (4 * kT)), dim3(kT), 0, u->ctx->stream, u->raw.p, u->w, u->h, u->xy.p, u->frac.p, n, level0);
  return lvf::image_chain(*out);
}

}  // namespace

extern "C" {

int lvf_undistort_create(lvf_ctx* ctx, const lvf_camera* cam, const lvf_distortion* d, int width, int height, lvf_undistort** out) {
  LVF_REQUIRE(ctx && cam && out, "lvf_undistort_create: null argument");
  LVF_REQUIRE(width >= 1 && height >= 1 && width <= kMaxSide && height <= kMaxSide, "lvf_undistort_create: bad image size %d x %d (sides 1 .. %d)", width, height,
              kMaxSide);
  LVF_REQUIRE(std::isfinite(cam->fx) && std::isfinite(cam->fy) && cam->fx > 0.0 && cam->fy > 0.0, "lvf_undistort_create: fx and fy must be finite and > 0");
  LVF_REQUIRE(std::isfinite(cam->cx) && std::isfinite(cam->cy), "lvf_undistort_create: non-finite principal point");
  lvf_distortion dd = {0.0, 0.0, 0.0, 0.0};
  if (d) dd = *d;
  LVF_REQUIRE(std::isfinite(dd.k1) && std::isfinite(dd.k2) && std::isfinite(dd.p1) && std::isfinite(dd.p2), "lvf_undistort_create: non-finite distortion coefficient");
  LVF_TRY(lvf::enter(ctx));
  std::unique_ptr<lvf_undistort> u(new lvf_undistort());
  u->ctx = ctx; u->w = width; u->h = height;
  const size_t n = (size_t)width * height;
  std::vector<short2> xy(n);
  std::vector<uint16_t> frac(n);
  build_map(*cam, dd, width, height, xy.data(), frac.data());
  LVF_TRY(u->raw.alloc(n));
  lvf::StreamWaitGuard wait(ctx->stream);      // (the host vectors feed the copies)
  LVF_TRY(u->xy.upload(xy.data(), n, ctx->stream));
  LVF_TRY(u->frac.upload(frac.data(), n, ctx->stream));
  LVF_HIP(hipStreamSynchronize(ctx->stream));
  wait.dismiss();
  *out = u.release();
  return LVF_OK;
}

int lvf_undistort_destroy(lvf_undistort* u) { delete u; return LVF_OK; }

int lvf_undistort_download_map(const lvf_undistort* u, int16_t* xy, uint16_t* frac) {
  LVF_REQUIRE(u, "lvf_undistort_download_map: null object");
  LVF_TRY(lvf::enter(u->ctx));
  hipStream_t s = u->ctx->stream;
  const size_t n = (size_t)u->w * u->h;
  if (xy) LVF_HIP(hipMemcpyAsync(xy, u->xy.p, n * sizeof(short2), hipMemcpyDeviceToHost, s));
  if (frac) LVF_HIP(hipMemcpyAsync(frac, u->frac.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_image_create_undistorted(lvf_undistort* u, const uint8_t* raw, int width, int height, size_t stride, int max_level, lvf_image** out) {
  LVF_REQUIRE(out, "lvf_image_create_undistorted: null argument");
  LVF_TRY(check_frame("lvf_image_create_undistorted", u, raw, width, height, stride));
  LVF_TRY(lvf::enter(u->ctx));
  hipStream_t s = u->ctx->stream;
  lvf_image* im = nullptr;
  int rc = queue_upload(u, raw, stride);
  if (rc == LVF_OK) rc = queue_image(u, "lvf_image_create_undistorted", max_level, &im);
  if (rc == LVF_OK) {
    hipError_t e = hipStreamSynchronize(s);      // the caller's pixel buffer may go on return
    if (e != hipSuccess) rc = lvf::hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
  } else {
    (void)hipStreamSynchronize(s);
  }
  if (rc != LVF_OK) { lvf_image_destroy(im); return rc; }
  *out = im;
  return LVF_OK;
}

int lvf_image_pair_create_undistorted(lvf_undistort* u0, lvf_undistort* u1, const uint8_t* raw0, const uint8_t* raw1, int width, int height, size_t stride0,
                                      size_t stride1, int max_level, lvf_image** out0, lvf_image** out1) {
  LVF_REQUIRE(out0 && out1, "lvf_image_pair_create_undistorted: null argument");
  LVF_TRY(check_frame("lvf_image_pair_create_undistorted", u0, raw0, width, height, stride0));
  LVF_TRY(check_frame("lvf_image_pair_create_undistorted", u1, raw1, width, height, stride1));
  LVF_REQUIRE(u0->ctx == u1->ctx, "lvf_image_pair_create_undistorted: the maps belong to different contexts");
  LVF_TRY(lvf::enter(u0->ctx));
  hipStream_t s = u0->ctx->stream;
  lvf_image *im0 = nullptr, *im1 = nullptr;
  // both uploads go first, so that the host never waits behind a launch chain; with u0 == u1 the two frames share one staging buffer and the
  // second upload is queued behind the first remap instead (one stream: it lands after the remap has read the first)
  int rc = queue_upload(u0, raw0, stride0);
  if (rc == LVF_OK && u1 != u0) rc = queue_upload(u1, raw1, stride1);
  if (rc == LVF_OK) rc = queue_image(u0, "lvf_image_pair_create_undistorted", max_level, &im0);
  if (rc == LVF_OK && u1 == u0) rc = queue_upload(u1, raw1, stride1);
  if (rc == LVF_OK) rc = queue_image(u1, "lvf_image_pair_create_undistorted", max_level, &im1);
  if (rc == LVF_OK) {
    hipError_t e = hipStreamSynchronize(s);      // the ONE wait: both pixel buffers may go on return
    if (e != hipSuccess) rc = lvf::hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
  } else {
    (void)hipStreamSynchronize(s);
  }
  if (rc != LVF_OK) { lvf_image_destroy(im0); lvf_image_destroy(im1); return rc; }
  *out0 = im0; *out1 = im1;
  return LVF_OK;
}

}  // extern "C"
