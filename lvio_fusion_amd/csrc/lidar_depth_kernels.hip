// lidar_depth_kernels.hip — LiDAR depth for visual features: the deskewed sensor-frame sweep is projected into camera 0 and binned
// on a pixel grid; a feature then takes its depth from a triangle of projected points around it.  The reference gives a landmark its depth from
// the stereo pair alone (LocalMap::Triangulate, local_map.cpp:233-269) although it marks everything deeper than 50 baselines as Far
// (camera.h:38-41); this is the join LIMO / LVI-SAM / DEMO make.  The semantics are the DECLARED ones of tests/lidar_depth_ref.py: every float
// step is one operation in a stated order (contraction is off for the whole unit), and every output is bit-equal to the restatement.
//
// A RECORD is 16 bytes {float u, v, z; int source_index}: pixel and depth rounded to float32 once.  Records are binned cell-row-major on a grid
// of cell x cell pixels with a start table of cells + 1 ints; the order inside a cell is whatever the atomic cursor gave (the selection is a
// total order on (d^2, source_index), so nothing downstream depends on it).
//   k_ld_project    a grid over the cloud, 1 024 points per workgroup: fp64 transform and pinhole projection of the float32 point, the keep
//                   test, the record into a scratch array in cloud order (source_index -1 = dropped) and the cell's count.  Sweeps arrive in
//                   scan order, so consecutive lanes share cells: one integer atomic per RUN of equal cells in a wave (lvf::cell_runs), straight
//                   into the global table — a per-workgroup LDS histogram would need 117 KB at cell = 4 on a 1241 x 376 image.
//                   16 bytes read and 16 written per point.
//   k_ld_scan       one workgroup: exclusive scan of the counts into the start table and the fill cursors, 4 096 cells per pass with one
//                   16-byte load per thread.  4 bytes read and 8 written per cell.
//   k_ld_fill       the same grid: a run's head lane takes the run's slots from the cell's cursor, every lane stores its record.
//                   16 bytes read per point, 16 written per kept point.
//   k_ld_query      one wavefront per feature, four per workgroup.  The cells of one cell row inside the window are ONE contiguous run of
//                   records: lanes stride it with one 16-byte load per candidate and keep the (d^2, source_index) minimum of each of the four
//                   quadrants; a __shfl_xor butterfly reduces the four, then every lane holds the same winners and forms the same fit:
//                   barycentric interpolation of 1 / z in pixel space, the gates, and stereo_triangulate's outputs for the accepted depth.
//                   8 bytes read per feature plus 16 per candidate, 49 written.
//   k_ld_merge      one thread per feature: LiDAR replaces the stereo result where the rule of lvf_stereo_triangulate_lidar says so.
//                   At most 66 bytes read and 42 written per feature.
// lvf_lidar_depth_create queues memset -> project -> scan -> fill and waits for nothing (the record array is sized by the cloud).
#pragma clang fp contract(off)      // ahead of the includes: camera_dev.hpp's chains are compiled contraction-free here, as the restatement states them

#include "lvf_internal.hpp"

#include <cmath>

namespace lvf {

constexpr int kLdThreads = 256, kLdPointsPerThread = 4, kLdScanThreads = 1024, kLdQueryBlock = 256;
constexpr int kLdMaxCells = 1 << 22;

struct LdRecord { float u, v, z; int src; };
static_assert(sizeof(LdRecord) == 16 && sizeof(LdRecord) == sizeof(lvf_lidar_depth_record), "a record is one 16-byte load");

struct LdGrid { int width, height, shift, ncx, ncy, cells; };
struct LdProjP { double M[12], fx, fy, cx, cy, min_depth, max_depth; LdGrid g; };
struct LdQueryP { LdGrid g; Pinhole c0, c1; double cell, radius, r2, min_depth, max_depth, max_spread, min_det, max_extrapolation; };

__device__ __forceinline__ int ld_cell_of(const LdRecord& r, const LdGrid& g) { return ((int)r.v >> g.shift) * g.ncx + ((int)r.u >> g.shift); }

__global__ __launch_bounds__(kLdThreads) void k_ld_project(int n, const float4* __restrict__ pts, LdRecord* __restrict__ tmp, int* __restrict__ count, const LdProjP P) {
  const long long base = (long long)blockIdx.x * (kLdThreads * kLdPointsPerThread);
#pragma unroll
  for (int k = 0; k < kLdPointsPerThread; ++k) {
    // (no early exit: cell_runs needs the whole wave)
    const long long i = base + (long long)k * kLdThreads + threadIdx.x;
    int c = -1;
    if (i < n) {
      const float4 p = pts[i];
      const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
      const double px = ((P.M[0] * x + P.M[1] * y) + P.M[2] * z) + P.M[3];
      const double py = ((P.M[4] * x + P.M[5] * y) + P.M[6] * z) + P.M[7];
      const double pz = ((P.M[8] * x + P.M[9] * y) + P.M[10] * z) + P.M[11];
      LdRecord r;
      r.u = (float)(P.fx * px / pz + P.cx);
      r.v = (float)(P.fy * py / pz + P.cy);
      r.z = (float)pz;
      const bool keep = isfinite(px) && isfinite(py) && isfinite(pz) && pz >= P.min_depth && pz < P.max_depth && r.u >= 0.0f && (double)r.u < (double)P.g.width &&
                        r.v >= 0.0f && (double)r.v < (double)P.g.height;
      r.src = keep ? (int)i : -1;
      tmp[i] = r;
      if (keep) c = ld_cell_of(r, P.g);
    }
    int start, len;
    if (cell_runs(c, start, len) && c >= 0) atomicAdd(&count[c], len);
  }
}

// start[i] = cursor[i] = sum of count[0 .. i), i = 0 .. cells (count lives in `cursor`; count[cells] is zero, so start[cells] is the total).
// Both arrays are padded to m4 ints, a multiple of 4 (the padding counts are zero): tiles of 4 096 counts, one 16-byte load per thread, a DPP
// scan inside the wave, the 16 wave totals through LDS (double-buffered by the tile's parity: one barrier per tile), the carry in a register.
__global__ __launch_bounds__(kLdScanThreads) void k_ld_scan(int m4, int4* __restrict__ cursor, int4* __restrict__ start) {
  __shared__ int s_wave[2][kLdScanThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0, it = 0; base < m4; base += 4 * kLdScanThreads, ++it) {      // (the trip count is the same for every thread)
    const int i = base / 4 + t;
    const bool live = 4 * i < m4;
    int4 c = make_int4(0, 0, 0, 0);
    if (live) c = cursor[i];
    const int sum = (c.x + c.y) + (c.z + c.w);
    const int incl = wave_incl_scan(sum);
    if (lane == 63) s_wave[it & 1][wave] = incl;
    __syncthreads();
    int before = carry + (incl - sum), total = 0;
#pragma unroll
    for (int w = 0; w < kLdScanThreads / 64; ++w) {
      const int v = s_wave[it & 1][w];
      before += w < wave ? v : 0;
      total += v;
    }
    if (live) {
      int4 o;
      o.x = before; o.y = o.x + c.x; o.z = o.y + c.y; o.w = o.z + c.z;
      start[i] = o; cursor[i] = o;
    }
    carry += total;
  }
}

__global__ __launch_bounds__(kLdThreads) void k_ld_fill(int n, const LdRecord* __restrict__ tmp, int* __restrict__ cursor, LdRecord* __restrict__ rec, const LdGrid g) {
  const long long base = (long long)blockIdx.x * (kLdThreads * kLdPointsPerThread);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kLdPointsPerThread; ++k) {
    const long long i = base + (long long)k * kLdThreads + threadIdx.x;
    int c = -1;
    LdRecord r{0.f, 0.f, 0.f, -1};
    if (i < n) {
      r = tmp[i];
      if (r.src >= 0) c = ld_cell_of(r, g);
    }
    int start, len, slot = 0;
    if (cell_runs(c, start, len) && c >= 0) slot = atomicAdd(&cursor[c], len);
    slot = __shfl(slot, start);
    if (c >= 0) rec[slot + (lane - start)] = r;
  }
}

// a quadrant's winner so far: the bit pattern of d^2 (>= +0, so it orders as the value does; all ones = none), the source index, the record's slot
struct LdBest { unsigned long long key; int src, slot; };

__device__ __forceinline__ bool ld_less(unsigned long long a, int ai, unsigned long long b, int bi) { return a < b || (a == b && ai < bi); }

__device__ __forceinline__ void ld_wave_min(LdBest& b) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(b.key >> 32), m), lo = __shfl_xor((unsigned)b.key, m);
    const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
    const int os = __shfl_xor(b.src, m), ot = __shfl_xor(b.slot, m);
    if (ld_less(ok, os, b.key, b.src)) { b.key = ok; b.src = os; b.slot = ot; }
  }
}

__device__ __forceinline__ void ld_swap(LdBest& a, LdBest& b) { const LdBest t = a; a = b; b = t; }

__global__ __launch_bounds__(kLdQueryBlock) void k_ld_query(int n, const float2* __restrict__ kps, const LdRecord* __restrict__ rec, const int* __restrict__ start,
                                                             uint8_t* __restrict__ status, double* __restrict__ depth, double* __restrict__ inv_depth,
                                                             double* __restrict__ p_robot, float2* __restrict__ right, const LdQueryP P) {
  const int f = blockIdx.x * (kLdQueryBlock / 64) + (threadIdx.x >> 6);
  if (f >= n) return;                                                  // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const float2 kp = kps[f];
  const double u0 = (double)kp.x, v0 = (double)kp.y;
  const unsigned long long kNone = ~0ull;
  LdBest best[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) best[q] = LdBest{kNone, 0x7fffffff, -1};
  if (isfinite(u0) && isfinite(v0)) {
    // the window's cells, clipped to the grid in double (a pixel far outside must not overflow the conversion)
    const double xl = fmax(floor((u0 - P.radius) / P.cell), 0.0), xh = fmin(floor((u0 + P.radius) / P.cell), (double)(P.g.ncx - 1));
    const double yl = fmax(floor((v0 - P.radius) / P.cell), 0.0), yh = fmin(floor((v0 + P.radius) / P.cell), (double)(P.g.ncy - 1));
    if (xl <= xh && yl <= yh) {
      const int cx0 = (int)xl, cx1 = (int)xh, cy0 = (int)yl, cy1 = (int)yh;
      for (int cy = cy0; cy <= cy1; ++cy) {
        const int b = start[cy * P.g.ncx + cx0], e = start[cy * P.g.ncx + cx1 + 1];
        for (int j = b + lane; j < e; j += 64) {
          const LdRecord r = rec[j];
          const double dx = (double)r.u - u0, dy = (double)r.v - v0;
          const double d2 = dx * dx + dy * dy;
          if (!(d2 <= P.r2)) continue;
          const int q = (dx >= 0.0 ? 1 : 0) + (dy >= 0.0 ? 2 : 0);
          const unsigned long long key = (unsigned long long)__double_as_longlong(d2);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k == q && ld_less(key, r.src, best[k].key, best[k].src)) best[k] = LdBest{key, r.src, j};
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) ld_wave_min(best[q]);
  // every lane holds the same four winners from here on
  int occupied = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) occupied += best[q].key != kNone ? 1 : 0;
  uint8_t st = 0;
  double out_depth = 0.0, out_inv = 0.0, pb[3] = {0.0, 0.0, 0.0};
  float2 out_right = make_float2(0.f, 0.f);
  if (occupied >= 3) {
    // ascending (d^2, source_index); an empty quadrant (all-ones key) sorts last, and of four winners the farthest is dropped: A, B, C = the first three
    if (ld_less(best[1].key, best[1].src, best[0].key, best[0].src)) ld_swap(best[0], best[1]);
    if (ld_less(best[3].key, best[3].src, best[2].key, best[2].src)) ld_swap(best[2], best[3]);
    if (ld_less(best[2].key, best[2].src, best[0].key, best[0].src)) ld_swap(best[0], best[2]);
    if (ld_less(best[3].key, best[3].src, best[1].key, best[1].src)) ld_swap(best[1], best[3]);
    if (ld_less(best[2].key, best[2].src, best[1].key, best[1].src)) ld_swap(best[1], best[2]);
    const LdRecord A = rec[best[0].slot], B = rec[best[1].slot], C = rec[best[2].slot];
    const double ax = (double)A.u - u0, ay = (double)A.v - v0, bx0 = (double)B.u - u0, by0 = (double)B.v - v0, cx0 = (double)C.u - u0, cy0 = (double)C.v - v0;
    const double zA = (double)A.z, zB = (double)B.z, zC = (double)C.z;
    // the feature (the origin) in the frame A + wb (B - A) + wc (C - A)
    const double bx = bx0 - ax, by = by0 - ay, cx = cx0 - ax, cy = cy0 - ay, px = 0.0 - ax, py = 0.0 - ay;
    const double det = bx * cy - cx * by;
    const double wb = (px * cy - cx * py) / det, wc = (bx * py - px * by) / det;
    const double wa = (1.0 - wb) - wc;
    const double inv_z = (wa / zA + wb / zB) + wc / zC;
    const double zmax = fmax(fmax(zA, zB), zC), zmin = fmin(fmin(zA, zB), zC);
    const double d = 1.0 / inv_z;
    if (fabs(det) < P.min_det) st = 3;
    else if (wa < -P.max_extrapolation || wb < -P.max_extrapolation || wc < -P.max_extrapolation) st = 4;
    else if (zmax - zmin > P.max_spread) st = 2;
    else if (!(inv_z > 0.0) || !(d >= P.min_depth && d < P.max_depth)) st = 5;
    else {
      st = 1;
      out_depth = d;
      double ps[3], r[3], s1[3];
      pixel2sensor(P.c0, u0, v0, d, ps);
      sensor2robot(P.c0, ps, r);
      pb[0] = r[0]; pb[1] = r[1]; pb[2] = r[2];      // (through a local: handing out the result array itself moves the register allocation)
      robot2sensor(P.c1, r, s1);
      out_inv = 1.0 / s1[2];                                                                              // local_map.cpp:258: camera ONE
      out_right = sensor2pixel(P.c1, s1);
    }
  }
  if (lane == 0) {
    status[f] = st; depth[f] = out_depth; inv_depth[f] = out_inv;
    p_robot[3 * f] = pb[0]; p_robot[3 * f + 1] = pb[1]; p_robot[3 * f + 2] = pb[2];
    right[f] = out_right;
  }
}

// the stereo result (right, status, inv_depth, p_robot) is overwritten in place where LiDAR replaces it; source: 0 none, 1 stereo, 2 LiDAR
__global__ __launch_bounds__(kLdThreads) void k_ld_merge(int n, float2* __restrict__ right, uint8_t* __restrict__ status, double* __restrict__ inv_depth,
                                                          double* __restrict__ p_robot, uint8_t* __restrict__ source, const uint8_t* __restrict__ l_status,
                                                          const double* __restrict__ l_inv, const double* __restrict__ l_pb, const float2* __restrict__ l_right,
                                                          const Pinhole c0, double far_depth, int always_far, int replace_lost) {
  const int i = blockIdx.x * kLdThreads + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = status[i];
  bool replace = false;
  if (l_status[i] == 1) {
    if (st == 1) {
      double s0[3];
      robot2sensor(c0, p_robot + 3 * i, s0);                                                              // (only the z row survives)
      replace = always_far || s0[2] > far_depth;
    } else {
      replace = replace_lost != 0;
    }
  }
  if (replace) {
    right[i] = l_right[i]; status[i] = 1; inv_depth[i] = l_inv[i];
    p_robot[3 * i] = l_pb[3 * i]; p_robot[3 * i + 1] = l_pb[3 * i + 1]; p_robot[3 * i + 2] = l_pb[3 * i + 2];
  }
  source[i] = replace ? 2 : (st == 1 ? 1 : 0);
}

}  // namespace lvf

struct lvf_lidar_depth {
  lvf_ctx* ctx = nullptr;
  lvf_lidar_depth_options opt{};
  lvf::LdGrid g{};
  double fx = 0, fy = 0, cx = 0, cy = 0;       // camera 0 as the sweep was projected
  int n = 0;                                   // points of the cloud
  int kept = -1;                               // read back on first demand
  lvf::DevBuf<lvf::LdRecord> rec;              // [n]: the first `kept` are records
  lvf::DevBuf<int> start;                      // [cells + 1]
};

namespace lvf {
namespace {

int ld_check_options(const char* who, const lvf_lidar_depth_options& o) {
  LVF_REQUIRE(o.cell == 4 || o.cell == 8 || o.cell == 16 || o.cell == 32, "%s: cell %d is not 4, 8, 16 or 32", who, o.cell);
  LVF_REQUIRE(o.radius > 0.0 && o.radius <= 64.0, "%s: radius %g outside (0, 64]", who, o.radius);
  LVF_REQUIRE(std::isfinite(o.min_depth) && std::isfinite(o.max_depth) && o.min_depth > 0.0 && o.min_depth < o.max_depth, "%s: need 0 < min_depth < max_depth (finite)", who);
  LVF_REQUIRE(std::isfinite(o.max_spread) && o.max_spread >= 0.0, "%s: max_spread must be finite and >= 0", who);
  LVF_REQUIRE(std::isfinite(o.min_det) && o.min_det > 0.0, "%s: min_det must be finite and > 0", who);
  LVF_REQUIRE(std::isfinite(o.max_extrapolation) && o.max_extrapolation >= 0.0, "%s: max_extrapolation must be finite and >= 0", who);
  LVF_REQUIRE(std::isfinite(o.far_factor) && o.far_factor >= 0.0, "%s: far_factor must be finite and >= 0", who);
  LVF_REQUIRE(o.replace_lost == 0 || o.replace_lost == 1, "%s: replace_lost must be 0 or 1", who);
  return LVF_OK;
}

// the query's launch on device arrays; nothing waits
int ld_launch_query(const lvf_lidar_depth* d, const Pinhole& c0, const Pinhole& c1, int n, const float2* kps, uint8_t* status, double* depth, double* inv_depth,
                    double* p_robot, float2* right) {
  LdQueryP P;
  P.g = d->g; P.c0 = c0; P.c1 = c1;
  P.cell = (double)d->opt.cell; P.radius = d->opt.radius; P.r2 = d->opt.radius * d->opt.radius;
  P.min_depth = d->opt.min_depth; P.max_depth = d->opt.max_depth; P.max_spread = d->opt.max_spread; P.min_det = d->opt.min_det;
  P.max_extrapolation = d->opt.max_extrapolation;
  hipLaunchKernelGGL(k_ld_query, dim3(grid_of(n, kLdQueryBlock / 64)), dim3(kLdQueryBlock), 0, d->ctx->stream, n, kps, (const LdRecord*)d->rec.p, (const int*)d->start.p,
                     status, depth, inv_depth, p_robot, right, P);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

}  // namespace

int lidar_depth_check(const char* who, const lvf_lidar_depth* d, lvf_ctx* ctx, const lvf_camera* cam0, const lvf_camera* cam1) {
  LVF_REQUIRE(d, "%s: null lvf_lidar_depth", who);
  LVF_REQUIRE(!ctx || d->ctx == ctx, "%s: the projected sweep belongs to another context", who);
  LVF_TRY(check_camera(who, cam0));
  LVF_TRY(check_camera(who, cam1));
  LVF_REQUIRE(cam0->fx == d->fx && cam0->fy == d->fy && cam0->cx == d->cx && cam0->cy == d->cy, "%s: cam0's intrinsics are not the ones the sweep was projected with", who);
  return LVF_OK;
}

int lidar_depth_merge_queue(const lvf_lidar_depth* d, const Pinhole& c0, const Pinhole& c1, double baseline, int n, const float2* left, float2* right, uint8_t* status,
                            double* inv_depth, double* p_robot, uint8_t* source) {
  DevBuf<uint8_t> l_st; DevBuf<double> l_depth, l_inv, l_pb; DevBuf<float2> l_right;
  LVF_TRY(l_st.alloc(n)); LVF_TRY(l_depth.alloc(n)); LVF_TRY(l_inv.alloc(n)); LVF_TRY(l_pb.alloc((size_t)3 * n)); LVF_TRY(l_right.alloc(n));
  LVF_TRY(ld_launch_query(d, c0, c1, n, left, l_st.p, l_depth.p, l_inv.p, l_pb.p, l_right.p));
  hipLaunchKernelGGL(k_ld_merge, dim3(grid_of(n, kLdThreads)), dim3(kLdThreads), 0, d->ctx->stream, n, right, status, inv_depth, p_robot, source,
                     (const uint8_t*)l_st.p, (const double*)l_inv.p, (const double*)l_pb.p, (const float2*)l_right.p, c0, d->opt.far_factor * baseline,
                     d->opt.far_factor == 0.0 ? 1 : 0, d->opt.replace_lost);
  LVF_HIP(hipGetLastError());
  // (the scratch goes back to the context's pool, whose reuse is ordered on the same stream)
  return LVF_OK;
}

}  // namespace lvf

using namespace lvf;

extern "C" {

void lvf_lidar_depth_options_default(lvf_lidar_depth_options* o) {
  if (!o) return;
  o->cell = 8; o->radius = 12.0; o->min_depth = 0.5; o->max_depth = 80.0; o->max_spread = 2.0; o->min_det = 4.0; o->max_extrapolation = 0.5;
  o->far_factor = 50.0; o->replace_lost = 1;
}

int lvf_lidar_depth_create(lvf_ctx* ctx, const lvf_cloud* cloud, const lvf_camera* cam0, const double* cam_from_lidar, int width, int height,
                           const lvf_lidar_depth_options* opt, lvf_lidar_depth** out) {
  LVF_REQUIRE(ctx && cloud && cam_from_lidar && out, "lvf_lidar_depth_create: null argument");
  LVF_REQUIRE(cloud->ctx == ctx, "lvf_lidar_depth_create: the cloud belongs to another context");
  LVF_TRY(check_camera("lvf_lidar_depth_create", cam0));
  for (int i = 0; i < 12; ++i) LVF_REQUIRE(std::isfinite(cam_from_lidar[i]), "lvf_lidar_depth_create: cam_from_lidar[%d] is not finite", i);
  std::unique_ptr<lvf_lidar_depth> d(new lvf_lidar_depth());
  if (opt) d->opt = *opt; else lvf_lidar_depth_options_default(&d->opt);
  LVF_TRY(ld_check_options("lvf_lidar_depth_create", d->opt));
  LVF_REQUIRE(width >= 1 && height >= 1 && width <= (1 << 16) && height <= (1 << 16), "lvf_lidar_depth_create: bad image size %d x %d", width, height);
  LdGrid& g = d->g;
  g.width = width; g.height = height;
  g.shift = d->opt.cell == 4 ? 2 : d->opt.cell == 8 ? 3 : d->opt.cell == 16 ? 4 : 5;
  g.ncx = (width + d->opt.cell - 1) >> g.shift; g.ncy = (height + d->opt.cell - 1) >> g.shift;
  LVF_REQUIRE((long long)g.ncx * g.ncy <= kLdMaxCells, "lvf_lidar_depth_create: %d x %d cells exceed %d", g.ncx, g.ncy, kLdMaxCells);
  g.cells = g.ncx * g.ncy;
  LVF_TRY(lvf::enter(ctx));
  d->ctx = ctx; d->n = cloud->n;
  d->fx = cam0->fx; d->fy = cam0->fy; d->cx = cam0->cx; d->cy = cam0->cy;
  const int n = cloud->n;
  DevBuf<LdRecord> tmp; DevBuf<int> cursor;
  const size_t m4 = ((size_t)g.cells + 1 + 3) & ~(size_t)3;      // the scan moves 16 bytes per thread
  LVF_TRY(d->rec.alloc((size_t)std::max(n, 1))); LVF_TRY(d->start.alloc(m4));
  LVF_TRY(tmp.alloc((size_t)std::max(n, 1))); LVF_TRY(cursor.alloc(m4));
  hipStream_t s = ctx->stream;
  LVF_HIP(hipMemsetAsync(cursor.p, 0, m4 * sizeof(int), s));
  const int per = kLdThreads * kLdPointsPerThread;
  if (n > 0) {
    LdProjP P;
    for (int i = 0; i < 12; ++i) P.M[i] = cam_from_lidar[i];
    P.fx = cam0->fx; P.fy = cam0->fy; P.cx = cam0->cx; P.cy = cam0->cy; P.min_depth = d->opt.min_depth; P.max_depth = d->opt.max_depth; P.g = g;
    hipLaunchKernelGGL(k_ld_project, dim3(grid_of(n, per)), dim3(kLdThreads), 0, s, n, (const float4*)cloud->pts.p, tmp.p, cursor.p, P);
  }
  hipLaunchKernelGGL(k_ld_scan, dim3(1), dim3(kLdScanThreads), 0, s, (int)m4, reinterpret_cast<int4*>(cursor.p), reinterpret_cast<int4*>(d->start.p));
  if (n > 0) hipLaunchKernelGGL(k_ld_fill, dim3(grid_of(n, per)), dim3(kLdThreads), 0, s, n, (const LdRecord*)tmp.p, cursor.p, d->rec.p, g);
  LVF_HIP(hipGetLastError());
  if (n == 0) d->kept = 0;
  *out = d.release();
  return LVF_OK;
}

// (a launch may still be in flight: the buffers go back to the context's pool, whose reuse is ordered on the same stream)
int lvf_lidar_depth_destroy(lvf_lidar_depth* depth) { delete depth; return LVF_OK; }

int lvf_lidar_depth_size(lvf_lidar_depth* depth) {
  if (!depth) return -1;
  if (depth->kept < 0) {
    if (lvf::enter(depth->ctx) != LVF_OK) return -1;
    int total = 0;
    if (read_back(depth->ctx, &total, depth->start.p + depth->g.cells, sizeof(int)) != LVF_OK) return -1;
    depth->kept = total;
  }
  return depth->kept;
}

int lvf_lidar_depth_download(lvf_lidar_depth* depth, lvf_lidar_depth_record* records, int32_t* cell_start) {
  LVF_REQUIRE(depth, "lvf_lidar_depth_download: null lvf_lidar_depth");
  const int kept = lvf_lidar_depth_size(depth);
  if (kept < 0) return LVF_ERR_HIP;
  LVF_TRY(lvf::enter(depth->ctx));
  if (records && kept > 0) LVF_TRY(copy_down_wait(depth->ctx, records, depth->rec.p, (size_t)kept * sizeof(LdRecord)));
  if (cell_start) LVF_TRY(copy_down_wait(depth->ctx, cell_start, depth->start.p, ((size_t)depth->g.cells + 1) * sizeof(int)));
  return LVF_OK;
}

int lvf_lidar_depth_query(const lvf_lidar_depth* depth, const lvf_camera* cam0, const lvf_camera* cam1, int n, const float* kps_left, uint8_t* status,
                          double* depth_out, double* inv_depth, double* p_robot, float* kps_right) {
  LVF_TRY(lidar_depth_check("lvf_lidar_depth_query", depth, nullptr, cam0, cam1));
  LVF_REQUIRE(n >= 0, "lvf_lidar_depth_query: negative point count");
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(kps_left && status && depth_out && inv_depth && p_robot && kps_right, "lvf_lidar_depth_query: null point arrays");
  lvf_ctx* ctx = depth->ctx;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  DevBuf<float2> p, q; DevBuf<uint8_t> st; DevBuf<double> dz, inv, pb;
  LVF_TRY(p.upload(reinterpret_cast<const float2*>(kps_left), n, s));
  LVF_TRY(q.alloc(n)); LVF_TRY(st.alloc(n)); LVF_TRY(dz.alloc(n)); LVF_TRY(inv.alloc(n)); LVF_TRY(pb.alloc((size_t)3 * n));
  StreamWaitGuard wait(s);                     // (an error below: the upload from the caller's array ends before the buffers go)
  LVF_TRY(ld_launch_query(depth, make_pinhole(*cam0), make_pinhole(*cam1), n, p.p, st.p, dz.p, inv.p, pb.p, q.p));
  LVF_HIP(hipMemcpyAsync(status, st.p, (size_t)n, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(depth_out, dz.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(inv_depth, inv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(p_robot, pb.p, (size_t)3 * n * 8, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(kps_right, q.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  wait.dismiss();
  return LVF_OK;
}

}  // extern "C"
