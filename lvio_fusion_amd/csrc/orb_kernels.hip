// orb_kernels.hip — the ORB part of the front-end on the device: Extractor's scale pyramid (extractor.cpp:455-477), the FAST-9/16 corner score
// of every level, ICAngle (:66-93), the blurred level and rBRIEF (:504-530 as ORB-SLAM2's computeDescriptors has it) and the numeric part of
// LocalMap::Search (local_map.cpp:313-368).  The semantics are the declared ones of tests/orb_ref.py: every integer result is bit
// equal to the restatement, nothing is pinned against OpenCV.
//
// Everything is wave-64 and stream-ordered on the context's stream.  Per-pixel kernels (resize, score) run one thread per pixel and gather
// through the cache hierarchy: a level is at most 466 KB at 1241 x 376 and stays in L2.  Per-keypoint kernels (angle, rBRIEF, search) run one
// wavefront per keypoint and reduce with a __shfl_xor butterfly in a fixed order: a keypoint's result depends on nothing but its own inputs,
// so two runs are bit-identical.  A keypoint's level coordinates rint(pt / scale) are formed ON THE HOST (one float division per coordinate,
// next to the bounds check every call makes anyway) and uploaded as integers, and the resize coefficient tables are built on the host in fp64
// with contraction off: no device rounding mode or FMA can move a pixel.
#include "lvf_internal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace {
using lvf::DevBuf; using lvf::Pinhole; using lvf::Rigid; using lvf::grid_of; using lvf::refl101;

constexpr int kOrbMaxLevels = 8;
constexpr int kT = 256;
constexpr int kHalf = 15;            // half_patch_size
constexpr int kEdge = 31;            // edge_threshold: no score closer than this to an edge
constexpr int kBorder = 19;          // a keypoint lies at least this far inside its level: |pattern| <= 13 rotates to at most rint(13 sqrt 2) = 18
constexpr int kPatternMax = 13;
constexpr int kBlurW = 64, kBlurH = 16;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kMinBorder = kEdge - 3;      // extractor.cpp:375
constexpr int kQtNodes = 1024;       // node table of the quadtree (LDS): max(num_desired + 2, 4 * initial nodes) must fit
constexpr int kMaxSide = 4096;       // 12 bits per coordinate in the packed corner records

struct OrbLevel { int w, h; unsigned off, first; };      // off: pixel offset of the level in gray / blurred / score; first: first thread of its score area
struct OrbLevels { OrbLevel l[kOrbMaxLevels]; int n; unsigned total; };
// the cell grid of ComputeKeyPointsQuadTree (:383-388) and the quadtree's initial nodes (:165-166) of one level; ncols == 0: the level has no cell
struct OrbGrid { int ncols, nrows, cw, ch, first, slots, slot_off, n_init, num; float hx; };
struct OrbGrids { OrbGrid g[kOrbMaxLevels]; int n, total_cells; };

// level L from level L - 1: cv::resize INTER_LINEAR's fixed-point arithmetic with host tables tx = {index[dw], a1[dw]}, ty = {index[dh], b1[dh]}
__global__ void __launch_bounds__(kT) k_orb_resize(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh,
                                                   const int* __restrict__ tx, const int* __restrict__ ty) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= dw * dh) return;
  const int y = i / dw, x = i - y * dw;
  const int ix = tx[x], a1 = tx[dw + x], a0 = 2048 - a1, ix1 = min(ix + 1, sw - 1);
  const int iy = ty[y], b1 = ty[dh + y], b0 = 2048 - b1, iy1 = min(iy + 1, sh - 1);
  const uint8_t* r0 = src + (size_t)iy * sw;
  const uint8_t* r1 = src + (size_t)iy1 * sw;
  const int H0 = a0 * (int)r0[ix] + a1 * (int)r0[ix1], H1 = a0 * (int)r1[ix] + a1 * (int)r1[ix1];
  dst[i] = (uint8_t)((((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2);
}

// max over the 16 arcs of 9 contiguous ring entries of the arc's minimum
__device__ __forceinline__ int arc_score(const int (&e)[16]) {
  int best = -256;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    int m = e[s];
#pragma unroll
    for (int k = 1; k < 9; ++k) m = min(m, e[(s + k) & 15]);
    best = max(best, m);
  }
  return best;
}

// FAST-9/16 score of every level in one launch, one thread per pixel of the area [31, w - 31) x [31, h - 31): the largest t at which the
// pixel is a corner, 0 below min_th.  An arc of 9 holds at least two of the four compass points of the ring: the quick reject.
__global__ void __launch_bounds__(kT) k_orb_fast_score(const uint8_t* __restrict__ gray, uint8_t* __restrict__ score, OrbLevels LV, int min_th) {
  const unsigned g = blockIdx.x * kT + threadIdx.x;
  if (g >= LV.total) return;
  int L = 0;
#pragma unroll
  for (int k = 1; k < kOrbMaxLevels; ++k)
    if (k < LV.n && g >= LV.l[k].first) L = k;
  int w = LV.l[0].w; unsigned off = LV.l[0].off, first = LV.l[0].first;
#pragma unroll
  for (int k = 1; k < kOrbMaxLevels; ++k)
    if (k == L) { w = LV.l[k].w; off = LV.l[k].off; first = LV.l[k].first; }
  const int aw = w - 2 * kEdge;
  const unsigned r = g - first;
  const int y = kEdge + (int)(r / (unsigned)aw), x = kEdge + (int)(r % (unsigned)aw);
  const size_t at = (size_t)off + (size_t)y * w + x;
  const uint8_t* p = gray + at;
  const int v = *p;
  const int n0 = (int)p[3 * w] - v, n4 = (int)p[3] - v, n8 = (int)p[-3 * w] - v, n12 = (int)p[-3] - v;
  const int hi = (n0 > min_th) + (n4 > min_th) + (n8 > min_th) + (n12 > min_th);
  const int lo = (n0 < -min_th) + (n4 < -min_th) + (n8 < -min_th) + (n12 < -min_th);
  int out = 0;
  if (hi >= 2 || lo >= 2) {
    int e[16];
    e[0] = n0; e[4] = n4; e[8] = n8; e[12] = n12;
    e[1] = (int)p[3 * w + 1] - v; e[2] = (int)p[2 * w + 2] - v; e[3] = (int)p[w + 3] - v;
    e[5] = (int)p[-w + 3] - v; e[6] = (int)p[-2 * w + 2] - v; e[7] = (int)p[-3 * w + 1] - v;
    e[9] = (int)p[-3 * w - 1] - v; e[10] = (int)p[-2 * w - 2] - v; e[11] = (int)p[-w - 3] - v;
    e[13] = (int)p[w - 3] - v; e[14] = (int)p[2 * w - 2] - v; e[15] = (int)p[3 * w - 1] - v;
    int s = arc_score(e);
#pragma unroll
    for (int k = 0; k < 16; ++k) e[k] = -e[k];
    s = max(s, arc_score(e)) - 1;
    out = s >= min_th ? s : 0;
  }
  score[at] = (uint8_t)out;
}

// ICAngle: one wavefront per keypoint; the 31 x 31 square is dealt 16 positions per lane, the disc test is umax; exact integer moments
__global__ void __launch_bounds__(kT) k_orb_angle(int n, const int* __restrict__ kp, const uint8_t* __restrict__ gray, OrbLevels LV, const int* __restrict__ umax,
                                                  float* __restrict__ angle) {
  const int f = blockIdx.x * (kT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= n) return;
  const int x = kp[3 * f], y = kp[3 * f + 1], o = kp[3 * f + 2];
  if (o < 0) return;                                             // (an empty slot of lvf_orb_detect's per-level table)
  int w = LV.l[0].w; unsigned off = LV.l[0].off;
#pragma unroll
  for (int k = 1; k < kOrbMaxLevels; ++k)
    if (k == o) { w = LV.l[k].w; off = LV.l[k].off; }
  const uint8_t* c = gray + (size_t)off + (size_t)y * w + x;
  int m10 = 0, m01 = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int idx = lane + 64 * k;
    if (idx < 31 * 31) {
      const int row = idx / 31, v = row - kHalf, u = idx - row * 31 - kHalf;
      if (abs(u) <= umax[abs(v)]) {
        const int val = c[v * w + u];
        m10 += u * val; m01 += v * val;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { m10 += __shfl_xor(m10, m); m01 += __shfl_xor(m01, m); }
  if (lane == 0) {
    float a = 0.f;
    if (m10 != 0 || m01 != 0) {
      double deg = atan2((double)m01, (double)m10) * (180.0 / M_PI);
      if (deg < 0) deg += 360.0;
      a = (float)deg;
      if (a >= 360.f) a = 0.f;
    }
    angle[f] = a;
  }
}

// 7 x 7 Gaussian, sigma 2, integer and separable: the row sums of a 64 x (16 + 6) tile go through LDS
__global__ void __launch_bounds__(kT) k_orb_blur(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h) {
  __shared__ int hs[kBlurH + 6][kBlurW];
  const int wt[7] = {72, 134, 195, 222, 195, 134, 72};
  const int t = threadIdx.x, cx = t & 63, x = blockIdx.x * kBlurW + cx, y0 = blockIdx.y * kBlurH;
  const int xc = min(x, w - 1);
  int xs[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) xs[k] = refl101(xc + k - 3, w);
  for (int r = t >> 6; r < kBlurH + 6; r += kT / 64) {
    const uint8_t* row = src + (size_t)refl101(y0 + r - 3, h) * w;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += wt[k] * (int)row[xs[k]];
    hs[r][cx] = s;
  }
  __syncthreads();
  for (int r = t >> 6; r < kBlurH; r += kT / 64) {
    const int y = y0 + r;
    if (x < w && y < h) {
      int acc = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) acc += wt[k] * hs[r + k][cx];
      dst[(size_t)y * w + x] = (uint8_t)((acc + (1 << 19)) >> 20);
    }
  }
}

// rBRIEF: one wavefront per keypoint, 4 comparisons per lane, two lanes per byte
__global__ void __launch_bounds__(kT) k_orb_brief(int n, const int* __restrict__ kp, const float* __restrict__ angle, const uint8_t* __restrict__ blurred, OrbLevels LV,
                                                  const char4* __restrict__ pat, uint8_t* __restrict__ desc) {
  const int f = blockIdx.x * (kT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= n) return;
  const int x = kp[3 * f], y = kp[3 * f + 1], o = kp[3 * f + 2];
  int w = LV.l[0].w; unsigned off = LV.l[0].off;
#pragma unroll
  for (int k = 1; k < kOrbMaxLevels; ++k)
    if (k == o) { w = LV.l[k].w; off = LV.l[k].off; }
  const uint8_t* c = blurred + (size_t)off + (size_t)y * w + x;
  const double th = (double)angle[f] * (M_PI / 180.0);
  const double a = cos(th), b = sin(th);
  int nib = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const char4 q = pat[4 * lane + k];
    const int x1 = (int)rint((double)q.x * a - (double)q.y * b), y1 = (int)rint((double)q.x * b + (double)q.y * a);
    const int x2 = (int)rint((double)q.z * a - (double)q.w * b), y2 = (int)rint((double)q.z * b + (double)q.w * a);
    nib |= ((int)c[y1 * w + x1] < (int)c[y2 * w + x2]) << k;
  }
  const int other = __shfl_down(nib, 1);
  if ((lane & 1) == 0) desc[(size_t)f * 32 + (lane >> 1)] = (uint8_t)(nib | (other << 4));
}

// LocalMap::Search's numeric part: one wavefront per current feature, lanes striding the last keyframe's features.  A candidate's key is
// (distance, level, index): the two smallest keys of the wave are the Hamming 2-NN with the declared tie rule.
__global__ void __launch_bounds__(kT) k_orb_search(int n_last, const float2* __restrict__ lpt, const int* __restrict__ loct, const float* __restrict__ lang,
                                                   const unsigned long long* __restrict__ ldesc, int n_cur, const double* __restrict__ pw, const int* __restrict__ coct,
                                                   const float* __restrict__ cang, const unsigned long long* __restrict__ cdesc, const uint8_t* __restrict__ skip, Pinhole c0,
                                                   Rigid T, const double* __restrict__ radius, int* __restrict__ match, int* __restrict__ best, int* __restrict__ second) {
  const int f = blockIdx.x * (kT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= n_cur) return;
  if (skip && skip[f]) return;                                   // (the outputs were preset to -1)
  double pb[3], pc[3];
  world2robot(T, pw + 3 * f, pb);                                // T: the last keyframe's pose, body -> world
  robot2sensor(c0, pb, pc);
  if (pc[2] < 0) return;                                         // local_map.cpp:316
  const float2 pix = sensor2pixel(c0, pc);
  const float px = pix.x, py = pix.y;
  const int o = coct[f];
  const float ca = cang[f];
  const double r0 = radius[o], r1 = radius[min(o + 1, kOrbMaxLevels - 1)];
  const unsigned long long q0 = cdesc[4 * (size_t)f], q1 = cdesc[4 * (size_t)f + 1], q2 = cdesc[4 * (size_t)f + 2], q3 = cdesc[4 * (size_t)f + 3];
  unsigned long long b = kNoKey, s = kNoKey;
  for (int j = lane; j < n_last; j += 64) {
    const int lv = loct[j];
    if (lv != o && lv != o + 1) continue;
    if (!(fabsf(lang[j] - ca) < 15.f)) continue;
    const float2 lp = lpt[j];
    const double dx = (double)px - (double)lp.x, dy = (double)py - (double)lp.y;
    if (!(sqrt(dx * dx + dy * dy) < (lv == o ? r0 : r1))) continue;
    const unsigned long long* t = ldesc + 4 * (size_t)j;
    const int dist = __popcll(t[0] ^ q0) + __popcll(t[1] ^ q1) + __popcll(t[2] ^ q2) + __popcll(t[3] ^ q3);
    const unsigned long long key = ((unsigned long long)dist << 40) | ((unsigned long long)lv << 32) | (unsigned)j;
    if (key < b) { s = b; b = key; } else if (key < s) s = key;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long ob = __shfl_xor(b, m), os = __shfl_xor(s, m);
    const unsigned long long lo = min(b, ob), hi = max(b, ob);
    b = lo; s = min(hi, min(s, os));
  }
  if (lane == 0) {
    const int bd = b == kNoKey ? -1 : (int)(b >> 40), sd = s == kNoKey ? -1 : (int)(s >> 40);
    if (best) best[f] = bd;
    if (second) second[f] = sd;
    if (sd >= 0 && bd < 50 && (float)bd < 0.8f * (float)sd) match[f] = (int)(b & 0xffffffffull);
  }
}

// exclusive scan of one int per thread over the workgroup (kT threads); wsum: 4 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < wave; ++k) base += wsum[k];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + inc - v;
}

// One workgroup per cell of every level (extractor.cpp:390-429): cv::FAST(cell, ini, nonmax) and, if that list is empty, cv::FAST(cell, min,
// nonmax), both from the one score map: keep_t(p) = score(p) >= t and score(p) > every neighbour's score, a neighbour outside the cell's own
// candidate range [init + 3, max - 3) counting as 0.  The survivors are compacted in pixel order (ballot + prefix) into the cell's own slot
// range — strict maxima of an 8-neighbourhood are never adjacent, so ceil(cw / 2) * ceil(ch / 2) slots always suffice — as records
// score << 24 | y << 12 | x relative to the (28, 28) border.
__global__ void __launch_bounds__(kT) k_orb_cells(const uint8_t* __restrict__ score, OrbLevels LV, OrbGrids G, int ini_th, unsigned* __restrict__ slots,
                                                  int* __restrict__ cell_count) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, t = threadIdx.x;
  int L = 0;
  for (int k = 1; k < G.n; ++k)
    if (G.g[k].ncols > 0 && b >= G.g[k].first) L = k;
  const OrbGrid g = G.g[L];
  const int w = LV.l[L].w, h = LV.l[L].h;
  const uint8_t* sc = score + LV.l[L].off;
  const int c = b - g.first, ci = c / g.ncols, cj = c - ci * g.ncols;
  const int max_bx = w - kMinBorder, max_by = h - kMinBorder;
  const int iy = kMinBorder + ci * g.ch, ix = kMinBorder + cj * g.cw;
  const int x0 = ix + 3, x1 = min(ix + g.cw + 6, max_bx) - 3, y0 = iy + 3, y1 = min(iy + g.ch + 6, max_by) - 3;
  if (iy >= max_by - 3 || ix >= max_bx - 6 || x1 <= x0 || y1 <= y0) {      // the `continue` tests of :395, :404
    if (t == 0) cell_count[b] = 0;
    return;
  }
  const int cwe = x1 - x0, npx = cwe * (y1 - y0), chunks = (npx + kT - 1) / kT;      // <= 60 x 60: at most 15 chunks
  unsigned keep = 0, keep_ini = 0;
  for (int k = 0; k < chunks; ++k) {
    const int q = k * kT + t;
    if (q >= npx) continue;
    const int yy = y0 + q / cwe, xx = x0 + q % cwe;
    const int s = sc[yy * w + xx];
    if (!s) continue;
    int nb = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (!dx && !dy) continue;
        const int ny = yy + dy, nx = xx + dx;
        if (ny >= y0 && ny < y1 && nx >= x0 && nx < x1) nb = max(nb, (int)sc[ny * w + nx]);
      }
    if (s > nb) { keep |= 1u << k; if (s >= ini_th) keep_ini |= 1u << k; }
  }
  const unsigned sel = __syncthreads_or(keep_ini != 0) ? keep_ini : keep;      // the fallback decision of :413-417, on the list AFTER NMS
  unsigned* out = slots + (size_t)g.slot_off + (size_t)c * g.slots;
  int base = 0;
  for (int k = 0; k < chunks; ++k) {
    const int flag = (sel >> k) & 1;
    int total;
    const int pos = base + block_excl_scan(flag, wsum, &total);
    if (flag && pos < g.slots) {
      const int q = k * kT + t, yy = y0 + q / cwe, xx = x0 + q % cwe;
      out[pos] = ((unsigned)sc[yy * w + xx] << 24) | ((unsigned)(yy - kMinBorder) << 12) | (unsigned)(xx - kMinBorder);
    }
    base += total;
  }
  if (t == 0) cell_count[b] = min(base, g.slots);
}

__device__ __forceinline__ int qt_child(short4 bx, int x, int y) {      // DivideNode :137-147: 0..3 = n1..n4; box = (UL.x, UL.y, BR.x, BR.y)
  const int hx = (bx.z - bx.x + 1) >> 1, hy = (bx.w - bx.y + 1) >> 1;  // ceil(float(d) / 2), :105-106
  return (x < bx.x + hx ? 0 : 1) + (y < bx.y + hy ? 0 : 2);
}
__device__ __forceinline__ short4 qt_child_box(short4 bx, int c) {
  const int hx = (bx.z - bx.x + 1) >> 1, hy = (bx.w - bx.y + 1) >> 1;
  return make_short4((short)((c & 1) ? bx.x + hx : bx.x), (short)((c & 2) ? bx.y + hy : bx.y), (short)((c & 1) ? bx.z : bx.x + hx), (short)((c & 2) ? bx.w : bx.y + hy));
}
// (count desc, UL.y, UL.x, index): the declared order of the careful passes
__device__ __forceinline__ bool qt_before(int ca, short4 a, int ia, int cb, short4 b, int ib) {
  if (ca != cb) return ca > cb;
  if (a.y != b.y) return a.y < b.y;
  if (a.x != b.x) return a.x < b.x;
  return ia < ib;
}

// DistributeQuadTree (extractor.cpp:160-366) on sets, one workgroup per level.  At any time the nodes that may still split are exactly those
// with more than one point, so a round is: child counts of every such node (one pass over the points, LDS integer atomics: order-free), the
// choice of the nodes that split (all of them in a full round; in a careful pass the prefix of the order (count desc, UL.y, UL.x) up to the
// first size >= num), the rebuild of the node table (a scan over the nodes' outputs) and the relabelling of the points.  The node table
// (<= kQtNodes) lives in LDS, double-buffered; the points stay in global memory with their node id.  Every branch is taken on values all
// threads read from LDS.  out_kp [levels][kQtNodes][3] = (x, y, level) in level pixels sorted by (y, x), level = -1 in the unused slots.
__global__ void __launch_bounds__(kT) k_orb_quadtree(OrbLevels LV, OrbGrids G, const unsigned* __restrict__ slots, const int* __restrict__ cell_count, int max_cand,
                                                     unsigned* __restrict__ pts_all, int* __restrict__ nid_all, int* __restrict__ out_kp, float* __restrict__ out_resp,
                                                     int* __restrict__ out_count, int* __restrict__ out_err) {
  __shared__ short4 box[2][kQtNodes];
  __shared__ int cnt[2][kQtNodes];
  __shared__ int ccnt[kQtNodes][4];
  __shared__ short newid[kQtNodes][4];
  __shared__ unsigned char split[kQtNodes];
  __shared__ int order[kQtNodes];
  __shared__ int wsum[4];
  __shared__ int sh_a;
  const int L = blockIdx.x, t = threadIdx.x;
  const OrbGrid g = G.g[L];
  int* kp = out_kp + (size_t)L * kQtNodes * 3;
  float* resp = out_resp + (size_t)L * kQtNodes;
  for (int k = t; k < kQtNodes; k += kT) { kp[3 * k] = 0; kp[3 * k + 1] = 0; kp[3 * k + 2] = -1; resp[k] = 0.f; }
  if (t == 0) { out_count[L] = 0; out_err[L] = 0; }
  if (g.ncols == 0) return;
  unsigned* pts = pts_all + (size_t)L * max_cand;
  int* nid = nid_all + (size_t)L * max_cand;
  // ---- pack the level: a scan over the cell counts
  const int ncells = g.ncols * g.nrows;
  int np = 0;
  for (int c0 = 0; c0 < ncells; c0 += kT) {
    const int c = c0 + t, mine = c < ncells ? cell_count[g.first + c] : 0;
    int total;
    const int at = np + block_excl_scan(mine, wsum, &total);
    const unsigned* src = slots + (size_t)g.slot_off + (size_t)c * g.slots;
    for (int k = 0; k < mine; ++k)
      if (at + k < max_cand) pts[at + k] = src[k];
    np += total;
  }
  if (np > max_cand) {                                            // never a silent truncation
    if (t == 0) out_err[L] = np;
    return;
  }
  __syncthreads();
  // ---- initial nodes (:165-202): point -> int(x / hx); empty nodes go in the first rebuild
  const int H = LV.l[L].h - 2 * kMinBorder;
  int n = g.n_init, cur = 0;
  for (int k = t; k < kQtNodes; k += kT) {
    box[0][k] = k < n ? make_short4((short)(int)(g.hx * (float)k), 0, (short)(int)(g.hx * (float)(k + 1)), (short)H) : make_short4(0, 0, 0, 0);
    cnt[0][k] = 0;
  }
  __syncthreads();
  for (int p = t; p < np; p += kT) {
    const int id = min((int)((float)(pts[p] & 0xfffu) / g.hx), n - 1);
    nid[p] = id;
    atomicAdd(&cnt[0][id], 1);
  }
  __syncthreads();
  bool first = true, careful = false;
  for (int round = 0; round < 64; ++round) {
    const int prev = first ? -1 : n;                              // (the removal of the empty initial nodes is not a round of the reference)
    // child counts of every node with more than one point
    for (int k = t; k < kQtNodes; k += kT) { ccnt[k][0] = ccnt[k][1] = ccnt[k][2] = ccnt[k][3] = 0; split[k] = 0; }
    __syncthreads();
    if (!first) {
      for (int p = t; p < np; p += kT) {
        const int id = nid[p];
        if (cnt[cur][id] > 1) {
          const unsigned r = pts[p];
          atomicAdd(&ccnt[id][qt_child(box[cur][id], (int)(r & 0xfffu), (int)((r >> 12) & 0xfffu))], 1);
        }
      }
      __syncthreads();
      if (!careful) {
        for (int k = t; k < n; k += kT) split[k] = cnt[cur][k] > 1;
      } else {
        if (t == 0) sh_a = 0;
        __syncthreads();
        for (int k = t; k < n; k += kT) {
          const int ck = cnt[cur][k];
          if (ck <= 1) continue;
          const short4 bk = box[cur][k];
          int rank = 0;
          for (int j = 0; j < n; ++j) {
            const int cj = cnt[cur][j];
            if (cj > 1 && j != k && qt_before(cj, box[cur][j], j, ck, bk, k)) ++rank;
          }
          order[rank] = k;
          atomicAdd(&sh_a, 1);
        }
        __syncthreads();
        if (t == 0) {                                             // the walk of :291-338: stop at the first size >= num
          int size = n;
          for (int r = 0, nc = sh_a; r < nc; ++r) {
            const int k = order[r];
            split[k] = 1;
            size += (ccnt[k][0] > 0) + (ccnt[k][1] > 0) + (ccnt[k][2] > 0) + (ccnt[k][3] > 0) - 1;
            if (size >= g.num) break;
          }
        }
      }
      __syncthreads();
    }
    // rebuild: thread t owns nodes 4 t .. 4 t + 3; a kept node gives one output (none if it is empty), a split node its non-empty children
    int outs = 0, expand = 0;
    for (int k = 4 * t; k < 4 * t + 4; ++k) {
      if (k >= n) break;
      if (split[k]) {
        for (int c = 0; c < 4; ++c) { outs += ccnt[k][c] > 0; expand += ccnt[k][c] > 1; }
      } else {
        outs += cnt[cur][k] > 0;
      }
    }
    int n_new, n_expand;
    int m = block_excl_scan(outs, wsum, &n_new);
    (void)block_excl_scan(expand, wsum, &n_expand);
    if (n_new > kQtNodes) {                                       // (the host's plan rules this out)
      if (t == 0) out_err[L] = -1;
      return;
    }
    for (int k = 4 * t; k < 4 * t + 4; ++k) {
      if (k >= n) break;
      if (split[k]) {
        for (int c = 0; c < 4; ++c)
          if (ccnt[k][c] > 0) { box[cur ^ 1][m] = qt_child_box(box[cur][k], c); cnt[cur ^ 1][m] = ccnt[k][c]; newid[k][c] = (short)m++; }
      } else if (cnt[cur][k] > 0) {
        box[cur ^ 1][m] = box[cur][k]; cnt[cur ^ 1][m] = cnt[cur][k]; newid[k][0] = (short)m++;
      }
    }
    __syncthreads();
    for (int p = t; p < np; p += kT) {
      const int id = nid[p];
      const unsigned r = pts[p];
      nid[p] = newid[id][split[id] ? qt_child(box[cur][id], (int)(r & 0xfffu), (int)((r >> 12) & 0xfffu)) : 0];
    }
    __syncthreads();
    cur ^= 1; n = n_new;
    if (first) { first = false; continue; }
    if (n >= g.num || n == prev) break;                           // :278, :340
    if (!careful && n + 3 * n_expand > g.num) careful = true;     // :282
  }
  // ---- the best point of every node (:346-363): maximum response, ties to the smallest (y, x)
  unsigned* best = reinterpret_cast<unsigned*>(&ccnt[0][0]);
  for (int k = t; k < kQtNodes; k += kT) best[k] = 0;
  __syncthreads();
  for (int p = t; p < np; p += kT) {
    const unsigned r = pts[p];
    atomicMax(&best[nid[p]], (r & 0xff000000u) | ((0xfffu - ((r >> 12) & 0xfffu)) << 12) | (0xfffu - (r & 0xfffu)));
  }
  __syncthreads();
  // ---- sorted by (y, x): rank among the level's keypoints
  for (int k = t; k < n; k += kT) {
    const unsigned mine = ~best[k] & 0xffffffu;                   // y << 12 | x
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (~best[j] & 0xffffffu) < mine;
    kp[3 * rank] = (int)(mine & 0xfffu) + kMinBorder; kp[3 * rank + 1] = (int)(mine >> 12) + kMinBorder; kp[3 * rank + 2] = L;
    resp[rank] = (float)(best[k] >> 24);
  }
  if (t == 0) out_count[L] = n;
}

__global__ void __launch_bounds__(kT) k_orb_fill(int* __restrict__ p, int n, int v) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
int check_options(const char* who, const lvf_orb_options* o) {
  LVF_REQUIRE(o->patch_size == 31 && o->edge_threshold == 31, "%s: patch_size and edge_threshold must be 31 (got %d, %d)", who, o->patch_size, o->edge_threshold);
  LVF_REQUIRE(o->num_levels >= 1 && o->num_levels <= kOrbMaxLevels, "%s: num_levels must be in [1, %d]", who, kOrbMaxLevels);
  LVF_REQUIRE(o->scale_factor > 1.0f && o->scale_factor <= 2.0f, "%s: scale_factor must be in (1, 2]", who);
  LVF_REQUIRE(o->num_features >= 1, "%s: num_features must be positive", who);
  LVF_REQUIRE(o->min_th_fast >= 1 && o->min_th_fast <= o->ini_th_fast && o->ini_th_fast <= 254, "%s: FAST thresholds must satisfy 1 <= min <= ini <= 254", who);
  LVF_REQUIRE(o->max_candidates >= 1 && o->max_candidates <= 65536, "%s: max_candidates must be in [1, 65536]", who);
  return LVF_OK;
}

// the built-in rBRIEF table: tests/orb_ref.py builtin_pattern, integer only
void builtin_pattern(int8_t* out) {
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto draw = [&s]() {
    for (;;) {
      int t = 0;
      for (int k = 0; k < 4; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        t += (int)((s >> 33) % 11);
      }
      if (std::abs(t - 20) <= kPatternMax) return t - 20;
    }
  };
  for (int n = 0; n < 256;) {
    int r[4];
    for (int k = 0; k < 4; ++k) r[k] = draw();
    if (r[0] == r[2] && r[1] == r[3]) continue;
    for (int k = 0; k < 4; ++k) out[4 * n + k] = (int8_t)r[k];
    ++n;
  }
}

// cv::resize's index / weight pair per output index (weights in 1 / 2048), fp64 without contraction
void resize_table(int src, int dst, int* idx, int* a1) {
#pragma clang fp contract(off)
  const double scale = (double)src / (double)dst;
  for (int d = 0; d < dst; ++d) {
    double f = ((double)d + 0.5) * scale - 0.5;
    int i = (int)std::floor(f);
    f -= (double)i;
    if (i < 0) { i = 0; f = 0.0; }
    if (i >= src - 1) { i = src - 1; f = 0.0; }
    idx[d] = i;
    a1[d] = (int)std::nearbyint(2048.0 * f);
  }
}

}  // namespace

struct lvf_orb {
  lvf_ctx* ctx = nullptr;
  lvf_orb_options opt;
  float scale[kOrbMaxLevels] = {0};
  int num_desired[kOrbMaxLevels] = {0};
  int8_t pattern[1024];
  DevBuf<char4> pat;
  DevBuf<int> umax;
  int w = 0, h = 0;                     // size of the image the pyramid holds; 0: none yet
  OrbLevels lv;
  bool blurred_ok[kOrbMaxLevels] = {false};
  DevBuf<uint8_t> gray, blurred, score;
  DevBuf<int> tables;                   // per level >= 1: {ix[w], a1[w], iy[h], b1[h]}
  size_t table_off[kOrbMaxLevels] = {0};
  // detection: the cell grids, the cells' slot ranges, the packed corners of every level with their node ids, the per-level keypoint tables
  OrbGrids grid;
  DevBuf<unsigned> slots, pts;
  DevBuf<int> cell_count, nid, out_kp, out_meta;      // out_meta: count[8], err[8]
  DevBuf<float> out_resp, out_angle;
};

namespace {

// the cell grid (:383-388) and the initial nodes (:165-166) of a cols x rows level, in float as the reference; false: no cell, no keypoints
bool level_grid(int cols, int rows, OrbGrid* g) {
  const float width = (float)(cols - 2 * kMinBorder), height = (float)(rows - 2 * kMinBorder);
  if (!(width > 0.f && height > 0.f)) return false;
  const int nc = (int)(width / 30.f), nr = (int)(height / 30.f);
  if (nc == 0 || nr == 0) return false;                           // (the reference divides by zero here)
  g->ncols = nc; g->nrows = nr;
  g->cw = (int)std::ceil(width / (float)nc); g->ch = (int)std::ceil(height / (float)nr);
  g->slots = ((g->cw + 1) / 2) * ((g->ch + 1) / 2);
  g->n_init = std::max((int)std::floor(width / height + 0.5f), 1);
  g->hx = width / (float)g->n_init;
  return true;
}

// the pyramid layout and the resize tables of a new image size
int orb_resize_plan(lvf_orb* orb, int w, int h) {
  OrbLevels lv = {};
  lv.n = orb->opt.num_levels;
  size_t total = 0, tab = 0;
  unsigned threads = 0;
  for (int L = 0; L < lv.n; ++L) {
    const float inv = 1.0f / orb->scale[L];
    const int lw = L ? (int)std::lrintf((float)w * inv) : w, lh = L ? (int)std::lrintf((float)h * inv) : h;      // cvRound: half to even
    LVF_REQUIRE(lw >= 1 && lh >= 1 && lw <= kMaxSide && lh <= kMaxSide, "lvf_orb_set_image: level %d of a %d x %d image is empty or wider than %d", L, w, h, kMaxSide);
    lv.l[L].w = lw; lv.l[L].h = lh; lv.l[L].off = (unsigned)total; lv.l[L].first = threads;
    total += ((size_t)lw * lh + 15) & ~(size_t)15;
    if (lw > 2 * kEdge && lh > 2 * kEdge) threads += (unsigned)(lw - 2 * kEdge) * (unsigned)(lh - 2 * kEdge);
    if (L) { orb->table_off[L] = tab; tab += 2 * (size_t)(lw + lh); }
  }
  lv.total = threads;
  OrbGrids G = {};
  G.n = lv.n;
  size_t slot_total = 0;
  for (int L = 0; L < lv.n; ++L) {
    OrbGrid& g = G.g[L];
    g.first = G.total_cells; g.slot_off = (int)slot_total; g.num = orb->num_desired[L];
    if (!level_grid(lv.l[L].w, lv.l[L].h, &g)) { g.ncols = g.nrows = 0; continue; }
    LVF_REQUIRE(4 * g.n_init <= kQtNodes, "lvf_orb_set_image: level %d (%d x %d) is too elongated (%d initial quadtree nodes)", L, lv.l[L].w, lv.l[L].h, g.n_init);
    G.total_cells += g.ncols * g.nrows;
    slot_total += (size_t)g.ncols * g.nrows * g.slots;
  }
  LVF_TRY(orb->slots.alloc(slot_total + 1));
  LVF_TRY(orb->cell_count.alloc((size_t)G.total_cells + 1));
  LVF_TRY(orb->pts.alloc((size_t)lv.n * orb->opt.max_candidates));
  LVF_TRY(orb->nid.alloc((size_t)lv.n * orb->opt.max_candidates));
  LVF_TRY(orb->out_kp.alloc((size_t)lv.n * kQtNodes * 3));
  LVF_TRY(orb->out_resp.alloc((size_t)lv.n * kQtNodes));
  LVF_TRY(orb->out_angle.alloc((size_t)lv.n * kQtNodes));
  LVF_TRY(orb->out_meta.alloc(2 * kOrbMaxLevels));
  orb->grid = G;
  LVF_TRY(orb->gray.alloc(total));
  LVF_TRY(orb->blurred.alloc(total));
  LVF_TRY(orb->score.alloc(total));
  std::vector<int> t(tab);
  for (int L = 1; L < lv.n; ++L) {
    int* p = t.data() + orb->table_off[L];
    resize_table(lv.l[L - 1].w, lv.l[L].w, p, p + lv.l[L].w);
    resize_table(lv.l[L - 1].h, lv.l[L].h, p + 2 * lv.l[L].w, p + 2 * lv.l[L].w + lv.l[L].h);
  }
  LVF_TRY(orb->tables.alloc(tab));
  if (tab) LVF_TRY(lvf::copy_up_wait(orb->ctx, orb->tables.p, t.data(), tab * sizeof(int)));
  orb->lv = lv; orb->w = w; orb->h = h;
  return LVF_OK;
}

int orb_blur_level(lvf_orb* orb, int L) {
  if (orb->blurred_ok[L]) return LVF_OK;
  const OrbLevel& l = orb->lv.l[L];
  hipLaunchKernelGGL(k_orb_blur, dim3((l.w + kBlurW - 1) / kBlurW, (l.h + kBlurH - 1) / kBlurH), dim3(kT), 0, orb->ctx->stream, orb->gray.p + l.off, orb->blurred.p + l.off,
                     l.w, l.h);
  orb->blurred_ok[L] = true;
  return LVF_OK;
}

// level coordinates rint(pt / scale) and the border check; kp = {x, y, level} per keypoint
int orb_level_coords(const char* who, const lvf_orb* orb, int n, const float* pt, const int32_t* octave, std::vector<int>* kp) {
  kp->resize((size_t)3 * n);
  for (int i = 0; i < n; ++i) {
    const int o = octave[i];
    LVF_REQUIRE(o >= 0 && o < orb->opt.num_levels, "%s: keypoint %d has octave %d of %d", who, i, o, orb->opt.num_levels);
    const float fx = std::rint(pt[2 * i] / orb->scale[o]), fy = std::rint(pt[2 * i + 1] / orb->scale[o]);
    const OrbLevel& l = orb->lv.l[o];
    LVF_REQUIRE(fx >= (float)kBorder && fx <= (float)(l.w - 1 - kBorder) && fy >= (float)kBorder && fy <= (float)(l.h - 1 - kBorder),
                "%s: keypoint %d (%g, %g) lies closer than %d pixels to the edge of level %d (%d x %d)", who, i, (double)pt[2 * i], (double)pt[2 * i + 1], kBorder, o, l.w, l.h);
    (*kp)[3 * i] = (int)fx; (*kp)[3 * i + 1] = (int)fy; (*kp)[3 * i + 2] = o;
  }
  return LVF_OK;
}

}  // namespace

extern "C" {

void lvf_orb_options_default(lvf_orb_options* o) {
  if (!o) return;
  o->num_features = 500; o->scale_factor = 1.2f; o->num_levels = 4;      // extractor.h:26
  o->ini_th_fast = 14; o->min_th_fast = 7;
  o->patch_size = 31; o->edge_threshold = 31;
  o->max_candidates = 16384;
}

int lvf_orb_create(lvf_ctx* ctx, const lvf_orb_options* opt, const int8_t* pattern, lvf_orb** out) {
  LVF_REQUIRE(ctx && out, "lvf_orb_create: null argument");
  lvf_orb_options o;
  if (opt) o = *opt; else lvf_orb_options_default(&o);
  LVF_TRY(check_options("lvf_orb_create", &o));
  if (pattern)
    for (int i = 0; i < 1024; ++i)
      LVF_REQUIRE(pattern[i] >= -kPatternMax && pattern[i] <= kPatternMax, "lvf_orb_create: pattern entry %d is %d, beyond +-%d", i, (int)pattern[i], kPatternMax);
  LVF_TRY(lvf::enter(ctx));
  std::unique_ptr<lvf_orb> orb(new lvf_orb());
  orb->ctx = ctx; orb->opt = o;
  // extractor.cpp:14-45: float products, cvRound = half to even
  orb->scale[0] = 1.0f;
  for (int i = 1; i < o.num_levels; ++i) orb->scale[i] = orb->scale[i - 1] * o.scale_factor;
  const float inv_factor = 1.0f / o.scale_factor;
  float nd = (float)o.num_features * (1.0f - inv_factor) / (1.0f - (float)std::pow((double)inv_factor, (double)o.num_levels));
  int sum = 0;
  for (int i = 0; i < o.num_levels - 1; ++i) {
    orb->num_desired[i] = (int)std::lrintf(nd);
    sum += orb->num_desired[i];
    nd *= inv_factor;
  }
  orb->num_desired[o.num_levels - 1] = std::max(o.num_features - sum, 0);
  for (int i = 0; i < o.num_levels; ++i)
    LVF_REQUIRE(orb->num_desired[i] + 2 <= kQtNodes, "lvf_orb_create: level %d would hold %d features, the quadtree's node table holds %d", i, orb->num_desired[i], kQtNodes - 2);
  // extractor.cpp:49-63
  int um[kHalf + 1] = {0};
  const float half = (float)kHalf * std::sqrt(2.f) / 2;
  const int vmax = (int)std::floor(half + 1), vmin = (int)std::ceil(half);
  for (int v = 0; v <= vmax; ++v) um[v] = (int)std::lrint(std::sqrt((double)(kHalf * kHalf - v * v)));
  for (int v = kHalf, v0 = 0; v >= vmin; --v) {
    while (um[v0] == um[v0 + 1]) ++v0;
    um[v] = v0;
    ++v0;
  }
  if (pattern) std::memcpy(orb->pattern, pattern, 1024); else builtin_pattern(orb->pattern);
  LVF_TRY(orb->umax.alloc(kHalf + 1));
  LVF_TRY(orb->pat.alloc(256));
  LVF_TRY(lvf::copy_up_wait(ctx, orb->umax.p, um, sizeof(um)));
  LVF_TRY(lvf::copy_up_wait(ctx, orb->pat.p, orb->pattern, 1024));
  *out = orb.release();
  return LVF_OK;
}

int lvf_orb_destroy(lvf_orb* orb) { delete orb; return LVF_OK; }

int lvf_orb_pattern(const lvf_orb* orb, int8_t* pattern) {
  LVF_REQUIRE(orb && pattern, "lvf_orb_pattern: null argument");
  std::memcpy(pattern, orb->pattern, 1024);
  return LVF_OK;
}

int lvf_orb_level_info(const lvf_orb* orb, int level, float* scale, int* num_desired) {
  LVF_REQUIRE(orb, "lvf_orb_level_info: null object");
  LVF_REQUIRE(level >= 0 && level < orb->opt.num_levels, "lvf_orb_level_info: level %d of %d", level, orb->opt.num_levels);
  if (scale) *scale = orb->scale[level];
  if (num_desired) *num_desired = orb->num_desired[level];
  return LVF_OK;
}

int lvf_orb_set_image(lvf_orb* orb, const lvf_image* img) {
  LVF_REQUIRE(orb && img, "lvf_orb_set_image: null argument");
  int w = 0, h = 0;
  lvf_ctx* ictx = nullptr;
  const uint8_t* src = lvf::image_level0(img, &w, &h, &ictx);
  LVF_REQUIRE(ictx == orb->ctx, "lvf_orb_set_image: the image belongs to another context");
  LVF_TRY(lvf::enter(orb->ctx));
  hipStream_t s = orb->ctx->stream;
  if (w != orb->w || h != orb->h) {
    orb->w = orb->h = 0;                                          // (no pyramid if the plan fails half way)
    LVF_TRY(orb_resize_plan(orb, w, h));
  }
  const OrbLevels& lv = orb->lv;
  for (int L = 0; L < lv.n; ++L) orb->blurred_ok[L] = false;
  LVF_HIP(hipMemcpyAsync(orb->gray.p, src, (size_t)w * h, hipMemcpyDeviceToDevice, s));
  for (int L = 1; L < lv.n; ++L) {
    const int* t = orb->tables.p + orb->table_off[L];
    hipLaunchKernelGGL(k_orb_resize, dim3(grid_of((size_t)lv.l[L].w * lv.l[L].h)), dim3(kT), 0, s, orb->gray.p + lv.l[L - 1].off, lv.l[L - 1].w, lv.l[L - 1].h,
                       orb->gray.p + lv.l[L].off, lv.l[L].w, lv.l[L].h, t, t + 2 * lv.l[L].w);
  }
  LVF_HIP(hipMemsetAsync(orb->score.p, 0, orb->score.n, s));
  if (lv.total) hipLaunchKernelGGL(k_orb_fast_score, dim3(grid_of(lv.total)), dim3(kT), 0, s, orb->gray.p, orb->score.p, lv, orb->opt.min_th_fast);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

int lvf_orb_capacity(const lvf_orb* orb, int width, int height, int* max_keypoints) {
  LVF_REQUIRE(orb && max_keypoints && width >= 1 && height >= 1, "lvf_orb_capacity: bad argument");
  int cap = 0;
  for (int L = 0; L < orb->opt.num_levels; ++L) {
    const float inv = 1.0f / orb->scale[L];
    const int lw = L ? (int)std::lrintf((float)width * inv) : width, lh = L ? (int)std::lrintf((float)height * inv) : height;
    OrbGrid g = {};
    if (level_grid(lw, lh, &g)) cap += std::max(orb->num_desired[L] + 2, 4 * g.n_init);
  }
  *max_keypoints = cap;
  return LVF_OK;
}

int lvf_orb_detect(lvf_orb* orb, const lvf_image* img, int capacity, int* n, int32_t* level_count, float* pt, int32_t* octave, float* angle, float* response,
                   float* size) {
  LVF_REQUIRE(orb && img && n && level_count && capacity >= 0, "lvf_orb_detect: bad argument");
  LVF_REQUIRE(capacity == 0 || (pt && octave && angle && response && size), "lvf_orb_detect: null keypoint arrays");
  LVF_TRY(lvf_orb_set_image(orb, img));
  hipStream_t s = orb->ctx->stream;
  const OrbLevels& lv = orb->lv;
  const int slots_n = lv.n * kQtNodes;
  if (orb->grid.total_cells)
    hipLaunchKernelGGL(k_orb_cells, dim3(orb->grid.total_cells), dim3(kT), 0, s, orb->score.p, lv, orb->grid, orb->opt.ini_th_fast, orb->slots.p, orb->cell_count.p);
  hipLaunchKernelGGL(k_orb_quadtree, dim3(lv.n), dim3(kT), 0, s, lv, orb->grid, orb->slots.p, orb->cell_count.p, orb->opt.max_candidates, orb->pts.p, orb->nid.p,
                     orb->out_kp.p, orb->out_resp.p, orb->out_meta.p, orb->out_meta.p + kOrbMaxLevels);
  hipLaunchKernelGGL(k_orb_angle, dim3((slots_n + 3) / 4), dim3(kT), 0, s, slots_n, orb->out_kp.p, orb->gray.p, lv, orb->umax.p, orb->out_angle.p);
  LVF_HIP(hipGetLastError());
  std::vector<int> meta(2 * kOrbMaxLevels), kp((size_t)3 * slots_n);
  std::vector<float> resp(slots_n), ang(slots_n);
  LVF_HIP(hipMemcpyAsync(meta.data(), orb->out_meta.p, meta.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(kp.data(), orb->out_kp.p, kp.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(resp.data(), orb->out_resp.p, resp.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipMemcpyAsync(ang.data(), orb->out_angle.p, ang.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));                              // the one download of the chain
  int total = 0;
  for (int L = 0; L < lv.n; ++L) {
    const int err = meta[kOrbMaxLevels + L];
    if (err > 0) { lvf::set_error("lvf_orb_detect: level %d holds %d corners, max_candidates is %d", L, err, orb->opt.max_candidates); return LVF_ERR_ORB_OVERFLOW; }
    if (err < 0) { lvf::set_error("lvf_orb_detect: the quadtree of level %d outgrew its node table", L); return LVF_ERR_STATE; }
    total += meta[L];
  }
  *n = total;
  if (total > capacity) { lvf::set_error("lvf_orb_detect: %d keypoints found, capacity is %d", total, capacity); return LVF_ERR_ORB_CAPACITY; }
  int at = 0;
  for (int L = 0; L < lv.n; ++L) {
    level_count[L] = meta[L];
    const float sc = orb->scale[L], sz = (float)(int)(31.f * sc);      // :437: int scaled_patch_size
    for (int k = 0; k < meta[L]; ++k, ++at) {
      const size_t q = (size_t)L * kQtNodes + k;
      pt[2 * at] = (float)kp[3 * q] * sc; pt[2 * at + 1] = (float)kp[3 * q + 1] * sc;      // :499
      octave[at] = L; angle[at] = ang[q]; response[at] = resp[q]; size[at] = sz;
    }
  }
  return LVF_OK;
}

int lvf_orb_orientation(lvf_orb* orb, int n, const float* pt, const int32_t* octave, float* angle) {
  LVF_REQUIRE(orb && n >= 0, "lvf_orb_orientation: bad argument");
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(pt && octave && angle, "lvf_orb_orientation: null keypoint arrays");
  LVF_REQUIRE(orb->w > 0, "lvf_orb_orientation: no image yet (lvf_orb_set_image)");
  std::vector<int> kp;
  LVF_TRY(orb_level_coords("lvf_orb_orientation", orb, n, pt, octave, &kp));
  LVF_TRY(lvf::enter(orb->ctx));
  hipStream_t s = orb->ctx->stream;
  DevBuf<int> k; DevBuf<float> a;
  LVF_TRY(k.upload(kp.data(), kp.size(), s));
  LVF_TRY(a.alloc(n));
  hipLaunchKernelGGL(k_orb_angle, dim3((n + 3) / 4), dim3(kT), 0, s, n, k.p, orb->gray.p, orb->lv, orb->umax.p, a.p);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(angle, a.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_orb_compute(lvf_orb* orb, int n, const float* pt, const int32_t* octave, const float* angle, uint8_t* desc) {
  LVF_REQUIRE(orb && n >= 0, "lvf_orb_compute: bad argument");
  if (n == 0) return LVF_OK;
  LVF_REQUIRE(pt && octave && angle && desc, "lvf_orb_compute: null keypoint arrays");
  LVF_REQUIRE(orb->w > 0, "lvf_orb_compute: no image yet (lvf_orb_set_image)");
  std::vector<int> kp;
  LVF_TRY(orb_level_coords("lvf_orb_compute", orb, n, pt, octave, &kp));
  for (int i = 0; i < n; ++i) LVF_REQUIRE(std::isfinite(angle[i]), "lvf_orb_compute: keypoint %d has a non-finite angle", i);
  LVF_TRY(lvf::enter(orb->ctx));
  hipStream_t s = orb->ctx->stream;
  for (int i = 0; i < n; ++i) LVF_TRY(orb_blur_level(orb, octave[i]));      // only levels that have keypoints are blurred (extractor.cpp:517-522)
  DevBuf<int> k; DevBuf<float> a; DevBuf<uint8_t> d;
  LVF_TRY(k.upload(kp.data(), kp.size(), s));
  LVF_TRY(a.upload(angle, n, s));
  LVF_TRY(d.alloc((size_t)32 * n));
  hipLaunchKernelGGL(k_orb_brief, dim3((n + 3) / 4), dim3(kT), 0, s, n, k.p, a.p, orb->blurred.p, orb->lv, orb->pat.p, d.p);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(desc, d.p, (size_t)32 * n, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_orb_download_level(lvf_orb* orb, int level, int* width, int* height, uint8_t* gray, uint8_t* blurred, uint8_t* score) {
  LVF_REQUIRE(orb, "lvf_orb_download_level: null object");
  LVF_REQUIRE(level >= 0 && level < orb->opt.num_levels, "lvf_orb_download_level: level %d of %d", level, orb->opt.num_levels);
  if (orb->w == 0) { lvf::set_error("lvf_orb_download_level: no image yet (lvf_orb_set_image)"); return LVF_ERR_STATE; }
  LVF_TRY(lvf::enter(orb->ctx));
  const OrbLevel& l = orb->lv.l[level];
  const size_t npx = (size_t)l.w * l.h;
  hipStream_t s = orb->ctx->stream;
  if (width) *width = l.w;
  if (height) *height = l.h;
  if (gray) LVF_HIP(hipMemcpyAsync(gray, orb->gray.p + l.off, npx, hipMemcpyDeviceToHost, s));
  if (blurred) {
    LVF_TRY(orb_blur_level(orb, level));
    LVF_HIP(hipGetLastError());
    LVF_HIP(hipMemcpyAsync(blurred, orb->blurred.p + l.off, npx, hipMemcpyDeviceToHost, s));
  }
  if (score) LVF_HIP(hipMemcpyAsync(score, orb->score.p + l.off, npx, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  return LVF_OK;
}

int lvf_orb_search(lvf_ctx* ctx, const lvf_orb_options* opt, const lvf_camera* cam0, const double* last_pose, int n_last, const float* last_pt,
                   const int32_t* last_octave, const float* last_angle, const uint8_t* last_desc, int n_cur, const double* cur_pw,
                   const int32_t* cur_octave, const float* cur_angle, const uint8_t* cur_desc, const uint8_t* skip, int32_t* match, int32_t* best,
                   int32_t* second) {
  LVF_REQUIRE(ctx && n_last >= 0 && n_cur >= 0, "lvf_orb_search: bad argument");
  lvf_orb_options o;
  if (opt) o = *opt; else lvf_orb_options_default(&o);
  LVF_TRY(check_options("lvf_orb_search", &o));
  if (n_cur == 0) return LVF_OK;
  LVF_TRY(lvf::check_camera("lvf_orb_search", cam0));
  LVF_REQUIRE(last_pose, "lvf_orb_search: null pose");
  LVF_TRY(lvf::check_pose("lvf_orb_search", "the last keyframe's pose", last_pose, nullptr));
  LVF_REQUIRE(cur_pw && cur_octave && cur_angle && cur_desc && match, "lvf_orb_search: null current-feature arrays");
  LVF_REQUIRE(n_last == 0 || (last_pt && last_octave && last_angle && last_desc), "lvf_orb_search: null last-feature arrays");
  for (int i = 0; i < n_cur; ++i) LVF_REQUIRE(cur_octave[i] >= 0 && cur_octave[i] < o.num_levels, "lvf_orb_search: current feature %d has octave %d", i, cur_octave[i]);
  for (int i = 0; i < n_last; ++i) LVF_REQUIRE(last_octave[i] >= 0 && last_octave[i] < o.num_levels, "lvf_orb_search: last feature %d has octave %d", i, last_octave[i]);
  LVF_TRY(lvf::enter(ctx));
  if (n_last == 0) {                                            // no candidates anywhere
    for (int i = 0; i < n_cur; ++i) { match[i] = -1; if (best) best[i] = -1; if (second) second[i] = -1; }
    return LVF_OK;
  }
  hipStream_t s = ctx->stream;
  const Pinhole c0 = lvf::make_pinhole(*cam0);
  const Rigid T = lvf::make_rigid(last_pose);
  double radius[kOrbMaxLevels], sf = 1.0;                        // local_map.h:26-31: double products of the float factor
  for (int L = 0; L < kOrbMaxLevels; ++L) { radius[L] = 31.0 * sf; sf *= (double)o.scale_factor; }
  DevBuf<float2> lp; DevBuf<int> lo, co, out; DevBuf<float> la, ca; DevBuf<unsigned long long> ld, cd; DevBuf<double> pw, rad; DevBuf<uint8_t> sk;
  LVF_TRY(lp.upload(reinterpret_cast<const float2*>(last_pt), n_last, s));
  LVF_TRY(lo.upload(last_octave, n_last, s));
  LVF_TRY(la.upload(last_angle, n_last, s));
  LVF_TRY(ld.upload(reinterpret_cast<const unsigned long long*>(last_desc), (size_t)4 * n_last, s));
  LVF_TRY(co.upload(cur_octave, n_cur, s));
  LVF_TRY(ca.upload(cur_angle, n_cur, s));
  LVF_TRY(cd.upload(reinterpret_cast<const unsigned long long*>(cur_desc), (size_t)4 * n_cur, s));
  LVF_TRY(pw.upload(cur_pw, (size_t)3 * n_cur, s));
  LVF_TRY(rad.upload(radius, kOrbMaxLevels, s));
  if (skip) LVF_TRY(sk.upload(skip, n_cur, s));
  LVF_TRY(out.alloc((size_t)3 * n_cur));
  hipLaunchKernelGGL(k_orb_fill, dim3(grid_of((size_t)3 * n_cur)), dim3(kT), 0, s, out.p, 3 * n_cur, -1);
  hipLaunchKernelGGL(k_orb_search, dim3((n_cur + 3) / 4), dim3(kT), 0, s, n_last, lp.p, lo.p, la.p, ld.p, n_cur, pw.p, co.p, ca.p, cd.p, skip ? sk.p : (const uint8_t*)nullptr, c0, T,
                     rad.p, out.p, out.p + n_cur, out.p + 2 * n_cur);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(match, out.p, (size_t)n_cur * sizeof(int), hipMemcpyDeviceToHost, s));
  if (best) LVF_HIP(hipMemcpyAsync(best, out.p + n_cur, (size_t)n_cur * sizeof(int), hipMemcpyDeviceToHost, s));
  if (second) LVF_HIP(hipMemcpyAsync(second, out.p + 2 * n_cur, (size_t)n_cur * sizeof(int), hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));                              // (also: the host arrays uploaded above may go on return)
  return LVF_OK;
}

}  // extern "C"
