// scanctx_kernels.hip — LiDAR place recognition on the device: Scan Context (Kim & Kim, IROS 2018) descriptors of a sweep, the
// column-shifted cosine distance against a database of old keyframes and the K best candidates, each with the yaw between the two visits as
// a column shift.  The reference proposes loop candidates by estimated position only (Relocator::DetectLoop, relocator.cpp:87-133), a gate
// that closes once drift exceeds its threshold; this is the appearance gate beside it.  The semantics are the DECLARED ones of
// tests/scanctx_ref.py, with two named deviations from the paper: heights are quantised to 8 bits (cell = 1 + floor(h * inv_height_step),
// capped at 255, 0 = empty), and the search is exhaustive (no ring key: that pre-filter exists to spare a CPU the full evaluation).
//
// An ENTRY is sector-major: num_sectors columns of num_rings bytes (num_rings / 4 dwords), then num_sectors uint32 column norms
// (sum of squares): 1 440 bytes at 20 x 60.
//   k_sc_describe   a grid over the cloud, 1 024 points per workgroup; the ring x sector table sits in LDS as one dword per cell and takes the
//                   points by integer atomicMax (order-free, hence bit-reproducible); its non-empty cells are merged into a zeroed global
//                   table by atomicMax.  16 bytes read per point.
//   k_sc_pack       one wave: the dword table becomes an entry (bytes + norms).  Also recomputes the norms of an uploaded descriptor.
//   k_sc_search     one wavefront per database entry, lane = column shift.  The workgroup keeps the query entry in LDS, each wave its own entry;
//                   a lane walks the columns in ascending order, forms each column pair's dot product with v_dot4_u32_u8 and adds the float64
//                   terms sequentially, as declared; then a lexicographic (distance, shift) minimum over the wave.  One entry read per entry,
//                   12 bytes written.  LDS columns are padded to an odd dword stride, so lanes reading consecutive shifted columns hit distinct
//                   banks whatever num_rings is.
//   k_sc_select     one workgroup: the K smallest (distance bits, index) by K passes of a block minimum (distances are >= +0, so their bit
//                   patterns order as uint64).  8 bytes read per entry and pass, one 256-byte record block written.
// lvf_scanctx_detect queues describe -> pack -> search -> select -> (append) and waits once, for the 256 bytes.
#include "cr_math.hpp"
#include "lvf_internal.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace lvf {

constexpr int kScMaxRings = 32, kScMaxSectors = 64, kScMaxK = 16;
constexpr int kScThreads = 256, kScPointsPerThread = 4, kScSelThreads = 1024;
constexpr int kScLdsEntry = kScMaxSectors * ((kScMaxRings / 4) | 1) + kScMaxSectors;      // dwords: padded columns, then the norms

struct ScP {
  int R, S, RW;                      // rings, sectors, dwords per column
  float min_range, max_range, sensor_height, inv_height_step, ring_scale, sector_scale;
};
struct ScRecords { double dist[kScMaxK]; int index[kScMaxK]; int shift[kScMaxK]; };

__host__ __device__ inline size_t sc_entry_bytes(const ScP& P) { return (size_t)P.S * P.R + (size_t)P.S * 4; }

__global__ __launch_bounds__(kScThreads) void k_sc_describe(int n, const float4* __restrict__ pts, unsigned* __restrict__ tab, const ScP P) {
  __shared__ unsigned s_tab[kScMaxRings * kScMaxSectors];
  const int cells = P.R * P.S;
  for (int c = threadIdx.x; c < cells; c += kScThreads) s_tab[c] = 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * (kScThreads * kScPointsPerThread);
  const float kPiF = 3.14159274101257324f;
#pragma unroll
  for (int k = 0; k < kScPointsPerThread; ++k) {
    const long long i = base + (long long)k * kScThreads + threadIdx.x;
    if (i >= n) break;
    const float4 p = pts[i];
    const float xx = p.x * p.x, yy = p.y * p.y;
    const float r = sqrtf(xx + yy);
    if (!(isfinite(r) && isfinite(p.z) && r >= P.min_range && r < P.max_range)) continue;
    const float h = p.z + P.sensor_height;
    if (!(h > 0.0f)) continue;                                        // cell 0: the table is zero already
    const float hq = floorf(h * P.inv_height_step);
    const unsigned cell = hq >= 254.0f ? 255u : 1u + (unsigned)(int)hq;
    const int ring = min(P.R - 1, (int)floorf(r * P.ring_scale));
    const float th = cr_atan2f(p.y, p.x);
    const int sector = min(max((int)floorf((th + kPiF) * P.sector_scale), 0), P.S - 1);
    atomicMax(&s_tab[sector * P.R + ring], cell);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kScThreads) {
    const unsigned v = s_tab[c];
    if (v) atomicMax(&tab[c], v);
  }
}

// thread = sector.  tab != null: the dword table becomes the entry's bytes; tab == null: the bytes are there already (an uploaded descriptor).
// Either way the column norms are (re)computed from the bytes.
__global__ __launch_bounds__(64) void k_sc_pack(const unsigned* __restrict__ tab, unsigned* __restrict__ entry, const ScP P) {
  const int j = threadIdx.x;
  if (j >= P.S) return;
  unsigned n2 = 0u;
  for (int w = 0; w < P.RW; ++w) {
    unsigned word;
    if (tab) {
      const unsigned* t = tab + j * P.R + w * 4;
      word = (t[0] & 255u) | ((t[1] & 255u) << 8) | ((t[2] & 255u) << 16) | ((t[3] & 255u) << 24);
      entry[j * P.RW + w] = word;
    } else {
      word = entry[j * P.RW + w];
    }
    n2 = __builtin_amdgcn_udot4(word, word, n2, false);
  }
  entry[P.S * P.RW + j] = n2;
}

__device__ __forceinline__ bool sc_key_less(unsigned long long a, int ai, unsigned long long b, int bi) { return a < b || (a == b && ai < bi); }

// lexicographic minimum of (key, idx) over the wave, delivered to every lane
__device__ __forceinline__ void sc_wave_min(unsigned long long& k, int& i) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(k >> 32), m), lo = __shfl_xor((unsigned)k, m);
    const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
    const int oi = __shfl_xor(i, m);
    if (sc_key_less(ok, oi, k, i)) { k = ok; i = oi; }
  }
}

__device__ __forceinline__ void sc_stage(const unsigned* __restrict__ g, unsigned* s, int lane_id, int stride, const ScP& P, int ls) {
  const int words = P.S * P.RW;
  for (int w = lane_id; w < words; w += stride) { const int col = w / P.RW; s[col * ls + (w - col * P.RW)] = g[w]; }
  for (int j = lane_id; j < P.S; j += stride) s[P.S * ls + j] = g[words + j];
}

__global__ __launch_bounds__(kScThreads) void k_sc_search(int n, const unsigned char* __restrict__ db, const unsigned* __restrict__ query, double* __restrict__ dist,
                                                          int* __restrict__ shift, const ScP P) {
  __shared__ unsigned s_q[kScLdsEntry];
  __shared__ unsigned s_e[kScThreads / 64][kScLdsEntry];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ls = P.RW | 1;                                             // odd column stride
  const size_t eb = sc_entry_bytes(P);
  sc_stage(query, s_q, threadIdx.x, kScThreads, P, ls);
  const unsigned* qn = s_q + P.S * ls;
  unsigned* se = s_e[wave];
  const unsigned* dn = se + P.S * ls;
  // (the trip count is the same for the waves of a workgroup: every wave reaches both barriers)
  for (int base = blockIdx.x * (kScThreads / 64); base < n; base += gridDim.x * (kScThreads / 64)) {
    const int e = base + wave;
    if (e < n) sc_stage(reinterpret_cast<const unsigned*>(db + (size_t)e * eb), se, lane, 64, P, ls);
    __syncthreads();
    if (e < n) {
      double d = __longlong_as_double(0x7ff0000000000000ll);
      int s = 64;
      if (lane < P.S) {
        double sum = 0.0;
        int count = 0;
        // no branch on validity and four columns in flight: a term's square root and division are ~50 dependent float64 instructions, and only
        // the additions have to wait for one another (an invalid pair's term is 0 / 0 and is dropped by the select)
#pragma unroll 4
        for (int j = 0; j < P.S; ++j) {
          int c = lane + j;
          if (c >= P.S) c -= P.S;
          const unsigned n2q = qn[j], n2d = dn[c];
          const bool valid = n2q != 0u && n2d != 0u;
          unsigned dot = 0u;
          for (int w = 0; w < P.RW; ++w) dot = __builtin_amdgcn_udot4(s_q[j * ls + w], se[c * ls + w], dot, false);
          const double term = (double)dot / sqrt((double)((unsigned long long)n2q * (unsigned long long)n2d));
          sum = valid ? sum + term : sum;
          count += valid ? 1 : 0;
        }
        d = count ? 1.0 - sum / (double)count : 1.0;
        s = lane;
      }
      // (d >= +0 or +inf: the bit patterns order as the values do)
      unsigned long long key = (unsigned long long)__double_as_longlong(d);
      sc_wave_min(key, s);
      if (lane == 0) { dist[e] = __longlong_as_double((long long)key); shift[e] = s; }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kScSelThreads) void k_sc_select(int n, int K, const double* __restrict__ dist, const int* __restrict__ shift, ScRecords* __restrict__ out) {
  // the wave minima of a pass, double-buffered by the pass's parity: EVERY thread folds them after the one barrier of the pass (they all arrive
  // at the same winner, so nothing is broadcast), and a wave can only write a buffer again two passes later, behind the barrier in between
  __shared__ unsigned long long s_key[2][kScSelThreads / 64];
  __shared__ int s_idx[2][kScSelThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long kNone = ~0ull;
  const int kNoIdx = 0x7fffffff;
  unsigned long long lk = 0ull;                                        // the previous pass's winner: this pass takes the smallest key above it
  int li = -1;
  unsigned long long win_key = kNone;                                  // thread k keeps pass k's winner
  int win_idx = kNoIdx;
  for (int k = 0; k < K; ++k) {
    unsigned long long bk = kNone;
    int bi = kNoIdx;
    if (li != kNoIdx) {                                                // (nothing was left in the previous pass: nothing is left now)
      // (four loads in flight per thread: a pass is bound by their latency)
      for (int i0 = threadIdx.x; i0 < n; i0 += 4 * kScSelThreads) {
        unsigned long long key[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = i0 + u * kScSelThreads; key[u] = i < n ? (unsigned long long)__double_as_longlong(dist[i]) : kNone; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * kScSelThreads;
          if (i >= n || (k > 0 && !sc_key_less(lk, li, key[u], i))) continue;
          if (sc_key_less(key[u], i, bk, bi)) { bk = key[u]; bi = i; }
        }
      }
    }
    sc_wave_min(bk, bi);
    if (lane == 0) { s_key[k & 1][wave] = bk; s_idx[k & 1][wave] = bi; }
    __syncthreads();
    bk = s_key[k & 1][0]; bi = s_idx[k & 1][0];
#pragma unroll
    for (int w = 1; w < kScSelThreads / 64; ++w) {
      const unsigned long long ok = s_key[k & 1][w];
      const int oi = s_idx[k & 1][w];
      if (sc_key_less(ok, oi, bk, bi)) { bk = ok; bi = oi; }
    }
    // (the key IS the distance; the winner's shift is fetched after the passes, off their critical path)
    if ((int)threadIdx.x == k) { win_key = bk; win_idx = bi; }
    lk = bk; li = bi;
  }
  if ((int)threadIdx.x < K) {
    const bool found = win_idx != kNoIdx;
    out->dist[threadIdx.x] = found ? __longlong_as_double((long long)win_key) : __longlong_as_double(0x7ff0000000000000ll);
    out->index[threadIdx.x] = found ? win_idx : -1;
    out->shift[threadIdx.x] = found ? shift[win_idx] : -1;
  }
}

}  // namespace lvf

struct lvf_scanctx_db {
  lvf_ctx* ctx = nullptr;
  lvf::ScP P{};
  int capacity = 0, size = 0;
  std::vector<double> stamps;                  // host: non-decreasing
  lvf::DevBuf<unsigned char> entries;          // [capacity + 1] entries; the last one is the query slot
  lvf::DevBuf<unsigned> tab;                   // the describe pass's dword table
  lvf::DevBuf<double> dist;                    // [capacity]
  lvf::DevBuf<int> shift;                      // [capacity]
  lvf::DevBuf<lvf::ScRecords> records;
};

namespace lvf {
namespace {

int sc_params(const char* who, const lvf_scanctx_options* opt, ScP* P) {
  lvf_scanctx_options o;
  if (opt) o = *opt; else lvf_scanctx_options_default(&o);
  LVF_REQUIRE(o.num_rings >= 4 && o.num_rings <= kScMaxRings && o.num_rings % 4 == 0, "%s: num_rings %d is not a multiple of 4 in [4, %d]", who, o.num_rings, kScMaxRings);
  LVF_REQUIRE(o.num_sectors >= 1 && o.num_sectors <= kScMaxSectors, "%s: num_sectors %d outside [1, %d]", who, o.num_sectors, kScMaxSectors);
  LVF_REQUIRE(std::isfinite(o.max_range) && std::isfinite(o.min_range) && o.min_range > 0.0f && o.min_range < o.max_range, "%s: need 0 < min_range < max_range (finite)", who);
  LVF_REQUIRE(std::isfinite(o.inv_height_step) && o.inv_height_step > 0.0f, "%s: inv_height_step must be positive", who);
  LVF_REQUIRE(std::isfinite(o.sensor_height), "%s: non-finite sensor_height", who);
  P->R = o.num_rings; P->S = o.num_sectors; P->RW = o.num_rings / 4;
  P->min_range = o.min_range; P->max_range = o.max_range; P->sensor_height = o.sensor_height; P->inv_height_step = o.inv_height_step;
  P->ring_scale = (float)((double)o.num_rings / (double)o.max_range);
  P->sector_scale = (float)((double)o.num_sectors / (2.0 * 3.141592653589793));
  return LVF_OK;
}

// zeroed table <- cloud <- pack into `entry`; nothing waits
int sc_describe_into(lvf_ctx* ctx, const lvf_cloud* cloud, const ScP& P, unsigned* tab, unsigned char* entry) {
  LVF_HIP(hipMemsetAsync(tab, 0, (size_t)P.R * P.S * sizeof(unsigned), ctx->stream));
  if (cloud->n > 0) {
    const int per = kScThreads * kScPointsPerThread;
    hipLaunchKernelGGL(k_sc_describe, dim3((unsigned)(((long long)cloud->n + per - 1) / per)), dim3(kScThreads), 0, ctx->stream, cloud->n, cloud->pts.p, tab, P);
    LVF_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sc_pack, dim3(1), dim3(64), 0, ctx->stream, (const unsigned*)tab, reinterpret_cast<unsigned*>(entry), P);
  LVF_HIP(hipGetLastError());
  return LVF_OK;
}

unsigned char* sc_slot(lvf_scanctx_db* db, int i) { return db->entries.p + (size_t)i * sc_entry_bytes(db->P); }

int sc_prefix(const lvf_scanctx_db* db, double max_stamp) {
  return (int)(std::upper_bound(db->stamps.begin(), db->stamps.end(), max_stamp) - db->stamps.begin());
}

// search the first n entries for `query` (an entry on the device), select K, download; ONE wait
int sc_search_tail(lvf_scanctx_db* db, const unsigned char* query, int n, int k, int32_t* out_index, int32_t* out_shift, double* out_distance) {
  lvf_ctx* ctx = db->ctx;
  if (n > 0) {
    const int waves = kScThreads / 64;
    const int grid = std::min((n + waves - 1) / waves, 65536);      // (one pass per workgroup up to 262 144 entries: short workgroups balance the tail)
    hipLaunchKernelGGL(k_sc_search, dim3(grid), dim3(kScThreads), 0, ctx->stream, n, (const unsigned char*)db->entries.p, reinterpret_cast<const unsigned*>(query), db->dist.p,
                       db->shift.p, db->P);
    LVF_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_sc_select, dim3(1), dim3(kScSelThreads), 0, ctx->stream, n, k, (const double*)db->dist.p, (const int*)db->shift.p, db->records.p);
  LVF_HIP(hipGetLastError());
  ScRecords rec;
  LVF_TRY(read_back(ctx, &rec, db->records.p, sizeof(rec)));
  for (int i = 0; i < k; ++i) { out_index[i] = rec.index[i]; out_shift[i] = rec.shift[i]; out_distance[i] = rec.dist[i]; }
  return LVF_OK;
}

int sc_check_search(const char* who, const lvf_scanctx_db* db, double max_stamp, int k, const int32_t* out_index, const int32_t* out_shift, const double* out_distance) {
  LVF_REQUIRE(db, "%s: null database", who);
  LVF_REQUIRE(k >= 1 && k <= kScMaxK, "%s: k = %d outside [1, %d]", who, k, kScMaxK);
  LVF_REQUIRE(out_index && out_shift && out_distance, "%s: null output array", who);
  LVF_REQUIRE(max_stamp == max_stamp, "%s: max_stamp is NaN", who);
  return LVF_OK;
}

int sc_check_append(const char* who, const lvf_scanctx_db* db, double stamp) {
  LVF_REQUIRE(std::isfinite(stamp), "%s: non-finite stamp", who);
  LVF_REQUIRE(db->size < db->capacity, "%s: the database is full (capacity %d)", who, db->capacity);
  LVF_REQUIRE(db->stamps.empty() || stamp >= db->stamps.back(), "%s: stamp %.9f lies before the last one (%.9f)", who, stamp, db->stamps.empty() ? 0.0 : db->stamps.back());
  return LVF_OK;
}

void sc_split(const unsigned char* entry, const ScP& P, uint8_t* out_desc, uint32_t* out_norm) {
  std::memcpy(out_desc, entry, (size_t)P.S * P.R);
  if (out_norm) std::memcpy(out_norm, entry + (size_t)P.S * P.R, (size_t)P.S * 4);
}

}  // namespace
}  // namespace lvf

using namespace lvf;

extern "C" {

void lvf_scanctx_options_default(lvf_scanctx_options* o) {
  if (!o) return;
  o->num_rings = 20; o->num_sectors = 60; o->max_range = 80.0f; o->min_range = 0.5f; o->sensor_height = 2.0f; o->inv_height_step = 10.0f;
}

int lvf_scanctx_describe(lvf_ctx* ctx, const lvf_cloud* cloud, const lvf_scanctx_options* opt, uint8_t* out_desc_u8, uint32_t* out_norm_u32) {
  LVF_REQUIRE(ctx && cloud && out_desc_u8, "lvf_scanctx_describe: null argument");
  LVF_REQUIRE(cloud->ctx == ctx, "lvf_scanctx_describe: the cloud belongs to another context");
  ScP P;
  LVF_TRY(sc_params("lvf_scanctx_describe", opt, &P));
  LVF_TRY(lvf::enter(ctx));
  DevBuf<unsigned> tab;
  DevBuf<unsigned char> entry;
  LVF_TRY(tab.alloc((size_t)P.R * P.S)); LVF_TRY(entry.alloc(sc_entry_bytes(P)));
  LVF_TRY(sc_describe_into(ctx, cloud, P, tab.p, entry.p));
  unsigned char host[kScMaxSectors * kScMaxRings + kScMaxSectors * 4];
  LVF_TRY(read_back(ctx, host, entry.p, sc_entry_bytes(P)));
  sc_split(host, P, out_desc_u8, out_norm_u32);
  return LVF_OK;
}

int lvf_scanctx_db_create(lvf_ctx* ctx, const lvf_scanctx_options* opt, int capacity, lvf_scanctx_db** out) {
  LVF_REQUIRE(ctx && out, "lvf_scanctx_db_create: null argument");
  LVF_REQUIRE(capacity >= 1 && capacity <= (1 << 20), "lvf_scanctx_db_create: capacity %d outside [1, 2^20]", capacity);
  std::unique_ptr<lvf_scanctx_db> db(new lvf_scanctx_db());
  LVF_TRY(sc_params("lvf_scanctx_db_create", opt, &db->P));
  LVF_TRY(lvf::enter(ctx));
  db->ctx = ctx; db->capacity = capacity;
  db->stamps.reserve((size_t)capacity);
  LVF_TRY(db->entries.alloc(((size_t)capacity + 1) * sc_entry_bytes(db->P)));
  LVF_TRY(db->tab.alloc((size_t)db->P.R * db->P.S));
  LVF_TRY(db->dist.alloc((size_t)capacity)); LVF_TRY(db->shift.alloc((size_t)capacity));
  LVF_TRY(db->records.alloc(1));
  *out = db.release();
  return LVF_OK;
}

// (an append may still be in flight: the buffers go back to the context's pool, whose reuse is ordered on the same stream)
int lvf_scanctx_db_destroy(lvf_scanctx_db* db) { delete db; return LVF_OK; }
int lvf_scanctx_db_size(const lvf_scanctx_db* db) { return db ? db->size : -1; }

int lvf_scanctx_db_append(lvf_scanctx_db* db, const lvf_cloud* cloud, double stamp) {
  LVF_REQUIRE(db && cloud, "lvf_scanctx_db_append: null argument");
  LVF_REQUIRE(cloud->ctx == db->ctx, "lvf_scanctx_db_append: the cloud belongs to another context");
  LVF_TRY(sc_check_append("lvf_scanctx_db_append", db, stamp));
  LVF_TRY(lvf::enter(db->ctx));
  LVF_TRY(sc_describe_into(db->ctx, cloud, db->P, db->tab.p, sc_slot(db, db->size)));
  db->stamps.push_back(stamp); db->size += 1;
  return LVF_OK;
}

int lvf_scanctx_db_append_descriptor(lvf_scanctx_db* db, const uint8_t* desc_u8, double stamp) {
  LVF_REQUIRE(db && desc_u8, "lvf_scanctx_db_append_descriptor: null argument");
  LVF_TRY(sc_check_append("lvf_scanctx_db_append_descriptor", db, stamp));
  LVF_TRY(lvf::enter(db->ctx));
  unsigned char* slot = sc_slot(db, db->size);
  LVF_TRY(copy_up_wait(db->ctx, slot, desc_u8, (size_t)db->P.S * db->P.R));
  hipLaunchKernelGGL(k_sc_pack, dim3(1), dim3(64), 0, db->ctx->stream, (const unsigned*)nullptr, reinterpret_cast<unsigned*>(slot), db->P);
  LVF_HIP(hipGetLastError());
  db->stamps.push_back(stamp); db->size += 1;
  return LVF_OK;
}

int lvf_scanctx_db_download(const lvf_scanctx_db* db, int index, uint8_t* out_desc_u8, uint32_t* out_norm_u32) {
  LVF_REQUIRE(db && out_desc_u8, "lvf_scanctx_db_download: null argument");
  LVF_REQUIRE(index >= 0 && index < db->size, "lvf_scanctx_db_download: index %d outside [0, %d)", index, db->size);
  LVF_TRY(lvf::enter(db->ctx));
  unsigned char host[kScMaxSectors * kScMaxRings + kScMaxSectors * 4];
  LVF_TRY(read_back(db->ctx, host, db->entries.p + (size_t)index * sc_entry_bytes(db->P), sc_entry_bytes(db->P)));
  sc_split(host, db->P, out_desc_u8, out_norm_u32);
  return LVF_OK;
}

int lvf_scanctx_search(lvf_scanctx_db* db, const uint8_t* query_desc_u8, double max_stamp, int k, int32_t* out_index, int32_t* out_shift, double* out_distance) {
  LVF_TRY(sc_check_search("lvf_scanctx_search", db, max_stamp, k, out_index, out_shift, out_distance));
  LVF_REQUIRE(query_desc_u8, "lvf_scanctx_search: null query");
  lvf_ctx* ctx = db->ctx;
  LVF_TRY(lvf::enter(ctx));
  // the query goes up through the context's pinned staging (no wait of its own: the read-back at the end waits) and gets its norms on the device
  const size_t bytes = (size_t)db->P.S * db->P.R;
  unsigned char* q = sc_slot(db, db->capacity);
  LVF_TRY(ctx->stage.reserve(bytes));
  std::memcpy(ctx->stage.p, query_desc_u8, bytes);
  StreamWaitGuard wait(ctx->stream);
  LVF_HIP(hipMemcpyAsync(q, ctx->stage.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_sc_pack, dim3(1), dim3(64), 0, ctx->stream, (const unsigned*)nullptr, reinterpret_cast<unsigned*>(q), db->P);
  LVF_HIP(hipGetLastError());
  LVF_TRY(sc_search_tail(db, q, sc_prefix(db, max_stamp), k, out_index, out_shift, out_distance));
  wait.dismiss();
  return LVF_OK;
}

int lvf_scanctx_detect(lvf_scanctx_db* db, const lvf_cloud* cloud, double stamp, double max_stamp, int k, int32_t* out_index, int32_t* out_shift, double* out_distance,
                       int append) {
  LVF_TRY(sc_check_search("lvf_scanctx_detect", db, max_stamp, k, out_index, out_shift, out_distance));
  LVF_REQUIRE(cloud, "lvf_scanctx_detect: null cloud");
  LVF_REQUIRE(cloud->ctx == db->ctx, "lvf_scanctx_detect: the cloud belongs to another context");
  if (append) LVF_TRY(sc_check_append("lvf_scanctx_detect", db, stamp));
  lvf_ctx* ctx = db->ctx;
  LVF_TRY(lvf::enter(ctx));
  // with append the descriptor is built straight into slot `size` (which lies behind every searched entry), else into the query slot
  unsigned char* q = sc_slot(db, append ? db->size : db->capacity);
  const int n = sc_prefix(db, max_stamp);
  LVF_TRY(sc_describe_into(ctx, cloud, db->P, db->tab.p, q));
  LVF_TRY(sc_search_tail(db, q, n, k, out_index, out_shift, out_distance));
  if (append) { db->stamps.push_back(stamp); db->size += 1; }
  return LVF_OK;
}

}  // extern "C"
