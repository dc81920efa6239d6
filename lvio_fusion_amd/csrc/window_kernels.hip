// window_kernels.hip — the kernels of the persistent window (window.hip is their host side, window_args.hpp what the two share):
// the device-side assembly of a tick's block lists (k_da_classify, k_da_scan, k_da_emit, and k_da_scatter_invd behind the solve), the
// tick's packed upload and read-back (k_window_unpack, k_window_pack) and the outlier gate's flags (k_flag_outliers).
#include "window_args.hpp"

namespace lvf {

// frame of global feature index g (frames' segments concatenated); s_start[n_kf] = total
__device__ __forceinline__ int da_frame_of(const int* s_start, int n_kf, int g) {
  int lo = 0, hi = n_kf - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[mid] <= g) lo = mid; else hi = mid - 1; }
  return lo;
}
__device__ __forceinline__ int da_birth_pos(const long long* s_id, int n_kf, long long id) {
  int lo = 0, hi = n_kf - 1;
  while (lo <= hi) { const int mid = (lo + hi) >> 1; if (s_id[mid] == id) return mid; if (s_id[mid] < id) lo = mid + 1; else hi = mid - 1; }
  return -1;
}
// Landmark::ToWorld (landmark.cpp:15-19) with the matrices the host expanded (same operation order as landmarks_to_world)
__device__ __forceinline__ void da_to_world(const DaArgs& a, const LmDev& L, const FrameDev& B, double pw[3]) {
  const double d = 1.0 / L.inv_depth;
  const double ps[3] = {(L.right_ob[0] - a.cx) * d / a.fx, (L.right_ob[1] - a.cy) * d / a.fy, d};
  const double pb[3] = {a.Re[0] * ps[0] + a.Re[1] * ps[1] + a.Re[2] * ps[2] + a.te[0], a.Re[3] * ps[0] + a.Re[4] * ps[1] + a.Re[5] * ps[2] + a.te[1],
                        a.Re[6] * ps[0] + a.Re[7] * ps[1] + a.Re[8] * ps[2] + a.te[2]};
  pw[0] = B.R[0] * pb[0] + B.R[1] * pb[1] + B.R[2] * pb[2] + B.t[0];
  pw[1] = B.R[3] * pb[0] + B.R[4] * pb[1] + B.R[5] * pb[2] + B.t[1];
  pw[2] = B.R[6] * pb[0] + B.R[7] * pb[1] + B.R[8] * pb[2] + B.t[2];
}
__global__ __launch_bounds__(256) void k_da_classify(DaArgs a) {
  __shared__ int s_start[kDaMaxKf + 1];
  __shared__ long long s_id[kDaMaxKf];
  __shared__ int s_cnt[3], s_tf[kDaMaxKf], s_near[kDaMaxKf];
  const int tid = threadIdx.x, g = blockIdx.x * 256 + tid;
  if (tid < a.n_kf) { s_start[tid] = a.frames[tid].start; s_id[tid] = a.frames[tid].id; s_tf[tid] = 0; s_near[tid] = 0; }
  if (tid == 0) s_start[a.n_kf] = a.total;
  if (tid < 3) s_cnt[tid] = 0;
  __syncthreads();
  if (g < a.total) {
    const int k = da_frame_of(s_start, a.n_kf, g);
    const FrameDev F = a.frames[k];
    const int lm = a.obs_lm[F.arena_off + (g - F.start)];
    const LmDev L = a.lm[lm];
    int c = 0;                                       // 0 none / 1 TwoCamera / 2 TwoFrame / 3 PoseOnly
    if (L.birth_kf == F.id) c = 1;
    else {
      const int bpos = da_birth_pos(s_id, a.n_kf, L.birth_kf);
      double pw[3];
      if (bpos < 0) { if (L.fixed) { c = 3; pw[0] = L.pw[0]; pw[1] = L.pw[1]; pw[2] = L.pw[2]; } }
      else { c = 2; da_to_world(a, L, a.frames[bpos], pw); }
      if (c && !(F.zrow[0] * pw[0] + F.zrow[1] * pw[1] + F.zrow[2] * pw[2] + F.zoff > a.far_z)) atomicAdd(&s_near[k], 1);      // !Camera::Far
      if (c == 2) atomicAdd(&s_tf[k], 1);
    }
    a.cls[g] = (unsigned char)c;
    if (c) atomicAdd(&s_cnt[c - 1], 1);
    if (c == 1 || c == 2) a.used[lm] = 1;
  }
  __syncthreads();
  if (tid < 3) a.wgcnt[3 * blockIdx.x + tid] = s_cnt[tid];
  if (tid < a.n_kf) {
    if (s_tf[tid]) atomicAdd(&a.counts[4 + tid], s_tf[tid]);
    if (s_near[tid]) atomicAdd(&a.counts[4 + kDaMaxKf + tid], s_near[tid]);
  }
}
__global__ __launch_bounds__(1024) void k_da_scan(DaArgs a) {
  // One workgroup, two barriers per 16 k landmarks: the scans run inside waves (shuffles), a Hillis-Steele scan of 1024 LDS entries
  // (20 workgroup barriers each, 16 waves) and a per-thread walk over runs of 64-byte landmark records made this launch 35 us.
  __shared__ int s_cnt[16 * 16];                    // used landmarks per (chunk, wave) of a pass, then their exclusive prefix
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // (1) exclusive scan of the per-workgroup block counts: wave t takes type t, 64 workgroups at a time with a running carry
  if (wv < 3) {
    int carry = 0;
    for (int sb = 0; sb < a.n_wg; sb += 8 * 64) {      // 512 workgroups per pass, their counts requested up front
      int v[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) { const int i = sb + 64 * g + lane; const int t = a.wgcnt[3 * min(i, a.n_wg - 1) + wv]; v[g] = i < a.n_wg ? t : 0; }
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int i = sb + 64 * g + lane;
        const int inc = wave_incl_scan(v[g]);
        if (i < a.n_wg) a.wgbase[3 * i + wv] = carry + inc - v[g];
        carry += __shfl(inc, 63);
      }
    }
    if (lane == 0) a.counts[wv] = carry;
  }
  // (2) dense landmark slots in ascending landmark index (thread = landmark: coalesced; rank = ballot prefix + wave prefix + chunk prefix).
  // 16 k landmarks per pass, the `used` flags and inverse depths of a pass requested up front (a load inside the per-1024 loop is waited
  // for before the next one is issued)
  constexpr int kG = 16;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int total = 0;
  for (int sb = 0; sb < a.nl; sb += kG * 1024) {
    unsigned ubits = 0;
    double invd[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid, lc = min(l, a.nl - 1);
      const unsigned char u = a.used[lc];                // (read unconditionally: behind `l < a.nl &&` each of the 16 loads sat in its own branch and was waited for there)
      ubits |= ((l < a.nl) & (u != 0)) ? (1u << g) : 0u;
      invd[g] = a.lm[lc].inv_depth;
    }
    int rank[kG];
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const unsigned long long m = __ballot((ubits >> g) & 1u);
      rank[g] = __popcll(m & below);
      if (lane == 0) s_cnt[g * 16 + wv] = __popcll(m);
    }
    __syncthreads();
    if (wv == 0) {
      int carry = 0;
#pragma unroll
      for (int base = 0; base < kG * 16; base += 64) {
        const int v = s_cnt[base + lane];
        const int inc = wave_incl_scan(v);
        s_cnt[base + lane] = carry + inc - v;
        carry += __shfl(inc, 63);
      }
      if (lane == 0) s_total = carry;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kG; ++g) {
      const int l = sb + g * 1024 + tid;
      if (l < a.nl) {
        a.lm_invd_out[l] = invd[g];
        if ((ubits >> g) & 1u) { const int at = total + s_cnt[g * 16 + wv] + rank[g]; a.slot[l] = at; a.slot_lm[at] = l; a.state_invd[at] = invd[g]; }
        else a.slot[l] = -1;
      }
    }
    total += s_total;
    __syncthreads();
  }
  if (tid == 0) a.counts[3] = total;
}
__global__ __launch_bounds__(256) void k_da_emit(DaArgs a) {
  __shared__ int s_start[kDaMaxKf + 1];
  __shared__ long long s_id[kDaMaxKf];
  __shared__ int s_wave[4][3];
  const int tid = threadIdx.x, g = blockIdx.x * 256 + tid, lane = tid & 63, wv = tid >> 6;
  if (tid < a.n_kf) { s_start[tid] = a.frames[tid].start; s_id[tid] = a.frames[tid].id; }
  if (tid == 0) s_start[a.n_kf] = a.total;
  const int c = g < a.total ? a.cls[g] : 0;
  // rank of this feature among the workgroup's features of the same type, in feature order
  int rank = 0;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
  for (int t = 1; t <= 3; ++t) {
    const unsigned long long m = __ballot(c == t);
    if (c == t) rank = __popcll(m & below);
    if (lane == 0) s_wave[wv][t - 1] = __popcll(m);
  }
  __syncthreads();
  if (!c) return;
  int idx = a.wgbase[3 * blockIdx.x + (c - 1)] + rank;
  for (int w = 0; w < wv; ++w) idx += s_wave[w][c - 1];
  const int k = da_frame_of(s_start, a.n_kf, g);
  const FrameDev F = a.frames[k];
  const long long i = F.arena_off + (g - F.start);
  const int lm = a.obs_lm[i];
  const double2 ob = a.obs_xy[i];
  const LmDev L = a.lm[lm];
  if (c == 1) {
    a.tc_l[idx] = ob; a.tc_r[idx] = make_double2(L.right_ob[0], L.right_ob[1]); a.tc_lm[idx] = a.slot[lm]; a.tc_kf[idx] = k; a.tc_w[idx] = F.w_tc;
  } else if (c == 2) {
    a.tf_f[idx] = make_double2(L.right_ob[0], L.right_ob[1]); a.tf_o[idx] = ob; a.tf_lm[idx] = a.slot[lm];
    a.tf_k1[idx] = da_birth_pos(s_id, a.n_kf, L.birth_kf); a.tf_k2[idx] = k;
  } else {
    a.po_o[idx] = ob; a.po_pw[3 * idx] = L.pw[0]; a.po_pw[3 * idx + 1] = L.pw[1]; a.po_pw[3 * idx + 2] = L.pw[2]; a.po_kf[idx] = k; a.po_pi[idx] = idx;
  }
}
// after the solve: the landmarks' inverse depths back into landmark-index order (the host mirror is indexed that way)
// ... and into the resident landmark table, which the next tick's assembly reads
__global__ __launch_bounds__(256) void k_da_scatter_invd(int n_lm, const int* __restrict__ slot_lm, const double* __restrict__ state_invd, double* __restrict__ lm_invd_out,
                                                         LmDev* __restrict__ lmtab) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < n_lm) { const int l = slot_lm[s]; const double v = state_invd[s]; lm_invd_out[l] = v; lmtab[l].inv_depth = v; }
}

__global__ __launch_bounds__(256) void k_window_pack(PackArgs a) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k >= a.n_segs) break;
    const uint4* src = reinterpret_cast<const uint4*>(a.src[k]);
    uint4* dst = reinterpret_cast<uint4*>(a.stage + a.off[k]);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < a.words[k]; i += gridDim.x * 256) dst[i] = src[i];
  }
}

// flags[i] = 1 iff |residual_i| > max_err  (residual pairs of a PoseOnly pass with unit weights = pixel errors)
__global__ __launch_bounds__(256) void k_flag_outliers(int n, const double2* __restrict__ res, double max_err, uint8_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double2 r = res[i];
  flags[i] = sqrt(r.x * r.x + r.y * r.y) > max_err ? 1 : 0;      // Vector2d::norm() > 10 (backend.cpp:239)
}

__global__ __launch_bounds__(256) void k_window_unpack(UnpackArgs a) {
  int b = blockIdx.x;
  const int t = threadIdx.x;
  if (b < a.g_tc) {
    const int i = b * 256 + t;
    if (i < a.ntc) { const TcRec r = reinterpret_cast<const TcRec*>(a.stage + a.off_tc)[i]; a.tc_l[i] = make_double2(r.l[0], r.l[1]); a.tc_r[i] = make_double2(r.r[0], r.r[1]); a.tc_lm[i] = r.lm; a.tc_kf[i] = r.kf; if (a.tc_w) a.tc_w[i] = r.w; }
    return;
  }
  b -= a.g_tc;
  if (b < a.g_tf) {
    const int i = b * 256 + t;
    if (i < a.ntf) {
      const TfRec r = reinterpret_cast<const TfRec*>(a.stage + a.off_tf)[i];
      a.tf_f[i] = make_double2(r.f[0], r.f[1]); a.tf_o[i] = make_double2(r.o[0], r.o[1]); a.tf_lm[i] = r.lm; a.tf_k1[i] = r.k1; a.tf_k2[i] = r.k2;
    }
    return;
  }
  b -= a.g_tf;
  if (b < a.g_po) {
    const int i = b * 256 + t;
    if (i < a.npo) {
      const PoRec r = reinterpret_cast<const PoRec*>(a.stage + a.off_po)[i];
      a.po_o[i] = make_double2(r.o[0], r.o[1]); a.po_pw[3 * i] = r.pw[0]; a.po_pw[3 * i + 1] = r.pw[1]; a.po_pw[3 * i + 2] = r.pw[2]; a.po_kf[i] = r.kf; a.po_pi[i] = r.pi;
    }
    return;
  }
  b -= a.g_po;
  // plain segments: workgroup b strides over every segment (static indices only: no scratch)
#pragma unroll
  for (int k = 0; k < kMaxSegs; ++k) {
    if (k >= a.n_segs) break;
    const uint4* src = reinterpret_cast<const uint4*>(a.stage + a.seg_off[k]);
    uint4* dst = reinterpret_cast<uint4*>(a.seg_dst[k]);
    for (unsigned i = (unsigned)b * 256 + t; i < a.seg_words[k]; i += (unsigned)a.g_seg * 256) dst[i] = src[i];
  }
  {
    const int32_t* idx = reinterpret_cast<const int32_t*>(a.stage + a.lm_idx_off);
    const uint4* rec = reinterpret_cast<const uint4*>(a.stage + a.lm_rec_off);
    for (unsigned i = (unsigned)b * 256 + t; i < 4u * (unsigned)a.n_lm_dirty; i += (unsigned)a.g_seg * 256)
      reinterpret_cast<uint4*>(a.lmtab)[4 * (size_t)idx[i >> 2] + (i & 3)] = rec[i];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint4* dst = reinterpret_cast<uint4*>(a.zero_dst[k]);
    for (unsigned i = (unsigned)b * 256 + t; i < a.zero_words[k]; i += (unsigned)a.g_seg * 256) dst[i] = make_uint4(0, 0, 0, 0);
  }
}

}  // namespace lvf
