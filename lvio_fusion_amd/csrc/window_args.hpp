// window_args.hpp — what the persistent window's kernels (window_kernels.hip) and its host side (window.hip) share: the device table
// records, every kernel argument block, the constants that size them, and a prototype of every kernel the host launches.  The kernels
// themselves, with their __launch_bounds__, are defined in window_kernels.hip.
#pragma once
#include "lvf_internal.hpp"

namespace lvf {

// ================================================================================================ device-side assembly
// The block lists of a tick assembled ON THE DEVICE from resident tables, so that the host neither walks ~10^5 features nor uploads
// ~4 MB of lists per tick:
//   feature arena   obs_lm[i] (landmark INDEX, stable: lvf_window::lms entries never move), obs_xy[i]; one segment per keyframe, in
//                   BuildProblem's order (ascending landmark id); only new / changed keyframes are uploaded
//   landmark table  LmDev[nl] (first observation, inverse depth, birth keyframe id, frozen world point) — resident: only entries the
//                   host changed are sent, the solved inverse depths are written into it by k_da_scatter_invd (64 B each)
//   frame table     FrameDev[n_kf] (id, segment, rotation + translation for Landmark::ToWorld, the Camera::Far row) — every tick
// k_da_classify : one thread per feature -> block type (BuildProblem's rules), per-workgroup and per-keyframe counts, landmarks in use
// k_da_scan     : one workgroup: output offsets per workgroup and type (features keep their order: keyframe by keyframe, ascending
//                 landmark id), dense landmark slots (ascending landmark index), inverse depths into the state
// k_da_emit     : one thread per feature -> its block's SoA entries
// The host reads back 4 + 2 n_kf counters (block totals, TwoFrame blocks and near visual blocks per keyframe) for the work list, the
// IMU / prior decisions and the launch shapes.
struct LmDev { double right_ob[2]; double pw[3]; double inv_depth; long long birth_kf; int fixed; int alive; };
// w_tc: the weight backend.cpp:123 hands TwoCameraReprojectionError::Create for a landmark born in this frame, `5 * frame->weights.visual` — a FLOAT
// product (adapt/weights.h:10 declares the weights float), widened to double by the call: (double)(5.0f * (float)w_visual)
struct FrameDev { long long id; int start, cnt; long long arena_off; double zrow[3], zoff; double R[9], t[3]; double w_tc; };
static_assert(sizeof(LmDev) == 64 && sizeof(FrameDev) % 8 == 0, "device table records");
constexpr int kDaMaxKf = 64;
struct DaArgs {
  int n_kf, total, nl, n_wg;
  const FrameDev* frames; const int32_t* obs_lm; const double2* obs_xy; const LmDev* lm;
  double Re[9], te[3], fx, fy, cx, cy, far_z;      // right camera (Landmark::ToWorld goes through it), Camera::Far threshold
  unsigned char* cls; unsigned char* used; int* wgcnt; int* wgbase; int* slot; int* slot_lm; int* counts;   // counts: [0..3] tc, tf, po, n_lm | tf per kf [64] | near per kf [64]
  double* state_invd; double* lm_invd_out;
  double2 *tc_l, *tc_r; int32_t *tc_lm, *tc_kf; double* tc_w;
  double2 *tf_f, *tf_o; int32_t *tf_lm, *tf_k1, *tf_k2;
  double2* po_o; double* po_pw; int32_t *po_kf, *po_pi;
};

// the read-back mirror of k_window_unpack's plain segments: device arrays -> one contiguous staging block (then ONE device-to-host copy
// instead of five, each a submission of its own)
struct PackArgs { unsigned char* stage; int n_segs; const unsigned char* src[8]; size_t off[8]; unsigned words[8]; };

// ---- the tick's upload: ONE host-to-device copy of a packed staging buffer, unpacked on the device.
// The block lists used to go up as ~25 separate copies; each is a blit launch of its own (~5 us) behind ~10 us of submission latency,
// and together they kept the GPU waiting for 0.33 ms per tick.  The host now writes one 48-byte record per block —
//   TwoCamera {left ob, right ob, landmark slot, keyframe}   TwoFrame {first ob, ob, landmark slot, k1, k2}   PoseOnly {ob, pw, keyframe, table row}
// — into one pinned buffer, followed by the small plain arrays (state, IMU pre-integrations and indices, priors); k_window_unpack turns
// the records into the batches' SoA arrays and copies the plain segments to their buffers.
struct TcRec { double l[2], r[2]; int32_t lm, kf; double w; };      // w: the block's weight (two_camera_weight)
struct TfRec { double f[2], o[2]; int32_t lm, k1, k2, pad0; };
struct PoRec { double o[2], pw[3]; int32_t kf, pi; };
static_assert(sizeof(TcRec) == 48 && sizeof(TfRec) == 48 && sizeof(PoRec) == 48, "staging records are 48 bytes");
constexpr int kMaxSegs = 96;            // (the whole UnpackArgs block stays under the 4 KB kernel-argument limit)
struct UnpackArgs {
  const unsigned char* stage;
  int ntc, ntf, npo; size_t off_tc, off_tf, off_po;
  double2 *tc_l, *tc_r; int32_t *tc_lm, *tc_kf; double* tc_w;
  double2 *tf_f, *tf_o; int32_t *tf_lm, *tf_k1, *tf_k2;
  double2* po_o; double* po_pw; int32_t *po_kf, *po_pi;
  int n_segs; unsigned char* seg_dst[kMaxSegs]; size_t seg_off[kMaxSegs]; unsigned seg_words[kMaxSegs];   // 16-byte words (sizes are padded up)
  int g_tc, g_tf, g_po, g_seg;
  unsigned char* zero_dst[2]; unsigned zero_words[2];      // buffers cleared by the same launch (16-byte words)
  // changed entries of the resident landmark table: record j (64 bytes at rec_off + 64 j) goes to entry idx[j] (int32 at idx_off + 4 j)
  int n_lm_dirty; size_t lm_idx_off, lm_rec_off; unsigned char* lmtab;
};
static_assert(sizeof(UnpackArgs) <= 4096, "kernel-argument limit");

// ---- kernels (window_kernels.hip)
__global__ void k_da_classify(DaArgs a);
__global__ void k_da_scan(DaArgs a);
__global__ void k_da_emit(DaArgs a);
__global__ void k_da_scatter_invd(int n_lm, const int* __restrict__ slot_lm, const double* __restrict__ state_invd, double* __restrict__ lm_invd_out,
                                  LmDev* __restrict__ lmtab);
__global__ void k_window_pack(PackArgs a);
__global__ void k_window_unpack(UnpackArgs a);
__global__ void k_flag_outliers(int n, const double2* __restrict__ res, double max_err, uint8_t* __restrict__ flags);

}  // namespace lvf
