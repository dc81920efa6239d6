// window.hip — a PERSISTENT sliding window (the problem-assembly step immediately before the hot path).
//
// The reference rebuilds its whole Ceres problem from the pointer graph twice per backend tick
// (Backend::BuildProblem, src/lvio_fusion/src/backend.cpp:96-183, called from Optimize :206 and UpdateFrontend :261): one
// heap-allocated functor per observation, std::map walks over frames -> features -> landmarks.  Here the window is kept as
// flat host arrays that are updated INCREMENTALLY when the front-end adds a keyframe / landmark / observation or the window
// slides, and the device SoA batches, parameter state and solver work buffers live across ticks (grow-only buffers, no
// hipMalloc / hipFree per tick).  lvf_window_solve assembles the block lists with BuildProblem's rules —
//   feature of frame k, landmark born in k            -> TwoCameraReprojectionError (weight 5 w_k)            :117-125
//   landmark's birth frame older than the window       -> PoseOnlyReprojectionError on landmark->ToWorld()    :126-131
//   otherwise                                          -> TwoFrameReprojectionError(inv_depth, birth, k)      :132-140
//   good_imu frame after a good_imu frame              -> ImuError                                            :143-161
//   no IMU block and < 20 near visual blocks           -> PoseGraphError(last, k, 100, 0) / PoseError(k, 100, 0)  :163-178
// ("near" = !Camera::Far: depth in cam0 <= 50 baselines, include/lvio_fusion/visual/camera.h:38-41) — in frame order, features
// by ascending landmark id (features_left is a std::map keyed by landmark id), uploads them and runs the device LM loop; results
// are read back into the host mirror.
//
// This file is the host side: lvf_window, the mirror's bookkeeping, the C entries and the tick.  The kernels are in window_kernels.hip,
// what the two share (table records, argument blocks) in window_args.hpp.  A tick (lvf_window_solve) is: ensure_objects (state and
// batches, created once); the assembly by ONE of two strategies — assemble_device (resident tables, k_da_*) or assemble_host (the host
// walks the features) — which share every step but the classification (stage_state, imu_pairs / shape_imu_batch, weak_prior /
// shape_prior_batch, ensure_visual / set_visual_counts); configure_problem; the solve with enqueue_read_back riding behind its last
// iteration; apply_read_back into the mirror.  begin_assembly is the one place where a strategy drops what the other left behind.
#include <algorithm>
#include <chrono>
#include <iterator>
#include <map>
#include <unordered_map>
#include "host_se3.hpp"
#include "window_args.hpp"

namespace lvf {
struct alignas(64) LmHot { double right_ob[2]; double pw[3]; int64_t birth_kf; int bpos; int slot; int fixed; int pad; };
static_assert(sizeof(LmHot) == 64, "one cache line per landmark");
}  // namespace lvf

struct lvf_window {
  struct Obs { int64_t lm_id; int lm; double ob[2]; };  // lm = index into lms
  struct Kf {
    int64_t id = 0;
    double pose[7], vel[3] = {0, 0, 0}, ba[3] = {0, 0, 0}, bg[3] = {0, 0, 0};
    double w_visual = 1.0;
    bool good_imu = false, has_pre = false;
    lvf_preint pre;
    unsigned pre_ver = 0;                                // identifies the CONTENT of `pre` (lvf_window::pre_counter at the time it last changed)
    std::vector<Obs> obs;                                // kept sorted by landmark id (BuildProblem's iteration order) lazily
    bool sorted = true;
    bool d_dirty = true;                                 // device-side assembly: the frame's segment of the feature arena is stale
    size_t d_off = 0, d_cap = 0;                         // ... its place there (elements)
    void put(const Obs& o) { if (!obs.empty() && o.lm_id <= obs.back().lm_id) sorted = false; obs.push_back(o); d_dirty = true; }
    void sort_unique() {                                 // std::map semantics: ascending key, a re-inserted key overwrites
      if (sorted) return;
      std::stable_sort(obs.begin(), obs.end(), [](const Obs& a, const Obs& b) { return a.lm_id < b.lm_id; });
      size_t o = 0;
      for (size_t i = 0; i < obs.size(); ++i) {
        if (i + 1 < obs.size() && obs[i + 1].lm_id == obs[i].lm_id) continue;   // keep the last of equal keys
        obs[o++] = obs[i];
      }
      obs.resize(o);
      sorted = true;
    }
  };
  struct Lm {
    int64_t id = 0, birth_kf = 0;
    double left_ob[2], right_ob[2], inv_depth = 0.0;
    bool fixed = false;                                  // birth frame left the window: world point frozen
    double pw[3] = {0, 0, 0};
    bool alive = true;                                  // false: a free entry of `lms` (indices are STABLE: Obs::lm and the device tables keep them)
  };
  lvf_ctx* ctx = nullptr;
  lvf_camera left, right;
  lvf_window_options opt;
  std::vector<Kf> kfs;                                   // active keyframes, oldest first
  std::unordered_map<int64_t, int> kf_index;             // id -> position in kfs
  std::unordered_map<int64_t, std::array<double, 7>> departed;   // poses of frames that left the window (for ToWorld)
  std::vector<Lm> lms;                                   // entries are re-used through lm_free, never moved
  std::vector<int> lm_free;
  // device-side assembly keeps the landmark table RESIDENT: only entries the host changed since the last tick are sent (the solved
  // inverse depths are written into the table by the device itself)
  std::vector<int> lm_dirty; std::vector<uint8_t> lm_dirty_flag; bool lmtab_valid = false;
  void mark_lm(int i) {
    if (lm_dirty_flag.size() <= (size_t)i) lm_dirty_flag.resize((size_t)i + 1 + lm_dirty_flag.size() / 2, 0);
    if (!lm_dirty_flag[i]) { lm_dirty_flag[i] = 1; lm_dirty.push_back(i); }
  }
  int n_lm_live = 0;
  std::unordered_map<int64_t, int> lm_index;
  // device side, persistent across ticks
  lvf_state* st = nullptr;
  lvf_batch *tc = nullptr, *tf = nullptr, *po = nullptr, *imu = nullptr, *prior = nullptr;
  lvf_batch* rej = nullptr;            // PoseOnly batch of the outlier gate (lvf_window_reject_outliers), persistent
  lvf_state* rej_st = nullptr;         // the window's poses with unit visual weights
  lvf::DevBuf<uint8_t> rej_flags;
  // pinned staging for the per-tick block lists (observations / indices per functor type)
  lvf::HostPin<double> h_state;      // poses | vel | ba | bg | w_visual | inv_depth (read-back staging)
  // device-side assembly (opt.device_assembly): resident feature arena + per-tick tables and scratch
  lvf::DevBuf<int32_t> d_obs_lm; lvf::DevBuf<double> d_obs_xy; size_t arena_end = 0;
  lvf::DevBuf<unsigned char> d_lmtab, d_frames, d_cls, d_used;
  lvf::DevBuf<int> d_wgcnt, d_wgbase, d_slot, d_slot_lm, d_counts;
  lvf::DevBuf<double> d_lm_invd_out;
  lvf::HostPin<int> h_counts;
  // ImuError information matrices across ticks: slot f of `sq_prev` holds sqrt_info of the pre-integration version sq_ver[f] (what the
  // previous tick left in the IMU batch); a factor whose version is found there is copied instead of factored again (k_imu_sqrt_info_cached)
  lvf::DevBuf<double> sq_prev; std::vector<unsigned> sq_ver; lvf::DevBuf<int> d_sq_src; unsigned pre_counter = 0; bool sq_valid = false;
  hipEvent_t ev_counts = nullptr;                        // recorded behind the counters' copy: the host waits for it, not for the work queued after it
  std::vector<lvf::LmHot> hot;                           // per-tick compact copy of what the feature walk reads of a landmark
  lvf::HostPin<unsigned char> h_stage;                   // the tick's packed upload (records + plain segments)
  lvf::DevBuf<unsigned char> d_stage;
  lvf_problem* prob = nullptr;
  // LiDAR planes (lvf_window_set_lidar_planes / _set_lidar_scan): one device segment per keyframe id (a batch on keyframe 0), concatenated in
  // active-keyframe order into `lidar` whenever a segment or the keyframes' positions changed; nothing here exists until a segment is set
  std::unordered_map<int64_t, lvf_batch*> lidar_seg;
  lvf_batch* lidar = nullptr;
  bool lidar_dirty = false;
  // assembly of the last solve
  enum class Assembler { none, host, device };
  Assembler assembled_by = Assembler::none;              // who made the block lists that sit in the batches (see begin_assembly)
  std::vector<int> slot_lm;                              // dense landmark slot -> index into lms (host assembly; the device's table is d_slot_lm)
  int n_tc = 0, n_tf = 0, n_po = 0, n_imu = 0, n_prior = 0, n_lm_problem = 0;
  // Dense prior (lvf_window_set_dense_prior, lvf_window_slide_marginalize): kept on the host by keyframe id; `dprior` is its device copy by
  // keyframe position, refreshed when the prior or the positions change and attached to the problem by every configure
  std::vector<int64_t> dp_ids; std::vector<double> dp_x0, dp_info, dp_eta; double dp_c0 = 0.0;
  std::vector<int32_t> dp_pos;                           // the positions `dprior` was last filled with (empty: stale)
  lvf_dense_prior* dprior = nullptr;
  // The sub-problem of the marginalising slide: a second persistent window over the departing keyframes and the first kept one, re-filled
  // by every lvf_window_slide_marginalize (its device objects are grow-only like this window's).  In it the last keyframe gets no
  // weak-constraint prior (is_sub) and the lidar segments are borrowed from this window.
  lvf_window* sub = nullptr;
  bool is_sub = false;
  ~lvf_window() {
    if (sub) { sub->lidar_seg.clear(); delete sub; }
    if (prob) lvf_problem_destroy(prob);
    if (dprior) lvf_dense_prior_destroy(dprior);
    for (lvf_batch* b : {tc, tf, po, imu, prior, rej, lidar}) if (b) lvf_batch_destroy(b);
    for (auto& kv : lidar_seg) lvf_batch_destroy(kv.second);
    if (st) lvf_state_destroy(st);
    if (rej_st) lvf_state_destroy(rej_st);
    if (ev_counts) (void)hipEventDestroy(ev_counts);
  }
};

namespace lvf {

// the TwoCamera block weight as the reference forms it (backend.cpp:123: `5 * frame->weights.visual`, float arithmetic: adapt/weights.h:10)
static inline double two_camera_weight(double w_visual) { return (double)(5.0f * (float)w_visual); }

// Landmark::ToWorld (src/lvio_fusion/src/landmark.cpp:15-19): Pixel2Robot through the RIGHT camera, then the birth pose
static void to_world(const lvf_camera& right, const double rob[2], double inv_depth, const double birth_pose[7], double pw[3]) {
  const double d = 1.0 / inv_depth;
  const double ps[3] = {(rob[0] - right.cx) * d / right.fx, (rob[1] - right.cy) * d / right.fy, d};
  double pb[3], r[3];
  hse3::rotate(right.extrinsic, ps, pb);
  for (int k = 0; k < 3; ++k) pb[k] += right.extrinsic[4 + k];
  hse3::rotate(birth_pose, pb, r);
  for (int k = 0; k < 3; ++k) pw[k] = r[k] + birth_pose[4 + k];
}

// Keeps the host mirror bounded over a long run (the reference removes a landmark once its last observation is gone:
// Landmark::RemoveObservation / Map::RemoveLandmark): landmarks no active keyframe observes any more are dropped and Obs::lm is
// re-indexed; poses of departed frames are kept only while a live landmark was born there.
static void prune(lvf_window* w) {
  const size_t nl = w->lms.size();
  std::vector<char> seen(nl, 0);
  for (const lvf_window::Kf& f : w->kfs)
    for (const lvf_window::Obs& o : f.obs) seen[o.lm] = 1;
  for (size_t i = 0; i < nl; ++i) {
    lvf_window::Lm& l = w->lms[i];
    if (l.alive && !seen[i]) {                 // the entry becomes free; nothing is moved, so every index held elsewhere stays valid
      w->lm_index.erase(l.id);
      l.alive = false; l.fixed = false;
      w->mark_lm((int)i);
      w->lm_free.push_back((int)i);
      --w->n_lm_live;
    }
  }
  if (!w->departed.empty()) {
    std::unordered_map<int64_t, char> anchor;
    for (const lvf_window::Lm& l : w->lms) if (l.alive) anchor[l.birth_kf] = 1;
    for (auto it = w->departed.begin(); it != w->departed.end();) it = anchor.count(it->first) ? std::next(it) : w->departed.erase(it);
  }
}

// the rotation of a unit quaternion, row-major
static void rot_of(const double q[4], double R[9]) {
  double e0[3] = {1, 0, 0}, e1[3] = {0, 1, 0}, e2[3] = {0, 0, 1}, c0[3], c1[3], c2[3];
  hse3::rotate(q, e0, c0); hse3::rotate(q, e1, c1); hse3::rotate(q, e2, c2);
  R[0] = c0[0]; R[1] = c1[0]; R[2] = c2[0]; R[3] = c0[1]; R[4] = c1[1]; R[5] = c2[1]; R[6] = c0[2]; R[7] = c1[2]; R[8] = c2[2];
}
// Rk[9 k] = rotation of keyframe k, Rk[9 n_kf] = rotation of the right camera's extrinsic: the matrices both landmarks_to_world and the
// device-side assembly (FrameDev::R, DaArgs::Re) multiply with
static void landmarks_to_world_prepare(const lvf_window* w, double* Rk) {
  const int n_kf = (int)w->kfs.size();
  for (int k = 0; k < n_kf; ++k) rot_of(w->kfs[k].pose, Rk + (size_t)9 * k);
  rot_of(w->right.extrinsic, Rk + (size_t)9 * n_kf);
}
// landmark->ToWorld() (src/lvio_fusion/src/landmark.cpp:15-19) for every landmark of the mirror: frozen points as stored, live ones
// from their birth keyframe's CURRENT pose and inverse depth.  lm_birth_pos[i] = position of the birth keyframe in kfs (-1: not active).
static void landmarks_to_world(const lvf_window* w, std::vector<double>& lm_pw, std::vector<int>& lm_birth_pos) {
  const int n_kf = (int)w->kfs.size();
  std::vector<double> Rk((size_t)9 * n_kf + 9);
  landmarks_to_world_prepare(w, Rk.data());
  const double* Re = &Rk[(size_t)9 * n_kf];
  const double* te = w->right.extrinsic + 4;
  const size_t nl = w->lms.size();
  lm_pw.assign((size_t)3 * nl, 0.0);
  lm_birth_pos.assign(nl, -1);
  const int64_t first_id = w->kfs.front().id;
  std::vector<int64_t> ids(n_kf);                          // ascending: lvf_window_add_keyframe only accepts increasing ids
  for (int k = 0; k < n_kf; ++k) ids[k] = w->kfs[k].id;
  for (size_t i = 0; i < nl; ++i) {
    const lvf_window::Lm& l = w->lms[i];
    if (!l.alive) continue;
    if (l.fixed) { std::memcpy(&lm_pw[3 * i], l.pw, 24); continue; }
    if (l.birth_kf < first_id) continue;
    // position of the birth frame: the window's ids ascend, so a binary search over <= a few dozen ids (a hash lookup per landmark
    // was most of this function: 10 k lookups per tick)
    const int64_t* ib = std::lower_bound(ids.data(), ids.data() + n_kf, l.birth_kf);
    if (ib == ids.data() + n_kf || *ib != l.birth_kf) continue;
    const int bp = (int)(ib - ids.data());
    lm_birth_pos[i] = bp;
    const double d = 1.0 / l.inv_depth;
    const double ps[3] = {(l.right_ob[0] - w->right.cx) * d / w->right.fx, (l.right_ob[1] - w->right.cy) * d / w->right.fy, d};
    const double pb[3] = {Re[0] * ps[0] + Re[1] * ps[1] + Re[2] * ps[2] + te[0], Re[3] * ps[0] + Re[4] * ps[1] + Re[5] * ps[2] + te[1],
                          Re[6] * ps[0] + Re[7] * ps[1] + Re[8] * ps[2] + te[2]};
    const double* R = &Rk[(size_t)9 * bp];
    const double* t = w->kfs[bp].pose + 4;
    lm_pw[3 * i] = R[0] * pb[0] + R[1] * pb[1] + R[2] * pb[2] + t[0];
    lm_pw[3 * i + 1] = R[3] * pb[0] + R[4] * pb[1] + R[5] * pb[2] + t[1];
    lm_pw[3 * i + 2] = R[6] * pb[0] + R[7] * pb[1] + R[8] * pb[2] + t[2];
  }
}

// What the per-feature walk of lvf_window_solve needs of a landmark, in ONE cache line (the walk is bound by its random accesses:
// through Lm + two side arrays it touched four lines per feature)
static void landmarks_hot(const lvf_window* w, std::vector<LmHot>& hot) {
  std::vector<double> lm_pw;
  std::vector<int> lm_birth_pos;
  landmarks_to_world(w, lm_pw, lm_birth_pos);
  const size_t nl = w->lms.size();
  hot.resize(nl);
  for (size_t i = 0; i < nl; ++i) {
    const lvf_window::Lm& l = w->lms[i];
    LmHot& h = hot[i];
    h.right_ob[0] = l.right_ob[0]; h.right_ob[1] = l.right_ob[1]; h.pw[0] = lm_pw[3 * i]; h.pw[1] = lm_pw[3 * i + 1]; h.pw[2] = lm_pw[3 * i + 2];
    h.birth_kf = l.birth_kf; h.bpos = lm_birth_pos[i]; h.slot = -1; h.fixed = l.fixed ? 1 : 0; h.pad = 0;
  }
}


}  // namespace lvf

using namespace lvf;

extern "C" {

void lvf_window_options_default(lvf_window_options* o) {
  if (!o) return;
  o->baseline = 0.537;                 // |t_cam1 - t_cam0| of the KITTI rig (config/kitti.yaml); Camera::baseline
  o->weak_visual_threshold = 20;       // backend.cpp:166
  o->prior_weight = 100.0; o->prior_v = 0.0;   // backend.cpp:170,175
  o->device_assembly = 1;
}

int lvf_window_create(lvf_ctx* ctx, const lvf_camera* left, const lvf_camera* right, const lvf_window_options* opt, lvf_window** out) {
  LVF_REQUIRE(ctx && left && right && out, "lvf_window_create: null argument");
  auto* w = new lvf_window();
  w->ctx = ctx; w->left = *left; w->right = *right;
  if (opt) w->opt = *opt; else lvf_window_options_default(&w->opt);
  *out = w;
  return LVF_OK;
}
int lvf_window_destroy(lvf_window* w) { delete w; return LVF_OK; }

int lvf_window_add_keyframe(lvf_window* w, int64_t kf_id, const double* pose7, double w_visual) {
  LVF_REQUIRE(w && pose7, "lvf_window_add_keyframe: null argument");
  LVF_REQUIRE(w->kfs.empty() || kf_id > w->kfs.back().id, "lvf_window_add_keyframe: keyframe ids must increase (got %lld after %lld)", (long long)kf_id,
              (long long)(w->kfs.empty() ? 0 : w->kfs.back().id));
  lvf_window::Kf k;
  k.id = kf_id; std::memcpy(k.pose, pose7, 56); k.w_visual = w_visual;
  w->kf_index[kf_id] = (int)w->kfs.size();
  w->kfs.push_back(std::move(k));
  return LVF_OK;
}
int lvf_window_set_imu(lvf_window* w, int64_t kf_id, const double* vel3, const double* ba3, const double* bg3, const lvf_preint* pre) {
  LVF_REQUIRE(w && vel3 && ba3 && bg3, "lvf_window_set_imu: null argument");
  auto it = w->kf_index.find(kf_id);
  LVF_REQUIRE(it != w->kf_index.end(), "lvf_window_set_imu: keyframe %lld is not in the window", (long long)kf_id);
  lvf_window::Kf& k = w->kfs[it->second];
  std::memcpy(k.vel, vel3, 24); std::memcpy(k.ba, ba3, 24); std::memcpy(k.bg, bg3, 24);
  const bool had = k.has_pre;
  k.good_imu = true; k.has_pre = pre != nullptr;
  if (pre && !(had && std::memcmp(&k.pre, pre, sizeof(lvf_preint)) == 0)) { k.pre = *pre; k.pre_ver = ++w->pre_counter; }      // (an unchanged pre-integration keeps its cached matrix)
  return LVF_OK;
}
int lvf_window_add_landmark(lvf_window* w, int64_t lm_id, int64_t birth_kf_id, const double* left_ob2, const double* right_ob2, double inv_depth) {
  LVF_REQUIRE(w && left_ob2 && right_ob2, "lvf_window_add_landmark: null argument");
  LVF_REQUIRE(!w->lm_index.count(lm_id), "lvf_window_add_landmark: landmark %lld exists", (long long)lm_id);
  auto it = w->kf_index.find(birth_kf_id);
  LVF_REQUIRE(it != w->kf_index.end(), "lvf_window_add_landmark: birth keyframe %lld is not in the window", (long long)birth_kf_id);
  LVF_REQUIRE(inv_depth != 0.0, "lvf_window_add_landmark: zero inverse depth");
  lvf_window::Lm l;
  l.id = lm_id; l.birth_kf = birth_kf_id; l.inv_depth = inv_depth;
  std::memcpy(l.left_ob, left_ob2, 16); std::memcpy(l.right_ob, right_ob2, 16);
  int idx;
  if (!w->lm_free.empty()) { idx = w->lm_free.back(); w->lm_free.pop_back(); w->lms[idx] = l; }
  else { idx = (int)w->lms.size(); w->lms.push_back(l); }
  w->mark_lm(idx);
  w->lm_index[lm_id] = idx;
  ++w->n_lm_live;
  // the landmark's own left feature in its birth frame (features_left[lm] of the first frame -> the TwoCamera block)
  lvf_window::Obs o; o.lm_id = lm_id; o.lm = idx; o.ob[0] = left_ob2[0]; o.ob[1] = left_ob2[1];
  w->kfs[it->second].put(o);
  return LVF_OK;
}
int lvf_window_add_observation(lvf_window* w, int64_t lm_id, int64_t kf_id, const double* ob2) {
  LVF_REQUIRE(w && ob2, "lvf_window_add_observation: null argument");
  auto il = w->lm_index.find(lm_id);
  LVF_REQUIRE(il != w->lm_index.end(), "lvf_window_add_observation: unknown landmark %lld", (long long)lm_id);
  auto ik = w->kf_index.find(kf_id);
  LVF_REQUIRE(ik != w->kf_index.end(), "lvf_window_add_observation: keyframe %lld is not in the window", (long long)kf_id);
  LVF_REQUIRE(w->lms[il->second].birth_kf < kf_id, "lvf_window_add_observation: observation in or before the birth frame");
  lvf_window::Obs o; o.lm_id = lm_id; o.lm = il->second; o.ob[0] = ob2[0]; o.ob[1] = ob2[1];
  w->kfs[ik->second].put(o);
  return LVF_OK;
}
int lvf_window_remove_observation(lvf_window* w, int64_t lm_id, int64_t kf_id) {
  LVF_REQUIRE(w, "lvf_window_remove_observation: null window");
  auto ik = w->kf_index.find(kf_id);
  LVF_REQUIRE(ik != w->kf_index.end(), "lvf_window_remove_observation: keyframe %lld is not in the window", (long long)kf_id);
  auto& v = w->kfs[ik->second].obs;
  v.erase(std::remove_if(v.begin(), v.end(), [&](const lvf_window::Obs& o) { return o.lm_id == lm_id; }), v.end());
  w->kfs[ik->second].d_dirty = true;
  return LVF_OK;
}

// Map::GetKeyFrames(finished) (src/map.cpp:49-55): frames older than first_active_kf_id leave the problem.  Landmarks born in a
// departing frame keep their world point at the departing frame's final pose and their last inverse depth (they become
// PoseOnly blocks, backend.cpp:126-131).
int lvf_window_slide(lvf_window* w, int64_t first_active_kf_id) {
  LVF_REQUIRE(w, "lvf_window_slide: null window");
  size_t drop = 0;
  while (drop < w->kfs.size() && w->kfs[drop].id < first_active_kf_id) ++drop;
  if (drop == 0) return LVF_OK;
  for (size_t k = 0; k < drop; ++k) {
    std::array<double, 7> p;
    std::memcpy(p.data(), w->kfs[k].pose, 56);
    w->departed[w->kfs[k].id] = p;
  }
  for (size_t i = 0; i < w->lms.size(); ++i) {
    lvf_window::Lm& l = w->lms[i];
    if (l.alive && !l.fixed && l.birth_kf < first_active_kf_id) {
      auto it = w->departed.find(l.birth_kf);
      if (it != w->departed.end()) { to_world(w->right, l.right_ob, l.inv_depth, it->second.data(), l.pw); l.fixed = true; w->mark_lm((int)i); }
    }
  }
  for (size_t k = 0; k < drop; ++k) {
    auto is = w->lidar_seg.find(w->kfs[k].id);
    if (is != w->lidar_seg.end()) { lvf_batch_destroy(is->second); w->lidar_seg.erase(is); }
  }
  if (w->lidar) w->lidar_dirty = true;                     // (the positions of the keyframes that stay have changed)
  for (int64_t id : w->dp_ids)
    if (id < first_active_kf_id) { w->dp_ids.clear(); w->dp_pos.clear(); break; }      // a dense prior whose keyframe leaves is dropped
  w->kfs.erase(w->kfs.begin(), w->kfs.begin() + drop);
  w->kf_index.clear();
  for (size_t k = 0; k < w->kfs.size(); ++k) w->kf_index[w->kfs[k].id] = (int)k;
  prune(w);
  return LVF_OK;
}

int lvf_window_set_pose(lvf_window* w, int64_t kf_id, const double* pose7) {
  LVF_REQUIRE(w && pose7, "lvf_window_set_pose: null argument");
  auto ik = w->kf_index.find(kf_id);
  LVF_REQUIRE(ik != w->kf_index.end(), "lvf_window_set_pose: keyframe %lld is not in the window", (long long)kf_id);
  std::memcpy(w->kfs[ik->second].pose, pose7, 56);
  return LVF_OK;
}
int lvf_window_get_pose(const lvf_window* w, int64_t kf_id, double* pose7) {
  LVF_REQUIRE(w && pose7, "lvf_window_get_pose: null argument");
  auto ik = w->kf_index.find(kf_id);
  if (ik != w->kf_index.end()) { std::memcpy(pose7, w->kfs[ik->second].pose, 56); return LVF_OK; }
  auto id = w->departed.find(kf_id);
  LVF_REQUIRE(id != w->departed.end(), "lvf_window_get_pose: unknown keyframe %lld", (long long)kf_id);
  std::memcpy(pose7, id->second.data(), 56);
  return LVF_OK;
}
int lvf_window_get_imu(const lvf_window* w, int64_t kf_id, double* vel3, double* ba3, double* bg3) {
  LVF_REQUIRE(w, "lvf_window_get_imu: null window");
  auto ik = w->kf_index.find(kf_id);
  LVF_REQUIRE(ik != w->kf_index.end(), "lvf_window_get_imu: keyframe %lld is not in the window", (long long)kf_id);
  const lvf_window::Kf& k = w->kfs[ik->second];
  if (vel3) std::memcpy(vel3, k.vel, 24);
  if (ba3) std::memcpy(ba3, k.ba, 24);
  if (bg3) std::memcpy(bg3, k.bg, 24);
  return LVF_OK;
}
int lvf_window_get_inv_depth(const lvf_window* w, int64_t lm_id, double* inv_depth) {
  LVF_REQUIRE(w && inv_depth, "lvf_window_get_inv_depth: null argument");
  auto il = w->lm_index.find(lm_id);
  LVF_REQUIRE(il != w->lm_index.end(), "lvf_window_get_inv_depth: unknown landmark %lld", (long long)lm_id);
  *inv_depth = w->lms[il->second].inv_depth;
  return LVF_OK;
}
static int window_put_lidar_segment(lvf_window* w, int64_t kf_id, lvf_batch* seg) {
  auto is = w->lidar_seg.find(kf_id);
  if (is != w->lidar_seg.end()) { lvf_batch_destroy(is->second); w->lidar_seg.erase(is); }
  if (seg && seg->n) w->lidar_seg[kf_id] = seg; else if (seg) lvf_batch_destroy(seg);
  w->lidar_dirty = true;
  return LVF_OK;
}
int lvf_window_set_lidar_planes(lvf_window* w, int64_t kf_id, int n, const double* p, const double* pa, const double* pb, const double* pc, const double* weight,
                                const double* huber_a) {
  LVF_REQUIRE(w, "lvf_window_set_lidar_planes: null window");
  LVF_REQUIRE(w->kf_index.count(kf_id), "lvf_window_set_lidar_planes: keyframe %lld is not in the window", (long long)kf_id);
  LVF_REQUIRE(n >= 0, "lvf_window_set_lidar_planes: negative size");
  lvf_batch* seg = nullptr;
  if (n > 0) {
    const std::vector<int32_t> kf((size_t)n, 0);
    LVF_TRY(lvf_lidar_pose_create(w->ctx, n, p, pa, pb, pc, kf.data(), weight, huber_a, &seg));
  }
  return window_put_lidar_segment(w, kf_id, seg);
}
int lvf_window_set_lidar_scan(lvf_window* w, int64_t kf_id, lvf_map* map, lvf_scan* scan, double weight, double huber_a) {
  LVF_REQUIRE(w && map && scan, "lvf_window_set_lidar_scan: null argument");
  LVF_REQUIRE(w->kf_index.count(kf_id), "lvf_window_set_lidar_scan: keyframe %lld is not in the window", (long long)kf_id);
  const int32_t kf = 0;
  lvf_batch* seg = nullptr;
  LVF_TRY(lvf_lidar_pose_from_scans(w->ctx, 1, &map, &scan, &kf, &weight, &huber_a, &seg));
  return window_put_lidar_segment(w, kf_id, seg);
}
/* lidar plane blocks the window holds for its active keyframes (zero-weight blocks of failed queries included) */
int lvf_window_lidar_count(const lvf_window* w, int32_t* n) {
  LVF_REQUIRE(w && n, "lvf_window_lidar_count: null argument");
  long long total = 0;
  for (const auto& kv : w->lidar_seg) total += kv.second->n;
  *n = (int32_t)total;
  return LVF_OK;
}
int lvf_window_counts(const lvf_window* w, int32_t* counts8) {
  LVF_REQUIRE(w && counts8, "lvf_window_counts: null argument");
  counts8[0] = (int)w->kfs.size(); counts8[1] = w->n_lm_problem; counts8[2] = w->n_tc; counts8[3] = w->n_tf; counts8[4] = w->n_po;
  counts8[5] = w->n_imu; counts8[6] = w->n_prior; counts8[7] = w->n_lm_live;
  return LVF_OK;
}

}  // extern "C"

// ================================================================================================ the tick (lvf_window_solve)
namespace lvf { int lidar_pose_assemble(lvf_ctx* ctx, int n_kf, lvf_batch* const* seg, lvf_batch** dst); }      // solver_lidar.hip
// the window's lidar planes -> its problem, behind the assembly of the other blocks (a window that never had a segment does nothing here)
static int window_attach_lidar(lvf_window* w) {
  if (!w->lidar && !w->lidar_dirty) return LVF_OK;
  if (w->lidar_dirty) {
    std::vector<lvf_batch*> seg(w->kfs.size(), nullptr);
    for (size_t k = 0; k < w->kfs.size(); ++k) {
      auto is = w->lidar_seg.find(w->kfs[k].id);
      if (is != w->lidar_seg.end()) seg[k] = is->second;
    }
    LVF_TRY(lvf::lidar_pose_assemble(w->ctx, (int)seg.size(), seg.data(), &w->lidar));
    w->lidar_dirty = false;
  }
  return lvf_problem_set_lidar_planes(w->prob, w->lidar->n ? w->lidar : nullptr);
}

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static bool window_timing() { static const bool on = getenv("LVF_WINDOW_TIMING") != nullptr; return on; }

// every segment of a staging block starts on a 16-byte boundary: k_window_unpack / k_window_pack copy 16-byte words (and every destination
// has two spare elements for the last word)
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Writes a tick's upload into the pinned staging block from `start` on and builds the UnpackArgs that distribute it on the device.
struct StageWriter {
  unsigned char* base; size_t cap, cur; UnpackArgs ua{}; bool overflow = false;
  StageWriter(const HostPin<unsigned char>& h, size_t start) : base(h.p), cap(h.cap), cur(start) {}
  // room that no plain segment describes (the landmark table's dirty records); *off = its place in the block
  unsigned char* raw(size_t bytes, size_t* off) { *off = cur; cur += up16(bytes); return base + *off; }
  // `bytes` that k_window_unpack copies to `dst`; returns where the host writes them
  unsigned char* seg(void* dst, size_t bytes) {
    size_t off;
    unsigned char* at = raw(bytes, &off);
    if (bytes && ua.n_segs == kMaxSegs) overflow = true;
    else if (bytes) { ua.seg_dst[ua.n_segs] = static_cast<unsigned char*>(dst); ua.seg_off[ua.n_segs] = off; ua.seg_words[ua.n_segs] = (unsigned)((bytes + 15) / 16); ++ua.n_segs; }
    return at;
  }
  template <typename T> T* seg_of(T* dst, size_t count) { return reinterpret_cast<T*>(seg(dst, count * sizeof(T))); }
  template <typename T> void put(T* dst, const std::vector<T>& v) { if (!v.empty()) std::memcpy(seg(dst, v.size() * sizeof(T)), v.data(), v.size() * sizeof(T)); }
  bool fits() const { return !overflow && cur <= cap; }
};
// the read-back's counterpart over PackArgs: device arrays -> one staging block; seg returns the segment's place in it
struct PackWriter {
  PackArgs pa{}; size_t cur = 0;
  size_t seg(const void* src, size_t bytes) {
    const size_t off = cur;
    if (bytes) { pa.src[pa.n_segs] = static_cast<const unsigned char*>(src); pa.off[pa.n_segs] = off; pa.words[pa.n_segs] = (unsigned)((bytes + 15) / 16); ++pa.n_segs; }
    cur += up16(bytes);
    return off;
  }
};

// The one row of the world -> cam0 transform of a frame that Camera::Far needs:
// z_cam(pw) = zrow . pw + zoff  with  pc = R_e^-1 (R_wc^-1 pw + t_inv) + t_e_inv   (inv_e: the inverse of the left camera's extrinsic)
static void frame_far_row(const double inv_e[7], const double pose[7], double zrow[3], double* zoff) {
  double inv_pose[7];
  hse3::inv(pose, inv_pose);
  double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1}, c0[3], c1[3], c2[3], t[3], r[3];
  hse3::rotate(inv_pose, ex, r); hse3::rotate(inv_e, r, c0);
  hse3::rotate(inv_pose, ey, r); hse3::rotate(inv_e, r, c1);
  hse3::rotate(inv_pose, ez, r); hse3::rotate(inv_e, r, c2);
  zrow[0] = c0[2]; zrow[1] = c1[2]; zrow[2] = c2[2];
  hse3::rotate(inv_e, inv_pose + 4, t);
  *zoff = t[2] + inv_e[6];
}

// ---- steps both assembly strategies take

// persistent device objects: created once (empty), re-filled every tick through grow-only buffers
static int ensure_objects(lvf_window* w) {
  if (w->st) return LVF_OK;
  lvf_ctx* ctx = w->ctx;
  LVF_TRY(lvf_state_create(ctx, 0, 0, &w->st));
  const double z2[2] = {0, 0}; const int32_t z = 0; const double id7[7] = {0, 0, 0, 1, 0, 0, 0};
  LVF_TRY(lvf_two_camera_create(ctx, &w->left, &w->right, 0, z2, z2, &z, &z, &w->tc));
  LVF_TRY(lvf_two_frame_create(ctx, &w->left, &w->right, 0, z2, z2, &z, &z, &z, &w->tf));
  LVF_TRY(lvf_pose_only_create(ctx, &w->left, 0, z2, &z, &z, 0, id7, &w->po));
  LVF_TRY(lvf_imu_create(ctx, 0, nullptr, nullptr, nullptr, &w->imu));
  LVF_TRY(lvf_pose_prior_create(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &w->prior));
  return LVF_OK;
}

// The hand-over between the strategies.  A window made for device assembly takes the host walk while it holds more than kDaMaxKf
// keyframes and comes back when it has slid below, so each strategy may find the other's residue:
//   device -> host : the resident landmark table misses the inverse depths this tick solves and the changes the host walk does not
//                    track, and the cached ImuError information matrices (sq_prev / sq_ver) describe a batch this tick overwrites
//   host -> device : the host's slot table (lvf_window_debug_blocks then reads the device's, d_slot_lm)
// The feature arena needs nothing: Kf::d_dirty is kept by the mirror's entries whichever strategy runs.
static void begin_assembly(lvf_window* w, lvf_window::Assembler by) {
  if (by == lvf_window::Assembler::host) { w->lmtab_valid = false; w->sq_valid = false; }
  else w->slot_lm.clear();
  w->assembled_by = by;
}

// poses | vel | ba | bg | w_visual of the mirror -> the state, by keyframe position.  The inverse depths go by dense landmark slot, which only
// the assembly knows: the state gets room for `inv_depth_capacity` of them and the caller fills them.
static int stage_state(lvf_window* w, StageWriter& sw, size_t inv_depth_capacity) {
  lvf_state* st = w->st;
  const size_t n_kf = w->kfs.size();
  st->n_kf = (int)n_kf;
  LVF_TRY(st->poses.ensure(7 * n_kf + 2)); LVF_TRY(st->vel.ensure(3 * n_kf + 2)); LVF_TRY(st->ba.ensure(3 * n_kf + 2)); LVF_TRY(st->bg.ensure(3 * n_kf + 2));
  LVF_TRY(st->w_visual.ensure(n_kf + 2)); LVF_TRY(st->inv_depth.ensure(inv_depth_capacity + 2));
  st->poses.n = 7 * n_kf; st->vel.n = st->ba.n = st->bg.n = 3 * n_kf; st->w_visual.n = n_kf;
  double *sp = sw.seg_of(st->poses.p, 7 * n_kf), *sv = sw.seg_of(st->vel.p, 3 * n_kf), *sa = sw.seg_of(st->ba.p, 3 * n_kf), *sg = sw.seg_of(st->bg.p, 3 * n_kf),
         *sv_w = sw.seg_of(st->w_visual.p, n_kf);
  for (size_t k = 0; k < n_kf; ++k) {
    const lvf_window::Kf& f = w->kfs[k];
    std::memcpy(&sp[7 * k], f.pose, 56); std::memcpy(&sv[3 * k], f.vel, 24); std::memcpy(&sa[3 * k], f.ba, 24); std::memcpy(&sg[3 * k], f.bg, 24);
    sv_w[k] = f.w_visual;
  }
  return LVF_OK;
}

// ImuError blocks (backend.cpp:141-153): both frames good, a pre-integration on the later one.  j ascends.
static void imu_pairs(const lvf_window* w, std::vector<int32_t>& i, std::vector<int32_t>& j) {
  for (int k = 1; k < (int)w->kfs.size(); ++k)
    if (w->kfs[k].good_imu && w->kfs[k - 1].good_imu && w->kfs[k].has_pre) { i.push_back(k - 1); j.push_back(k); }
}
// the IMU batch for these pairs: sizes, and the pre-integrations and indices into the upload.  The information matrices are the caller's
// launch (launch_imu_sqrt_info, or the cached form behind imu_cache_sources).
static int shape_imu_batch(lvf_window* w, StageWriter& sw, const std::vector<int32_t>& imu_i, const std::vector<int32_t>& imu_j) {
  static_assert(sizeof(lvf_preint) == 467 * 8, "lvf_preint is 467 doubles");
  lvf_batch* b = w->imu;
  const size_t ni = imu_j.size();
  LVF_TRY(b->pre.ensure(467 * ni + 2)); LVF_TRY(b->idx_a.ensure(ni + 4)); LVF_TRY(b->idx_b.ensure(ni + 4));
  b->pre.n = 467 * ni; b->idx_a.n = b->idx_b.n = ni;
  if (ni) {
    lvf_preint* dst = reinterpret_cast<lvf_preint*>(sw.seg(b->pre.p, 467 * ni * 8));
    for (size_t f = 0; f < ni; ++f) dst[f] = w->kfs[imu_j[f]].pre;
    sw.put(b->idx_a.p, imu_i); sw.put(b->idx_b.p, imu_j);
  }
  b->host_kf1 = imu_i; b->host_kf2 = imu_j;
  LVF_TRY(b->sqrt_info.ensure((size_t)225 * ni)); LVF_TRY(b->res.ensure((size_t)15 * ni));
  for (int q = 0; q < 8; ++q) LVF_TRY(b->jac[q].ensure((size_t)15 * b->block_size[q] * ni));
  b->n = (int)ni; b->min_n_kf = (int)w->kfs.size(); b->min_n_lm = 0; b->evaluated = false;
  w->n_imu = (int)ni;
  return LVF_OK;
}

// Weak-constraint priors (backend.cpp:163-178): a frame without an ImuError block whose near visual blocks (!Camera::Far) number fewer than
// the threshold gets PoseGraphError(previous, k, weight, v), the first frame PoseError(k, weight, v).
struct PriorLists { std::vector<double> t, wt, v; std::vector<int32_t> a, b; };
static int weak_prior(const lvf_window* w, int k, bool has_imu_block, int near_count, PriorLists& pl) {
  if (has_imu_block || near_count >= w->opt.weak_visual_threshold) return LVF_OK;
  if (w->is_sub && k + 1 == (int)w->kfs.size()) return LVF_OK;      // the first kept keyframe of a marginalising slide: no prior of its own
  const lvf_window::Kf& f = w->kfs[k];
  double t7[7] = {0, 0, 0, 0, 0, 0, 0};
  if (k > 0) { LVF_TRY(lvf_relative_rpyxyz(w->kfs[k - 1].pose, f.pose, t7)); pl.a.push_back(k - 1); }
  else { std::memcpy(t7, f.pose, 56); pl.a.push_back(-1); }
  pl.b.push_back(k); pl.t.insert(pl.t.end(), t7, t7 + 7); pl.wt.push_back(w->opt.prior_weight); pl.v.push_back(w->opt.prior_v);
  return LVF_OK;
}
static int shape_prior_batch(lvf_window* w, StageWriter& sw, const PriorLists& pl) {
  lvf_batch* b = w->prior;
  const size_t np_ = pl.b.size();
  LVF_TRY(b->idx_a.ensure(np_ + 4)); LVF_TRY(b->idx_b.ensure(np_ + 4)); LVF_TRY(b->table.ensure(7 * np_ + 2)); LVF_TRY(b->ob_a.ensure(np_ + 2)); LVF_TRY(b->ob_b.ensure(np_ + 2));
  b->idx_a.n = b->idx_b.n = np_; b->table.n = 7 * np_; b->ob_a.n = b->ob_b.n = np_;
  sw.put(b->idx_a.p, pl.a); sw.put(b->idx_b.p, pl.b); sw.put(b->table.p, pl.t); sw.put(b->ob_a.p, pl.wt); sw.put(b->ob_b.p, pl.v);
  LVF_TRY(b->res.ensure(6 * np_)); LVF_TRY(b->jac[0].ensure(42 * np_)); LVF_TRY(b->jac[1].ensure(42 * np_));
  b->n = (int)np_; b->min_n_kf = (int)w->kfs.size(); b->min_n_lm = 0; b->evaluated = false;
  b->host_kf1 = pl.a; b->host_kf2 = pl.b;
  w->n_prior = (int)np_;
  return LVF_OK;
}

// room in the three visual batches (the device strategy asks for upper bounds ahead of its counters, the host walk for what it counted)
static int ensure_visual(lvf_window* w, size_t cap_tc, size_t cap_tf, size_t cap_po) {
  lvf_batch *tc = w->tc, *tf = w->tf, *po = w->po;
  LVF_TRY(tc->ob_a.ensure(2 * cap_tc + 2)); LVF_TRY(tc->ob_b.ensure(2 * cap_tc + 2)); LVF_TRY(tc->idx_a.ensure(cap_tc + 2)); LVF_TRY(tc->idx_b.ensure(cap_tc + 2)); LVF_TRY(tc->wblk.ensure(cap_tc + 2));
  LVF_TRY(tf->ob_a.ensure(2 * cap_tf + 2)); LVF_TRY(tf->ob_b.ensure(2 * cap_tf + 2)); LVF_TRY(tf->idx_a.ensure(cap_tf + 2)); LVF_TRY(tf->idx_b.ensure(cap_tf + 2)); LVF_TRY(tf->idx_c.ensure(cap_tf + 2));
  LVF_TRY(po->ob_a.ensure(2 * cap_po + 2)); LVF_TRY(po->idx_a.ensure(cap_po + 2)); LVF_TRY(po->idx_b.ensure(cap_po + 2)); LVF_TRY(po->table.ensure(3 * cap_po + 2));
  return LVF_OK;
}
// what this tick's assembly came to: element counts and flags of the visual batches, the state's landmarks, the window's counters.
// Kf::sort_unique keeps one observation per (keyframe, landmark) and both strategies emit frame by frame: TwoFrame and PoseOnly are sorted
// by current keyframe, kf2_counts[k] = TwoFrame blocks of keyframe k.
static void set_visual_counts(lvf_window* w, size_t ntc, size_t ntf, size_t npo, int n_lm, std::vector<int32_t>&& kf2_counts) {
  const int n_kf = (int)w->kfs.size();
  lvf_batch *tc = w->tc, *tf = w->tf, *po = w->po;
  auto shape = [n_kf](lvf_batch* b, size_t n, int nlm) { b->n = (int)n; b->min_n_kf = n_kf; b->min_n_lm = nlm; b->evaluated = false; };
  w->n_lm_problem = n_lm; w->n_tc = (int)ntc; w->n_tf = (int)ntf; w->n_po = (int)npo;
  w->st->n_lm = n_lm; w->st->inv_depth.n = n_lm;
  tc->ob_a.n = tc->ob_b.n = 2 * ntc; tc->idx_a.n = tc->idx_b.n = tc->wblk.n = ntc;
  shape(tc, ntc, n_lm);
  tf->ob_a.n = tf->ob_b.n = 2 * ntf; tf->idx_a.n = tf->idx_b.n = tf->idx_c.n = ntf;
  shape(tf, ntf, n_lm);
  tf->sorted_by_kf = true; tf->host_kf1.clear(); tf->host_kf2.clear(); tf->host_lm.clear(); tf->unique_lk2_known = true; tf->kf2_counts = std::move(kf2_counts);
  po->ob_a.n = 2 * npo; po->idx_a.n = po->idx_b.n = npo; po->table.n = 3 * npo;
  shape(po, npo, 0); po->n_table = (int)npo; po->sorted_by_kf = true;
}

namespace lvf { int dense_prior_assign(lvf_ctx* ctx, lvf_dense_prior** d, int n_sel, const int32_t* kf, const double* x0, const double* info, const double* eta, double c0); }      // solver_dense_prior.hip
// the window's dense prior by keyframe POSITION, as the problem takes it (null: none); the device copy is refilled only when the prior or
// the positions of its keyframes changed
static int window_dense_prior(lvf_window* w, lvf_dense_prior** out) {
  *out = nullptr;
  if (w->dp_ids.empty()) return LVF_OK;
  std::vector<int32_t> pos;
  for (int64_t id : w->dp_ids) {
    const auto it = w->kf_index.find(id);
    LVF_REQUIRE(it != w->kf_index.end(), "lvf_window: the dense prior's keyframe %lld is not in the window", (long long)id);
    pos.push_back(it->second);
  }
  if (pos != w->dp_pos || !w->dprior) {
    LVF_TRY(lvf::dense_prior_assign(w->ctx, &w->dprior, (int)pos.size(), pos.data(), w->dp_x0.data(), w->dp_info.data(), w->dp_eta.data(), w->dp_c0));
    w->dp_pos = pos;
  }
  *out = w->dprior;
  return LVF_OK;
}

static int configure_problem(lvf_window* w) {
  lvf_dense_prior* dense = nullptr;
  LVF_TRY(window_dense_prior(w, &dense));
  if (!w->prob) {
    LVF_TRY(lvf_problem_create(w->ctx, w->st, w->tc, w->tf, w->po, w->imu, &w->prob));
    LVF_TRY(lvf_problem_set_pose_priors(w->prob, w->prior));
    if (dense) LVF_TRY(problem_configure(w->prob, dense));
  } else {
    LVF_TRY(problem_configure(w->prob, dense));      // (the prior's keyframes are part of the elimination plan's key)
  }
  return window_attach_lidar(w);
}

// ---- the read-back: poses, velocities, biases by keyframe position and the inverse depths, gathered on the device into one block
// (k_window_pack) and copied with ONE device-to-host copy.  Where the inverse depths come from is the strategy's:
//   host walk        st->inv_depth, by dense slot (lvf_window::slot_lm translates)
//   device assembly  d_lm_invd_out, by landmark index, behind k_da_scatter_invd (which also writes them into the resident landmark table)
struct ReadBack { lvf_window* w; bool by_landmark; size_t off[5]; };
// (the tail of lvf_problem_solve_then: enqueued behind the last iteration and ahead of the wait that ends the solve)
static int enqueue_read_back(void* user) {
  ReadBack& rb = *static_cast<ReadBack*>(user);
  lvf_window* w = rb.w; lvf_state* st = w->st; hipStream_t s = w->ctx->stream;
  const size_t n_kf = w->kfs.size(), n_lm = (size_t)w->n_lm_problem, nl = w->lms.size();
  if (rb.by_landmark && n_lm)
    hipLaunchKernelGGL(k_da_scatter_invd, dim3((unsigned)((n_lm + 255) / 256)), dim3(256), 0, s, (int)n_lm, w->d_slot_lm.p, st->inv_depth.p, w->d_lm_invd_out.p, reinterpret_cast<LmDev*>(w->d_lmtab.p));
  PackWriter pw;
  rb.off[0] = pw.seg(st->poses.p, 7 * n_kf * 8); rb.off[1] = pw.seg(st->vel.p, 3 * n_kf * 8); rb.off[2] = pw.seg(st->ba.p, 3 * n_kf * 8); rb.off[3] = pw.seg(st->bg.p, 3 * n_kf * 8);
  rb.off[4] = rb.by_landmark ? pw.seg(w->d_lm_invd_out.p, nl * 8) : pw.seg(st->inv_depth.p, n_lm * 8);
  LVF_TRY(w->d_stage.ensure(pw.cur + 16)); LVF_TRY(w->h_state.reserve(pw.cur / 8 + 2));
  pw.pa.stage = w->d_stage.p;
  hipLaunchKernelGGL(k_window_pack, dim3(32), dim3(256), 0, s, pw.pa);
  LVF_HIP(hipGetLastError());
  LVF_HIP(hipMemcpyAsync(w->h_state.p, w->d_stage.p, pw.cur, hipMemcpyDeviceToHost, s));
  return LVF_OK;
}
// ... into the mirror (frame->pose, Vw, biases, landmark->inv_depth), once the copy has arrived
static void apply_read_back(lvf_window* w, const ReadBack& rb) {
  const double *poses = w->h_state.p + rb.off[0] / 8, *vel = w->h_state.p + rb.off[1] / 8, *ba = w->h_state.p + rb.off[2] / 8, *bg = w->h_state.p + rb.off[3] / 8,
               *invd = w->h_state.p + rb.off[4] / 8;
  for (size_t k = 0; k < w->kfs.size(); ++k) {
    lvf_window::Kf& f = w->kfs[k];
    std::memcpy(f.pose, &poses[7 * k], 56);
    if (f.good_imu) { std::memcpy(f.vel, &vel[3 * k], 24); std::memcpy(f.ba, &ba[3 * k], 24); std::memcpy(f.bg, &bg[3 * k], 24); }
  }
  if (rb.by_landmark) { for (size_t i = 0; i < w->lms.size(); ++i) if (w->lms[i].alive) w->lms[i].inv_depth = invd[i]; }
  else for (size_t l = 0; l < w->slot_lm.size(); ++l) w->lms[w->slot_lm[l]].inv_depth = invd[l];
}

// ---- strategy 1: the block lists assembled on the device (window_args.hpp describes the tables and the three kernels)

// Where each ImuError factor's information matrix sits in what the previous tick left in the IMU batch (-1: not there, factor it): slot f
// of `sq_prev` holds sqrt_info of the pre-integration version sq_ver[f].  Swaps the batch's matrices into sq_prev, so it runs ahead of
// shape_imu_batch; launch_imu_sqrt_info_cached then copies what is found there and factors the rest.
static int imu_cache_sources(lvf_window* w, StageWriter& sw, const std::vector<int32_t>& imu_j) {
  const size_t ni = imu_j.size();
  if (!ni) { w->sq_ver.clear(); return LVF_OK; }
  LVF_TRY(w->d_sq_src.ensure(ni + 4));
  int32_t* src = sw.seg_of(w->d_sq_src.p, ni);
  std::vector<unsigned> ver(ni);
  if (!w->sq_valid) w->sq_ver.clear();            // (a tick that failed after the swap below, or the host walk, left nothing to reuse)
  for (size_t f = 0; f < ni; ++f) {
    ver[f] = w->kfs[imu_j[f]].pre_ver;
    src[f] = -1;
    for (size_t g = 0; g < w->sq_ver.size(); ++g) if (w->sq_ver[g] == ver[f]) { src[f] = (int32_t)g; break; }
  }
  w->imu->sqrt_info.swap(w->sq_prev);             // last tick's matrices become the source; the batch gets the other buffer
  w->sq_ver = std::move(ver);
  w->sq_valid = false;                            // until this tick's matrices are on their way (assemble_device)
  return LVF_OK;
}

static int assemble_device(lvf_window* w, char* timing_note, size_t note_len) {
  hipStream_t s = w->ctx->stream;
  const int n_kf = (int)w->kfs.size();
  const auto t_begin = Clock::now();
  const size_t nl = w->lms.size();
  lvf_state* st = w->st;
  // ---- feature arena: every frame owns a segment; new / changed frames are (re)sent, a frame that outgrew its segment moves to the
  // end, and when the end is reached everything is laid out again from the start
  size_t n_obs = 0, need_new = 0;
  for (lvf_window::Kf& f : w->kfs) {
    f.sort_unique();
    n_obs += f.obs.size();
    if (f.d_cap < f.obs.size()) { f.d_dirty = true; need_new += f.obs.size() + f.obs.size() / 4 + 64; }
  }
  LVF_REQUIRE(n_obs < (size_t)1 << 30, "lvf_window_solve: too many features");
  if (w->arena_end + need_new > w->d_obs_lm.cap) {       // re-layout (also the first tick): capacity for twice the window
    size_t total_cap = 0;
    for (const lvf_window::Kf& f : w->kfs) total_cap += f.obs.size() + f.obs.size() / 4 + 64;
    const size_t want = std::max<size_t>(2 * total_cap, 4096);
    if (want > w->d_obs_lm.cap) { LVF_TRY(w->d_obs_lm.ensure(want)); LVF_TRY(w->d_obs_xy.ensure(2 * want)); }
    w->arena_end = 0;
    for (lvf_window::Kf& f : w->kfs) { f.d_cap = 0; f.d_dirty = true; }
  }
  for (lvf_window::Kf& f : w->kfs)
    if (f.d_cap < f.obs.size()) { f.d_off = w->arena_end; f.d_cap = f.obs.size() + f.obs.size() / 4 + 64; w->arena_end += f.d_cap; }
  // ---- staging: frame table | landmark table | state | IMU | dirty feature segments (one copy, one unpack launch)
  size_t dirty_obs = 0; int dirty_frames = 0;
  for (const lvf_window::Kf& f : w->kfs) if (f.d_dirty) { dirty_obs += f.obs.size(); ++dirty_frames; }
  const bool direct_segments = 2 * dirty_frames + 16 > kMaxSegs;      // (a full re-layout of a long window: copy those segments one by one)
  const size_t stage_bound = up16((size_t)n_kf * sizeof(FrameDev)) + up16(nl * sizeof(LmDev)) + up16(nl * 4) + 64 + up16((size_t)17 * n_kf * 8) + 8 * 64 + dirty_obs * 24 + (size_t)dirty_frames * 64 + 4096 +
                             up16((size_t)n_kf * 467 * 8) + (size_t)n_kf * 16 + 64;
  LVF_TRY(w->h_stage.reserve(stage_bound));
  LVF_TRY(w->d_stage.ensure(stage_bound));
  StageWriter sw(w->h_stage, 0);
  const unsigned char* lmtab_before = w->d_lmtab.p;
  LVF_TRY(w->d_frames.ensure((size_t)n_kf * sizeof(FrameDev) + 16)); LVF_TRY(w->d_lmtab.ensure(nl * sizeof(LmDev) + 16));
  if (w->d_lmtab.p != lmtab_before) w->lmtab_valid = false;          // re-allocated: the resident table is gone
  // frame table
  std::vector<double> Rk((size_t)9 * n_kf + 9);
  landmarks_to_world_prepare(w, Rk.data());
  double inv_e[7];
  hse3::inv(w->left.extrinsic, inv_e);
  FrameDev* fd = reinterpret_cast<FrameDev*>(sw.seg(w->d_frames.p, (size_t)n_kf * sizeof(FrameDev)));
  for (int k = 0, start = 0; k < n_kf; ++k) {
    const lvf_window::Kf& f = w->kfs[k];
    FrameDev& d = fd[k];
    d.id = f.id; d.start = start; d.cnt = (int)f.obs.size(); d.arena_off = (long long)f.d_off;
    start += d.cnt;
    frame_far_row(inv_e, f.pose, d.zrow, &d.zoff);
    std::memcpy(d.R, &Rk[(size_t)9 * k], 72); std::memcpy(d.t, f.pose + 4, 24);
    d.w_tc = two_camera_weight(f.w_visual);
  }
  // landmark table: all of it after a (re)allocation or a tick of the host walk, otherwise only what add_landmark / slide / prune touched
  {
    auto fill = [&](LmDev& d, const lvf_window::Lm& l) {
      d.right_ob[0] = l.right_ob[0]; d.right_ob[1] = l.right_ob[1]; d.pw[0] = l.pw[0]; d.pw[1] = l.pw[1]; d.pw[2] = l.pw[2];
      d.inv_depth = l.inv_depth; d.birth_kf = l.alive ? (long long)l.birth_kf : -1; d.fixed = (l.alive && l.fixed) ? 1 : 0; d.alive = l.alive ? 1 : 0;
    };
    const bool resident = w->lmtab_valid;
    w->lmtab_valid = false;                    // (set again once this tick has gone through: an error below leaves the table to be re-sent)
    if (!resident) {
      LmDev* ld = reinterpret_cast<LmDev*>(sw.seg(w->d_lmtab.p, nl * sizeof(LmDev)));
      for (size_t i = 0; i < nl; ++i) fill(ld[i], w->lms[i]);
    } else if (!w->lm_dirty.empty()) {
      const size_t nd = w->lm_dirty.size();
      sw.ua.n_lm_dirty = (int)nd; sw.ua.lmtab = w->d_lmtab.p;
      int32_t* di = reinterpret_cast<int32_t*>(sw.raw(nd * 4, &sw.ua.lm_idx_off));
      LmDev* dr = reinterpret_cast<LmDev*>(sw.raw(nd * sizeof(LmDev), &sw.ua.lm_rec_off));
      for (size_t j = 0; j < nd; ++j) { di[j] = w->lm_dirty[j]; fill(dr[j], w->lms[w->lm_dirty[j]]); }
    }
    for (int i : w->lm_dirty) w->lm_dirty_flag[i] = 0;
    w->lm_dirty.clear();
  }
  // state: the inverse depths are filled on the device, by slot (k_da_scan)
  LVF_TRY(stage_state(w, sw, nl));
  // the ImuError blocks do not depend on the assembly: their pre-integrations ride in this upload and their information matrices are
  // factored while the host waits for the assembly's counters
  std::vector<int32_t> imu_i, imu_j;
  imu_pairs(w, imu_i, imu_j);
  LVF_TRY(imu_cache_sources(w, sw, imu_j));
  LVF_TRY(shape_imu_batch(w, sw, imu_i, imu_j));
  // dirty feature segments
  for (lvf_window::Kf& f : w->kfs) {
    if (!f.d_dirty) continue;
    const size_t c = f.obs.size();
    if (c) {
      int32_t* dl; double* dx;
      std::vector<int32_t> tl; std::vector<double> tx;
      if (direct_segments) { tl.resize(c); tx.resize(2 * c); dl = tl.data(); dx = tx.data(); }
      else { dl = sw.seg_of(w->d_obs_lm.p + f.d_off, c); dx = sw.seg_of(w->d_obs_xy.p + 2 * f.d_off, 2 * c); }
      for (size_t j = 0; j < c; ++j) { dl[j] = f.obs[j].lm; dx[2 * j] = f.obs[j].ob[0]; dx[2 * j + 1] = f.obs[j].ob[1]; }
      if (direct_segments) {
        LVF_HIP(hipMemcpyAsync(w->d_obs_lm.p + f.d_off, dl, c * 4, hipMemcpyHostToDevice, s));
        LVF_HIP(hipMemcpyAsync(w->d_obs_xy.p + 2 * f.d_off, dx, c * 16, hipMemcpyHostToDevice, s));
        LVF_HIP(hipStreamSynchronize(s));                 // (pageable temporaries)
      }
    }
    f.d_dirty = false;
  }
  LVF_REQUIRE(sw.fits(), "lvf_window_solve: staging overflow");
  const auto t_staged = Clock::now();
  LVF_HIP(hipMemcpyAsync(w->d_stage.p, sw.base, sw.cur, hipMemcpyHostToDevice, s));
  UnpackArgs& ua = sw.ua;
  ua.stage = w->d_stage.p; ua.g_seg = 64;
  // (the assembly's `used` flags and counters are cleared by the unpack launch: two fill launches less)
  LVF_TRY(w->d_used.ensure(nl + 32)); LVF_TRY(w->d_counts.ensure(4 + 2 * kDaMaxKf));
  ua.zero_dst[0] = w->d_used.p; ua.zero_words[0] = (unsigned)((nl + 16 + 15) / 16);
  ua.zero_dst[1] = reinterpret_cast<unsigned char*>(w->d_counts.p); ua.zero_words[1] = (unsigned)(((4 + 2 * kDaMaxKf) * sizeof(int) + 15) / 16);
  hipLaunchKernelGGL(k_window_unpack, dim3(ua.g_seg), dim3(256), 0, s, ua);
  // ---- assembly kernels
  const int n_wg = (int)((n_obs + 255) / 256);
  LVF_TRY(w->d_cls.ensure(n_obs + 16)); LVF_TRY(w->d_wgcnt.ensure((size_t)3 * n_wg + 4)); LVF_TRY(w->d_wgbase.ensure((size_t)3 * n_wg + 4));
  LVF_TRY(w->d_slot.ensure(nl + 4)); LVF_TRY(w->d_slot_lm.ensure(nl + 4)); LVF_TRY(w->d_lm_invd_out.ensure(nl + 4));
  LVF_TRY(w->h_counts.reserve(4 + 2 * kDaMaxKf));
  LVF_TRY(ensure_visual(w, std::min(n_obs, nl), n_obs, n_obs));      // upper bounds: one TwoCamera block per landmark at most
  DaArgs da{};
  da.n_kf = n_kf; da.total = (int)n_obs; da.nl = (int)nl; da.n_wg = n_wg;
  da.frames = reinterpret_cast<const FrameDev*>(w->d_frames.p); da.obs_lm = w->d_obs_lm.p; da.obs_xy = reinterpret_cast<const double2*>(w->d_obs_xy.p);
  da.lm = reinterpret_cast<const LmDev*>(w->d_lmtab.p);
  std::memcpy(da.Re, &Rk[(size_t)9 * n_kf], 72); std::memcpy(da.te, w->right.extrinsic + 4, 24);
  da.fx = w->right.fx; da.fy = w->right.fy; da.cx = w->right.cx; da.cy = w->right.cy; da.far_z = w->opt.baseline * 50.0;
  da.cls = w->d_cls.p; da.used = w->d_used.p; da.wgcnt = w->d_wgcnt.p; da.wgbase = w->d_wgbase.p; da.slot = w->d_slot.p; da.slot_lm = w->d_slot_lm.p; da.counts = w->d_counts.p;
  da.state_invd = st->inv_depth.p; da.lm_invd_out = w->d_lm_invd_out.p;
  da.tc_l = reinterpret_cast<double2*>(w->tc->ob_a.p); da.tc_r = reinterpret_cast<double2*>(w->tc->ob_b.p); da.tc_lm = w->tc->idx_a.p; da.tc_kf = w->tc->idx_b.p; da.tc_w = w->tc->wblk.p;
  da.tf_f = reinterpret_cast<double2*>(w->tf->ob_a.p); da.tf_o = reinterpret_cast<double2*>(w->tf->ob_b.p); da.tf_lm = w->tf->idx_a.p; da.tf_k1 = w->tf->idx_b.p; da.tf_k2 = w->tf->idx_c.p;
  da.po_o = reinterpret_cast<double2*>(w->po->ob_a.p); da.po_pw = w->po->table.p; da.po_kf = w->po->idx_a.p; da.po_pi = w->po->idx_b.p;
  if (n_wg) hipLaunchKernelGGL(k_da_classify, dim3(n_wg), dim3(256), 0, s, da);
  hipLaunchKernelGGL(k_da_scan, dim3(1), dim3(1024), 0, s, da);
  if (n_wg) hipLaunchKernelGGL(k_da_emit, dim3(n_wg), dim3(256), 0, s, da);
  LVF_HIP(hipGetLastError());
  // the counter event: the host waits for the counters' copy, not for the work queued after it
  LVF_HIP(hipMemcpyAsync(w->h_counts.p, w->d_counts.p, (4 + 2 * kDaMaxKf) * sizeof(int), hipMemcpyDeviceToHost, s));
  if (!w->ev_counts) LVF_HIP(hipEventCreateWithFlags(&w->ev_counts, hipEventDisableTiming));
  LVF_HIP(hipEventRecord(w->ev_counts, s));
  if (w->n_imu) { LVF_TRY(launch_imu_sqrt_info_cached(w->imu, w->d_sq_src.p, w->sq_prev.p)); w->sq_valid = true; }      // runs while the host reads the counters and configures the problem
  LVF_HIP(hipEventSynchronize(w->ev_counts));
  const int* hc = w->h_counts.p;       // [0..3] tc, tf, po, n_lm | TwoFrame blocks per keyframe | near visual blocks per keyframe
  const auto t_assembled = Clock::now();
  // ---- priors, decided with the near counts k_da_classify made
  PriorLists pl;
  size_t fi = 0;
  for (int k = 0; k < n_kf; ++k) {
    const bool imu_block = fi < imu_j.size() && imu_j[fi] == k;
    if (imu_block) ++fi;
    LVF_TRY(weak_prior(w, k, imu_block, hc[4 + kDaMaxKf + k], pl));
  }
  set_visual_counts(w, (size_t)hc[0], (size_t)hc[1], (size_t)hc[2], hc[3], std::vector<int32_t>(hc + 4, hc + 4 + n_kf));
  // second (small) staged upload: the priors
  LVF_TRY(w->h_stage.reserve(16 * 64 + (size_t)n_kf * 128 + 4096));      // (grow-only: the first copy above has completed)
  StageWriter sp(w->h_stage, 0);
  LVF_TRY(shape_prior_batch(w, sp, pl));
  LVF_REQUIRE(sp.fits(), "lvf_window_solve: staging overflow");
  if (sp.ua.n_segs) {
    LVF_TRY(w->d_stage.ensure(sp.cur + 16));
    LVF_HIP(hipMemcpyAsync(w->d_stage.p, sp.base, sp.cur, hipMemcpyHostToDevice, s));
    sp.ua.stage = w->d_stage.p; sp.ua.g_seg = 8;
    hipLaunchKernelGGL(k_window_unpack, dim3(sp.ua.g_seg), dim3(256), 0, s, sp.ua);
    LVF_HIP(hipGetLastError());
  }
  if (timing_note)
    std::snprintf(timing_note, note_len, " (device assembly): host tables %.3f ms (%zu bytes staged), upload + assembly + counters %.3f ms, small uploads %.3f ms", ms_between(t_begin, t_staged),
                  sw.cur, ms_between(t_staged, t_assembled), ms_between(t_assembled, Clock::now()));
  return LVF_OK;
}

// ---- strategy 2: the host walks the features in BuildProblem's order and writes the block lists as 48-byte records into ONE pinned
// staging buffer (see TcRec / TfRec / PoRec), the plain segments behind them
static int assemble_host(lvf_window* w, char* timing_note, size_t note_len) {
  hipStream_t s = w->ctx->stream;
  const int n_kf = (int)w->kfs.size();
  const auto t_begin = Clock::now();
  // landmark->ToWorld() once per live landmark per tick (the reference recomputes it per feature) with the keyframe rotations
  // expanded once, and per frame the one row of the world->cam0 transform that Camera::Far needs
  std::vector<LmHot>& hot = w->hot;
  landmarks_hot(w, hot);
  double inv_e[7];
  hse3::inv(w->left.extrinsic, inv_e);
  const double far_z = w->opt.baseline * 50.0;
  size_t n_obs = 0;
  for (const lvf_window::Kf& f : w->kfs) n_obs += f.obs.size();
  // record regions sized by their upper bounds: one TwoCamera block per live landmark at most, every other feature one TwoFrame or
  // PoseOnly block; the PoseOnly region comes last so that the copy ends where its data ends
  const size_t cap_tc = std::min(n_obs, w->lms.size());
  const size_t off_tc = 0, off_tf = off_tc + cap_tc * 48, off_po = off_tf + n_obs * 48;
  const size_t tail_bound = up16((size_t)(17 * n_kf) * 8) + 8 * up16((size_t)n_kf * 8 + 64) + up16(w->lms.size() * 8 + 16) + up16((size_t)n_kf * 467 * 8) + 4096;
  LVF_TRY(w->h_stage.reserve(off_po + n_obs * 48 + tail_bound));
  unsigned char* hs = w->h_stage.p;
  TcRec* tcr = reinterpret_cast<TcRec*>(hs + off_tc);
  TfRec* tfr = reinterpret_cast<TfRec*>(hs + off_tf);
  PoRec* por = reinterpret_cast<PoRec*>(hs + off_po);
  std::vector<int32_t> kf2_counts(n_kf, 0);
  size_t ntc = 0, ntf = 0, npo = 0;
  // large windows: the records written so far go up while the rest is still being assembled (two extra submissions per third of the
  // frames; the 4 MB copy of a 50-keyframe window otherwise sits, ~0.1 ms, between the assembly and everything on the device)
  LVF_TRY(w->d_stage.ensure(off_po + n_obs * 48 + tail_bound));
  const bool chunked = n_obs >= 30000 && n_kf >= 6;
  size_t tc_sent = 0, tf_sent = 0;
  auto send_records = [&]() -> int {
    if (ntc > tc_sent) LVF_HIP(hipMemcpyAsync(w->d_stage.p + off_tc + tc_sent * 48, hs + off_tc + tc_sent * 48, (ntc - tc_sent) * 48, hipMemcpyHostToDevice, s));
    if (ntf > tf_sent) LVF_HIP(hipMemcpyAsync(w->d_stage.p + off_tf + tf_sent * 48, hs + off_tf + tf_sent * 48, (ntf - tf_sent) * 48, hipMemcpyHostToDevice, s));
    tc_sent = ntc; tf_sent = ntf;
    return LVF_OK;
  };
  std::vector<int32_t> imu_i, imu_j;
  imu_pairs(w, imu_i, imu_j);
  PriorLists pl;
  size_t fi = 0;
  w->slot_lm.clear();                                  // dense slots in the order the walk first meets a landmark
  auto slot_of =[&](LmHot& l, int lm) { if (l.slot < 0) { l.slot = (int)w->slot_lm.size(); w->slot_lm.push_back(lm); } return l.slot; };
  for (int k = 0; k < n_kf; ++k) {
    if (chunked && (k == n_kf / 3 || k == (2 * n_kf) / 3)) LVF_TRY(send_records());
    lvf_window::Kf& f = w->kfs[k];
    f.sort_unique();
    double zrow[3], zoff;
    frame_far_row(inv_e, f.pose, zrow, &zoff);
    int near_visual = 0;
    for (const lvf_window::Obs& ob : f.obs) {
      LmHot& l = hot[ob.lm];
      if (l.birth_kf == f.id) {
        TcRec& r = tcr[ntc++];
        r.l[0] = ob.ob[0]; r.l[1] = ob.ob[1]; r.r[0] = l.right_ob[0]; r.r[1] = l.right_ob[1]; r.lm = slot_of(l, ob.lm); r.kf = k; r.w = two_camera_weight(f.w_visual);
        continue;
      }
      const double* pw = l.pw;
      const int bpos = l.bpos;
      if (bpos < 0) {
        if (!l.fixed) continue;                        // birth frame unknown (never happens through this API)
        PoRec& r = por[npo];
        r.o[0] = ob.ob[0]; r.o[1] = ob.ob[1]; r.pw[0] = pw[0]; r.pw[1] = pw[1]; r.pw[2] = pw[2]; r.kf = k; r.pi = (int)npo;
        ++npo;
      } else {
        TfRec& r = tfr[ntf];
        r.f[0] = l.right_ob[0]; r.f[1] = l.right_ob[1]; r.o[0] = ob.ob[0]; r.o[1] = ob.ob[1]; r.lm = slot_of(l, ob.lm); r.k1 = bpos; r.k2 = k;
        ++kf2_counts[k];
        ++ntf;
      }
      if (!(zrow[0] * pw[0] + zrow[1] * pw[1] + zrow[2] * pw[2] + zoff > far_z)) ++near_visual;   // !Camera::Far
    }
    const bool imu_block = fi < imu_j.size() && imu_j[fi] == k;
    if (imu_block) ++fi;
    LVF_TRY(weak_prior(w, k, imu_block, near_visual, pl));
  }
  LVF_REQUIRE(ntc <= cap_tc, "lvf_window_solve: more TwoCamera blocks than live landmarks (%zu > %zu)", ntc, cap_tc);
  const int n_lm = (int)w->slot_lm.size();
  const auto t_assembled = Clock::now();
  // the plain segments behind the PoseOnly records: state (with the inverse depths, by slot), IMU, priors
  StageWriter sw(w->h_stage, up16(off_po + npo * 48));
  LVF_TRY(stage_state(w, sw, (size_t)n_lm));
  double* si = sw.seg_of(w->st->inv_depth.p, (size_t)n_lm);
  for (int l = 0; l < n_lm; ++l) si[l] = w->lms[w->slot_lm[l]].inv_depth;
  LVF_TRY(ensure_visual(w, ntc, ntf, npo));
  set_visual_counts(w, ntc, ntf, npo, n_lm, std::move(kf2_counts));
  LVF_TRY(shape_imu_batch(w, sw, imu_i, imu_j));
  LVF_TRY(shape_prior_batch(w, sw, pl));
  LVF_REQUIRE(sw.fits(), "lvf_window_solve: staging overflow");
  // the rest of the records, then the PoseOnly records and the plain segments in one copy; one unpack launch: its record half fills the
  // batches' SoA arrays
  LVF_TRY(send_records());
  if (sw.cur > off_po) LVF_HIP(hipMemcpyAsync(w->d_stage.p + off_po, hs + off_po, sw.cur - off_po, hipMemcpyHostToDevice, s));
  UnpackArgs& ua = sw.ua;
  ua.stage = w->d_stage.p; ua.ntc = (int)ntc; ua.ntf = (int)ntf; ua.npo = (int)npo; ua.off_tc = off_tc; ua.off_tf = off_tf; ua.off_po = off_po;
  ua.tc_l = reinterpret_cast<double2*>(w->tc->ob_a.p); ua.tc_r = reinterpret_cast<double2*>(w->tc->ob_b.p); ua.tc_lm = w->tc->idx_a.p; ua.tc_kf = w->tc->idx_b.p; ua.tc_w = w->tc->wblk.p;
  ua.tf_f = reinterpret_cast<double2*>(w->tf->ob_a.p); ua.tf_o = reinterpret_cast<double2*>(w->tf->ob_b.p); ua.tf_lm = w->tf->idx_a.p; ua.tf_k1 = w->tf->idx_b.p; ua.tf_k2 = w->tf->idx_c.p;
  ua.po_o = reinterpret_cast<double2*>(w->po->ob_a.p); ua.po_pw = w->po->table.p; ua.po_kf = w->po->idx_a.p; ua.po_pi = w->po->idx_b.p;
  ua.g_tc = (int)((ntc + 255) / 256); ua.g_tf = (int)((ntf + 255) / 256); ua.g_po = (int)((npo + 255) / 256); ua.g_seg = 64;
  hipLaunchKernelGGL(k_window_unpack, dim3(ua.g_tc + ua.g_tf + ua.g_po + ua.g_seg), dim3(256), 0, s, ua);
  LVF_HIP(hipGetLastError());
  if (w->n_imu) LVF_TRY(launch_imu_sqrt_info(w->imu));      // (this strategy factors every pair: nothing is tracked for the cached form)
  if (timing_note)
    std::snprintf(timing_note, note_len, ": assemble %.3f ms, upload %.3f ms", ms_between(t_begin, t_assembled), ms_between(t_assembled, Clock::now()));
  return LVF_OK;
}

extern "C" {
int lvf_window_solve(lvf_window* w, const lvf_solver_options* o, lvf_solver_summary* summary) {
  LVF_REQUIRE(w && o && summary, "lvf_window_solve: null argument");
  LVF_REQUIRE(!w->kfs.empty(), "lvf_window_solve: empty window");
  LVF_TRY(lvf::enter(w->ctx));
  using Assembler = lvf_window::Assembler;
  static const bool host_asm = getenv("LVF_WINDOW_HOST_ASM") != nullptr;
  const Assembler by = w->opt.device_assembly && !host_asm && (int)w->kfs.size() <= kDaMaxKf ? Assembler::device : Assembler::host;
  char note[256] = "";
  char* timing_note = window_timing() ? note : nullptr;
  LVF_TRY(ensure_objects(w));
  // the block lists, the state, the IMU and prior batches: assembled, uploaded, the batches shaped
  begin_assembly(w, by);
  LVF_TRY(by == Assembler::device ? assemble_device(w, timing_note, sizeof note) : assemble_host(w, timing_note, sizeof note));
  const auto t_uploaded = Clock::now();
  LVF_TRY(configure_problem(w));
  const auto t_configured = Clock::now();
  // solve, with the read-back enqueued behind the last iteration and ahead of the wait that ends the solve: ONE stream wait per tick for both
  ReadBack rb{w, by == Assembler::device, {0, 0, 0, 0, 0}};
  LVF_TRY(lvf_problem_solve_then(w->prob, o, summary, enqueue_read_back, &rb));      // (the wait for the control block also covers the read-back's copy: same stream, enqueued first)
  if (o->max_num_iterations <= 0) LVF_HIP(hipStreamSynchronize(w->ctx->stream));       // (no iteration, no control block to wait for; lvf_window_marginal relies on this)
  const auto t_solved = Clock::now();
  apply_read_back(w, rb);
  if (by == Assembler::device) w->lmtab_valid = true;      // the resident landmark table holds what this tick solved (k_da_scatter_invd)
  if (timing_note)
    std::fprintf(stderr, "lvf_window_solve%s, configure %.3f ms, solve %.3f ms (%d its), read-back %.3f ms\n", note, ms_between(t_uploaded, t_configured),
                 ms_between(t_configured, t_solved), summary->num_iterations, ms_between(t_solved, Clock::now()));
  return LVF_OK;
}

// Backend::Optimize's outlier gate (src/lvio_fusion/src/backend.cpp:185-190, :229-245): every feature that is not its landmark's first
// observation is re-projected with weight 1 — compute_reprojection_error = |PoseOnlyReprojectionError(ob, landmark->ToWorld(), camera, 1)
// (frame->pose)| — and removed when the error exceeds max_px (10 in the reference).  The residual pass is the PoseOnly hot-path kernel
// on device (one batch over all such features of the window); the host only applies the removals to its mirror, like
// landmark->RemoveObservation(feature) + frame->RemoveFeature(feature).  removed_lm / removed_kf (may be NULL) receive up to `capacity`
// (landmark id, keyframe id) pairs in frame order; *n_removed the total.
int lvf_window_reject_outliers(lvf_window* w, double max_px, int64_t* removed_lm, int64_t* removed_kf, int capacity, int* n_removed) {
  LVF_REQUIRE(w && n_removed, "lvf_window_reject_outliers: null argument");
  LVF_REQUIRE(capacity >= 0 && (capacity == 0 || (removed_lm && removed_kf)), "lvf_window_reject_outliers: bad output arrays");
  *n_removed = 0;
  if (w->kfs.empty()) return LVF_OK;
  lvf_ctx* ctx = w->ctx;
  LVF_TRY(lvf::enter(ctx));
  hipStream_t s = ctx->stream;
  const int n_kf = (int)w->kfs.size();
  std::vector<double> lm_pw;
  std::vector<int> lm_birth_pos;
  landmarks_to_world(w, lm_pw, lm_birth_pos);
  // features that are not their landmark's first observation, in frame order / ascending landmark id
  std::vector<double> ob, pw, poses((size_t)7 * n_kf), ones(n_kf, 1.0);
  std::vector<int32_t> kf, pi;
  std::vector<std::pair<int, int>> where;          // (keyframe position, index into its obs)
  for (int k = 0; k < n_kf; ++k) {
    lvf_window::Kf& f = w->kfs[k];
    f.sort_unique();
    std::memcpy(&poses[(size_t)7 * k], f.pose, 56);
    for (size_t j = 0; j < f.obs.size(); ++j) {
      const lvf_window::Obs& o = f.obs[j];
      const lvf_window::Lm& l = w->lms[o.lm];
      if (l.birth_kf == f.id) continue;
      if (!l.fixed && lm_birth_pos[o.lm] < 0) continue;   // birth pose unknown (never happens through this API)
      ob.push_back(o.ob[0]); ob.push_back(o.ob[1]);
      pw.insert(pw.end(), &lm_pw[(size_t)3 * o.lm], &lm_pw[(size_t)3 * o.lm] + 3);
      pi.push_back((int32_t)kf.size()); kf.push_back(k);
      where.emplace_back(k, (int)j);
    }
  }
  const int n = (int)kf.size();
  if (n == 0) return LVF_OK;
  if (!w->rej) {
    const double z2[2] = {0, 0}; const int32_t z = 0; const double id7[7] = {0, 0, 0, 1, 0, 0, 0};
    LVF_TRY(lvf_pose_only_create(ctx, &w->left, 0, z2, &z, &z, 0, id7, &w->rej));
    LVF_TRY(lvf_state_create(ctx, 0, 0, &w->rej_st));
  }
  lvf_batch* b = w->rej;
  lvf_state* st = w->rej_st;
  st->n_kf = n_kf; st->n_lm = 0;
  LVF_TRY(st->poses.assign(poses.data(), poses.size(), s)); LVF_TRY(st->w_visual.assign(ones.data(), ones.size(), s));
  LVF_TRY(b->ob_a.assign(ob.data(), ob.size(), s)); LVF_TRY(b->idx_a.assign(kf.data(), kf.size(), s)); LVF_TRY(b->idx_b.assign(pi.data(), pi.size(), s));
  LVF_TRY(b->table.assign(pw.data(), pw.size(), s)); LVF_TRY(b->res.ensure((size_t)2 * n));
  b->n = n; b->n_table = n; b->min_n_kf = n_kf; b->min_n_lm = 0; b->sorted_by_kf = true; b->evaluated = false;
  LVF_TRY(launch_pose_only(b, st, false));
  LVF_TRY(w->rej_flags.ensure(n));
  hipLaunchKernelGGL(k_flag_outliers, dim3((n + 255) / 256), dim3(256), 0, s, n, reinterpret_cast<const double2*>(b->res.p), max_px, w->rej_flags.p);
  LVF_HIP(hipGetLastError());
  std::vector<uint8_t> flags(n);
  LVF_HIP(hipMemcpyAsync(flags.data(), w->rej_flags.p, n, hipMemcpyDeviceToHost, s));
  LVF_HIP(hipStreamSynchronize(s));
  // apply the removals (back to front inside each keyframe so the stored positions stay valid)
  int total = 0;
  for (int i = 0; i < n; ++i)
    if (flags[i]) {
      if (total < capacity) { removed_lm[total] = w->kfs[where[i].first].obs[where[i].second].lm_id; removed_kf[total] = w->kfs[where[i].first].id; }
      ++total;
    }
  for (int i = n - 1; i >= 0; --i)
    if (flags[i]) { auto& v = w->kfs[where[i].first].obs; v.erase(v.begin() + where[i].second); w->kfs[where[i].first].d_dirty = true; }
  *n_removed = total;
  if (total) prune(w);
  return LVF_OK;
}

// Test hook (tests/test_gpu_window.py): the block lists of the LAST lvf_window_solve as they sit in the device batches — in the batch's order,
// keyframe positions translated to keyframe ids and landmark slots to landmark ids — so that the assembly (host walk or device kernels) can be
// compared with the reference's Backend::BuildProblem block by block (backend.cpp:96-183; tests/golden/ref_v4.npz).
//   kind 0 TwoCamera : ids {landmark, -1, keyframe}            vals {5 w_visual[kf], left ob x, y, right ob x, y, 0, 0, 0}
//   kind 1 PoseOnly  : ids {-1, -1, keyframe}                  vals {w_visual[kf], ob x, y, 0, 0, pw x, y, z}
//   kind 2 TwoFrame  : ids {landmark, first keyframe, keyframe} vals {w_visual[kf], ob x, y, first (right) ob x, y, 0, 0, 0}
//   kind 3 ImuError  : ids {-1, keyframe i, keyframe j}
//   kind 4 priors    : ids {-1, previous keyframe or -1 (PoseError), keyframe}   vals {weight, v, 0, ...}
// ids [capacity][3], vals [capacity][8]; *n = blocks of that kind (may exceed capacity: only `capacity` are written).
int lvf_window_debug_blocks(lvf_window* w, int kind, int capacity, int64_t* ids, double* vals, int* n) {
  LVF_REQUIRE(w && n && kind >= 0 && kind <= 4 && capacity >= 0 && (capacity == 0 || (ids && vals)), "lvf_window_debug_blocks: bad arguments");
  LVF_TRY(lvf::enter(w->ctx));
  hipStream_t s = w->ctx->stream;
  lvf_batch* b = kind == 0 ? w->tc : kind == 1 ? w->po : kind == 2 ? w->tf : kind == 3 ? w->imu : w->prior;
  const int nb = kind == 0 ? w->n_tc : kind == 1 ? w->n_po : kind == 2 ? w->n_tf : kind == 3 ? w->n_imu : w->n_prior;
  *n = nb;
  if (!b || nb == 0 || capacity == 0) return LVF_OK;
  const int m = std::min(nb, capacity), n_kf = (int)w->kfs.size();
  auto get_i = [&](const lvf::DevBuf<int32_t>& d, std::vector<int32_t>& h, size_t cnt) -> int { h.resize(cnt); LVF_HIP(hipMemcpyAsync(h.data(), d.p, cnt * 4, hipMemcpyDeviceToHost, s)); return LVF_OK; };
  auto get_d = [&](const lvf::DevBuf<double>& d, std::vector<double>& h, size_t cnt) -> int { h.resize(cnt); LVF_HIP(hipMemcpyAsync(h.data(), d.p, cnt * 8, hipMemcpyDeviceToHost, s)); return LVF_OK; };
  std::vector<int32_t> ia, ib, ic, slot_lm;
  std::vector<double> oa, ob, tab;
  if (kind <= 2) { LVF_TRY(get_i(b->idx_a, ia, m)); LVF_TRY(get_d(b->ob_a, oa, (size_t)2 * m)); }
  if (kind == 0 || kind == 2) { LVF_TRY(get_i(b->idx_b, ib, m)); LVF_TRY(get_d(b->ob_b, ob, (size_t)2 * m)); }
  std::vector<double> wb;
  if (kind == 0 && b->wblk.n >= (size_t)m) LVF_TRY(get_d(b->wblk, wb, m));
  if (kind == 2) LVF_TRY(get_i(b->idx_c, ic, m));
  if (kind == 1) { LVF_TRY(get_i(b->idx_b, ib, m)); LVF_TRY(get_d(b->table, tab, (size_t)3 * b->n_table)); }
  if (kind == 3) { LVF_TRY(get_i(b->idx_a, ia, m)); LVF_TRY(get_i(b->idx_b, ib, m)); }
  if (kind == 4) { LVF_TRY(get_i(b->idx_a, ia, m)); LVF_TRY(get_i(b->idx_b, ib, m)); LVF_TRY(get_d(b->ob_a, oa, m)); LVF_TRY(get_d(b->ob_b, ob, m)); }
  // dense landmark slot -> landmark index, from where the strategy that assembled these lists left it
  if (kind == 0 || kind == 2) {
    if (w->assembled_by == lvf_window::Assembler::device) {
      slot_lm.resize((size_t)w->n_lm_problem);
      if (w->n_lm_problem) LVF_HIP(hipMemcpyAsync(slot_lm.data(), w->d_slot_lm.p, (size_t)w->n_lm_problem * 4, hipMemcpyDeviceToHost, s));
    } else slot_lm.assign(w->slot_lm.begin(), w->slot_lm.end());
  }
  LVF_HIP(hipStreamSynchronize(s));
  auto kf_id = [&](int pos) -> int64_t { return (pos >= 0 && pos < n_kf) ? w->kfs[pos].id : -1; };
  auto lm_id = [&](int slot) -> int64_t { return (slot >= 0 && slot < (int)slot_lm.size()) ? w->lms[slot_lm[slot]].id : -1; };
  auto wv = [&](int pos) { return (pos >= 0 && pos < n_kf) ? w->kfs[pos].w_visual : 0.0; };
  for (int i = 0; i < m; ++i) {
    int64_t* I = ids + 3 * (size_t)i; double* V = vals + 8 * (size_t)i;
    I[0] = I[1] = I[2] = -1;
    for (int q = 0; q < 8; ++q) V[q] = 0.0;
    if (kind == 0) { I[0] = lm_id(ia[i]); I[2] = kf_id(ib[i]); V[0] = wb.empty() ? 5 * wv(ib[i]) : wb[i]; V[1] = oa[2 * i]; V[2] = oa[2 * i + 1]; V[3] = ob[2 * i]; V[4] = ob[2 * i + 1]; }
    else if (kind == 1) { I[2] = kf_id(ia[i]); V[0] = wv(ia[i]); V[1] = oa[2 * i]; V[2] = oa[2 * i + 1]; const int t = ib[i]; if (t >= 0 && t < b->n_table) { V[5] = tab[3 * t]; V[6] = tab[3 * t + 1]; V[7] = tab[3 * t + 2]; } }
    else if (kind == 2) { I[0] = lm_id(ia[i]); I[1] = kf_id(ib[i]); I[2] = kf_id(ic[i]); V[0] = wv(ic[i]); V[1] = ob[2 * i]; V[2] = ob[2 * i + 1]; V[3] = oa[2 * i]; V[4] = oa[2 * i + 1]; }
    else if (kind == 3) { I[1] = kf_id(ia[i]); I[2] = kf_id(ib[i]); }
    else { I[1] = kf_id(ia[i]); I[2] = kf_id(ib[i]); V[0] = oa[i]; V[1] = ob[i]; }
  }
  return LVF_OK;
}

// Marginal information / covariance of keyframes of the window (marginal_kernels.hip).  The window's problem is brought up to date by the
// code path of lvf_window_solve itself, asked for no iteration (it assembles the block lists, configures the problem, evaluates the cost and
// copies the unchanged state back), then the problem's entry does the rest with the ids translated to positions.
int lvf_window_marginal(lvf_window* w, const lvf_solver_options* o, const int64_t* kf_ids, int n_sel, double* info, double* cov, lvf_marginal_stats* stats) {
  LVF_REQUIRE(w && o && kf_ids && stats, "lvf_window_marginal: null argument");
  LVF_REQUIRE(info || cov, "lvf_window_marginal: info and cov are both NULL");
  LVF_REQUIRE(n_sel >= 1 && n_sel <= 8, "lvf_window_marginal: %d keyframes selected (1 .. 8)", n_sel);
  int kfs[8];
  for (int i = 0; i < n_sel; ++i) {
    const auto it = w->kf_index.find(kf_ids[i]);
    LVF_REQUIRE(it != w->kf_index.end(), "lvf_window_marginal: keyframe %lld is not in the window", (long long)kf_ids[i]);
    kfs[i] = it->second;
    for (int j = 0; j < i; ++j) LVF_REQUIRE(kfs[j] != kfs[i], "lvf_window_marginal: keyframe %lld listed twice", (long long)kf_ids[i]);
  }
  lvf_solver_options refresh = *o;
  refresh.max_num_iterations = 0;
  lvf_solver_summary summary;
  LVF_TRY(lvf_window_solve(w, &refresh, &summary));
  return lvf_problem_marginal(w->prob, o, kfs, n_sel, info, cov, stats);
}

// ---- the dense prior of the window and the marginalising slide
int lvf_window_set_dense_prior(lvf_window* w, int n_sel, const int64_t* kf_ids, const double* x0, const double* info, const double* eta, double c0) {
  LVF_REQUIRE(w, "lvf_window_set_dense_prior: null window");
  if (n_sel == 0) { w->dp_ids.clear(); w->dp_pos.clear(); return LVF_OK; }
  LVF_REQUIRE(n_sel >= 1 && n_sel <= 8, "lvf_window_set_dense_prior: %d keyframes (1 .. 8, or 0 to remove the prior)", n_sel);
  LVF_REQUIRE(kf_ids && x0 && info, "lvf_window_set_dense_prior: null input array");
  const int m = 15 * n_sel;
  for (int i = 0; i < n_sel; ++i) {
    LVF_REQUIRE(w->kf_index.count(kf_ids[i]), "lvf_window_set_dense_prior: keyframe %lld is not in the window", (long long)kf_ids[i]);
    for (int j = 0; j < i; ++j) LVF_REQUIRE(kf_ids[j] != kf_ids[i], "lvf_window_set_dense_prior: keyframe %lld listed twice", (long long)kf_ids[i]);
    double n2 = 0.0;
    for (int c = 0; c < 16; ++c) LVF_REQUIRE(std::isfinite(x0[16 * i + c]), "lvf_window_set_dense_prior: x0 of keyframe %lld is not finite", (long long)kf_ids[i]);
    for (int c = 0; c < 4; ++c) n2 += x0[16 * i + c] * x0[16 * i + c];
    LVF_REQUIRE(n2 > 0.0, "lvf_window_set_dense_prior: x0 of keyframe %lld has a zero quaternion", (long long)kf_ids[i]);
  }
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j <= i; ++j) LVF_REQUIRE(std::isfinite(info[(size_t)i * m + j]), "lvf_window_set_dense_prior: info[%d][%d] is not finite", i, j);
    LVF_REQUIRE(!eta || std::isfinite(eta[i]), "lvf_window_set_dense_prior: eta[%d] is not finite", i);
  }
  LVF_REQUIRE(std::isfinite(c0), "lvf_window_set_dense_prior: c0 is not finite");
  w->dp_ids.assign(kf_ids, kf_ids + n_sel);
  w->dp_x0.assign(x0, x0 + 16 * n_sel);
  w->dp_info.assign(info, info + (size_t)m * m);
  if (eta) w->dp_eta.assign(eta, eta + m); else w->dp_eta.assign(m, 0.0);
  w->dp_c0 = c0;
  w->dp_pos.clear();                         // the device copy is stale
  return LVF_OK;
}

int lvf_window_get_dense_prior(const lvf_window* w, int* n_sel, int64_t* kf_ids, double* x0, double* info, double* eta, double* c0) {
  LVF_REQUIRE(w && n_sel, "lvf_window_get_dense_prior: null argument");
  const int n = (int)w->dp_ids.size();
  *n_sel = n;
  if (n == 0) return LVF_OK;
  if (kf_ids) std::copy(w->dp_ids.begin(), w->dp_ids.end(), kf_ids);
  if (x0) std::copy(w->dp_x0.begin(), w->dp_x0.end(), x0);
  if (info) std::copy(w->dp_info.begin(), w->dp_info.end(), info);
  if (eta) std::copy(w->dp_eta.begin(), w->dp_eta.end(), eta);
  if (c0) *c0 = w->dp_c0;
  return LVF_OK;
}

// The sub-problem over D (the departing keyframes) and s (the first kept one): every block BuildProblem's rules give for that keyframe
// list that touches D — D's visual blocks, weak-constraint priors and lidar planes, the ImuError blocks along D and into s, the window's
// dense prior — and nothing of s's own: no visual block (what kept frames see of D's landmarks lives on as PoseOnly blocks after the slide,
// so no factor is counted twice and none is lost), no weak-constraint prior.  Its marginal on s becomes the window's dense prior.
int lvf_window_slide_marginalize(lvf_window* w, int64_t first_active_kf_id, const lvf_solver_options* o, lvf_marginal_stats* stats) {
  LVF_REQUIRE(w && o && stats, "lvf_window_slide_marginalize: null argument");
  *stats = lvf_marginal_stats{0, 0, 0, 0.0};
  size_t drop = 0;
  while (drop < w->kfs.size() && w->kfs[drop].id < first_active_kf_id) ++drop;
  if (drop == 0) return LVF_OK;
  LVF_REQUIRE(drop < w->kfs.size(), "lvf_window_slide_marginalize: no keyframe at or after %lld would stay", (long long)first_active_kf_id);
  const int64_t s_id = w->kfs[drop].id;
  for (int64_t id : w->dp_ids)
    LVF_REQUIRE(id <= s_id, "lvf_window_slide_marginalize: the window's dense prior sits on keyframe %lld, beyond the first kept keyframe %lld: it cannot be "
                "absorbed into a prior on that keyframe alone (remove it, or slide further)", (long long)id, (long long)s_id);
  LVF_TRY(lvf::enter(w->ctx));
  if (!w->sub) {
    lvf_window_options so = w->opt;
    so.device_assembly = 0;                  // (re-filled from scratch at every slide: the resident tables of the device-side assembly have nothing to keep)
    LVF_TRY(lvf_window_create(w->ctx, &w->left, &w->right, &so, &w->sub));
    w->sub->is_sub = true;
  }
  lvf_window* q = w->sub;
  q->kfs.assign(w->kfs.begin(), w->kfs.begin() + drop + 1);
  q->kfs.back().obs.clear();
  for (lvf_window::Kf& f : q->kfs) f.d_dirty = true;
  q->kf_index.clear();
  for (size_t k = 0; k < q->kfs.size(); ++k) q->kf_index[q->kfs[k].id] = (int)k;
  q->departed = w->departed;
  q->lms = w->lms; q->lm_index = w->lm_index; q->lm_free = w->lm_free; q->n_lm_live = w->n_lm_live;      // (indices are stable: the observations keep theirs)
  q->lidar_seg.clear();
  for (size_t k = 0; k < drop; ++k) {
    const auto is = w->lidar_seg.find(w->kfs[k].id);
    if (is != w->lidar_seg.end()) q->lidar_seg[is->first] = is->second;      // borrowed
  }
  q->lidar_dirty = q->lidar != nullptr || !q->lidar_seg.empty();
  q->dp_ids = w->dp_ids; q->dp_x0 = w->dp_x0; q->dp_info = w->dp_info; q->dp_eta = w->dp_eta; q->dp_c0 = w->dp_c0; q->dp_pos.clear();
  lvf_solver_options refresh = *o;
  refresh.max_num_iterations = 0;
  lvf_solver_summary summary;
  const int kf_s = (int)drop;
  std::vector<double> info(225), eta(15);
  double c0 = 0.0;
  int rc = lvf_window_solve(q, &refresh, &summary);
  if (rc == LVF_OK) rc = lvf_problem_marginal_prior(q->prob, o, &kf_s, 1, info.data(), eta.data(), &c0, stats);
  q->lidar_seg.clear();                      // (this window's segments: the slide below destroys the departing ones)
  LVF_TRY(rc);
  const lvf_window::Kf s = w->kfs[drop];
  LVF_TRY(lvf_window_slide(w, first_active_kf_id));
  w->dp_ids.clear(); w->dp_pos.clear();
  if (stats->fail != 0) return LVF_OK;       // soft failure: the window has slid, without a prior
  double x0[16];
  std::memcpy(x0, s.pose, 56); std::memcpy(x0 + 7, s.vel, 24); std::memcpy(x0 + 10, s.ba, 24); std::memcpy(x0 + 13, s.bg, 24);
  return lvf_window_set_dense_prior(w, 1, &s_id, x0, info.data(), eta.data(), c0);
}

}  // extern "C"

