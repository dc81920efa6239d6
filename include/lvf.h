/* lvf.h — C-ABI of the MI355X-native lvio_fusion hot path (local-BA factor evaluation,
 * normal-equation / Schur reduction, LiDAR scan-to-map 3-NN association + point-to-plane ICP).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each group cites
 * the reference interface it replaces (paths under src/lvio_fusion/ of jypjypjypjyp/lvio_fusion):
 *
 *   lvf_pose_only_*    <- PoseOnlyReprojectionError::Create / AutoDiffCostFunction<..,2,7>::Evaluate
 *                         include/lvio_fusion/ceres/visual_error.hpp:48-76
 *   lvf_two_frame_*    <- TwoFrameReprojectionError  <2,1,7,7>   visual_error.hpp:78-107
 *   lvf_two_camera_*   <- TwoCameraReprojectionError <2,1>       visual_error.hpp:109-137
 *   lvf_lidar_plane_*  <- LidarPlaneErrorRPZ / LidarPlaneErrorYXY <1,1,1,1>
 *                         include/lvio_fusion/ceres/lidar_error.hpp:42-110 (+ ctor normal :13-18)
 *   lvf_imu_*          <- ImuError : SizedCostFunction<15,7,3,3,3,7,3,3,3>
 *                         include/lvio_fusion/ceres/imu_error.hpp:12-122, src/preintegration.cpp:144-165
 *   lvf_pose_prior_*   <- PoseGraphError <6,7,7> / PoseError <6,7>   include/lvio_fusion/ceres/pose_error.hpp:10-86
 *   lvf_preintegrate   <- imu::Preintegration::{Append,Propagate,MidPointIntegration}
 *                         src/preintegration.cpp:30-127, include/lvio_fusion/imu/preintegration.h:29-41
 *   lvf_map_* / lvf_scan_* / lvf_knn3_*
 *                      <- pcl::KdTreeFLANN::setInputCloud + nearestKSearch(point,3,..) + the 3x(d2<thr) gate
 *                         src/association.cpp:278-301 (ground), :336-359 (surf)
 *   lvf_icp_*          <- FeatureAssociation::ScanToMapWith{Ground,Segmented} + the DENSE_QR solve
 *                         src/association.cpp:270-384, src/mapping.cpp:154-178
 *   lvf_cloud_*        <- Mapping::MergeScan/ToWorld/BuildMapFrame, pcl::VoxelGrid / RadiusOutlierRemoval / SACSegmentation
 *                         src/mapping.cpp:78-137,193-220, src/association.cpp:210-268
 *   lvf_trajectory_* / lvf_cloud_deskew / lvf_lidar_extract_deskewed
 *                      <- Map::ComputePose, FeatureAssociation::UndistortPointCloud, the TODO of AdjustDistortion
 *                         src/map.cpp:92-102, src/association.cpp:65-83, :142-145
 *   lvf_lidar_depth_* / lvf_stereo_triangulate_lidar
 *                      <- declared (no reference text): the sweep's depth for the features LocalMap::Triangulate leaves Far or lost
 *                         src/local_map.cpp:233-269, include/lvio_fusion/visual/camera.h:38-41
 *   lvf_scan_match     <- Mapping::Optimize's per-frame body / Mapping::Relocate   src/mapping.cpp:147-178, :251-300
 *   lvf_window_*       <- Backend::BuildProblem's assembly kept incrementally          src/backend.cpp:96-183
 *   lvf_problem_*      <- adapt::Problem::{AddParameterBlock,AddResidualBlock,SetParameterBlockConstant}
 *                         + adapt::Solve (include/lvio_fusion/adapt/problem.h:34-88) as driven by
 *                         Backend::BuildProblem / Backend::Optimize (src/backend.cpp:96-183, :192-246)
 *
 * Conventions
 *   - pose block = Sophus SE3d::data() = [qx,qy,qz,qw,tx,ty,tz] (7 doubles), Twc maps body->world.
 *   - Jacobians are row-major num_residuals x block_size, w.r.t. AMBIENT parameters
 *     (the ceres::CostFunction::Evaluate contract).
 *   - every function returns 0 (LVF_OK) on success; on failure outputs are untouched and
 *     lvf_last_error() (thread-local) describes the problem.  No exceptions cross the boundary.
 *   - "create" calls copy their inputs to HBM; evaluate/solve calls are asynchronous on the
 *     context's HIP stream and leave their outputs resident in HBM; *_download calls synchronise.
 *   - a context is bound to one device and one stream; use one context per host thread
 *     (Backend::Optimize and Relocator can be in flight concurrently: src/relocator.cpp:188).
 *   - there is NO CPU fallback: without a usable gfx950 device lvf_ctx_create fails.
 */
#ifndef LVF_H_
#define LVF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVF_OK 0
#define LVF_ERR_INVALID 1   /* bad argument */
#define LVF_ERR_HIP 2       /* HIP runtime error (see lvf_last_error) */
#define LVF_ERR_NO_DEVICE 3 /* no usable GPU: the product path refuses to run */
#define LVF_ERR_STATE 4     /* call sequence error (e.g. download before evaluate) */

typedef struct lvf_ctx lvf_ctx;
typedef struct lvf_state lvf_state;
typedef struct lvf_batch lvf_batch;
typedef struct lvf_map lvf_map;
typedef struct lvf_scan lvf_scan;
typedef struct lvf_icp lvf_icp;
typedef struct lvf_cloud lvf_cloud;
typedef struct lvf_window lvf_window;
typedef struct lvf_problem lvf_problem;
typedef struct lvf_comm lvf_comm;
typedef struct lvf_problem_batch lvf_problem_batch;
typedef struct lvf_image lvf_image;

/* Camera = intrinsics + sensor->robot extrinsic (include/lvio_fusion/sensor.h:41-44, visual/camera.h:74). */
typedef struct lvf_camera {
  double fx, fy, cx, cy;
  double extrinsic[7];
} lvf_camera;

/* Snapshot of imu::Preintegration after the last Append (include/lvio_fusion/imu/preintegration.h:66-86). */
typedef struct lvf_preint {
  double sum_dt;
  double lin_ba[3];
  double lin_bg[3];
  double dp[3];
  double dq[4]; /* x,y,z,w */
  double dv[3];
  double jac[225]; /* 15x15 row-major */
  double cov[225]; /* 15x15 row-major */
} lvf_preint;

const char* lvf_last_error(void);
const char* lvf_version(void);

/* Host memory the device can copy from without the runtime pinning and unpinning the pages around every copy (page-locked, recycled
 * process-wide in size buckets).  For arrays that are filled on the host and then handed to lvf_*_create / lvf_state_set: the adapter
 * (include/lvf_ceres_adapter.hpp) records the window's block lists straight into it while Backend::BuildProblem adds blocks
 * (src/lvio_fusion/src/backend.cpp:96-183), so gpu::Solve's uploads are plain DMA.  Falls back to ordinary memory when no device is
 * usable (host-only tools).  lvf_host_free takes the SAME byte count the block was allocated with.  Thread-safe. */
void* lvf_host_alloc(size_t bytes);
void lvf_host_free(void* p, size_t bytes);

/* ---- context ------------------------------------------------------------------------------ */
/* stream: an existing hipStream_t to run on (e.g. the caller's), or NULL to create a private one. */
int lvf_ctx_create(int device, void* hip_stream, lvf_ctx** out);
int lvf_ctx_destroy(lvf_ctx* ctx);
int lvf_ctx_synchronize(lvf_ctx* ctx);
void* lvf_ctx_stream(lvf_ctx* ctx);
/* HIP-event timing of the context's stream, for bench.py: begin/end record events, elapsed synchronises. */
int lvf_timer_begin(lvf_ctx* ctx);
int lvf_timer_end(lvf_ctx* ctx);
int lvf_timer_elapsed_ms(lvf_ctx* ctx, float* ms);
/* Box calibration for the latency-bound legs (bench.py `box_calibration`): out8 = {ns per dependent fp64 FMA of one wave, shader clocks per
 * such FMA, effective shader clock MHz during the chain, us per empty launch back to back, us for launch + stream wait of one empty
 * kernel, rated shader clock MHz, memory clock MHz, compute units}.  Not part of the reference surface. */
int lvf_box_calibration(lvf_ctx* ctx, double* out8);

/* ---- parameter state (the caller-owned double* blocks of the Ceres problem, mirrored in HBM) - */
enum lvf_field {
  LVF_POSES = 0,     /* n_kf x 7   frame->pose.data()                      backend.cpp:110 */
  LVF_VEL = 1,       /* n_kf x 3   frame->Vw.data()                        backend.cpp:147 */
  LVF_BA = 2,        /* n_kf x 3   frame->bias.linearized_ba.data()        backend.cpp:149 */
  LVF_BG = 3,        /* n_kf x 3   frame->bias.linearized_bg.data()        backend.cpp:148 */
  LVF_INV_DEPTH = 4, /* n_lm       &landmark->inv_depth                    backend.cpp:121 */
  LVF_W_VISUAL = 5   /* n_kf       frame->weights.visual                   frame.cpp:13    */
};
int lvf_state_create(lvf_ctx* ctx, int n_kf, int n_lm, lvf_state** out);
int lvf_state_destroy(lvf_state* st);
int lvf_state_set(lvf_state* st, int field, const double* host);
int lvf_state_get(lvf_state* st, int field, double* host);
/* lvf_state_create + the fields in one staged upload and one wait; a NULL field takes its default (identity poses, zeros, unit weights). */
int lvf_state_create_from(lvf_ctx* ctx, int n_kf, int n_lm, const double* poses, const double* vel, const double* ba, const double* bg,
                          const double* inv_depth, const double* w_visual, lvf_state** out);
/* lvf_state_set for every field at once: ONE staged upload and one wait; a NULL pointer leaves that field as it is. */
int lvf_state_set_all(lvf_state* st, const double* poses, const double* vel, const double* ba, const double* bg, const double* inv_depth,
                      const double* w_visual);
/* dst <- src (all fields; same n_kf / n_lm), device to device, asynchronous on dst's context: restoring a saved estimate without a host
 * round trip. */
int lvf_state_copy(lvf_state* dst, const lvf_state* src);

/* ---- factor batches (one batch = all residual blocks of one functor type) ------------------ */
/* n blocks; ob[n][2]; kf_idx[n] selects the pose block and the per-frame weight; pw_idx[n] indexes
 * pw[n_pw][3] (landmark->ToWorld(), constant during the solve: backend.cpp:129). */
int lvf_pose_only_create(lvf_ctx* ctx, const lvf_camera* cam0, int n, const double* ob, const int32_t* kf_idx,
                         const int32_t* pw_idx, int n_pw, const double* pw, lvf_batch** out);
/* first_ob[n][2] = right-image observation in the birth frame, ob[n][2] = current left observation;
 * parameter blocks (inv_depth[lm_idx], pose[kf1_idx], pose[kf2_idx]); weight = w_visual[kf2]. backend.cpp:134-139 */
int lvf_two_frame_create(lvf_ctx* ctx, const lvf_camera* left, const lvf_camera* right, int n,
                         const double* first_ob, const double* ob, const int32_t* lm_idx, const int32_t* kf1_idx,
                         const int32_t* kf2_idx, lvf_batch** out);
/* parameter block inv_depth[lm_idx]; weight = 5 * w_visual[kf_idx]   backend.cpp:119-124 */
int lvf_two_camera_create(lvf_ctx* ctx, const lvf_camera* left, const lvf_camera* right, int n,
                          const double* left_ob, const double* right_ob, const int32_t* lm_idx,
                          const int32_t* kf_idx, lvf_batch** out);
/* parameter blocks (pose,v,ba,bg)[kf_i], (pose,v,ba,bg)[kf_j]; sqrt_info = LLT(cov^-1).L^T is factorised
 * once here (the reference re-inverts on every Evaluate: imu_error.hpp:32). */
/* The caller VOUCHES that a TwoFrame batch has the shape Backend::BuildProblem always produces (backend.cpp:105-140) — sorted by current
 * keyframe, first keyframe < current keyframe, at most one block per (landmark, current keyframe), one first keyframe per landmark — and hands
 * blocks_per_kf2[n_kf]: lvf_problem_create then skips its host pass over the blocks.  A false claim gives wrong results; callers that cannot
 * prove it do not call this (include/lvf_ceres_adapter.hpp proves it block by block while adapt::Problem is being filled). */
int lvf_two_frame_set_shape(lvf_batch* two_frame, int n_kf, const int32_t* blocks_per_kf2);
/* Optional per-block weights of a TwoCamera batch = each functor's `weight` constructor argument (visual_error.hpp:112; the reference
 * passes 5 * frame->weights.visual, backend.cpp:123).  weight[n] replaces 5 * w_visual[kf_idx[i]]; NULL restores the per-keyframe rule. */
int lvf_two_camera_set_block_weights(lvf_batch* b, const double* weight);
int lvf_imu_create(lvf_ctx* ctx, int n, const lvf_preint* pre, const int32_t* kf_i, const int32_t* kf_j,
                   lvf_batch** out);
/* mode 0 = RPZ (pitch,roll,z), 1 = YXY (yaw,x,y).  p/pa/pb/pc [n][3]: the scan point and its three
 * map neighbours (association.cpp:303-314); the unit normal (pa-pb)x(pa-pc) is computed on device. */
int lvf_lidar_plane_create(lvf_ctx* ctx, int mode, int n, const double* p, const double* pa, const double* pb,
                           const double* pc, const double* Twc1, double weight, lvf_batch** out);
/* Weak-constraint pose priors of a window (backend.cpp:164-178).  Block i with kf_a[i] >= 0 is
 * PoseGraphError<6,7,7>(Twc1 = pose[kf_a], Twc2 = pose[kf_b]) with target[i][0..6) = rpyxyz_ (pose_error.hpp:13-17,
 * see lvf_relative_rpyxyz); with kf_a[i] < 0 it is PoseError<6,7>(pose[kf_b]) with target[i][0..7) = the origin pose
 * (pose_error.hpp:55-76); with kf_a[i] == -2 it is RError<4,7>(pose[kf_b]) with target[i][0..4) = the stored quaternion (x,y,z,w)
 * (pose_error.hpp:88-110; residual rows 4,5 and their Jacobian rows are zero padding).
 * target is [n][7]; weight[n], v[n] are the functor's (weight, v) ctor arguments.
 * Parameter blocks: 0 = pose[kf_a] (all-zero Jacobian for PoseError blocks), 1 = pose[kf_b]; 6 residuals. */
int lvf_pose_prior_create(lvf_ctx* ctx, int n, const int32_t* kf_a, const int32_t* kf_b, const double* target,
                          const double* weight, const double* v, lvf_batch** out);
/* rpyxyz6 = SE3ToRpyxyz(last_pose^-1 * pose): the constant PoseGraphError's constructor stores (host arithmetic). */
int lvf_relative_rpyxyz(const double* last_pose, const double* pose, double* rpyxyz6);
/* LiDAR planes on full keyframe poses: LidarPlaneError<1,7> (lidar_error.hpp:10-40, declared by the reference and never added to a
 * problem) as blocks of the sliding-window problem (lvf_problem_set_lidar_planes).  Block i: r = w_i n_i . (R(q/|q|) p_i + t - pa_i) on
 * pose[kf_idx[i]], n_i the unit normal of (pa - pb) x (pa - pc) (a zero cross product stays zero: a null block), p in the keyframe's body
 * frame, pa, pb, pc in the world frame; all [n][3].  weight (NULL = 1) and huber_a (NULL or <= 0 = no loss) are per block — the one
 * deviation from the functor: ground blocks take w = 1 and no loss, surf blocks w = 0.01 and a = 0.1 (mapping.cpp's conventions).  Blocks may
 * come in any order.  LVF_ERR_INVALID: a negative index, a non-finite input, a negative weight.  Declared semantics: tests/lidar_window_ref.py.
 * Parameter block 0 = pose[kf_idx]; 1 residual (lvf_batch_evaluate: st required; the raw residual, no loss applied). */
int lvf_lidar_pose_create(lvf_ctx* ctx, int n, const double* p, const double* pa, const double* pb, const double* pc, const int32_t* kf_idx,
                          const double* weight, const double* huber_a, lvf_batch** out);
/* The same batch from what lvf_knn3 left in n_scans (map, scan) pairs, gathered on the device (one launch per 16 scans, no wait): scan k's
 * queries become blocks on keyframe kf_idx[k] (non-decreasing) with the scan's weight[k] / huber_a[k] (NULL as above), the floats widened
 * to double as association.cpp:303-314 does.  Nothing is compacted: a query that failed the gate is a block of weight 0.
 * LVF_ERR_INVALID for a scan that was not searched (an empty scan has nothing to search and is accepted). */
int lvf_lidar_pose_from_scans(lvf_ctx* ctx, int n_scans, lvf_map* const* maps, lvf_scan* const* scans, const int32_t* kf_idx,
                              const double* weight, const double* huber_a, lvf_batch** out);
/* blocks of weight > 0; for a device-built batch this is the one call that waits for the gather */
int lvf_lidar_pose_num_valid(lvf_batch* b, int* n);
/* copies of the batch's inputs (each may be NULL): p, pa [n][3], kf_idx, weight, huber_a [n] */
int lvf_lidar_pose_download(lvf_batch* b, double* p, double* pa, int32_t* kf_idx, double* weight, double* huber_a);
int lvf_batch_destroy(lvf_batch* b);
int lvf_batch_size(const lvf_batch* b);
int lvf_batch_num_param_blocks(const lvf_batch* b);

/* Batched CostFunction::Evaluate: residuals (+ Jacobians if want_jacobians) in Ceres layout, left in HBM.
 * st supplies the parameter blocks.  For lidar batches st may be NULL and rpyxyz (host, 6 doubles — the
 * caller's LIVE array, lidar_error.hpp:52,87) is read at call time. */
int lvf_batch_evaluate(lvf_batch* b, const lvf_state* st, const double* rpyxyz, int want_jacobians);
/* Copies of the last evaluate's outputs.  block = parameter-block index in the functor's template order.
 * Sizes: residuals n*R doubles; jacobian(block) n*R*size_block doubles (row-major R x size per block). */
int lvf_batch_download_residuals(lvf_batch* b, double* host);
int lvf_batch_download_jacobian(lvf_batch* b, int block, double* host);
/* lidar batches only: the device-computed unit normals [n][3] */
int lvf_batch_download_normals(lvf_batch* b, double* host);
/* device pointers of the same buffers (valid until the batch is destroyed) */
void* lvf_batch_residuals_dev(lvf_batch* b);
void* lvf_batch_jacobian_dev(lvf_batch* b, int block);

/* Batched Problem::Evaluate surface (upstream ceres::Problem::Evaluate with apply_loss_function = true): residuals [n][R] with the loss
 * function's Corrector applied (visual batches: rows scaled by sqrt(rho'(|r|^2)) of HuberLoss(huber_a); huber_a <= 0 or non-visual
 * batches: unchanged; lidar-pose batches: each block's OWN huber_a, the argument does not apply) and Jacobians [n][R][L] in LOCAL coordinates, the block's parameter blocks concatenated in functor order with every
 * 7-sized pose block reduced to its 6 tangent columns (ProductParameterization(EigenQuaternion, Identity3), backend.cpp:99-101); absent
 * pose blocks (PoseError / RError priors) are zero.  L = lvf_batch_local_columns(b).  jacobians_local may be NULL.  Host outputs. */
int lvf_batch_local_columns(const lvf_batch* b);
int lvf_batch_evaluate_local(lvf_batch* b, const lvf_state* st, double huber_a, double* residuals, double* jacobians_local);

/* ---- IMU pre-integration on device ---------------------------------------------------------- */
/* n independent keyframe pairs; pair k owns samples[offset[k] .. offset[k+1]) rows of (dt, acc[3], gyr[3]);
 * acc0/gyr0 [n][3] are the measurements latched by the first Append; ba/bg [n][3] the linearisation biases;
 * noise4 = (ACC_N, GYR_N, ACC_W, GYR_W).  out[n] receives the propagated state. */
int lvf_preintegrate(lvf_ctx* ctx, int n, const int32_t* offset, const double* samples, const double* acc0,
                     const double* gyr0, const double* ba, const double* bg, const double* noise4, lvf_preint* out);

/* ---- scan-to-map association (float32, bit-exact 3-NN) --------------------------------------- */
/* map cloud: M points, xyz at the start of each `stride_floats`-float record (pcl::PointXYZI: 8).
 * Builds a uniform-grid index on device.  max_radius2 = the largest squared gate that will be queried
 * (e.g. resolution^2*100); it only sizes the cells, any thr may be queried later. */
int lvf_map_create(lvf_ctx* ctx, const float* map_xyz, int M, int stride_floats, float max_radius2, lvf_map** out);
/* n indices at once: out[i] is what lvf_map_create(ctx, map_xyz[i], M[i], stride_floats, max_radius2[i]) builds (the same pyramid, the same
 * association results), with the host waits shared between the maps — the old-frame maps of a set of loop-closure candidates
 * (relocator.cpp:196-206 -> Mapping::Relocate, mapping.cpp:251-262: one BuildOldMapFrame + kd-tree build per candidate and cloud).
 * On error no map is returned (out[i] = NULL for all i). */
int lvf_map_create_batch(lvf_ctx* ctx, int n, const float* const* map_xyz, const int* M, int stride_floats, const float* max_radius2,
                         lvf_map** out);
int lvf_map_destroy(lvf_map* m);
int lvf_scan_create(lvf_ctx* ctx, const float* scan_xyz, int Q, int stride_floats, lvf_scan** out);
int lvf_scan_destroy(lvf_scan* s);
/* For every scan point: point = SE3TransformPoint<float>(pose.cast<float>(), p); its 3 nearest map points by
 * squared L2 in float ((dx*dx+dy*dy)+dz*dz, no FMA), ties by ascending map index; valid iff all three
 * d2 < thr.  Outputs stay in HBM (owned by the scan).  idx/d2 are exact for valid points; for invalid
 * points they hold the best candidates found inside the gate radius (or -1/inf).  thr = +inf asks for the
 * exact 3-NN of every point. */
int lvf_knn3(lvf_map* m, lvf_scan* s, const double* pose, float thr);
int lvf_scan_download(lvf_scan* s, int32_t* idx3, float* d2_3, uint8_t* valid);
/* Diagnostic only: per-point search statistics and the grid pyramid levels4[L][4] = {cell, nx, ny, nz}; the caller provides room for 8
 * levels (the pyramid halves the cell per level, at most 8 levels).
 *   lvf_knn3_debug_stats : stats4[Q][4] = {candidates, range lookups, last grid level, shells}.
 *   lvf_knn3_debug_stats2: stats[Q][stride], 4 <= stride <= 6, the same four + {start, end} (the 100 MHz wall clock when the point's wave
 *                          began and finished, low 31 bits).  The record width is an ARGUMENT: it grew once under a fixed name. */
int lvf_knn3_debug_stats(lvf_map* m, lvf_scan* s, const double* pose, float thr, int32_t* stats4, float* levels4,
                         int* n_levels);
int lvf_knn3_debug_stats2(lvf_map* m, lvf_scan* s, const double* pose, float thr, int32_t* stats, int stride, float* levels4,
                          int* n_levels);

/* Test hook: the stable (key, value) pair sort under lvf_cloud_voxel_filter on host arrays; only the low key_bits bits of a key order the
 * pairs, equal keys keep their input order.  Not part of the reference surface. */
int lvf_debug_sort_pairs_u32(lvf_ctx* ctx, const uint32_t* keys, const int32_t* vals, int n, int key_bits, uint32_t* keys_out,
                             int32_t* vals_out);

/* ---- map-cloud maintenance on device (the steps immediately before the association) ------------- */
/* A cloud is n x (x, y, z, intensity) float32 in HBM (pcl::PointXYZI payload).  points: strided host records, xyz at the
 * start, intensity at float offset `intensity_offset` (4 for pcl::PointXYZI; -1 = none -> 0). */
int lvf_cloud_create(lvf_ctx* ctx, const float* points, int n, int stride_floats, int intensity_offset, lvf_cloud** out);
int lvf_cloud_destroy(lvf_cloud* c);
int lvf_cloud_size(const lvf_cloud* c);
int lvf_cloud_download(const lvf_cloud* c, float* xyzi /* [n][4] */);
/* Mapping::MergeScan / ToWorld / Sensor2Robot (mapping.cpp:193-220, association.cpp:236-247): out_i = SE3TransformPoint<float>
 * (pose.cast<float>(), in_i), intensity copied.  Bit-exact float arithmetic (normalise-then-rotate polynomial, no FMA). */
int lvf_cloud_transform(const lvf_cloud* in, const double* pose, lvf_cloud** out);
/* `merged += pointclouds[t]` of BuildMapFrame / BuildOldMapFrame (mapping.cpp:78-137): device-side concatenation. */
int lvf_cloud_concat(lvf_ctx* ctx, const lvf_cloud* const* parts, int n_parts, lvf_cloud** out);
/* FeatureAssociation::AlignScan (association.cpp:39-64): the keyframe's sweep [time - cycle/2, time + cycle/2] cut out of two consecutive raw
 * revolutions pc1 (stamped stamp1) + pc2 (stamp2 > stamp1) with the reference's index arithmetic (double, truncated); output points carry
 * intensity 0 (copyPointCloud from PointXYZ).  *aligned = 0 and an empty cloud where the reference returns false (sweep not covered). */
int lvf_cloud_align_scan(const lvf_cloud* pc1, double stamp1, const lvf_cloud* pc2, double stamp2, double cycle_time, double time, lvf_cloud** out,
                         int* aligned);
/* pcl::VoxelGrid<PointXYZI> with a cubic leaf (association.cpp:210-215, 222-224): per-voxel centroid of all four fields (float accumulation
 * over the voxel's points in ascending input index — reproducible bit for bit), voxels in ascending (i + j*dx + k*dx*dy) order. */
int lvf_cloud_voxel_filter(const lvf_cloud* in, float leaf, lvf_cloud** out);
/* pcl::RadiusOutlierRemoval (association.cpp:217-221): keeps a point iff more than min_neighbors points (itself
 * included) lie at squared distance < radius^2; input order preserved. */
int lvf_cloud_radius_outlier_filter(const lvf_cloud* in, float radius, int min_neighbors, lvf_cloud** out);
/* FeatureAssociation::SegmentGround (association.cpp:249-268): RANSAC plane (all hypotheses scored in one launch, PCL's
 * adaptive stopping rule applied in hypothesis order), least-squares refit, inliers extracted in input order.
 * coefficients4 (may be NULL) = (nx, ny, nz, d) with nz >= 0; iterations_used (may be NULL) = hypotheses consumed.
 * Sampling is splitmix64(seed, hypothesis, draw) — PCL's boost::mt19937 stream is not reproducible without PCL. */
int lvf_cloud_segment_plane(const lvf_cloud* in, float distance_threshold, int max_iterations, uint64_t seed, lvf_cloud** out,
                            double* coefficients4, int* iterations_used);
/* ---- LiDAR feature extraction of one keyframe scan: FeatureAssociation::Process, association.cpp:86-235 - */
typedef struct lvf_lidar_params {
  int num_scans, horizon_scan;       /* 64, 1800 (config/kitti.yaml:35-36); num_scans <= 64 */
  float ang_res_y, ang_bottom;       /* 0.427, 24.9 */
  int ground_rows;                   /* 60 */
  double cycle_time;                 /* 0.1036 (a double in FeatureAssociation) */
  float min_range, max_range, resolution;   /* 5, 30, 0.2 */
  uint64_t ransac_seed;              /* SegmentGround's sampler (see lvf_cloud_segment_plane) */
} lvf_lidar_params;
void lvf_lidar_params_default(lvf_lidar_params* p);
/* optional taps for parity tests: host arrays (may each be NULL) sized num_scans*horizon_scan (label/ground/range) or
 * num_scans*horizon_scan*4 floats (ground_raw / surf_raw = ExtractFeatures' picks before the PCL filters) */
typedef struct lvf_lidar_extract_debug {
  int n_filtered, n_segmented, n_ground_raw, n_surf_raw;
  int32_t* label_mat; int8_t* ground_mat; float* range_mat; float* ground_raw; float* surf_raw;
} lvf_lidar_extract_debug;
/* points: the raw sensor-frame scan (xyz at the start of each stride_floats record, scan order = acquisition order);
 * extrinsic7 = Lidar::Get()->extrinsic (sensor -> robot).  ground_out / surf_out = frame->feature_lidar->points_ground /
 * points_surf as NEW device clouds (robot frame; intensity = ring + relative time as the reference writes it). */
int lvf_lidar_extract(lvf_ctx* ctx, const float* points, int n, int stride_floats, const lvf_lidar_params* prm, const double* extrinsic7,
                      lvf_cloud** ground_out, lvf_cloud** surf_out, lvf_lidar_extract_debug* dbg);
/* Test / A-B hook, process-wide: 1 = lvf_lidar_extract takes the host-counted path of rounds 2-4 (every stage's output count is read back
 * before the next stage is sized: 13 stream waits per scan) instead of the device-counted one (one wait); returns the previous setting.  The
 * environment variable LVF_EXTRACT_HOST_COUNTS=1 sets the initial value.  Not part of the reference surface. */
int lvf_debug_extract_host_counts(int on);
/* Test hook, process-wide: the number of scans, since the library was loaded, that entered the device-counted path and were handed to the
 * host-counted one (parameters outside the tail's plan, or the tail's verdict).  A test that compares the two paths reads it before and after
 * to show which one produced a result.  Not part of the reference surface. */
int lvf_debug_extract_fallbacks(void);

/* ---- LiDAR sweep deskew: motion compensation along a stamped trajectory ------------------------------------------------------------------ */
/* The step the reference declares and never calls: the `deskew` key of its configs (estimator.cpp:152), FeatureAssociation::deskew_
 * (association.h:22,65), the `//TODO:deskew` of AdjustDistortion (association.cpp:142-145), and the implementation written for it
 * (association.cpp:65-83, map.cpp:92-102).  The semantics are DECLARED (tests/deskew_ref.py): the reference's arithmetic with two
 * deviations — the bracket of a time is (last stamp <= t, the next stamp) and the fraction s is not clamped, so the end brackets extrapolate
 * (Map::ComputePose's lower_bound / upper_bound pair names ONE keyframe for every time that is not a stamp: t_t = 0); the time offset of a
 * point is I - floorf(I + 0.5f) (UndistortPoint's I - int(I) is a second off for a negative offset on ring >= 1). */
/* lvf_trajectory: Map::keyframes as ComputePose reads it (map.h: time -> Frame, Frame::pose): n >= 1 stamps, strictly increasing, with
 * poses [qx,qy,qz,qw,tx,ty,tz] (the quaternion is normalised on entry, as Sophus' SE3d(q, t) constructor does), mirrored on the device.
 * _append adds a keyframe behind the last one; _set_pose replaces the pose of keyframe i (the backend moves keyframes after they were
 * inserted); both are in effect for the next call.  LVF_ERR_INVALID, before anything touches the device: n < 1, a stamp that does not
 * increase, a non-finite stamp or pose, a zero quaternion, an index outside [0, size). */
typedef struct lvf_trajectory lvf_trajectory;
int lvf_trajectory_create(lvf_ctx* ctx, const double* stamps, const double* poses7, int n, lvf_trajectory** out);
int lvf_trajectory_append(lvf_trajectory* traj, double stamp, const double* pose7);
int lvf_trajectory_set_pose(lvf_trajectory* traj, int i, const double* pose7);
int lvf_trajectory_size(const lvf_trajectory* traj);
int lvf_trajectory_destroy(lvf_trajectory* traj);
/* Map::ComputePose (map.cpp:92-102) for m times, evaluated on the device by the function the cloud kernel calls: n == 1 returns that pose;
 * else i = clamp(#{stamps <= t} - 1, 0, n - 2), s = (t - stamp_i) / (stamp_i+1 - stamp_i), Eigen's slerp(s, q_i, q_i+1) normalised, and
 * (1 - s) t_i + s t_i+1.  poses7_out: [m][7] host doubles. */
int lvf_trajectory_compute_pose(const lvf_trajectory* traj, const double* times, int m, double* poses7_out);
/* FeatureAssociation::UndistortPointCloud (association.cpp:65-83) on a SENSOR-frame cloud whose intensity carries ring + time offset as
 * AdjustDistortion writes it (association.cpp:141-143; lvf_lidar_extract's picks): for every point, t = frame_time - cycle_time / 2 + offset,
 * p1 = ComputePose(t) * extrinsic * p (Sensor2World, sensor.h:21-24), p2 = extrinsic^-1 * frame_pose^-1 * p1 (World2Sensor, sensor.h:16-19),
 * in double, rounded to float; intensity copied.  A new cloud of the same size and order; a point with a non-finite field is copied
 * unchanged; with a one-pose trajectory the cloud is copied bit for bit.  cycle_time must lie in (0, 0.4): the offset has to stay inside
 * (-0.5, 0.5) for the ring to be recoverable.  LVF_ERR_INVALID on the host for a null trajectory, non-finite arguments or a zero quaternion. */
int lvf_cloud_deskew(const lvf_cloud* in, const lvf_trajectory* traj, double frame_time, const double* frame_pose7, double cycle_time, const double* extrinsic7,
                     lvf_cloud** out);
/* lvf_lidar_extract with the deskew applied where AdjustDistortion's TODO stands (association.cpp:144).  Everything behind that line that
 * reads coordinates is the PCL tail (association.cpp:210-232) — the smoothness and the six-sector picks read segmented_info.range and flags
 * only (:149-207) — so the pass runs on ExtractFeatures' two pick clouds ahead of their VoxelGrid: a few thousand points, inside the same
 * one-wait launch chain.  The outputs equal lvf_cloud_deskew of the plain call's picks pushed through lvf_cloud_voxel_filter /
 * _radius_outlier_filter / _segment_plane / _transform bit for bit; dbg->ground_raw / surf_raw hold the DESKEWED picks, the other taps
 * are lvf_lidar_extract's.  cycle_time is prm->cycle_time. */
int lvf_lidar_extract_deskewed(lvf_ctx* ctx, const float* points, int n, int stride_floats, const lvf_lidar_params* prm, const double* extrinsic7,
                               const lvf_trajectory* traj, double frame_time, const double* frame_pose7, lvf_cloud** ground_out, lvf_cloud** surf_out,
                               lvf_lidar_extract_debug* dbg);
/* ---- LiDAR edge picks inside the extraction chain ---------------------------------------------------------------------------------------- */
/* The reference declares points_sharp / points_less_sharp (lidar/feature.h:23-24, commented out) and computes the curvature that would
 * select them (association.cpp:149-166) but only uses it to keep points out of the surf set (:202).  DECLARED pick rule (LOAM's, restated
 * in tests/edge_ref.py): per ring and per sector [sp, ep] of ExtractFeatures (association.cpp:186-194), independently, a candidate is a
 * non-ground point with curvature >= edge_threshold (the curvature array of the surf test, stale ends read as 0; the default 1.0f is the
 * complement of that test, so surf and edge sets are disjoint).  Repeatedly the unsuppressed candidate that is largest under (curvature
 * descending, segmented index ascending) is taken and every point of the sector within +-5 segmented indices of it is suppressed, until
 * n_less_sharp picks were made or no candidate is left.  The first n_sharp picks of a sector form `sharp`, all of them `less_sharp`; both
 * clouds are emitted in ascending segmented index, intensity = ring + relative time as for the other picks. */
typedef struct lvf_edge_params {
  float edge_threshold;    /* 1.0f */
  int n_sharp;             /* 2 (LOAM) */
  int n_less_sharp;        /* 20 (LOAM) */
} lvf_edge_params;
void lvf_edge_params_default(lvf_edge_params* p);
/* optional taps (host arrays, may each be NULL): sharp_raw / less_sharp_raw = the picks in the SENSOR frame before any deskew, sized
 * min(num_scans*horizon_scan, n)*4 floats; curvature, sharp_flags, less_sharp_flags = one entry per segmented point
 * (lvf_lidar_extract_debug.n_segmented of them; size min(num_scans*horizon_scan, n)) */
typedef struct lvf_edge_extract_debug {
  int n_sharp_raw, n_less_sharp_raw;
  float* sharp_raw; float* less_sharp_raw; float* curvature; int32_t* sharp_flags; int32_t* less_sharp_flags;
} lvf_edge_extract_debug;
/* lvf_lidar_extract (traj == NULL; frame_time and frame_pose7 are ignored) or lvf_lidar_extract_deskewed (traj given) with the edge picks
 * made inside the same one-wait launch chain: ground_out / surf_out are that call's, bit for bit.  sharp_out / less_sharp_out are NEW device
 * clouds in the robot frame: the raw picks, deskewed like lvf_cloud_deskew when traj is given, then lvf_cloud_transform by extrinsic7.  No
 * voxel or outlier filter is applied to them (lvf_cloud_voxel_filter is there for callers who want one). */
int lvf_lidar_extract_edges(lvf_ctx* ctx, const float* points, int n, int stride_floats, const lvf_lidar_params* prm, const double* extrinsic7,
                            const lvf_edge_params* edge, const lvf_trajectory* traj, double frame_time, const double* frame_pose7,
                            lvf_cloud** ground_out, lvf_cloud** surf_out, lvf_cloud** sharp_out, lvf_cloud** less_sharp_out,
                            lvf_lidar_extract_debug* dbg, lvf_edge_extract_debug* edge_dbg);
/* kNN index / query scan straight from device-resident clouds (no host round trip) */
int lvf_map_create_from_cloud(const lvf_cloud* c, float max_radius2, lvf_map** out);
/* ... of n device-resident clouds in one call (lvf_map_create_batch's shared waits and launches, no upload): the old-frame maps of a set of
 * loop-closure candidates whose per-keyframe clouds are kept as lvf_cloud (relocator.cpp:196-206 -> mapping.cpp:251-262) */
int lvf_map_create_batch_from_clouds(lvf_ctx* ctx, int n, const lvf_cloud* const* clouds, const float* max_radius2, lvf_map** out);
int lvf_scan_create_from_cloud(const lvf_cloud* c, lvf_scan** out);

/* ---- one scan-to-map sub-problem (3-DoF LM on device) ---------------------------------------- */
typedef struct lvf_icp_options {
  int mode;                /* 0 = ground/RPZ (TrivialLoss), 1 = surf/YXY (HuberLoss(0.1)) */
  float thr;               /* squared distance gate */
  double weight;           /* frame->weights.lidar_ground / lidar_surf */
  double huber_a;          /* <=0: TrivialLoss (association.cpp:272), 0.1 for surf (:330) */
  double prior_weight;     /* PoseErrorRPZ/YXY weight = |features_left| * weights.visual; 0 = relocate mode */
  int max_num_iterations;  /* 4 (mapping.cpp:161) */
} lvf_icp_options;
typedef struct lvf_icp_summary {
  double initial_cost, final_cost;
  int num_residual_blocks; /* valid correspondences (+1 if prior) — Summary::num_residual_blocks_reduced */
  int num_iterations;
  int num_successful_steps;
} lvf_icp_summary;
/* Runs association at frame_pose (the frame's current pose, cast to float as association.cpp:287), builds the
 * point-to-plane problem against map_pose (Twc1) and solves it on device; rpyxyz (host, 6 doubles =
 * se32rpyxyz(map_pose^-1 * frame_pose), mapping.cpp:154) is updated IN PLACE like the reference's stack array
 * (mapping.cpp:153-165).  The caller then sets frame->pose = map_pose * rpyxyz2se3(rpyxyz) (mapping.cpp:164). */
int lvf_icp_solve(lvf_map* m, lvf_scan* s, const double* map_pose, const double* frame_pose, double* rpyxyz,
                  const lvf_icp_options* opt, lvf_icp_summary* summary);

/* ---- LiDAR edge features: line association, point-to-line factor, the yaw-x-y solve over planes AND lines ----
 * The reference declares edge clouds (lidar/feature.h:23-24, commented out) and has no edge functor at this commit: the semantics below
 * are DECLARED (LOAM's published line test and point-to-line distance), restated in numpy in tests/edge_ref.py.
 *
 * Line association.  Per scan point: the float transform of lvf_knn3, its FIVE nearest map points by the same float d2 (ties by
 * ascending map index) on the grid pyramid the map owns.  From the five float points as doubles, in neighbour order: centroid
 * c = (plain sum) / 5, C = sum (x - c)(x - c)^T, eigenvalues l1 >= l2 >= l3; d = unit eigenvector of l1.  valid iff all five d2 < thr
 * and l1 > 0 and l1 > min_eigen_ratio * l2 (LOAM: 3).  The line is stored as c and the projector I - d d^T (independent of d's sign).
 * Outputs are owned by the scan, beside (not over) the plane correspondences of lvf_knn3 / lvf_icp_solve. */
int lvf_edge_associate(lvf_map* m, lvf_scan* s, const double* pose, float thr, double min_eigen_ratio);
/* idx5[Q][5], d2_5[Q][5], valid[Q], corr12[12][Q] (SoA rows: scan point xyz | centroid xyz | projector 00 01 02 11 12 22; zero for an
 * invalid point).  Any output may be NULL.  idx5 / d2_5 are exact for valid points (as lvf_knn3's). */
int lvf_scan_download_edges(lvf_scan* s, int32_t* idx5, float* d2_5, uint8_t* valid, double* corr12);

/* LidarEdgeErrorYXY / LidarEdgeErrorRPZ <3,1,1,1> evaluated stand-alone for n blocks: r = weight * P (Twc2 p - c) with
 * Twc2 = Twc1 * RpyxyzToSE3(rpyxyz) as LidarPlaneErrorYXY / RPZ form it (lidar_error.hpp:42-110); row k is the plane residual with normal
 * P[k,:] and anchor c.  mode 0: parameters (pitch, roll, z); mode 1: (yaw, x, y).  Host arrays p[n][3], c[n][3], proj6[n][6]
 * (00 01 02 11 12 22); residuals[n][3]; jacobians (may be NULL) [n][3][3] = d r_k / d parameter_j.  No loss function is applied. */
int lvf_lidar_edge_evaluate(lvf_ctx* ctx, int mode, int n, const double* p, const double* c, const double* proj6, const double* Twc1,
                            const double* rpyxyz, double weight, double* residuals, double* jacobians);

typedef struct lvf_edge_icp_options {
  float thr;               /* squared distance gate of the 5-NN */
  double weight;           /* factor weight */
  double huber_a;          /* HuberLoss width on the BLOCK (s = |r|^2, all three rows scaled by sqrt(rho'(s))); <= 0: TrivialLoss */
  double min_eigen_ratio;  /* line test */
} lvf_edge_icp_options;
/* declared values (no reference value exists): the surf gate resolution^2 * 25, the surf weight (double)0.01f, HuberLoss(0.1), ratio 3 */
void lvf_edge_icp_options_default(lvf_edge_icp_options* o, double lidar_resolution);
/* lvf_icp_solve's (yaw, x, y) problem with point-to-line blocks beside the point-to-plane blocks: both associations run at frame_pose,
 * then the same device-resident LM runs over planes and lines (an edge block adds three rows to the normal equations, rho(s) / 2 to the
 * cost and one residual block).  opt->mode must be 1.  Either (map, scan) pair may be NULL; with the edge pair NULL this IS
 * lvf_icp_solve.  num_residual_blocks = planes + lines (+ 1 with the prior). */
int lvf_icp_solve_edges(lvf_map* map_surf, lvf_scan* scan_surf, lvf_map* map_edge, lvf_scan* scan_edge, const double* map_pose,
                        const double* frame_pose, double* rpyxyz, const lvf_icp_options* opt, const lvf_edge_icp_options* edge_opt,
                        lvf_icp_summary* summary);

/* ---- one frame's scan-to-map update: Mapping::Optimize's body (mapping.cpp:147-178) / Mapping::Relocate (:251-300) ---- */
typedef struct lvf_scan_match_options {
  float thr_ground, thr_surf;      /* resolution^2 * 100 / * 25 (association.cpp:285,343) */
  double weight_ground, weight_surf; /* frame->weights.lidar_ground / lidar_surf — FLOAT fields in the reference (adapt/weights.h:10-12): pass the
                                      * float's value, e.g. (double)0.01f, which is what lvf_scan_match_options_default sets */
  double huber_surf;               /* 0.1 (association.cpp:330); ground uses TrivialLoss */
  double prior_weight;             /* |features_left| * weights.visual; 0 = relocate mode (association.cpp:321,379) */
  int outer_iterations;            /* 1 = Mapping::Optimize, 4 = Mapping::Relocate (mapping.cpp:264) */
  int max_num_iterations;          /* 4 */
} lvf_scan_match_options;
typedef struct lvf_scan_match_result {
  double pose[7];                  /* the frame's pose after the update */
  double relative_o_c[7];          /* last_pose^-1 * pose (mapping.cpp:298); = pose when last_pose is NULL */
  double score_ground, score_surf; /* mapping.cpp:279-280, :293-294 (last outer iteration) */
  int score;                       /* (int)(score_ground + score_surf): Mapping::Relocate's return value */
  lvf_icp_summary ground, surf;    /* summaries of the last ground / surf sub-problem */
} lvf_scan_match_result;
void lvf_scan_match_options_default(lvf_scan_match_options* o, double lidar_resolution);
/* Either (map, scan) pair may be NULL (empty cloud: the reference skips that sub-problem).  All four handles must
 * belong to one context. */
int lvf_scan_match(lvf_map* map_ground, lvf_scan* scan_ground, lvf_map* map_surf, lvf_scan* scan_surf, const double* map_pose,
                   const double* frame_pose, const double* last_pose, const lvf_scan_match_options* opt,
                   lvf_scan_match_result* result);
/* The same update with lvf_icp_solve_edges as the second sub-problem of every outer iteration (planes and lines together; result->surf
 * and score_surf count both).  With the edge pair NULL this IS lvf_scan_match.  A single-frame chain: the pose is composed on the host
 * between the sub-problems. */
int lvf_scan_match_edges(lvf_map* map_ground, lvf_scan* scan_ground, lvf_map* map_surf, lvf_scan* scan_surf, lvf_map* map_edge,
                         lvf_scan* scan_edge, const double* map_pose, const double* frame_pose, const double* last_pose,
                         const lvf_scan_match_options* opt, const lvf_edge_icp_options* edge_opt, lvf_scan_match_result* result);

/* Many scan-to-map updates of ONE context advanced side by side: the loop-closure candidates Relocator::Relocate evaluates one after the
 * other (relocator.cpp:196-206 -> Mapping::Relocate, mapping.cpp:251-300: no shared mutable state between candidates).  Every launch of
 * the chain covers all candidates (the candidate is a grid dimension), each candidate's pose / rpyxyz / scores live in a device record
 * between its sub-problems, and the n results are read back once.  results[i] equals lvf_scan_match on candidate i (which IS this call
 * with n = 1).  A candidate's pairs may be NULL like lvf_scan_match's; scan handles must not repeat across candidates (a scan owns its
 * association outputs).  best (may be NULL) = the reference's choice: the LAST candidate whose score - relocate_base_score is > 0 and
 * >= every earlier one (relocator.cpp:181,198-204; 20 in the reference), or -1. */
typedef struct lvf_scan_match_job {
  lvf_map* map_ground; lvf_scan* scan_ground; lvf_map* map_surf; lvf_scan* scan_surf;
  double map_pose[7], frame_pose[7], last_pose[7];
  int has_last_pose;               /* 0: relative_o_c = pose (lvf_scan_match's last_pose == NULL) */
} lvf_scan_match_job;
int lvf_scan_match_batch(lvf_ctx* ctx, const lvf_scan_match_job* jobs, int n, const lvf_scan_match_options* opt, int relocate_base_score,
                         lvf_scan_match_result* results, int* best);

/* The same device-resident 3-DoF solve over a caller-built lidar batch (lvf_lidar_plane_create): what adapt::Solve
 * does for the problem ScanToMapWithGround/Segmented assembled (mapping.cpp:157-163, :270-296).  mode, weight and Twc1
 * are the batch's; opt supplies huber_a, prior_weight and max_num_iterations (opt->mode/weight/thr are ignored). */
int lvf_lidar_solve(lvf_batch* lidar_batch, double* rpyxyz, const lvf_icp_options* opt, lvf_icp_summary* summary);

/* PoseErrorRPZ / PoseErrorYXY <3,1,1,1> (pose_error.hpp:135-190) evaluated stand-alone.  target3 and x3 are in PARAMETER
 * order — (pitch, roll, z) for mode 0, (yaw, x, y) for mode 1; residuals3 in the functor's order — (roll, pitch, z) /
 * (yaw, x, y); jacobians9 (may be NULL) = three 3x1 blocks, one per parameter block, concatenated. */
int lvf_prior3_evaluate(lvf_ctx* ctx, int mode, const double* target3, double weight, const double* x3, double* residuals3,
                        double* jacobians9);

/* ---- sliding-window BA problem (adapt::Problem + adapt::Solve) --------------------------------- */
typedef struct lvf_solver_options {
  int max_num_iterations;          /* Ceres default 50; UpdateFrontend uses 1 (backend.cpp:264) */
  double max_solver_time_in_seconds; /* backend.cpp:208 ; <=0 = unlimited */
  double huber_a;                  /* shared HuberLoss(1.0) on visual blocks (backend.cpp:98) */
  double initial_trust_region_radius; /* 1e4 */
  double function_tolerance;       /* 1e-6 */
  double gradient_tolerance;       /* 1e-10 */
  double parameter_tolerance;      /* 1e-8 */
  double min_relative_decrease;    /* 1e-3 */
} lvf_solver_options;
typedef struct lvf_solver_summary {
  double initial_cost, final_cost;
  int num_iterations, num_successful_steps;
  int num_residual_blocks;
  int termination; /* 0 convergence, 1 no_convergence (iteration/time cap), 2 failure */
  int num_unsuccessful_steps; /* rejected + invalid steps (Summary::num_unsuccessful_steps) */
  int termination_reason;     /* LVF_WHY_*: which test of ceres::Solve's TrustRegionMinimizer ended the loop */
  int hand_over_retries;      /* iterations this problem has re-run (over its lifetime) because an in-launch hand-over between chained sparse levels
                               * timed out on a busy GPU; each was repeated with un-chained launches — results are unaffected, only slower */
} lvf_solver_summary;
/* ceres::Solve's termination tests in the order the loop applies them (upstream trust_region_minimizer.cc; the test oracle restates the same loop):
 * before a step — gradient_max_norm <= gradient_tolerance, radius < 1e-32 (both CONVERGENCE, the pass does not count as an iteration);
 * after the linear solve — 5 consecutive invalid steps (solver failure or model_cost_change <= 0; FAILURE, else radius *= 0.5);
 * with the candidate — step_norm <= parameter_tolerance (x_norm + parameter_tolerance), then |cost - candidate_cost| <= function_tolerance cost
 * (both CONVERGENCE, the candidate is NOT taken); after the step — num_iterations >= max_num_iterations (NO_CONVERGENCE), radius < 1e-32. */
enum { LVF_WHY_NONE = 0, LVF_WHY_GRADIENT = 1, LVF_WHY_PARAMETER = 2, LVF_WHY_FUNCTION = 3, LVF_WHY_MIN_RADIUS = 4, LVF_WHY_MAX_ITERATIONS = 5,
       LVF_WHY_INVALID_STEPS = 6, LVF_WHY_TIME = 7,
       LVF_WHY_HANDOVER = 8 /* internal: the device loop stopped for a hand-over retry; only reported if the retry could not run either */ };
void lvf_solver_options_default(lvf_solver_options* o);
/* The problem borrows the state and the batches (they must outlive it).  Any of the batch pointers may
 * be NULL.  Pose blocks use ProductParameterization(EigenQuaternion, Identity3) (backend.cpp:99-101). */
int lvf_problem_create(lvf_ctx* ctx, lvf_state* st, lvf_batch* two_camera, lvf_batch* two_frame,
                       lvf_batch* pose_only, lvf_batch* imu, lvf_problem** out);
int lvf_problem_destroy(lvf_problem* p);
/* Adds (or with NULL removes) the window's pose-prior batch (ProblemType::Other blocks with no loss function). */
int lvf_problem_set_pose_priors(lvf_problem* p, lvf_batch* pose_priors);
/* Adds (or with NULL removes) LiDAR plane blocks on the window's keyframe poses (lvf_lidar_pose_create / _from_scans; the batch is
 * borrowed).  Every entry that linearises or evaluates the problem sees them: cost, gradient, lm_iteration, solve, download_reduced,
 * marginal.  A problem with such blocks runs the chain a problem with pose priors runs (no fused candidate pass, no table launches). */
int lvf_problem_set_lidar_planes(lvf_problem* p, lvf_batch* lidar_planes);
int lvf_problem_set_pose_constant(lvf_problem* p, int kf, int is_constant);
/* SetParameterBlockConstant on keyframe kf's velocity / accelerometer-bias / gyroscope-bias blocks (Environment::Optimize holds all of
 * them, and the previous frame's, constant: environment.cpp:62-68): the ImuError factors keep their residuals, the blocks get no
 * Jacobian columns and are left out of the step norm's x_norm like Ceres' reduced program does. */
int lvf_problem_set_vbb_constant(lvf_problem* p, int kf, int v_constant, int ba_constant, int bg_constant);
/* Problem::Evaluate-style cost at the current state: 0.5 * sum rho(|r|^2). */
int lvf_problem_cost(lvf_problem* p, const lvf_solver_options* o, double* cost);
/* One Levenberg-Marquardt iteration from the current state with trust-region radius *radius (updated);
 * accepted != 0 if the step was taken.  Deterministic per-iteration parity point. */
int lvf_problem_lm_iteration(lvf_problem* p, const lvf_solver_options* o, double* radius, double* decrease_factor,
                             double* cost_before, double* cost_after, int* accepted);
int lvf_problem_solve(lvf_problem* p, const lvf_solver_options* o, lvf_solver_summary* summary);
/* Debug/parity taps of the last linearisation: reduced (Schur) system S [d x d row-major], rhs [d],
 * d = 15 * n_kf (pose tangent 6 | v 3 | ba 3 | bg 3 per keyframe).  Available after lvf_problem_lm_iteration (the per-call API keeps the
 * normal equations of its iteration); lvf_problem_solve / lvf_problem_batch_solve clear them at the end of every iteration for the
 * next one, so after those the tap returns LVF_ERR_STATE ("no linearisation yet"). */
int lvf_problem_reduced_dim(lvf_problem* p);
int lvf_problem_download_reduced(lvf_problem* p, double* S, double* rhs);

/* ---- a batch of independent windows on ONE GPU -------------------------------------------------------------------------------------
 * W windows (each its own lvf_state / batches / lvf_problem, all of one context) advanced by ONE chain of launches per LM iteration: every
 * kernel of the iteration takes the window as blockIdx.y and reads that window's argument block from a device table.  A single window's
 * iteration is a chain of small launches that leaves most of the 256 CUs idle; a batch fills the same launches W times over — the shape of
 * the reference's independent-window clients (RL environments: src/environment.cpp:18-115; loop-closure candidates: relocator.cpp:196-206)
 * and of what one GPU of the 8-GPU sharding works on.  The LM loop of every window runs on device (accept / reject, trust region and
 * termination per window; a finished window's launches return immediately).  Per-window results equal lvf_problem_solve /
 * lvf_problem_lm_iteration on that window alone up to summation order (a batch of more than one window sums its Schur complement over
 * wider landmark slices: same accept / reject decisions and iteration counts, states within ~1e-12 relative).  Windows that cannot use the table launches (no sorted TwoFrame work list, pose priors,
 * no IMU blocks) make the batch fall back to running the windows' own chains back to back on the context's stream.
 * All result arrays have one entry per window, in the order of `problems`. */
int lvf_problem_batch_create(lvf_ctx* ctx, lvf_problem* const* problems, int n, lvf_problem_batch** out);
/* The batch BORROWS its problems and changes nothing of theirs (its wider Schur slices and their work lists are the batch's own): a window
 * solved alone, in a batch, and alone again runs the same arithmetic the first and the third time.  Destroy order is free: a batch whose
 * member was destroyed first is marked orphaned (later calls on it return LVF_ERR_STATE) and may still be destroyed. */
int lvf_problem_batch_destroy(lvf_problem_batch* b);
int lvf_problem_batch_size(const lvf_problem_batch* b);
/* 1: table launches (one chain for all windows), 0: fallback, -1: error */
int lvf_problem_batch_uses_tables(lvf_problem_batch* b, const lvf_solver_options* o);
int lvf_problem_batch_lm_iteration(lvf_problem_batch* b, const lvf_solver_options* o, double* radius, double* decrease_factor, double* cost_before,
                                   double* cost_after, int* accepted);
int lvf_problem_batch_solve(lvf_problem_batch* b, const lvf_solver_options* o, lvf_solver_summary* summaries);

/* Measurement tap (bench.py's roofline lines): `reps` LM iterations from the current state, timed on the library's stream.  us[k] = average
 * duration of stage k in microseconds (the sum of its kernels' own durations: see lvf_problem_stage_times2), launches[k] (may be NULL) =
 * kernel launches it consists of; k < lvf_problem_stage_count(), names from lvf_problem_stage_name. */
int lvf_problem_stage_count(void);
const char* lvf_problem_stage_name(int stage);
int lvf_problem_stage_times(lvf_problem* p, const lvf_solver_options* o, double radius, int reps, double* us, int* launches);
/* The same with both clocks: us[k] = the sum of the stage's KERNEL durations (a start / stop event pair recorded with every launch — the
 * dispatch's own timestamps, what rocprofv3 --kernel-trace reports); spans_us[k] (may be NULL) = the time between the events that bracket
 * the stage on the stream (kernels + gaps + the markers' own cost). */
int lvf_problem_stage_times2(lvf_problem* p, const lvf_solver_options* o, double radius, int reps, double* us, double* spans_us, int* launches);

/* Problem::Evaluate's gradient at the current state: J^T r with the Corrector applied and pose blocks in tangent coordinates.
 * gc[15 n_kf] = (6 x n_kf pose tangents | 9 x n_kf (v, ba, bg)); gl[n_lm] (may be NULL) = the inverse-depth entries.  Constant poses: 0. */
int lvf_problem_gradient(lvf_problem* p, const lvf_solver_options* o, double* gc, double* gl);
/* Test hook (tests/test_gpu_solver.py): the next n chained hand-overs of this problem wait for a producer that never arrives and time out
 * after 20 us, so the retry path (LVF_WHY_HANDOVER -> un-chained re-run, lvf_solver_summary::hand_over_retries) can be exercised on an
 * idle GPU.  Also re-enables chaining for the problem.  Not part of the reference surface. */
int lvf_problem_debug_force_handover_timeout(lvf_problem* p, int n);
/* Diagnostic: 1 when the problem's current launch chain takes the (v, ba, bg) back substitution as one product with the matrix G formed
 * under the dense factorisation, 0 when it runs the sequential sparse levels (environment LVF_BACK_PRODUCT=0, more sparse levels than block
 * steps, or the two-launch back substitution); negative on error.  Builds the chain if it is stale.  It describes the problem's OWN
 * single-window chain: a batch (lvf_problem_batch_*) always runs the sequential levels, whatever this returns for its members.  Not part of
 * the reference surface. */
int lvf_problem_debug_back_product(lvf_problem* p);
/* Diagnostic: 1 when the problem's current launch chain runs the dense part of the back substitution on the block products
 * T_kj = -Dinv_k L_jk^T that riders of the block-step launches store, 0 when it reads the factor and Dinv (one block, a corner with more
 * blocks than the kernel holds products for, a dense corner of a multiple of 64 unknowns, LVF_BACK_BLOCKS=0, the re-run after a hand-over
 * time-out); negative on error.  Builds the chain if it is stale; a batch never takes the block form.  Not part of the reference surface. */
int lvf_problem_debug_back_blocks(lvf_problem* p);
/* Diagnostic (environment LVF_LM_HISTORY=1 when the problem's launch chain is built): out512 receives eight doubles per closed pass of the
 * last device-loop solve, slot = iteration & 63: {iteration, cost at the point, candidate cost, model cost change, accepted, failure flag,
 * trust-region radius used, gradient max norm}.  LVF_ERR_STATE without the environment variable. */
int lvf_problem_debug_history(lvf_problem* p, double* out512);
/* Test tap of the reduced solve (tests/test_gpu_reduced_solve.py): S [d x d] (symmetric, only the lower triangle is read) and rhs [d] in the
 * layout and natural unknown order of lvf_problem_download_reduced are COPIED (the caller's arrays are free afterwards), and from then on every
 * iteration of lvf_problem_lm_iteration / lvf_problem_solve on this problem linearises as usual, assembles its own damped system the way
 * lvf_problem_download_reduced does (so the elimination order, the identity padding of the last block, Dinv / Ldiag are production's), writes
 * the caller's d x d entries and rhs row over the assembled ones and then runs the production chain on that: the (v, ba, bg) elimination
 * levels (each a launch of its own), the block steps with their G riders, the back substitution lvf_problem_debug_back_product reports, the
 * candidate cost and the decision.  Not used while it is set: the placement of the early levels inside the launches ahead of them, and the
 * fused candidate pass.  The step satisfies S x = rhs; the model cost change the decision judges still comes from the problem's own gradient
 * and blocks.  The system must keep the sparsity pattern of the problem's own (the elimination plan reads no other entry of the (v, ba, bg)
 * columns).  Both NULL: clear (clearing twice is fine); one NULL: LVF_ERR_INVALID.  After a change of the problem's size the override must
 * be set again (LVF_ERR_INVALID from the iteration).  lvf_problem_batch_* calls on a batch holding such a problem return LVF_ERR_STATE. */
int lvf_problem_debug_override_reduced(lvf_problem* p, const double* S, const double* rhs);
/* The reduced step x [d] of the last lvf_problem_lm_iteration / lvf_problem_solve iteration, in the natural unknown order and the coordinates of
 * the system it solved (the chain solves the unscaled system: Jacobi scaling only shapes the damping), and the raw failure flag that iteration
 * left: 0, 1 + kb (block step kb of the dense corner met a non-positive or NaN pivot), the sparse base + keyframe (an elimination level did),
 * or the hand-over base + ... (lvf_debug_fail_codes).  After a failed factor x is not meaningful.  A solve that ran the fused candidate pass
 * has reset the flag.  LVF_ERR_STATE before any iteration. */
int lvf_problem_debug_download_step(lvf_problem* p, double* x, int* fail);
/* 1 / 0: the last iteration's linear solve succeeded (no failure flag, finite model and candidate cost) or not; -1 before any iteration. */
int lvf_problem_debug_last_solved(lvf_problem* p);
/* What the elimination plan made of the problem (after a configure, i.e. after any iteration; LVF_ERR_STATE before): *nb = block steps of the
 * dense corner (the largest dense failure code), dense_kf[n_kf] (may be NULL) = 1 where the keyframe's (v, ba, bg) block was left in the dense
 * corner instead of an elimination level. */
int lvf_problem_debug_plan(lvf_problem* p, int* nb, int* dense_kf);
/* The bases of the failure flag's sparse-level and hand-over codes (either pointer may be NULL). */
void lvf_debug_fail_codes(int* sparse_base, int* handover_base);
/* Diagnostic: how many entries of a landmark's E band, counted from the 16-aligned start of the band, the landmark workgroups of the merged
 * back-substitution launch request before they wait for the pose increments (the rest of a longer band is read afterwards). */
int lvf_debug_landmark_window(void);

/* ---- loop-correction tail: Relocator::UpdateNewSubmap / PoseGraph::ForwardUpdate ---------------------------------- */
/* RelocateRError <7,4> (pose_error.hpp:192-222) batched: block i = RelocateRError(relocated[i], unrelocated[i]) evaluated at the shared
 * quaternion q4 (x,y,z,w, NOT normalised by the functor).  residuals [n][7]; jacobians [n][7][4] row-major ambient, or NULL. */
int lvf_relocate_r_evaluate(lvf_ctx* ctx, int n, const double* relocated, const double* unrelocated, const double* q4, double* residuals,
                            double* jacobians);
/* The rotation solve of Relocator::UpdateNewSubmap (relocator.cpp:251-267): one quaternion parameter under EigenQuaternionParameterization,
 * n RelocateRError blocks, no loss, LM (the DENSE_QR solve of 3 tangent unknowns) — the whole loop is one device launch.  q4 (x,y,z,w) is
 * updated IN PLACE like `para` (identity in the reference); on failure (summary->termination == 2) it is left untouched. */
int lvf_relocate_rotation_solve(lvf_ctx* ctx, int n, const double* relocated, const double* unrelocated, double* q4, const lvf_solver_options* o,
                                lvf_solver_summary* summary);
/* PoseGraph::ForwardUpdate (pose_graph.cpp:245-252; also Backend::UpdateFrontend, backend.cpp:256): pose <- transform * pose (Sophus SE3
 * product: Hamilton product re-normalised, t_T + R(q_T) t) and Vw <- R(q_T) Vw for n keyframes; host arrays updated in place, vw may be NULL. */
int lvf_forward_update(lvf_ctx* ctx, const double* transform7, int n, double* poses, double* vw);
/* the same on a device-resident state: keyframes [first_kf, n_kf) of st (poses and velocities), nothing crosses PCIe but the transform */
int lvf_state_forward_update(lvf_state* st, const double* transform7, int first_kf);

/* ---- GNSS (NavSat) alignment: navsat_error.hpp + Navsat::{Initialize, OptimizeBC, Optimize, QuickFix} ----------------- */
/* All arithmetic fp64.  Poses are [qx,qy,qz,qw,tx,ty,tz], rpyxyz / para is [yaw,pitch,roll,x,y,z].  cov is the diagonal covariance the
 * reference hands to cov2sqrt_info (navsat_error.hpp:9-15): sqrt_info_k = sqrt(1.0 / cov_k); every cov_k must be > 0.
 * NavsatInitError <3,1,1,1> (navsat_error.hpp:17-51) batched: block i = NavsatInitError(p0[i], p1[i], cov[i]) at the shared x3 = (yaw, x, y).
 * residuals [n][3]; jacobians [n][3][3] row-major with columns (yaw, x, y), or NULL. */
int lvf_navsat_init_evaluate(lvf_ctx* ctx, int n, const double* p0, const double* p1, const double* cov, const double* x3, double* residuals,
                             double* jacobians);
/* NavsatRXError <3,1,1,1,1,1,1> (navsat_error.hpp:53-91) batched: block i = NavsatRXError(p0[i], p1[i], pose7, cov[i]) at the shared
 * x6 = (yaw, pitch, roll, x, y, z).  residuals [n][3]; jacobians [n][3][6] row-major, or NULL. */
int lvf_navsat_rx_evaluate(lvf_ctx* ctx, int n, const double* p0, const double* p1, const double* pose7, const double* cov, const double* x6,
                           double* residuals, double* jacobians);
/* NavsatRError <1,1> (navsat_error.hpp:93-120): NavsatRError(y3, pose7) at roll; one residual, one derivative (jacobian may be NULL). */
int lvf_navsat_r_evaluate(lvf_ctx* ctx, const double* y3, const double* pose7, double roll, double* residual, double* jacobian);
/* Navsat::Initialize (navsat.cpp:100-133): n blocks NavsatInitError(position[i], raw[i], cov[i]) (the keyframes that have a fix), no loss;
 * stage 1 solves yaw with x, y constant, stage 2 continues with all three free; both stages are ONE device launch.  para6 receives para
 * (only yaw, x, y can be non-zero), extrinsic7 = rpyxyz2se3(para).  n == 0: para = 0, extrinsic = identity, no launch. */
int lvf_navsat_initialize(lvf_ctx* ctx, int n, const double* position, const double* raw, const double* cov, const lvf_solver_options* o,
                          double* para6, double* extrinsic7, lvf_solver_summary* stage1, lvf_solver_summary* stage2);
typedef struct lvf_navsat_bc_options {
  int mode;                     /* bit i set = para[i] constant (navsat.cpp:210-214); 0b000000 for the section, 0b110111 per keyframe */
  double distance;              /* frames_distance(frame->time, end) */
  double trust_distance_yaw;    /* PoseGraph::min_BC_distance at construction (navsat.h:51) */
  double trust_distance_pitch;  /* accuracy * 10 (navsat.h:52) */
  double z_lower, z_upper;      /* A.z - B.z -/+ trust_distance_z * section.degree / 360 (navsat.cpp:244-246); used when z is free */
  double huber_a;               /* HuberLoss(0.1) (navsat.cpp:200) */
  lvf_solver_options solver;    /* ceres::Solver::Options defaults (huber_a of this member is not used) */
} lvf_navsat_bc_options;
typedef struct lvf_navsat_bc_result {
  int skipped;                  /* 1: the early return of navsat.cpp:195-197 was taken: nothing ran, the arrays are untouched */
  int line_search_contractions; /* step-size contractions of the bounded solve's projected line search (0 when z is constant) */
  double para[6];
  double transform[7];          /* new_pose * old_pose^-1: what every later pose was multiplied with */
  lvf_solver_summary roll;      /* the roll pre-solve (navsat.cpp:216-232); all zero when it did not run */
  lvf_solver_summary main;
} lvf_navsat_bc_result;
void lvf_navsat_bc_options_default(lvf_navsat_bc_options* o);
/* Navsat::OptimizeBC (navsat.cpp:192-269) in ONE device launch.  poses [n + n_update][7]: the n active keyframes GetKeyFrames(frame->time, end)
 * with the frame itself first, then n_update further poses (up to C) that only receive the forward update; has_fix[n], fix_point[n][3]
 * (what GetFixPoint returned; read where has_fix), cov[n][3].  Follows the function's control flow: the early return; the roll pre-solve
 * (one NavsatRError over all active keyframes) when roll is free and distance > trust_distance_yaw, roll constant afterwards; pitch constant
 * when distance < trust_distance_pitch; z inside [z_lower, z_upper] when free; one NavsatRXError(fix_i, frame^-1 * t_i, frame, cov_i) under
 * HuberLoss(huber_a) per keyframe with a fix; then poses[0] <- poses[0] * rpyxyz2se3(para) and poses[1..] <- (new * old^-1) * pose, in place.
 * No keyframe with a fix: para = 0 and the products are still applied, as in the reference.  Costs are those of the reduced program. */
int lvf_navsat_optimize_bc(lvf_ctx* ctx, int n, int n_update, double* poses, const int32_t* has_fix, const double* fix_point, const double* cov,
                           const lvf_navsat_bc_options* opt, lvf_navsat_bc_result* result);
/* The per-keyframe loop of Navsat::Optimize / QuickFix (navsat.cpp:150-155, :171-176) in ONE device launch.  poses [n][7]: the keyframes strictly
 * after B in time order, the last one being C (updated, not solved).  For k = 0 .. n-2: OptimizeBC(k, t_k + epsilon, 0b110111) — only x free, one
 * NavsatRXError(fix_k, pose_k^-1 * t_k, pose_k, cov_k) under HuberLoss(huber_a) if has_fix[k] — then the forward update of poses k+1 .. n-1.
 * has_fix[n-1], fix_point[n-1][3], cov[n-1][3].  Out: poses in place, x[n-1] (may be NULL), iterations[n-1] (may be NULL) = num_iterations of
 * each step's solve, summary = sums over the steps (termination: the worst).  n < 2: nothing to do. */
int lvf_navsat_fix_chain(lvf_ctx* ctx, int n, double* poses, const int32_t* has_fix, const double* fix_point, const double* cov, double huber_a,
                         const lvf_solver_options* o, double* x, int32_t* iterations, lvf_solver_summary* summary);

/* ---- pose chain: block-tridiagonal Levenberg-Marquardt (Navsat::OptimizeAB, navsat.cpp:271-307; the chain of PoseGraph::BuildProblem) ----- */
/* n poses [qx,qy,qz,qw,tx,ty,tz] in a row; pose 0 and pose n-1 are constant, the m = n - 2 poses between them are free under
 * ProductParameterization(EigenQuaternion, Identity3) (6 unknowns each).  Residual blocks:
 *   edge k (k = 0 .. n-2): PoseGraphError <6,7,7> between pose k and pose k+1 with rpyxyz_ = edge_target6[k], weight edge_weight[k], v edge_v[k],
 *     no loss.  edge_target6 == NULL: every target is taken from the poses as they come, on the device (PoseGraphError(last_pose, pose));
 *   one unary block per free pose i (unary_kind[i], entries 0 and n-1 are not read): LVF_CHAIN_NONE; LVF_CHAIN_T = TError <3,7>
 *     r = w (t - p), p = unary_target4[i][0..3), under HuberLoss(huber_a) (huber_a <= 0: no loss); LVF_CHAIN_R = RError <4,7>
 *     r = w (q - q0), q0 = unary_target4[i], no loss; w = unary_weight[i].
 * The whole ceres::Solve is ONE launch of one workgroup: the declared trust-region loop of the other small solves (Jacobi scaling frozen at
 * iteration 0, the clamped damping term, the order of the termination tests, five invalid steps in a row fail) around a linear solve by
 * odd-even block cyclic reduction — the Cholesky factorisation of the odd-even permuted block-tridiagonal matrix, depth log2 m.  Costs are
 * 1/2 sum rho, edges first, then unaries.  n == 2: the cost only, nothing moves.  A FAILURE (termination 2) leaves poses7 bit-equal to the
 * input and still returns LVF_OK.  n < 2 or n - 2 > lvf_pose_chain_capacity(): LVF_ERR_INVALID. */
#define LVF_CHAIN_NONE 0
#define LVF_CHAIN_T 1
#define LVF_CHAIN_R 2
int lvf_pose_chain_capacity(void);      /* free poses one call takes (1022) */
int lvf_pose_chain_solve(lvf_ctx* ctx, int n, double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v,
                         const int32_t* unary_kind, const double* unary_target4, const double* unary_weight, double huber_a,
                         const lvf_solver_options* o, lvf_solver_summary* summary);
/* Debug / tests: ONE linearisation of the same problem at poses7 and ONE damped solve at `radius` with the Jacobi scaling of this
 * linearisation; nothing is written back.  dx [6 (n-2)] (zero when *fail), *model = -dx.(g + H dx / 2) on the undamped blocks, *cost, *fail = 1
 * when a pivot of the reduction was not positive (the numerical "invalid step"). */
int lvf_pose_chain_debug_step(lvf_ctx* ctx, int n, const double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v,
                              const int32_t* unary_kind, const double* unary_target4, const double* unary_weight, double huber_a, double radius,
                              double* dx, double* model, double* cost, int32_t* fail);
/* Debug / tests: the undamped normal equations of one linearisation: D [n-2][6][6] (diagonal blocks), O [n-3][6][6] (O[i] = the block in
 * block-row i+1, block-column i), g [6 (n-2)] = J^T r. */
int lvf_pose_chain_debug_system(lvf_ctx* ctx, int n, const double* poses7, const double* edge_target6, const double* edge_weight, const double* edge_v,
                                const int32_t* unary_kind, const double* unary_target4, const double* unary_weight, double huber_a, double* D, double* O,
                                double* g);
/* Navsat::OptimizeAB (navsat.cpp:271-307) in ONE launch.  poses7 [n][7] = A, the keyframes of AB in time order, B; stamps [n]; fix_point [n][3]
 * = what GetFixPoint returns for each keyframe of AB (entries 0 and n-1 are not read); relative_B7 = section.relative_B.  The launch's set-up
 * phase replaces z of every fix by a B.z + (1 - a) A.z with a = (t - t_A) / (t_B - t_A), takes the edges PoseGraphError(last, frame, 1, 20)
 * from the poses as they come and the last one as PoseGraphError(relative_B, 10, 20); TError has weight 1 under HuberLoss(huber_a). */
int lvf_navsat_optimize_ab(lvf_ctx* ctx, int n, double* poses7, const double* stamps, const double* fix_point, const double* relative_B7, double huber_a,
                           const lvf_solver_options* o, lvf_solver_summary* summary);

/* ---- front-end tracking: utility.cpp optical_flow + triangulate, LocalMap::Triangulate, Frontend::TrackLastFrame --------------------------- */
/* The semantics of cv::calcOpticalFlowPyrLK are DECLARED (tests/klt_ref.py): OpenCV's structure with floating-point interpolation,
 * not a bit pin against OpenCV.  Points are cv::Point2f = float[2]; images are 8-bit grey.
 * lvf_image: what a cv::Mat image becomes once it is tracked on the device (frame->image_left / image_right, frame.h): the uint8 pyramid of
 * max_level + 1 levels (5-tap decimation as cv::buildOpticalFlowPyramid) and, per level, the Scharr derivative pair.  Built once per image
 * and used in every role the image plays (current, then last; left / right).  data: height rows of width pixels, stride bytes apart (host
 * memory; from lvf_host_alloc the upload is plain DMA).  The pixels may be overwritten as soon as the call returns.  0 <= max_level <= 7. */
int lvf_image_create(lvf_ctx* ctx, const uint8_t* data, int width, int height, size_t stride, int max_level, lvf_image** out);
int lvf_image_destroy(lvf_image* img);
int lvf_image_size(const lvf_image* img, int* width, int* height, int* levels);      /* levels = max_level + 1; any pointer may be NULL */
/* Debug / tests: one pyramid level, tightly packed: gray[h][w] and deriv[h][w][2] = (Sx, Sy) (either may be NULL); *width, *height (may be
 * NULL) receive the level's size ((w + 1) / 2, (h + 1) / 2 per level). */
int lvf_image_download_level(const lvf_image* img, int level, int* width, int* height, uint8_t* gray, int16_t* deriv);
typedef struct lvf_flow_options {
  int win, max_level;           /* forward pass: cv::Size(21, 21), maxLevel 3 (utility.cpp:64); win <= 21 */
  int back_win, back_max_level; /* backward pass: cv::Size(3, 3), maxLevel 1 (utility.cpp:71) */
  int max_iter;                 /* TermCriteria COUNT 30 (utility.cpp:65) */
  double eps;                   /* TermCriteria EPS 0.01 (utility.cpp:65) */
  double min_eig;               /* minEigThreshold 1e-4, the default the reference leaves in place */
  double fb_max;                /* forward-backward distance gate 0.5 (utility.cpp:79) */
} lvf_flow_options;
void lvf_flow_options_default(lvf_flow_options* o);
/* optical_flow (utility.cpp:55-89) in ONE device launch, one wavefront per point: the forward pass prev_img -> next_img started at next_pts
 * (OPTFLOW_USE_INITIAL_FLOW), the backward pass started at prev_pts, and the gate of :78-81.  next_pts [n][2]: in = initial flow, out = the
 * forward pass's result (for every point, as OpenCV leaves it); status [n] = 1 / 0; fb [n] (may be NULL) = the forward-backward distance,
 * +inf where a pass failed.  n == 0 returns at once (:59-60).  opt == NULL: the defaults.  Both images of one context and one size. */
int lvf_optical_flow(const lvf_image* prev_img, const lvf_image* next_img, int n, const float* prev_pts, float* next_pts, uint8_t* status, float* fb,
                     const lvf_flow_options* opt);
/* LocalMap::Triangulate (local_map.cpp:233-269) without the map bookkeeping: kps_right = the left pixel at depth 50 * baseline seen by camera 1
 * (:240-242), optical_flow(left, right) (:245), triangulate (utility.cpp:7-18; one-sided Jacobi SVD of the 4x4 in fp64) with the inverse
 * extrinsics and Pixel2Sensor of both pixels (:255).  status [n]: 0 = lost by the flow, 1 = landmark accepted, 2 = tracked but
 * Robot2Sensor_0(pb).z <= 0 (:256).  inv_depth [n] = 1 / Robot2Sensor_1(pb).z — camera ONE, as :258 has it; p_robot [n][3] = pb.  Both are
 * zero where status == 0.  What lvf_window_add_landmark takes: (kps_left, kps_right, inv_depth) of the points with status 1.
 * A non-finite camera field or extrinsic returns LVF_ERR_INVALID before anything is launched. */
int lvf_stereo_triangulate(const lvf_image* left, const lvf_image* right, const lvf_camera* cam0, const lvf_camera* cam1, double baseline, int n,
                           const float* kps_left, float* kps_right, uint8_t* status, double* inv_depth, double* p_robot, const lvf_flow_options* opt);
/* The numeric part of Frontend::TrackLastFrame (frontend.cpp:163-256): predictions = World2Pixel(pw[i], current_pose) (:168-170), optical_flow
 * (last, current, kps_last, predictions) (:189), deviation = prediction - tracked minus its mean over the tracked points (:195-212), class
 * per point cls [n]: 0 lost, 1 far (Camera::Far, camera.h:38-41), 2 near (!remove_moving_points or |deviation| < 30, :220), 3 moving;
 * *num_good = far + near if that exceeds num_features_tracking_bad, else 0 (:236).  kps_current [n][2] = the tracked pixels; predictions
 * [n][2] may be NULL.  What lvf_window_add_observation takes: kps_current of the points of class 1 or 2 when *num_good > 0.
 * A non-finite camera field, extrinsic or current_pose returns LVF_ERR_INVALID before anything is launched. */
int lvf_track_last_frame(const lvf_image* last, const lvf_image* current, const lvf_camera* cam0, double baseline, const double* current_pose, int n,
                         const double* pw, const float* kps_last, int remove_moving_points, int num_features_tracking_bad, float* kps_current,
                         float* predictions, uint8_t* cls, int* num_good, const lvf_flow_options* opt);

/* ---- image undistortion: the cv::undistort of Estimator::InputImage (estimator.cpp:178-179) with Camera's K, D (camera.h:22-26, 81-89) ------ */
/* The semantics are DECLARED (tests/undistort_ref.py): cv::undistort's structure — initUndistortRectifyMap with R = I and the new
 * camera matrix = K into a fixed-point map, then remap(INTER_LINEAR, BORDER_CONSTANT 0) — with the map evaluated directly per pixel in fp64
 * and exact integer weights; the device is bit equal to the restatement, nothing is pinned against OpenCV.
 * lvf_distortion: D = (k1, k2, p1, p2, 0) as camera.h:89 builds it (k3 and the rational terms are zero in the reference). */
typedef struct lvf_distortion { double k1, k2, p1, p2; } lvf_distortion;
/* lvf_undistort: what a Camera's K, D and the image size become: the map, built ONCE per camera and size on the host and kept on the device,
 * and a device staging buffer for the raw pixels (no allocation per frame beyond what lvf_image_create does).  Of `cam` only fx, fy, cx, cy
 * are read.  d == NULL: zero distortion (the output equals the input bit for bit).  LVF_ERR_INVALID: fx or fy <= 0, a non-finite intrinsic
 * or coefficient, a side outside [1, 4096] (the limit lvf_orb_detect states). */
typedef struct lvf_undistort lvf_undistort;
int lvf_undistort_create(lvf_ctx* ctx, const lvf_camera* cam, const lvf_distortion* d, int width, int height, lvf_undistort** out);
int lvf_undistort_destroy(lvf_undistort* u);
/* Debug / tests: the map in the declared layout: xy [h][w][2] = the integer source pixel (x, y) of the top-left tap, saturated to int16;
 * frac [h][w] = b * 32 + a, the 5-bit fractions along y and x (either pointer may be NULL). */
int lvf_undistort_download_map(const lvf_undistort* u, int16_t* xy, uint16_t* frac);
/* lvf_image_create of the undistorted image: the raw pixels are uploaded once, the remap writes level 0 of the new lvf_image on the device and
 * the pyramid / derivative chain of lvf_image_create follows.  An ordinary lvf_image comes back: every consumer takes it unchanged.  width
 * and height must be the map's.  raw: as `data` of lvf_image_create; it may be overwritten as soon as the call returns. */
int lvf_image_create_undistorted(lvf_undistort* u, const uint8_t* raw, int width, int height, size_t stride, int max_level, lvf_image** out);
/* Estimator::InputImage's two cv::undistort calls in one: both uploads, both remaps and both pyramid / derivative chains are queued on the
 * context's stream with ONE wait at the end.  u0 and u1 (one context, one size; they may be the same object) are the two cameras' maps. */
int lvf_image_pair_create_undistorted(lvf_undistort* u0, lvf_undistort* u1, const uint8_t* raw0, const uint8_t* raw1, int width, int height,
                                      size_t stride0, size_t stride1, int max_level, lvf_image** out0, lvf_image** out1);

/* ---- ORB features: Extractor's pyramid, FAST score, orientation and rBRIEF (extractor.cpp), LocalMap::Search (local_map.cpp:313-368) -------- */
/* The semantics are DECLARED (tests/orb_ref.py): integer arithmetic is bit equal to the restatement, nothing is pinned against
 * OpenCV.  lvf_orb holds what Extractor holds: the options' derived tables, the rBRIEF pattern and the scale pyramid of the last image. */
typedef struct lvf_orb lvf_orb;
typedef struct lvf_orb_options {
  int num_features;               /* 500 (extractor.h:26) */
  float scale_factor;             /* 1.2f */
  int num_levels;                 /* 4; 1 .. 8 */
  int ini_th_fast, min_th_fast;   /* 14, 7; 1 <= min_th_fast <= ini_th_fast <= 254 */
  int patch_size, edge_threshold; /* 31, 31: any other value is refused */
  int max_candidates;             /* 16384: FAST corners (after the per-cell NMS) one level may hold before the quadtree; more is an error, never a
                                   * silent truncation; 1 .. 65536 */
} lvf_orb_options;
#define LVF_ERR_ORB_CAPACITY 5   /* lvf_orb_detect: `capacity` is smaller than the number of keypoints found (see lvf_orb_capacity) */
#define LVF_ERR_ORB_OVERFLOW 6   /* lvf_orb_detect: a level holds more than max_candidates corners */
void lvf_orb_options_default(lvf_orb_options* o);
/* pattern: int8 [256][4] = (x1, y1, x2, y2) of bit 8 j + k of byte j, every |coordinate| <= 13; NULL: the built-in table (a documented
 * integer generator, tests/orb_ref.py builtin_pattern — NOT OpenCV's learned bit_pattern_31_; INTEGRATION.md tells how to pass that one). */
int lvf_orb_create(lvf_ctx* ctx, const lvf_orb_options* opt, const int8_t* pattern, lvf_orb** out);
int lvf_orb_destroy(lvf_orb* orb);
int lvf_orb_pattern(const lvf_orb* orb, int8_t* pattern);                                  /* the table in use, [256][4] */
/* scale_factor_per_levels_[level] (float32 running product), num_desired_features_[level] (extractor.cpp:14-45); pointers may be NULL */
int lvf_orb_level_info(const lvf_orb* orb, int level, float* scale, int* num_desired);
/* Extractor::ComputePyramid (extractor.cpp:455-477) of level 0 of an lvf_image (the frame's image is uploaded once, for tracking and here),
 * device to device: level L = fixed-point bilinear resize of level L - 1 to (cvRound(float(w) / scale_L), cvRound(float(h) / scale_L)); then
 * the FAST-9/16 corner score of every level in one launch (uint8; 0 = no corner at min_th_fast; pixels closer than 31 to an edge are 0).
 * The pyramid stays in `orb` until the next call, as Extractor::image_pyramid_ does. */
int lvf_orb_set_image(lvf_orb* orb, const lvf_image* img);
/* The exact upper bound of what lvf_orb_detect can return for a width x height image: per level with a usable area, the quadtree ends with at
 * most max(num_desired + 2, 4 * initial nodes) nodes (tests/orb_ref.py capacity). */
int lvf_orb_capacity(const lvf_orb* orb, int width, int height, int* max_keypoints);
/* Extractor::Detect (extractor.cpp:368-502) in one launch chain with one download at its end: lvf_orb_set_image, then per 30 x 30 cell the
 * non-maximum suppression with the ini -> min threshold fallback (:372-429; one workgroup per cell, every level in one launch), the quadtree
 * (DistributeQuadTree :160-366, one workgroup per level; count ties broken by smaller (UL.y, UL.x), the best point of a node = maximum response,
 * ties to the smallest (y, x)) and ICAngle.  Out: *n keypoints in level-major order, each level sorted by (y, x): level_count [num_levels],
 * pt [n][2] = (level pixel) * scale_level, octave [n], angle [n], response [n] = the FAST score, size [n] = float(int(31 * scale_level)).
 * A level whose usable area (cols - 56) x (rows - 56) is smaller than one 30 x 30 cell has no keypoints.  LVF_ERR_ORB_CAPACITY when more than
 * `capacity` keypoints were found (*n = that number, the arrays untouched), LVF_ERR_ORB_OVERFLOW when a level exceeds max_candidates; the
 * object stays usable after either.  Image sides up to 4096. */
int lvf_orb_detect(lvf_orb* orb, const lvf_image* img, int capacity, int* n, int32_t* level_count, float* pt, int32_t* octave, float* angle, float* response,
                   float* size);
/* Keypoints are (pt [n][2] in level-0 pixels as Extractor::Detect returns them, octave [n]); their level coordinates rint(pt / scale_octave)
 * must lie at least 19 pixels inside the level (the reference's own keypoints lie 31 inside), else LVF_ERR_INVALID.  n == 0 returns at once.
 * lvf_orb_orientation: ICAngle (extractor.cpp:66-93) with exact integer moments, one wavefront per keypoint; angle [n] = atan2(m01, m10) in
 * degrees in [0, 360), evaluated in fp64 and rounded to float (cv::fastAtan2's polynomial is not reproduced).
 * lvf_orb_compute: Extractor::Compute (extractor.cpp:504-530) as ORB-SLAM2's computeDescriptors has it: the levels named by `octave` are
 * blurred (7 x 7, sigma 2, integer, reflect-101) and rBRIEF is read at the LEVEL coordinates with the pattern rotated by `angle` (an input,
 * as the reference passes its keypoints back in); desc [n][32]. */
int lvf_orb_orientation(lvf_orb* orb, int n, const float* pt, const int32_t* octave, float* angle);
int lvf_orb_compute(lvf_orb* orb, int n, const float* pt, const int32_t* octave, const float* angle, uint8_t* desc);
/* Debug / tests: one level, tightly packed [h][w] each (any pointer may be NULL); `blurred` blurs the level if it has not been yet. */
int lvf_orb_download_level(lvf_orb* orb, int level, int* width, int* height, uint8_t* gray, uint8_t* blurred, uint8_t* score);
/* The numeric part of LocalMap::Search (local_map.cpp:313-368), one wavefront per current feature.  last_*: the features of the last
 * keyframe; cur_pw [n_cur][3]: the current features' landmark positions.  Per current feature with skip[i] == 0 (skip may be NULL):
 * pc = World2Sensor(pw, last_pose), none if pc.z < 0; p = float(Sensor2Pixel(pc)); candidates = last features of levels octave and octave + 1
 * (< num_levels) with |angle_last - angle| < 15 (no wrap-around, as the reference) and |p - pt_last| < 31 * scale_factors_[level] (the
 * fp64 running product of the float scale_factor, local_map.h:26-31); Hamming 2-NN, ties to the lower (level, index); accepted iff >= 2
 * candidates, best < 50 and float(best) < 0.8f * float(second).  match [n_cur] = index into last_* or -1; best / second [n_cur] (may be
 * NULL) = the two distances, -1 where there is no such candidate.  The keyframe loop and the map insertion stay with the caller.
 * A non-finite camera field, extrinsic or last_pose returns LVF_ERR_INVALID before anything is launched. */
int lvf_orb_search(lvf_ctx* ctx, const lvf_orb_options* opt, const lvf_camera* cam0, const double* last_pose, int n_last, const float* last_pt,
                   const int32_t* last_octave, const float* last_angle, const uint8_t* last_desc, int n_cur, const double* cur_pw,
                   const int32_t* cur_octave, const float* cur_angle, const uint8_t* cur_desc, const uint8_t* skip, int32_t* match, int32_t* best,
                   int32_t* second);

/* ---- visual relocalisation: the body Relocator::RelocateByImage declares (relocator.cpp:164-173) ------------------------- */
/* Semantics are DECLARED (the reference never builds the step); tests/reloc_ref.py is the statement of record.
 * lvf_orb_match: cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, k = 2) plus the gate of local_map.cpp:342-346, without the radius /
 * level / angle pre-selection.  Per query: the best and second-best Hamming distance over ALL train descriptors (ties to the lower train
 * index); accepted iff nt >= 2, best < max_distance, float(best) < ratio * float(second) and, with cross_check, the query is the best
 * (ties to the lower index) of its train descriptor.  match [nq] = train index or -1; best / second [nq] (may be NULL), -1 where absent.
 * nq, nt <= 8192 (LVF_ERR_INVALID beyond); nq == 0 or nt == 0 returns at once with no match. */
typedef struct lvf_match_options {
  int max_distance;     /* 50 */
  float ratio;          /* 0.8f */
  int cross_check;      /* 1 */
} lvf_match_options;
void lvf_match_options_default(lvf_match_options* o);
int lvf_orb_match(lvf_ctx* ctx, int nq, const uint8_t* query_desc, int nt, const uint8_t* train_desc, const lvf_match_options* opt, int32_t* match, int32_t* best,
                  int32_t* second);
/* Robust absolute pose from 3D-2D correspondences.  A hypothesis is a body pose Twb; its error for correspondence i is the norm of
 * PoseOnlyReprojectionError's residual at weight 1 for (pt_i, pw_i, cam0), +inf where the sensor-frame depth is <= 0; an inlier has squared
 * error < max_reproj_px^2.  num_hypotheses (1 .. 4096, no adaptive stopping) triples are drawn by the counter-based sampler
 * mix32(seed ^ mix32(h * 0x9E3779B1 + c)) % n (c = 0, 1, ...; a draw equal to an earlier one of the same hypothesis is skipped; at most 64
 * draws), each solved by P3P (at most four poses, positive depth at the three points); a hypothesis counts the inliers of its best pose
 * (ties to the pose the solver lists first), the winner is the largest count (ties to init_pose7, then to the lowest index).  Then
 * refine_rounds rounds of {classify every correspondence at the current pose; solve LocalMap::LocalBA's problem (local_map.cpp:158-181: one
 * pose, EigenQuaternionParameterization + Identity(3), one PoseOnlyReprojectionError per inlier at weight 1 under HuberLoss(huber_a)) by up
 * to refine_iterations iterations of the declared Ceres loop}; a last classification gives inlier [n] (may be NULL) and *score = its
 * population count.  summary (may be NULL) is the last round's.  With n < min_matches nothing is launched, *score = 0 and pose7 is left
 * untouched; the same when no hypothesis yields a pose.  pt [n][2] are float pixels, widened to double.  n <= 8192. */
typedef struct lvf_pnp_options {
  int num_hypotheses;       /* 512 */
  uint32_t seed;            /* 0 */
  double max_reproj_px;     /* 3.0 */
  int min_matches;          /* 21: with the base score of 20 (relocator.cpp:167) anything less is a rejection anyway; >= 3 */
  int refine_rounds;        /* 2 */
  int refine_iterations;    /* 10 */
  double huber_a;           /* 1.0 */
} lvf_pnp_options;
void lvf_pnp_options_default(lvf_pnp_options* o);
int lvf_pnp_ransac(lvf_ctx* ctx, const lvf_camera* cam0, int n, const double* pw, const float* pt, const double* init_pose7, const lvf_pnp_options* opt, double* pose7,
                   int32_t* score, uint8_t* inlier, lvf_solver_summary* summary);
/* RelocateByImage: queries = the current frame's features (cur_pt [n_cur][2], cur_desc [n_cur][32]), train = the old frame's (old_pw
 * [n_old][3] world, old_desc [n_old][32]).  The match, the gate and compaction, the hypotheses and the refinement are queued on the
 * context's stream with one wait and one download at the end; the matched pairs never leave the device in between.  relative_o_c7: in, the
 * caller's initial value (old_pose^-1 * init_pose, relocator.cpp:141), which joins as the initial pose old_pose * relative_o_c; out,
 * old_pose^-1 * pose (the Sophus product as lvf_forward_update forms it).  *score is the integer of `loop_closure->score += score - 20`.
 * With fewer than min_matches accepted pairs the pose kernels return at once, *score = 0 and relative_o_c7 is left untouched.
 * match is lvf_orb_match's result whatever becomes of the candidate (n_old == 0 or n_cur == 0: nothing is launched, no match).
 * match [n_cur] (may be NULL) = index into the old features or -1; inlier [n_cur] (may be NULL). */
int lvf_relocate_by_image(lvf_ctx* ctx, const lvf_camera* cam0, const double* old_pose7, int n_old, const double* old_pw, const uint8_t* old_desc, int n_cur,
                          const float* cur_pt, const uint8_t* cur_desc, const lvf_match_options* match_opt, const lvf_pnp_options* pnp_opt, double* relative_o_c7,
                          int32_t* score, int32_t* match, uint8_t* inlier, lvf_solver_summary* summary);
/* Test tap: per hypothesis the sample triple (-1: none), the number of P3P poses, the best inlier count and (poses may be NULL) that pose
 * [num_hypotheses][7].  3 <= n <= 8192.  Not part of the reference surface. */
int lvf_pnp_debug_hypotheses(lvf_ctx* ctx, const lvf_camera* cam0, int n, const double* pw, const float* pt, const lvf_pnp_options* opt, int32_t* triples,
                             int32_t* n_poses, int32_t* count, double* poses);

/* ---- LiDAR place recognition: Scan Context descriptors and their search, the appearance gate beside DetectLoop ----------- */
/* Semantics are DECLARED (the reference proposes candidates by position only, relocator.cpp:87-133); tests/scanctx_ref.py is the statement of
 * record.  Descriptor of a SENSOR-FRAME cloud: per point r = sqrtf(x*x + y*y) and th = the correctly rounded atan2f(y, x); a point counts iff r
 * and z are finite and min_range <= r < max_range; ring = min(num_rings - 1, floor(r * ring_scale)), sector = clamp(floor((th + pi) *
 * sector_scale), 0, num_sectors - 1), the scales formed once in double and rounded to float; h = z + sensor_height; cell = h > 0 ?
 * min(255, 1 + floor(h * inv_height_step)) : 0.  The descriptor is the per-cell maximum as uint8 (0 = empty), stored SECTOR-MAJOR:
 * desc[sector * num_rings + ring]; norm[sector] = sum over rings of cell^2.  Bit-reproducible (an integer maximum has no order).
 * Distance of query Q to entry D at shift s: column j of Q pairs with column (j + s) % num_sectors of D; pairs with both norms non-zero
 * contribute dot / sqrt(n2q * n2d) in float64, added in ascending j; d(s) = 1 - sum / count (1 when no pair is valid); the entry's distance is
 * the minimum over s, the lowest s on a tie.  A query taken at yaw psi_old + s * 2 pi / num_sectors matches at shift s.
 * LVF_ERR_INVALID: num_rings not a multiple of 4 in [4, 32], num_sectors outside [1, 64], a non-positive range or step, min_range >= max_range.
 * opt == NULL: the defaults. */
typedef struct lvf_scanctx_options {
  int num_rings;            /* 20 */
  int num_sectors;          /* 60 */
  float max_range;          /* 80.0f */
  float min_range;          /* 0.5f */
  float sensor_height;      /* 2.0f */
  float inv_height_step;    /* 10.0f */
} lvf_scanctx_options;
typedef struct lvf_scanctx_db lvf_scanctx_db;
void lvf_scanctx_options_default(lvf_scanctx_options* o);
/* describes one cloud and downloads the result: out_desc_u8 [num_sectors * num_rings], out_norm_u32 [num_sectors] (may be NULL).  An empty
 * cloud gives an all-zero descriptor. */
int lvf_scanctx_describe(lvf_ctx* ctx, const lvf_cloud* cloud, const lvf_scanctx_options* opt, uint8_t* out_desc_u8, uint32_t* out_norm_u32);
/* The database of old keyframes: up to `capacity` (1 .. 2^20) entries on the device, their stamps on the host.  Entries are numbered in the
 * order they were appended; stamps must be finite and non-decreasing, appending past the capacity is refused (LVF_ERR_INVALID both). */
int lvf_scanctx_db_create(lvf_ctx* ctx, const lvf_scanctx_options* opt, int capacity, lvf_scanctx_db** out);
int lvf_scanctx_db_destroy(lvf_scanctx_db* db);
int lvf_scanctx_db_size(const lvf_scanctx_db* db);
/* the cloud's descriptor is built on the device straight into the next entry; nothing is downloaded and nothing waits */
int lvf_scanctx_db_append(lvf_scanctx_db* db, const lvf_cloud* cloud, double stamp);
/* uploads a descriptor made elsewhere (desc_u8 [num_sectors * num_rings]); the library recomputes the norms */
int lvf_scanctx_db_append_descriptor(lvf_scanctx_db* db, const uint8_t* desc_u8, double stamp);
int lvf_scanctx_db_download(const lvf_scanctx_db* db, int index, uint8_t* out_desc_u8, uint32_t* out_norm_u32);
/* Searches the longest prefix of entries whose stamps are <= max_stamp (the reference looks among keyframes older than frame->time - 30,
 * relocator.cpp:92) for the k (1 .. 16) smallest (distance, index): out_index / out_shift / out_distance [k], ordered by (distance, index);
 * slots beyond the prefix's size hold index -1, shift -1, distance +inf (an empty prefix: all of them, LVF_OK).  One wait, 256 bytes down. */
int lvf_scanctx_search(lvf_scanctx_db* db, const uint8_t* query_desc_u8, double max_stamp, int k, int32_t* out_index, int32_t* out_shift, double* out_distance);
/* describe + search + (append != 0) append as ONE launch chain with one wait; the descriptor never leaves the device.  The search sees the
 * database as it was before the call. */
int lvf_scanctx_detect(lvf_scanctx_db* db, const lvf_cloud* cloud, double stamp, double max_stamp, int k, int32_t* out_index, int32_t* out_shift, double* out_distance,
                       int append);

/* ---- LiDAR depth for visual features: the sweep projected into camera 0, a triangle fit per feature -------------------------- */
/* Semantics are DECLARED (the reference takes a landmark's depth from the stereo pair only, local_map.cpp:233-269, and merely labels what lies
 * deeper than 50 baselines, camera.h:38-41); tests/lidar_depth_ref.py is the statement of record and every output is bit equal to it.
 * PROJECTION of a sensor-frame cloud (deskewed to the image's pose with lvf_cloud_deskew) by cam_from_lidar = [R | t], double[12] row-major
 * 3x4: in fp64 from the float32 coordinates pc = ((m0*x + m1*y) + m2*z) + m3 per row, u = fx*pc.x/pc.z + cx, v = fy*pc.y/pc.z + cy.  u, v and
 * pc.z are rounded to float32 ONCE (cv::Point2f); a point is kept iff pc is finite, min_depth <= pc.z < max_depth and the ROUNDED pixel lies
 * in [0, width) x [0, height).  A kept point is one record; records are binned on a grid of cell x cell pixels (the last row / column may be
 * partial), cell-row-major, cell_start [cells + 1].  The order of the records inside a cell is not defined.
 * DEPTH of a feature (u0, v0): the candidates are the records of the cells floor((u0 -+ radius) / cell) x floor((v0 -+ radius) / cell),
 * clipped to the grid, with d2 = dx*dx + dy*dy <= radius*radius (dx = u - u0, dy = v - v0, fp64).  Quadrant q = (dx >= 0) + 2 (dy >= 0); per
 * quadrant the winner is the minimum of (d2, source_index).  Fewer than three occupied quadrants: status 0.  Of four winners the largest by
 * the same order is dropped; the three are A, B, C in ascending order.  With b = B - A, c = C - A, p = -A (pixel offsets from the feature):
 * det = b.x*c.y - c.x*b.y, wb = (p.x*c.y - c.x*p.y) / det, wc = (b.x*p.y - p.x*b.y) / det, wa = (1 - wb) - wc,
 * inv_z = (wa/zA + wb/zB) + wc/zC — on a plane inverse depth is affine in the pixel.  Gates, in this order: status 3 |det| < min_det; 4 a
 * weight < -max_extrapolation; 2 max(z) - min(z) > max_spread (the triangle straddles an occlusion edge); 5 !(inv_z > 0) or 1/inv_z outside
 * [min_depth, max_depth); else 1 = accepted: depth = 1/inv_z, p_robot = Sensor2Robot_0(Pixel2Sensor_0(kp, depth)), inv_depth =
 * 1 / Robot2Sensor_1(p_robot).z (camera ONE, local_map.cpp:258), kps_right = float32(Robot2Pixel_1(p_robot)): lvf_stereo_triangulate's
 * conventions.  All outputs are zero where status != 1; a non-finite feature pixel has status 0.
 * LVF_ERR_INVALID (nothing launched): cell not 4 / 8 / 16 / 32, radius outside (0, 64], not 0 < min_depth < max_depth, a negative max_spread,
 * max_extrapolation or far_factor, min_det <= 0, replace_lost not 0 / 1, width or height outside [1, 65536], a non-finite matrix or camera. */
typedef struct lvf_lidar_depth_options {
  int cell;                 /* 8: grid cell in pixels (4, 8, 16 or 32) */
  double radius;            /* 12.0 px */
  double min_depth;         /* 0.5 m */
  double max_depth;         /* 80.0 m */
  double max_spread;        /* 2.0 m, as LVI-SAM's check */
  double min_det;           /* 4.0 px^2: twice the triangle's area */
  double max_extrapolation; /* 0.5 */
  double far_factor;        /* 50.0: lvf_stereo_triangulate_lidar replaces stereo depths beyond far_factor * baseline (0 = always) */
  int replace_lost;         /* 1: ... and gives depth to the features the stereo flow lost */
} lvf_lidar_depth_options;
typedef struct lvf_lidar_depth_record { float u, v, z; int32_t source_index; } lvf_lidar_depth_record;
typedef struct lvf_lidar_depth lvf_lidar_depth;
void lvf_lidar_depth_options_default(lvf_lidar_depth_options* o);
/* projects and bins the cloud: three launches, nothing is downloaded and nothing waits (the record array is sized by the cloud).  Of cam0 the
 * intrinsics are used.  opt == NULL: the defaults.  An empty cloud gives an empty grid. */
int lvf_lidar_depth_create(lvf_ctx* ctx, const lvf_cloud* cloud, const lvf_camera* cam0, const double* cam_from_lidar, int width, int height,
                           const lvf_lidar_depth_options* opt, lvf_lidar_depth** out);
int lvf_lidar_depth_destroy(lvf_lidar_depth* depth);
/* the number of kept points (the first call waits for the chain and reads 4 bytes); -1 on error */
int lvf_lidar_depth_size(lvf_lidar_depth* depth);
/* Test tap: records [lvf_lidar_depth_size] (may be NULL) and cell_start [cells + 1] (may be NULL), cells = ceil(width / cell) * ceil(height / cell). */
int lvf_lidar_depth_download(lvf_lidar_depth* depth, lvf_lidar_depth_record* records, int32_t* cell_start);
/* one launch, one wavefront per feature, one wait.  kps_left [n][2]; status [n], depth_out [n], inv_depth [n], p_robot [n][3], kps_right
 * [n][2] as above.  cam0's intrinsics must be the ones given to lvf_lidar_depth_create.  n == 0 returns at once. */
int lvf_lidar_depth_query(const lvf_lidar_depth* depth, const lvf_camera* cam0, const lvf_camera* cam1, int n, const float* kps_left, uint8_t* status,
                          double* depth_out, double* inv_depth, double* p_robot, float* kps_right);
/* lvf_stereo_triangulate with the query and one merge launch appended on the same stream; ONE wait.  LiDAR replaces the stereo result of a
 * feature iff its LiDAR status is 1 AND either the stereo status is 1 and Robot2Sensor_0(p_robot_stereo).z > far_factor * baseline
 * (far_factor == 0: always), or the stereo status is not 1 and replace_lost is set.  A replaced feature gets status 1, source 2 and the
 * LiDAR kps_right / inv_depth / p_robot; every other feature keeps exactly what lvf_stereo_triangulate writes, source [n] = 1 where its
 * status is 1, else 0.  `depth` belongs to the images' context.  A non-finite camera field or extrinsic returns LVF_ERR_INVALID before
 * anything is launched. */
int lvf_stereo_triangulate_lidar(const lvf_image* left, const lvf_image* right, const lvf_camera* cam0, const lvf_camera* cam1, double baseline, int n,
                                 const float* kps_left, float* kps_right, uint8_t* status, double* inv_depth, double* p_robot, const lvf_flow_options* opt,
                                 const lvf_lidar_depth* depth, uint8_t* source);

/* ---- multi-GPU: the path's only exchange, for a C / C++ host ----------------------------------------------------------- */
/* Independent windows / loop-closure candidates shard one per GPU: one process per GPU, one lvf_ctx each, no data-path collective.  The
 * single exchange is an all-gather of fixed-size records (score, relative_o_c[7], candidate id: relocator.cpp:196-206) over RCCL / xGMI.
 * Rank 0 calls lvf_comm_get_unique_id and hands the 128 bytes to the other ranks out of band (file, socket, MPI_Bcast); every rank then
 * calls lvf_comm_create with the same id.  id128 == NULL with world_size == 1 gives a communicator that needs no RCCL.
 * lvf_comm_allgather: every rank contributes n_doubles (equal on all ranks); recv[world_size][n_doubles] in rank order (host buffers). */
#define LVF_COMM_ID_BYTES 128
int lvf_comm_get_unique_id(void* id128);
int lvf_comm_create(lvf_ctx* ctx, int world_size, int rank, const void* id128, lvf_comm** out);
int lvf_comm_destroy(lvf_comm* c);
int lvf_comm_world_size(const lvf_comm* c);
int lvf_comm_rank(const lvf_comm* c);
int lvf_comm_allgather(lvf_comm* c, const double* send, int n_doubles, double* recv);

/* ---- persistent sliding window (Backend::BuildProblem's assembly, kept incrementally) -------------- */
/* The window mirrors Map's active keyframes, their features_left and the landmarks behind them as flat arrays that the
 * front-end updates as it goes; lvf_window_solve assembles the block lists with BuildProblem's rules (backend.cpp:96-183) in
 * frame order / ascending landmark id, re-fills persistent device batches (no per-tick allocation) and runs adapt::Solve's
 * device loop.  Keyframe and landmark ids are the caller's (frame->id, landmark->id); keyframe ids must increase. */
typedef struct lvf_window_options {
  double baseline;              /* Camera::baseline: a landmark deeper than 50 baselines is "Far" (camera.h:38-41) */
  int weak_visual_threshold;    /* 20 (backend.cpp:166) */
  double prior_weight, prior_v; /* PoseGraphError / PoseError (.., 100, 0)  (backend.cpp:170,175) */
  int device_assembly;          /* 1 (default): the per-tick block lists are assembled ON THE DEVICE from resident feature / landmark tables (only
                                 * what changed since the last tick is uploaded); 0: the host walks every feature and uploads the lists */
} lvf_window_options;
void lvf_window_options_default(lvf_window_options* o);
int lvf_window_create(lvf_ctx* ctx, const lvf_camera* left, const lvf_camera* right, const lvf_window_options* opt, lvf_window** out);
int lvf_window_destroy(lvf_window* w);
/* w_visual = frame->weights.visual.  The reference keeps its weights as FLOAT (adapt/weights.h:10): pass the float's value.  PoseOnly / TwoFrame
 * blocks of the keyframe take it as it is (backend.cpp:129, :138); its TwoCamera blocks take `5 * frame->weights.visual` formed as the reference
 * forms it, a float product widened to double: (double)(5.0f * (float)w_visual) (backend.cpp:123). */
int lvf_window_add_keyframe(lvf_window* w, int64_t kf_id, const double* pose7, double w_visual);
/* marks the frame good_imu with its Vw / linearised biases; pre (may be NULL) = frame->preintegration from the previous keyframe */
int lvf_window_set_imu(lvf_window* w, int64_t kf_id, const double* vel3, const double* ba3, const double* bg3, const lvf_preint* pre);
/* a landmark triangulated in keyframe birth_kf_id: its left feature there and first_observation (right image) */
int lvf_window_add_landmark(lvf_window* w, int64_t lm_id, int64_t birth_kf_id, const double* left_ob2, const double* right_ob2, double inv_depth);
int lvf_window_add_observation(lvf_window* w, int64_t lm_id, int64_t kf_id, const double* ob2);
int lvf_window_remove_observation(lvf_window* w, int64_t lm_id, int64_t kf_id);   /* outlier rejection, backend.cpp:232-243 */
int lvf_window_slide(lvf_window* w, int64_t first_active_kf_id);                  /* Map::GetKeyFrames(finished); also forgets landmarks nobody observes */
/* Backend::Optimize's outlier gate (backend.cpp:185-190, :229-245): every feature that is not its landmark's first observation is
 * re-projected on device with weight 1 (PoseOnly residual pass at the window's current poses / inverse depths) and removed from the window
 * when the pixel error exceeds max_px (10 in the reference).  Up to `capacity` removed (landmark id, keyframe id) pairs are reported. */
int lvf_window_reject_outliers(lvf_window* w, double max_px, int64_t* removed_lm, int64_t* removed_kf, int capacity, int* n_removed);
int lvf_window_solve(lvf_window* w, const lvf_solver_options* o, lvf_solver_summary* summary);
int lvf_window_set_pose(lvf_window* w, int64_t kf_id, const double* pose7);       /* front-end / ForwardUpdate writes */
int lvf_window_get_pose(const lvf_window* w, int64_t kf_id, double* pose7);
int lvf_window_get_imu(const lvf_window* w, int64_t kf_id, double* vel3, double* ba3, double* bg3);
int lvf_window_get_inv_depth(const lvf_window* w, int64_t lm_id, double* inv_depth);
/* counts8 = {keyframes, landmarks in the problem, TwoCamera, TwoFrame, PoseOnly, ImuError, prior blocks, landmarks known} of the last solve */
int lvf_window_counts(const lvf_window* w, int32_t* counts8);
/* LiDAR planes of one active keyframe's sweep (lvf_lidar_pose_create's blocks, all on kf_id): replaces that keyframe's set, n = 0 removes
 * it.  _set_lidar_scan takes them from what lvf_knn3 left in `scan` against `map`, on the device, with one weight and Huber a for the
 * scan.  The next lvf_window_solve adds the sets of the active keyframes to its problem; lvf_window_slide drops those of departed ones. */
int lvf_window_set_lidar_planes(lvf_window* w, int64_t kf_id, int n, const double* p, const double* pa, const double* pb, const double* pc,
                                const double* weight, const double* huber_a);
int lvf_window_set_lidar_scan(lvf_window* w, int64_t kf_id, lvf_map* map, lvf_scan* scan, double weight, double huber_a);
/* lidar plane blocks held for the active keyframes (blocks of weight 0 included) */
int lvf_window_lidar_count(const lvf_window* w, int32_t* n);
/* Test hook: the block lists of the last lvf_window_solve, kind 0 TwoCamera / 1 PoseOnly / 2 TwoFrame / 3 ImuError / 4 weak-constraint priors,
 * in the device batches' order with keyframe and landmark IDS: ids[capacity][3] = {landmark, first / previous keyframe, keyframe} (-1 where a
 * kind has none), vals[capacity][8] = {weight handed to the reference's Create, ob x, y, first (right) ob x, y, pw x, y, z}; *n = blocks of the
 * kind.  What tests compare with Backend::BuildProblem's own output (backend.cpp:96-183).  Not part of the reference surface. */
int lvf_window_debug_blocks(lvf_window* w, int kind, int capacity, int64_t* ids, double* vals, int* n);

/* ---- Marginal information and covariance of selected keyframe unknowns (what ceres::Covariance answers for a few parameter blocks).
 * For the reduced (Schur) system S over the keyframe unknowns — order of lvf_problem_download_reduced: [pose tangent 6 x n_kf | (v, ba, bg)
 * 9 x n_kf], d = 15 n_kf — and a selection s of m <= 120 unknowns with r the rest:
 *     info = S_ss - S_sr S_rr^-1 S_rs     (what marginalising the rest leaves as a prior on s)
 *     cov  = info^-1 = (S^-1)_ss
 * both [m x m] row-major, row i belonging to sel[i], exactly symmetric; either pointer may be NULL, not both.  S is the UNDAMPED Gauss-Newton
 * matrix J^T J of the robustified tangent-space Jacobian at the current state, pose priors included.  An unknown whose Jacobian column is
 * identically zero (a constant pose or (v, ba, bg) block, one no factor touches: S_jj == 0 exactly, never a threshold) is ABSENT: it is left
 * out of the system and its rows and columns of both outputs are zero.
 * Stats: fail = 0, or 1 + kb of the 64-column block step of the elimination of the rest that met a non-positive or NaN pivot (rest unknowns in
 * ascending order, absent ones keeping their place), or one past the last such step for a pivot inside the selection; n_present + n_absent =
 * d; min_pivot_ratio = the smallest L_jj^2 / S_jj over the present unknowns, in (0, 1]: a conditioning indicator for the caller to gate on
 * (the library applies no threshold).  A numeric failure is soft: LVF_OK, fail != 0, info / cov untouched, min_pivot_ratio unspecified.
 * Argument errors (m outside 1 .. 120, an index out of range or twice, both outputs NULL): LVF_ERR_INVALID before anything reaches the device. */
typedef struct { int fail, n_present, n_absent; double min_pivot_ratio; } lvf_marginal_stats;
/* The linear algebra alone on a caller's matrix: S [d x d] row-major, only the lower triangle is read; absent iff S_jj == 0. */
int lvf_marginal_dense(lvf_ctx* ctx, const double* S, int d, const int* sel, int m, double* info, double* cov, lvf_marginal_stats* stats);
/* Of keyframes kfs[n_sel] (1 .. 8, distinct) of a problem: m = 15 n_sel, each keyframe's unknowns in the order [pose 6, v 3, ba 3, bg 3].
 * Linearises at the current state with o->huber_a and assembles the undamped reduced system; the state, the step of the last iteration and a
 * debug override are left alone, and the next iteration computes what it would have computed without the call. */
int lvf_problem_marginal(lvf_problem* p, const lvf_solver_options* o, const int* kfs, int n_sel, double* info, double* cov, lvf_marginal_stats* stats);
/* The same for the persistent window, by keyframe id: the window's problem is refreshed as lvf_window_solve refreshes it, without iterating. */
int lvf_window_marginal(lvf_window* w, const lvf_solver_options* o, const int64_t* kf_ids, int n_sel, double* info, double* cov, lvf_marginal_stats* stats);

/* ---- Dense keyframe prior: what marginalising other unknowns leaves on a few keyframes, fed back as a factor.
 * On n_sel distinct keyframes (1 .. 8), m = 15 n_sel unknowns, per keyframe [rotation 3, translation 3, v 3, ba 3, bg 3] (the order of
 * lvf_problem_marginal's outputs):
 *     cost(x) = c0 + eta^T e + 1/2 e^T info e,        e = x [-] x0
 * x0 [n_sel][16] = {pose 7, v 3, ba 3, bg 3} per keyframe, info [m][m] row-major of which only the lower triangle is read, eta [m] (NULL:
 * zero).  e is the local coordinate of x at x0 in the solver's parameterisation: with u = q/|q|, u0 = q0/|q0|, d = u (x) u0^-1 (negated if
 * d.w < 0), the rotation part is atan2(|d.v|, d.w) d.v/|d.v| (so that Plus(q0, e_rot) = q); the other twelve entries are plain differences.
 * No loss function and no first-estimate Jacobians: e is re-evaluated at every state.  With T the tangent Jacobian of e (the identity at
 * x = x0, so an info that lvf_problem_marginal / _marginal_prior computed at x0 needs no conversion) the gradient is T^T (info e + eta) and
 * the Gauss-Newton matrix T^T info T; a constant block gets zero columns.  A zero row / column of info (an absent unknown) is legal and info
 * may be singular; the caller vouches that [info eta; eta^T 2 c0] is positive semi-definite.  Declared semantics: tests/dense_prior_ref.py.
 * LVF_ERR_INVALID before anything reaches the device: n_sel outside 1 .. 8, a negative index, a keyframe listed twice, a non-finite entry of
 * x0, eta, c0 or the lower triangle of info, a zero quaternion in x0.  kf_idx are keyframe POSITIONS in the state / problem. */
typedef struct lvf_dense_prior lvf_dense_prior;
int lvf_dense_prior_create(lvf_ctx* ctx, int n_sel, const int32_t* kf_idx, const double* x0, const double* info, const double* eta, double c0,
                           lvf_dense_prior** out);
int lvf_dense_prior_destroy(lvf_dense_prior* prior);
/* keyframes of the prior; what it was created with (any pointer may be NULL) */
int lvf_dense_prior_size(const lvf_dense_prior* prior);
int lvf_dense_prior_download(lvf_dense_prior* prior, int32_t* kf_idx, double* x0, double* info, double* eta, double* c0);
/* Materialised parity mode: cost, gradient [m] and Gauss-Newton matrix [m][m] (row-major, exactly symmetric) at the state, in the prior's own
 * order.  const_bits (NULL: nothing constant): one byte per keyframe of the state, bit 0 = pose constant, bits 1 .. 3 = v, ba, bg constant.
 * Any output may be NULL. */
int lvf_dense_prior_evaluate(lvf_dense_prior* prior, const lvf_state* st, const uint8_t* const_bits, double* cost, double* gradient, double* matrix);
/* Adds (or with NULL removes) a dense prior on keyframes of the problem (the prior is borrowed).  Every entry that linearises or evaluates
 * the problem sees it: cost, gradient, lm_iteration, solve, download_reduced, marginal, marginal_prior.  A problem with such a prior runs the
 * chain a problem with pose priors runs (no fused candidate pass, no table launches), and the (v, ba, bg) blocks of the prior's keyframes stay
 * in the dense corner of the elimination plan; a change of that set of keyframes configures the problem again (constant flags are kept). */
int lvf_problem_set_dense_prior(lvf_problem* p, lvf_dense_prior* prior);
/* lvf_problem_marginal with the reduced right-hand side carried along: for the local model c + g^T eps + 1/2 eps^T H eps of the problem at its
 * current state (landmarks minimised out; H the undamped Gauss-Newton matrix, g the gradient, c the cost, all with o->huber_a) and the
 * unknowns of keyframes kfs[n_sel] as the selection s, r the rest,
 *     info = H_ss - H_sr H_rr^-1 H_rs,      eta = g_s - H_sr H_rr^-1 g_r,      c0 = c - 1/2 g_r^T H_rr^-1 g_r
 * — with x0 = the selected keyframes' current state exactly the arguments of lvf_dense_prior_create.  m + 1 <= 121 rows ride behind the rest.
 * Stats, absent unknowns and the soft failure are lvf_problem_marginal's, except that no covariance is formed: a singular SELECTED block is
 * no failure (an unanchored sub-problem leaves the gauge free), fail only reports the elimination of the rest, and min_pivot_ratio is taken
 * over the rest's pivots (1 when there is no rest).  Any of info / eta / c0 may be NULL. */
int lvf_problem_marginal_prior(lvf_problem* p, const lvf_solver_options* o, const int* kfs, int n_sel, double* info, double* eta, double* c0,
                               lvf_marginal_stats* stats);
/* The persistent window's dense prior, by keyframe ID (arguments of lvf_dense_prior_create otherwise; n_sel = 0 removes it).  Every
 * lvf_window_solve and lvf_window_marginal translates the ids to positions and attaches it to the window's problem.  A prior one of whose
 * keyframes leaves by plain lvf_window_slide is dropped.  LVF_ERR_INVALID, before anything reaches the device: n_sel outside 0 .. 8, a
 * keyframe that is not in the window or listed twice, a non-finite entry. */
int lvf_window_set_dense_prior(lvf_window* w, int n_sel, const int64_t* kf_ids, const double* x0, const double* info, const double* eta, double c0);
/* What the window holds: *n_sel = 0 when there is none; the arrays (each may be NULL) must have room for 8 keyframes' worth. */
int lvf_window_get_dense_prior(const lvf_window* w, int* n_sel, int64_t* kf_ids, double* x0, double* info, double* eta, double* c0);
/* lvf_window_slide that keeps what the departing keyframes knew.  With D the keyframes older than first_active_kf_id and s the first kept
 * one, a sub-problem over D and s is built at the window's current state from every block BuildProblem's rules give for that keyframe list
 * that touches D: D's TwoCamera, PoseOnly and TwoFrame blocks, D's weak-constraint priors and LiDAR plane sets, the ImuError blocks along D
 * and into s, and the window's dense prior (which must not sit on keyframes beyond s: LVF_ERR_INVALID).  s contributes no visual block and no
 * weak-constraint prior of its own: what kept frames observe of D's landmarks lives on as PoseOnly blocks after the slide (the reference's
 * rule), so no factor is counted twice and none is lost.  lvf_problem_marginal_prior of s in that sub-problem, with o->huber_a and
 * x0 = s's current state, becomes the window's dense prior; then the window slides as lvf_window_slide does.  No departing keyframe: nothing
 * happens (LVF_OK); no kept keyframe: LVF_ERR_INVALID.  A soft failure (stats->fail != 0) slides without a prior.  The sub-problem is a second
 * persistent window owned by this one: its DEVICE buffers only grow; its host mirror (keyframes, observations, the landmark table) is copied
 * from this window's at every call. */
int lvf_window_slide_marginalize(lvf_window* w, int64_t first_active_kf_id, const lvf_solver_options* o, lvf_marginal_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* LVF_H_ */
