// pipeline_capi.h — C entry points of the host pipeline, shared by the product
// build (pipeline_capi.cpp, bound to libsvslam_hip.so) and by the CPU twin that
// the oracle directory builds for tests / the cpu_baseline leg.
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct svs_pipe_config {
    int num_features, num_features_init, num_features_tracking, num_features_tracking_bad;
    int num_features_needed_for_keyframe;
    double max_triangulation_depth;
    int num_active_keyframes, backend_on;   /* backend_on: 0 off, 1 BA completes before the next frame,
                                               2 BA runs beside the next frame, result lands one frame late */
    double chi2_th;
    int width, height;
    double cam_l[4], ext_l[7], cam_r[4], ext_r[7];
    int max_lm, max_obs;      /* BA limits per problem */
    int host_threads;         /* threads for the per-stream host bookkeeping (>=1) */
    int src_width, src_height; /* > 0: the frames handed in are full-resolution src_width x src_height and
                                  are decimated 2:1 to width x height on the way into the pyramid (the
                                  resize of Dataset::NextFrame, src/dataset.cpp:126-129, fused)        */
    int resident_track;       /* 1: the features of every stream's last frame stay in device memory
                                  (svslam_rtrack_*); used when backend_on <= 1                      */
    int low_latency;          /* 1: latency shape of the serial kernels (svslam_set_low_latency), for a
                                  few streams per GPU                                                */
    int max_pts;              /* features per frame the kernel provider holds per stream (0 = 512)   */
    int device_map;           /* 1: the map of every stream lives in device memory (svslam_dmap_*): the
                                  keyframe path costs the host O(window) per keyframe, no per-feature work.
                                  Needs resident_track = 1, backend_on = 1.  The HIP provider only.          */
    int backend_lag;          /* backend_on == 2: frames a submitted local BA may stay in flight (0 / 1: one frame) */
} svs_pipe_config;

typedef struct svs_frame_result {
    double pose[7];
    int status, is_keyframe, n_features, n_inliers;
    long long frame_id, keyframe_id;
} svs_frame_result;

typedef struct svs_pipe_counters {
    long long frames, keyframes, track_pts, pose_edges, gftt_calls, gftt_rects, corners, right_pts, tri_pts;
    long long ba_calls, ba_edges, ba_kf, ba_lm, ba_iters, pyr_left, pyr_right;
    long long ns_step, ns_kernel_calls;
    long long corners_dropped, ba_skipped;   /* per-stream capacity events (max_pts / max_lm / max_obs) */
    long long ba_pairs, ba_trials;           /* block pairs of the Schur complements, LM trials: the flop accounting of bench.py */
    long long lm_total, lm_resident;         /* landmarks ever created / MapPoint objects the host still holds (the rest
                                                were evicted to the 16-byte archive, Map::ReleaseRetired)              */
    long long lm_full;                       /* device map: keyframes that ran out of landmark slots (max_lm = LIVE landmarks of a
                                                stream there); their surplus points were not created                     */
} svs_pipe_counters;

void *svs_pipe_create(const svs_pipe_config *cfg, int nstreams, int device);
void svs_pipe_destroy(void *p);
/* Which detector Frontend::DetectFeatures runs: 0 = GFTT (the default), 1 = ORB (keypoint_feature_detector: ORB of the reference's
 * configuration, svslam_orb_detect_batch).  A setter and not a field of svs_pipe_config, whose layout the CPU twin shares.
 * -1 (svs_pipe_last_error, nothing changed): another kind; a call after the first frame; ORB with device_map or resident_track (there
 * GFTT is fused into the keyframe chain); a kernel provider without the ORB detector ("this kernel provider has no ORB detector"). */
int svs_pipe_set_detector(void *p, int kind);
const char *svs_pipe_last_error(void);
/* Process-wide glibc malloc settings for a host that drives thousands of streams: the per-frame
 * Frame / feature-list churn otherwise makes every thread's heap top shrink and regrow (munmap /
 * mmap / page faults, all under the process' mm lock).  Never trims, serves large vectors from the
 * heaps, grows them in 64 MB steps.  Optional; call once before creating pipelines.            */
void svs_pipe_tune_allocator(void);
/* completes a backend optimisation still in flight (backend_on 2) */
int svs_pipe_flush(void *p);
/* one frame for every stream; left/right: nstreams image pointers (host or device) */
int svs_pipe_step(void *p, const void *const *left, const void *const *right, int is_device,
                  svs_frame_result *out);
/* run `nframes` steps over device-resident sequences laid out [stream][frame][h*w]
 * (left and right), writing results [frame][stream]; the whole loop stays in C++ */
int svs_pipe_run_device(void *p, const void *left_base, const void *right_base, long long stream_stride,
                        long long frame_stride, int first_frame, int nframes, svs_frame_result *out);
int svs_pipe_counters_get(void *p, svs_pipe_counters *out);
/* keyframes.txt + landmarks.pcd of one stream, in the reference's formats (src/visual_odometry.cpp:198-310) */
int svs_pipe_save_outputs(void *p, int stream, const char *dir, const char *dataset_dir, int left_cam_index);
/* Frame::loop_keyframe_ / loop_relative_pose_ of keyframe kf_id (src/loopclosure.cpp:598-606): T_rel7 = T_kf * T_loop^-1 as a loop
 * detector measured it.  -1 (svs_pipe_last_error): ids that are not keyframes of the stream, loop_kf_id >= kf_id. */
int svs_pipe_add_loop_edge(void *p, int stream, long long kf_id, long long loop_kf_id, const double *T_rel7);
/* LoopClosure::PoseGraphOptimization (src/loopclosure.cpp:641-799) for `nstreams` streams (streams == NULL: all) in one kernel call:
 * keyframe poses and every landmark svs_pipe_save_outputs writes are corrected, relative_pose_pkf refreshed.  stats7_or_null: per
 * stream nkf, nedge, npt, iterations, trials, chi2 before, chi2 after.  -1: the map lives on the device (device_map = 1: nothing
 * is done), a bad stream, the kernel's refusal.  Product library only. */
int svs_pipe_pose_graph_optimization(void *p, int nstreams, const int *streams, int iters, double *stats7_or_null);
/* LoopClosure::KeypointMatchWithLoopCandid + CalculatePose (src/loopclosure.cpp:286-437) for nqueries keyframe pairs in one kernel call
 * (svslam_loop_verify_batch); every ACCEPTED pair is recorded like svs_pipe_add_loop_edge(stream, kf, cand, T_rel).  Per query:
 * descriptors [n][32] of both keyframes and desc_feat_indx, the reference's map from descriptor row to index in feature_left_.
 * params: svslam_loop_params (include/svslam.h); its cam and ext_l are replaced by the pipeline's left camera.  results: one
 * svs_loop_result per query; match4_or_null: 4 ints per candidate descriptor row, query after query (candidate row, current row,
 * Hamming distance, inlier flag for the first n_matches rows of a query's block).  LocalFusion (:439-582) is not done.
 * -1 (svs_pipe_last_error, nothing done): the map lives on the device (device_map = 1), an unknown stream, ids that are not
 * keyframes, cand >= kf, a desc_feat_indx entry out of range or repeated, descriptor count != index count, the kernel's refusal.
 * Product library only. */
typedef struct svs_loop_query {
    int stream; long long kf_id, cand_kf_id;
    int n_desc_q, n_idx_q; const uint8_t *desc_q; const int *feat_q;
    int n_desc_c, n_idx_c; const uint8_t *desc_c; const int *feat_c;
} svs_loop_query;
typedef struct svs_loop_result {
    int status, n_matches, n_points, n_inliers, need_correction, reserved;
    double T_corr[7], T_rel[7], d;
} svs_loop_result;
int svs_pipe_verify_loops(void *p, int nqueries, const svs_loop_query *queries, const void *params, svs_loop_result *results, int *match4_or_null);
/* LoopClosure::ExtractKeypointsDescriptor (src/loopclosure.cpp:131-171) for every stream whose last step made a keyframe: BRIEF-256
 * (svslam_brief_describe_batch) at the keyframe's non-outlier left features, stored with the keyframe (descriptor row -> feature
 * index); one kernel call for all streams.  Call it after the step and before the next one: the keyframe's image is level 0 of a
 * pyramid slot only until then.  brief_params_or_null: svslam_brief_params (include/svslam.h) or NULL for the default table, -1
 * degree, edge 31.  Returns the number of keyframes described, -1 (svs_pipe_last_error, nothing stored): the map lives on the device
 * (device_map = 1), the kernel's refusal.  Product library only. */
int svs_pipe_describe_new_keyframes(void *p, const void *brief_params_or_null);
/* svs_pipe_describe_new_keyframes with every feature described at its own angle and octave (svslam_orb_describe_batch): what
 * cv::ORB::compute gives the reference when keypoint_feature_detector is ORB.  A tracked feature and a GFTT corner carry -1 degree and
 * octave 0, so with GFTT the stored rows are svs_pipe_describe_new_keyframes' rows.  orb_desc_params_or_null: svslam_orb_desc_params or
 * NULL for the default table, edge 31, 8 levels.  Returns and refusals as svs_pipe_describe_new_keyframes.  Product library only. */
int svs_pipe_describe_new_keyframes_oriented(void *p, const void *orb_desc_params_or_null);
/* x, y, angle, octave of every left feature of keyframe kf_id, rows4 [n][4] floats in the order of svs_pipe_keyframe_features: what
 * the oriented descriptors were computed at.  Returns n (nothing is written when cap < n or rows4 is NULL), -1 for a bad stream / id. */
long long svs_pipe_keyframe_keypoints(void *p, int stream, long long kf_id, float *rows4, long long cap);
/* the stored descriptors of keyframe kf_id: desc32 [n][32] and feat [n] = index of each row's feature in the keyframe's left list.
 * Returns n (nothing is written when cap < n or an array is NULL: call again), -1 for a bad stream / id or a keyframe that was never
 * described (a keyframe described with zero rows returns 0). */
long long svs_pipe_keyframe_descriptors(void *p, int stream, long long kf_id, uint8_t *desc32, int *feat, long long cap);
/* svs_pipe_verify_loops on the stored descriptors of both keyframes of every pair.  match4_or_null has match_rows rows of 4 ints: at
 * least the sum of the candidate keyframes' descriptor rows, laid out as svs_pipe_verify_loops does.  -1 (nothing done): what
 * svs_pipe_verify_loops refuses, a keyframe that was never described, a match array that is too short. */
typedef struct svs_loop_pair { int stream; long long kf_id, cand_kf_id; } svs_loop_pair;
int svs_pipe_verify_loops_stored(void *p, int npairs, const svs_loop_pair *pairs, const void *params, svs_loop_result *results, int *match4_or_null,
                                 long long match_rows);
/* The store of global image descriptors svs_pipe_detect_loops searches (svslam_loopdb_configure): capacity rows of dim
 * floats for every stream, emptied; every stream's last closed keyframe is forgotten.  Product library only. */
int svs_pipe_loopdb_configure(void *p, int capacity, int dim);
/* LoopClosure::AddNewKeyFrame and one turn of LoopClosurePipeline (src/loopclosure.cpp:182-198, :801-872) for every stream whose last
 * step made a keyframe, after svs_pipe_describe_new_keyframes: the skip rule after a closed loop, the candidate search
 * (svslam_loop_candidates_batch, one call), the verification of every FOUND candidate (svs_pipe_verify_loops_stored, one call; an
 * ACCEPTED pair is a loop edge and the stream's last closed keyframe, and is not stored), the append of every other keyframe (one
 * call).  vecs: [nstreams][dim] global descriptors, the rows of streams without a new keyframe are not read.  loop_params:
 * svslam_loop_params (cam and ext_l are filled in by the pipeline).  results: [nstreams]; cand_status and loop.status are -1 where that
 * stage did not run.  The matches of a verified stream: svs_pipe_loop_matches.  -1 (svs_pipe_last_error, nothing done): device_map =
 * 1, a store that was not configured, a new keyframe that was never described, a full stream, a kernel's refusal.  LocalFusion is
 * not done here (svs_pipe_detect_loops_fused, or svs_pipe_local_fusion with the result).  vecs == NULL: the vectors come from the network svs_pipe_gdesc_configure set, computed here for the keyframes this call
 * handles; refused when no network is configured or when the store's dim is not the network's. */
typedef struct svs_loop_detect_params { float weak, strong; int max_num_weak, min_gap; long long keyframes_to_ignore_after_loop; } svs_loop_detect_params;
typedef struct svs_loop_detection {
    int is_keyframe, skipped, searched, verified, stored, reserved;
    long long kf_id;
    int cand_status, cand_kf, best_kf, n_weak, n_compared; float best_sim;
    svs_loop_result loop;
} svs_loop_detection;
int svs_pipe_detect_loops(void *p, const float *vecs, const svs_loop_detect_params *dp, const void *loop_params, svs_loop_detection *results);
/* svs_pipe_detect_loops that, with local_fusion != 0, ends with LoopClosure::LocalFusion (src/loopclosure.cpp:439-582, as
 * LoopClosureUpdate calls it: only where need_correction is set) for every stream whose pair was ACCEPTED, in one kernel call: its
 * pairs are the match rows whose candidate feature had a landmark, mapped through desc_feat_indx.  fusion_or_null: [nstreams], fused = 1
 * where it ran.  With local_fusion == 0 this IS svs_pipe_detect_loops; the structs of that call are unchanged.  -1 after the
 * detection itself succeeded (a refusal of the fusion): the loop edges and the store are as svs_pipe_detect_loops leaves them, no
 * map was fused, and results (and fusion_or_null, fused = 0) are filled as on success. */
typedef struct svs_fusion_stats { int fused, nkf, npt, n_unanchored, pairs, merged, revived, repointed, same_deleted, reserved; } svs_fusion_stats;
int svs_pipe_detect_loops_fused(void *p, const float *vecs, const svs_loop_detect_params *dp, const void *loop_params, int local_fusion,
                                svs_loop_detection *results, svs_fusion_stats *fusion_or_null);
/* LoopClosure::LocalFusion for njobs closed loops (at most one per stream) in one kernel call (svslam_local_fusion_batch), for a
 * caller who verified the loop itself: the active window, the active landmarks and the frontend's last frame move with the
 * corrected pose T_corr of keyframe kf_id; then, for every pair (feature index in the loop keyframe cand_kf_id, feature index in
 * kf_id) in ascending order, the loop keyframe's landmark - brought back from the archive when it is dead - takes over the
 * observations of the current feature's landmark, which is removed from the map.  pairs2: 2 ints per pair, a job's pairs start at
 * pair_ofs.  stats_or_null: [njobs].  A local BA in flight is collected first; with resident tracking the stream's feature list is
 * uploaded again.  -1 (svs_pipe_last_error, NOTHING changed for any job): device_map = 1, an unknown stream, two jobs on one
 * stream, ids that are not keyframes, cand >= kf, a keyframe whose feature list was released (svs_pipe_keep_keyframe_features), an
 * index out of range, a repeated pair, a T_corr that is no unit quaternion, resident tracking where the stream's last frame is not
 * kf_id (its features are then held only by the kernel provider).  Product library only. */
typedef struct svs_fusion_job { int stream, npairs; long long kf_id, cand_kf_id, pair_ofs; double T_corr[7]; } svs_fusion_job;
int svs_pipe_local_fusion(void *p, int njobs, const svs_fusion_job *jobs, const int *pairs2, svs_fusion_stats *stats_or_null);
/* Map::landmarks_ of a stream, read-only, id-ascending: 7 doubles each (id, x, y, z, observation counter, active flag, keyframe id of
 * the anchor or -1); dead landmarks come from the archive (float positions, counter 0).  Returns their number (nothing written when
 * cap is smaller or out7 is NULL), -1 for a bad stream. */
long long svs_pipe_all_landmarks(void *p, int stream, double *out7, long long cap);
/* the frontend's last frame of a stream: its pose, and its keyframe id or -1 when it is no keyframe; -2: a bad stream / no frame yet */
long long svs_pipe_last_frame(void *p, int stream, double *pose7);
/* The network behind the global image descriptor (svslam_gdesc_configure): layers is svslam_gd_layer [nlayers], params the
 * weights and biases in table order, prep_or_null svslam_gd_prep or NULL for the reference's call.  -1: the kernel's refusal, the
 * network configured before is kept.  svs_pipe_gdesc_dim: floats per descriptor, 0 while none is configured.  Product library only. */
int svs_pipe_gdesc_configure(void *p, int nlayers, const void *layers, const float *params, long long nparams, const void *prep_or_null);
int svs_pipe_gdesc_dim(void *p);
/* LoopClosure::ExtractFeatureVec (src/loopclosure.cpp:92-129) for every stream whose last step made a keyframe, on the keyframe's left
 * image (level 0 of its pyramid slot, until the stream's next step); one kernel call for all streams.  vecs: [nstreams][dim], raw; the
 * rows of the other streams are zeroed.  Works with device_map = 1 as well.  Returns the number of rows computed, -1 (nothing
 * written): no network configured, the kernel's refusal. */
int svs_pipe_describe_global_new_keyframes(void *p, float *vecs);
/* the matches (candidate row, current row, distance, inlier) of the pair the last svs_pipe_detect_loops verified on a stream: returns
 * their number (nothing written when cap is smaller or match4 is NULL), -1 when it verified none there */
long long svs_pipe_loop_matches(void *p, int stream, int *match4, long long cap);
/* the keyframe ids a stream's store holds: returns their number (nothing written when cap is smaller or ids is NULL) */
long long svs_pipe_loopdb_ids(void *p, int stream, int *ids, long long cap);
/* the keyframe that last closed a loop on the stream, -1: none */
long long svs_pipe_last_closed_keyframe(void *p, int stream);
/* on != 0: keyframes that leave the window from now on keep their feature lists, as the reference's do (svs_pipe_verify_loops
 * reads the candidate keyframe's; a keyframe whose lists were released is refused there).  Off by default. */
int svs_pipe_keep_keyframe_features(void *p, int on);
/* the left features of keyframe kf_id, read-only: 8 doubles each (x, y, landmark id or -1, outlier flag, has_xyz, X, Y, Z — the
 * landmark position svs_pipe_verify_loops would gather: the live one, else the archived float one) and, if asked for, the keyframe's
 * pose.  Returns the number of features (nothing is written when cap is too small: call again), -1 for a bad stream / id or a map
 * on the device.  svs_pipe_map_snapshot's format is unchanged. */
long long svs_pipe_keyframe_features(void *p, int stream, long long kf_id, double *out8, long long cap, double *pose7_or_null);
/* Inspection hook (host map only): the map of one stream as it stands after the last step, flat.
 *   ints: n_active_keyframes, (keyframe id)*, n_active_landmarks, per landmark { id, observed_times, n_obs,
 *         (keyframe id, 0 left / 1 right, index of the feature in that keyframe's list)* }  — ids ascending, observations in list order
 *   dbl:  7 per active keyframe (pose, T_cw), then 3 per active landmark (position)
 * Returns the number of ints the snapshot has (nothing is written when cap_i or cap_d is too small: call again), -1 for a bad
 * stream, -2 when the map lives on the device (svslam_dmap_read is the reader there), -3 when a BA in flight cannot be completed. */
long long svs_pipe_map_snapshot(void *p, int stream, long long *ints, long long cap_i, double *dbl, long long cap_d);
/* underlying svslam_ctx (product build) or NULL (CPU twin) */
void *svs_pipe_kernel_ctx(void *p);
/* context the backend's local BA runs on: a second one when backend_on == 2, else the same */
void *svs_pipe_backend_ctx(void *p);

#ifdef __cplusplus
}
#endif
