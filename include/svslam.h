/*
 * svslam.h — C ABI of libsvslam_hip.so: the MI355X (gfx950) implementation of the
 * per-frame hot path of farhad-dalirani/StereoVision-SLAM.
 *
 * The reference has no FFI layer; its hot path is five third-party library call
 * sites inside two private C++ members (Frontend::Track, Backend::Optimize).
 * Each entry point below replaces exactly one of those call sites (cited per
 * function, file:line into the reference tree).  The ABI is flat: plain
 * pointers and sizes, caller-owned host buffers, no C++/torch types, int
 * return codes (0 = ok, <0 = error, see svslam_last_error), never throws.
 *
 * Everything is *batched over jobs*: one job = one call site invocation of one
 * SLAM stream.  A single-stream caller passes njobs = 1; a multi-stream host
 * (one process per GPU, S streams in lockstep) passes S jobs and gets one
 * launch sequence for all of them.  Jobs are independent.
 *
 * Conventions
 *   - images: u8, row-major, (width,height) fixed at context creation
 *   - points: float32 (x,y) interleaved, exactly cv::Point2f
 *   - SE(3):  double[7] = unit quaternion (x,y,z,w) + translation (x,y,z),
 *             the memory layout of Sophus::SE3d; T_cw (world -> stereo rig)
 *   - camera: double[4] = fx, fy, cx, cy ; extrinsic = SE(3) rig -> camera
 */
#ifndef SVSLAM_H
#define SVSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVSLAM_PYR_LEVELS 4      /* maxLevel 3  (src/frontend.cpp:107,355) */
#define SVSLAM_LK_WIN 11         /* cv::Size(11,11) (src/frontend.cpp:107,355) */

typedef struct svslam_ctx svslam_ctx;

typedef struct svslam_limits {
    int device;        /* HIP device ordinal                                   */
    int width, height; /* working resolution (620x188 for KITTI-00, F3)        */
    int max_slots;     /* resident image pyramids (3 per stream)               */
    int max_jobs;      /* max jobs per batched call (= streams per GPU)        */
    int max_pts;       /* max points per job (tracked + new corners)           */
    int max_corners;   /* max corners returned per GFTT job                    */
    int max_kf;        /* BA: max keyframes per problem                        */
    int max_lm;        /* BA: max landmarks per problem                        */
    int max_obs;       /* BA: max observations (edges) per problem             */
    int max_streams;   /* streams whose last-frame features stay resident in HBM
                          (svslam_rtrack_*); 0 = none                          */
    int device_map;    /* 1: every resident stream also keeps its MAP in HBM (keyframe window of
                          max_kf slots x max_pts features, max_lm landmark slots — a power of two):
                          svslam_dmap_*                                          */
} svslam_limits;

/* ---- lifetime -------------------------------------------------------- */
int  svslam_create(const svslam_limits *lim, svslam_ctx **out);
void svslam_destroy(svslam_ctx *ctx);
const char *svslam_last_error(const svslam_ctx *ctx);
/* version / build info string (arch, compiler) */
const char *svslam_build_info(void);

/* ---- image pyramids ---------------------------------------------------
 * Replaces cv::buildOpticalFlowPyramid as run inside cv::calcOpticalFlowPyrLK
 * (src/frontend.cpp:105-109, 353-357).  Builds the 4-level u8 pyramid of each
 * image into a resident slot; LK and GFTT refer to slots, so the previous
 * frame's pyramid is reused instead of rebuilt.
 * src_is_device: imgs[i] are device pointers already in HBM (bench / pipelined
 * use) instead of host pointers.                                            */
int svslam_pyramid_batch(svslam_ctx *ctx, int n, const int *slots,
                         const void *const *imgs, const int *strides,
                         int src_is_device);
/* Same, but the source is the full-resolution frame and the 1/2 nearest
 * decimation of Dataset::NextFrame (src/dataset.cpp:126-129) is fused into the
 * level-0 write: dst(x,y) = src(2x,2y).  src size = (src_w, src_h); the
 * context's (width,height) must equal (cvRound(src_w/2), cvRound(src_h/2)). */
int svslam_pyramid_decimate_batch(svslam_ctx *ctx, int n, const int *slots,
                                  const void *const *imgs, const int *strides,
                                  int src_w, int src_h, int src_is_device);
/* Declares that every image handed to svslam_pyramid_batch / svslam_track_batch from now on
 * is a full-resolution src_w x src_h frame to be decimated the same way (0,0 switches it
 * off): a caller that keeps the camera frames in HBM never stores the half-size copies the
 * reference makes in Dataset::NextFrame.                                          */
int svslam_set_source_size(svslam_ctx *ctx, int src_w, int src_h);
/* Shape of the latency-bound kernels.  0 (default): least total work per job, for batches of
 * hundreds of streams.  1: a few streams per launch (one camera per GPU, BASELINE config 4) —
 * the pose-only LM of EstimateCurrentPose (src/frontend.cpp:394-558) runs on four wavefronts per
 * job instead of one (about half the latency per frame, ~1.3x the arithmetic).  The two shapes
 * sum the normal equations in different orders: results agree to rounding, each is deterministic.
 * In this mode the blocking calls also wait inside the HIP runtime instead of sleep-polling.
 * A local BA of at most a few problems (Backend::Optimize, src/backend.cpp:22-164) is then dealt over 4 / 8 / 16 workgroups per
 * problem that meet at in-launch barriers.  Those need every workgroup resident at once, so the mode sizes itself from the
 * device: shards x problems <= co-resident solver workgroups per CU x CUs (SVSLAM_LL_CUS=<n> tells it a smaller CU count, for
 * a CU-masked process or a partition); calls with more problems — or a device without room for one — use one workgroup per
 * problem, and a problem whose shards still do not all arrive (the CUs were busy with other work) is solved again that way
 * inside the same call.  Restriction: the solver scratch is one per context — svslam_local_ba_submit / _batch are refused while
 * a deferred local BA of the device map (svslam_dmap_params::ba_defer) is in flight on the context.                          */
int svslam_set_low_latency(svslam_ctx *ctx, int on);
/* Parameter tolerance of the pose-only LM (svslam_pose_only_batch, svslam_track_batch, svslam_rtrack_batch; default 1e-12,
 * environment SVSLAM_PO_XTOL at svslam_create).  A round of EstimateCurrentPose (src/frontend.cpp:482-493: optimize(10)) ends
 * when the first trial of an LM iteration, taken at a damping not above g2o's initial one for the present system (1e-5 x the
 * largest diagonal entry of H), asks for a step whose six
 * components are all <= xtol (metres / radians): the round stands at a stationary point of its cost.  g2o has no such test;
 * it runs the ten iterations, and where a round has converged earlier it spends the rest on trials that move the pose by
 * rounding noise and are accepted or rejected by the sign of that noise.  The trials that are run are g2o's, bit for bit;
 * what the rule leaves out moves the pose by about xtol.  At the default that is what another summation order moves, and
 * every comparison with the oracle holds unchanged; 1e-9 ends the slowly (linearly) converging Huber rounds three
 * iterations earlier (-20 % of the kernel for a tracked frame) at the price that two runs which differ in it part ways as
 * early as runs of different kernel shapes do (LK rounds its initial guesses to f32): DESIGN 4.4 has the table.
 * xtol = 0: g2o's schedule to the last trial.  0 <= xtol <= 1e-6.  Local BA is not touched: its ten iterations all move
 * the window.                                                                                                           */
int svslam_set_pose_only_xtol(svslam_ctx *ctx, double xtol);
/* the tolerance the context actually uses (the default, svslam_set_pose_only_xtol or the SVSLAM_PO_XTOL environment variable
 * read by svslam_create — which fails on a value outside [0, 1e-6] instead of ignoring it); -1 for a null context */
double svslam_get_pose_only_xtol(const svslam_ctx *ctx);
/* test hook: read one level back (tight rows of *w bytes) */
int svslam_pyramid_read(svslam_ctx *ctx, int slot, int level, uint8_t *out,
                        int *w, int *h);

/* test hook: the level with its stored 16-pixel BORDER_REFLECT_101 continuation (what LK windows, pyrDown taps
 * and the GFTT stencils read without index arithmetic): (h + 32) tight rows of (w + 32) bytes */
int svslam_pyramid_read_padded(svslam_ctx *ctx, int slot, int level, uint8_t *out);

/* ---- pyramidal LK -----------------------------------------------------
 * Replaces cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err,
 * Size(11,11), 3, TermCriteria(COUNT+EPS,30,0.01), OPTFLOW_USE_INITIAL_FLOW)
 * at src/frontend.cpp:353-357 (TrackLastFrame) and :105-109
 * (FindFeaturesInRight).  next_xy holds the initial guess on entry.          */
typedef struct svslam_lk_job {
    int prev_slot, next_slot; /* pyramids built by svslam_pyramid_batch      */
    int pt_ofs, npts;         /* range in the concatenated point arrays      */
} svslam_lk_job;

typedef struct svslam_lk_params {
    int    max_level;   /* 3                                                 */
    int    max_iter;    /* 30 (clamped to [0,100] like OpenCV)               */
    double epsilon;     /* 0.01 (squared internally like OpenCV)             */
    double min_eig_thr; /* 1e-4 (OpenCV default)                             */
    int    use_initial_flow; /* 1                                            */
} svslam_lk_params;

int svslam_lk_batch(svslam_ctx *ctx, int njobs, const svslam_lk_job *jobs,
                    int total_pts, const float *prev_xy, float *next_xy,
                    uint8_t *status, float *err, const svslam_lk_params *p);

/* ---- GFTT (Shi-Tomasi) --------------------------------------------------
 * Replaces the mask construction + cv::GFTTDetector::detect at
 * src/frontend.cpp:42-51 (detector created at :24 with
 * (num_features, 0.01, 20)).  rect_xy are the positions of the existing left
 * features; each masks the inclusive square [round(pt-10), round(pt+10)].
 * Output: up to max_corners integer-valued corners per job, quality-descending,
 * out_xy laid out [njobs][max_corners][2].                                  */
typedef struct svslam_gftt_job {
    int slot;              /* level 0 of this pyramid slot is the image      */
    int rect_ofs, nrect;   /* range in rect_xy                               */
} svslam_gftt_job;

int svslam_gftt_batch(svslam_ctx *ctx, int njobs, const svslam_gftt_job *jobs,
                      int total_rects, const float *rect_xy, int max_corners,
                      double quality, double min_dist, float *out_xy,
                      int *out_n);
/* test hook: min-eigenvalue map of a slot's level-0 image (w*h floats) */
int svslam_gftt_eigmap(svslam_ctx *ctx, int slot, float *out);

/* ---- dense stereo: the reference's second program (run_dense_reconstruction) ---------------
 * svslam_stereo_bm_batch replaces stereo_depth_est_->compute(left, right, disparity_map) at
 * src/dense_reconstruction.cpp:114 (matcher created at :89 as cv::StereoBM::create(128, 15),
 * include/StereoVisionSLAM/dense_reconstruction.h:56-57; everything else at OpenCV's defaults:
 * PREFILTER_XSOBEL, minDisparity 0, no speckle filter, no disp12MaxDiff).  The images are level 0
 * of two pyramid slots.  Output: CV_16S maps of 16 x disparity, -16 where OpenCV writes none.
 * An image too small for one window (nd - 1 + r >= w - r, or h < 2 r + 1 with r = block_size / 2)
 * succeeds with every pixel -16, like OpenCV.
 * num_disparities: positive multiple of 16, <= 256; block_size: odd, 5 .. 21; pre_filter_cap: 1 .. 63.
 * PREFILTER_NORMALIZED_RESPONSE, the speckle filter and disp12MaxDiff are not built.  Colour input:
 * svslam_pyramid_bgr_batch and svslam_dense_cloud_bgr_batch, below.                                */
typedef struct svslam_bm_params {
    int num_disparities;   /* 128 */
    int block_size;        /* 15  */
    int pre_filter_cap;    /* 31  */
    int texture_threshold; /* 10  */
    int uniqueness_ratio;  /* 15; 0 disables the uniqueness test (OpenCV: if( uniquenessRatio > 0 )), 1..10000 apply it */
    int reserved;
} svslam_bm_params;
typedef struct svslam_bm_job { int slot_left, slot_right; } svslam_bm_job;   /* level 0 of each pyramid slot */

int svslam_stereo_bm_batch(svslam_ctx *ctx, int njobs, const svslam_bm_job *jobs, const svslam_bm_params *p,
                           int16_t *out_disp /* [njobs][height][width] */);

/* test hook: the output rows per workgroup strip (16, 8 or 4, by the number of workgroups the call has) that a
 * call of njobs jobs with these parameters runs with; 0 where the image is too small for one window.  The
 * result of the matcher does not depend on it; the tests use it to know that they cover every strip height. */
int svslam_stereo_bm_strip_rows(svslam_ctx *ctx, int njobs, const svslam_bm_params *p);

/* The matcher followed by the loop of src/dense_reconstruction.cpp:116-173 with its types: disparity
 * x 1/16 in float, depth = (float fx * float baseline) / disparity (0 where disparity <= 0), pixels with
 * depth < min_depth (1 in the reference) dropped, the rest through Camera::pixel2world (src/camera.cpp:
 * 39-44, 58-86: T_cw^-1 * ext_l^-1 * pixel2camera) in double and rounded to float (PointXYZRGB).
 * Job i's points are written from out_xyz[3 * pt_ofs] / out_pix[pt_ofs] on in the reference's order —
 * x outer, y inner; out_pix holds y * width + x of each point, for the caller to colour it from the
 * image it holds (svslam_dense_cloud_bgr_batch, below, returns the colours itself).  n_points (out) beyond max_pts_per_job is an error, nothing of that call is returned.
 * out_disp_or_null: the disparity maps as svslam_stereo_bm_batch returns them.
 * The StatisticalOutlierRemoval and the VoxelGrid of :175-209 (PCL) are calls of their own, below:
 * svslam_cloud_sor_batch and svslam_cloud_voxel_grid take the clouds this call returned.             */
typedef struct svslam_dense_job {
    int    slot_left, slot_right;
    int    pt_ofs;         /* in: where this job's points start in out_xyz / out_pix */
    int    n_points;       /* out                                                     */
    double T_cw[7];        /* keyframe pose (keyframes_poses_[i].cast<double>())      */
} svslam_dense_job;

int svslam_dense_cloud_batch(svslam_ctx *ctx, int njobs, svslam_dense_job *jobs, const double cam_l[4],
                             const double ext_l[7], double baseline, const svslam_bm_params *p,
                             double min_depth, int max_pts_per_job, float *out_xyz, int *out_pix,
                             int16_t *out_disp_or_null);

/* ---- colour input of run_dense_reconstruction ----------------------------------------------
 * Every dense config of the reference sets is_color_input: 1: Dataset reads cv::IMREAD_COLOR, DenseReconstruct()
 * converts both images with cv::cvtColor(COLOR_BGR2GRAY) for the matcher and gives every point the left image's
 * b, g, r at its pixel (src/dense_reconstruction.cpp:104-171).  BGR is the only byte order: it is the cv::Mat
 * the reference holds.
 * The grey of a colour pixel, in integers: the one definition the device kernel (csrc/k_colour.h) and the host
 * PNG reader (facade::read_png) share.  Parity of these weights with OpenCV's own 8-bit BGR2GRAY is unpinned
 * (DESIGN 9).                                                                                            */
#define SVSLAM_GREY_FROM_RGB(r, g, b) (((r) * 4899 + (g) * 9617 + (b) * 1868 + 8192) >> 14)

/* nplanes colour planes of width x height x 3 bytes (b, g, r) on the device; 0 frees them; a new count drops
 * the contents, the present count keeps them. */
int svslam_colour_reserve(svslam_ctx *ctx, int nplanes);
/* n packed 8-bit BGR images (3 bytes per pixel, strides[i] >= 3 * src_w bytes per row, host or device memory)
 * -> pyramid slots slots[i], built from the grey image exactly as svslam_pyramid_batch builds them from that
 * grey image, and, where planes[i] >= 0, the working-resolution BGR image into that colour plane (-1: keep no
 * colour).  src_w x src_h is the context's width x height, or a size that halves to it by
 * svslam_pyramid_decimate_batch's rule; then dst(x, y) = src(2x, 2y) and only the even source rows are read.
 * No byte beyond strides[i] * (src_h - 1) + 3 * src_w of a source is read.
 * Errors, all decided before anything is launched or written: a null pointer, n > max_jobs, a bad slot, a
 * plane outside [-1, nplanes), a plane named while none is reserved, the same plane named twice, a stride
 * below 3 * src_w, a source size that is neither the context's nor halves to it.                          */
int svslam_pyramid_bgr_batch(svslam_ctx *ctx, int n, const int *slots, const int *planes, const void *const *imgs,
                             const int *strides, int src_w, int src_h, int src_is_device);
/* test hook: a colour plane, [height][width][3] */
int svslam_colour_read(svslam_ctx *ctx, int plane, uint8_t *out);
/* svslam_dense_cloud_batch with the colour of every point: out_bgr holds 3 bytes (b, g, r) per point, indexed
 * like out_xyz, taken on the device from plane planes[i] of job i at out_pix.  out_xyz, out_pix, n_points and
 * the disparity maps have the bits svslam_dense_cloud_batch gives for the same slots; the max_pts_per_job rule
 * is the same.  Further errors, decided before anything is launched: null planes / out_bgr, no planes reserved,
 * a plane outside [0, nplanes), a plane no upload has written since it was reserved.                       */
int svslam_dense_cloud_bgr_batch(svslam_ctx *ctx, int njobs, svslam_dense_job *jobs, const double cam_l[4],
                                 const double ext_l[7], double baseline, const svslam_bm_params *p,
                                 double min_depth, int max_pts_per_job, const int *planes, float *out_xyz,
                                 int *out_pix, uint8_t *out_bgr, int16_t *out_disp_or_null);

/* ---- the cloud filters of run_dense_reconstruction -----------------------------------------
 * The numeric contract of both is tests/ref_cloud_filters.py (parity with PCL itself is unpinned).
 * pcl::StatisticalOutlierRemoval (src/dense_reconstruction.cpp:180-184, :195-199) on nseg independent clouds:
 * segment s is xyz[3*seg_ofs[s]] .. xyz[3*seg_ofs[s+1]].  out_keep: 1 / 0 per point; out_mean_dist_or_null;
 * out_threshold[nseg] (NaN where the segment has fewer than mean_k + 1 points: all kept).  mean_k 1 .. 64.
 * out_keep and out_mean_dist_or_null are indexed like the points (point seg_ofs[s] + i at [seg_ofs[s] + i]).
 * The exact k-nearest-neighbour mean distances come from the device; the statistics, the threshold and the
 * mask are computed on the host in PCL's sequential order.  A non-finite coordinate is an error (PCL's
 * branch for such points is not built); at most 2^30 points per call.                                   */
int svslam_cloud_sor_batch(svslam_ctx *ctx, int nseg, const int64_t *seg_ofs, const float *xyz, int mean_k,
                           double stddev_mul, uint8_t *out_keep, float *out_mean_dist_or_null, double *out_threshold);
/* pcl::VoxelGrid (:203-209), downsample_all_data: returns the number of output points in *out_n (<= n), out_overflowed = 1
 * and output = input where PCL's int32 index guard trips ("Leaf size is too small for the input dataset").
 * rgb: 3 bytes per point.  out_xyz / out_rgb hold n points.  One output point per occupied voxel, in ascending
 * voxel index; a voxel's sums run in ascending point index.                                              */
int svslam_cloud_voxel_grid(svslam_ctx *ctx, int64_t n, const float *xyz, const uint8_t *rgb, double leaf,
                            float *out_xyz, uint8_t *out_rgb, int64_t *out_n, int *out_overflowed);
/* measurement hook: since the last call of it, the nearest-neighbour queries svslam_cloud_sor_batch ran and how many
 * of them had to scan a larger block of cells than the one they started with */
int svslam_debug_cloud_sor_climbs(svslam_ctx *ctx, long long *out_queries, long long *out_climbed);

/* ---- stereo triangulation ----------------------------------------------
 * Replaces slam::triangulation() (include/StereoVisionSLAM/algorithm.h:10-87)
 * as called from BuildInitMap (src/frontend.cpp:165-174) and
 * TriangulateNewPoints (:277-295): pixel2camera on both pixels, 4x4 DLT + SVD,
 * gate sv[3]/sv[2] < 1e-2 && z > 0 && (zmax <= 0 || z <= zmax), then
 * p_world = T_wc * p.                                                        */
typedef struct svslam_tri_job {
    int    pt_ofs, npts;
    double T_wc[7];     /* current_frame->Pose().inverse(); identity at init */
    double zmax;        /* max_triangulation_depth, <=0: no upper gate       */
} svslam_tri_job;

int svslam_triangulate_batch(svslam_ctx *ctx, int njobs,
                             const svslam_tri_job *jobs, int total_pts,
                             const double cam_l[4], const double ext_l[7],
                             const double cam_r[4], const double ext_r[7],
                             const float *uv_l, const float *uv_r,
                             double *out_xyz, uint8_t *out_ok);

/* ---- pose-only refinement ------------------------------------------------
 * Replaces the g2o problem of Frontend::EstimateCurrentPose
 * (src/frontend.cpp:394-558; VertexPose + EdgeProjectionPoseOnly,
 * include/StereoVisionSLAM/g2o_types.h:25-65,94-174): 4 rounds x optimize(10)
 * of Levenberg-Marquardt, estimate reset to the prior each round, chi2 > 5.991
 * => outlier (excluded next round), Huber(1) in rounds 0-2.                  */
typedef struct svslam_pose_job {
    int    pt_ofs, npts;
    double pose[7];     /* in: prior T_cw; out: refined                      */
    int    n_inlier;    /* out                                                */
    int    reserved;
} svslam_pose_job;

int svslam_pose_only_batch(svslam_ctx *ctx, int njobs, svslam_pose_job *jobs,
                           int total_pts, const double cam[4],
                           const double *xyz, const float *uv,
                           uint8_t *outlier, double chi2_th, int rounds,
                           int iters);

/* ---- local bundle adjustment ----------------------------------------------
 * Replaces optimizer.initializeOptimization(); optimizer.optimize(10) of
 * Backend::Optimize (src/backend.cpp:22-164; VertexPose, VertexXYZ
 * marginalised, EdgeProjection with Huber(delta = chi2_th),
 * g2o_types.h:67-92,176-229): LM with Schur complement over the landmarks,
 * dense solve of the reduced camera system, no vertex fixed.  Returns the
 * optimised poses / points and the per-edge chi2 the caller thresholds
 * (src/backend.cpp:167-213).  obs_kf / obs_lm are indices local to the job.  */
typedef struct svslam_ba_job {
    int kf_ofs, nkf;
    int lm_ofs, nlm;
    int obs_ofs, nobs;
    int iters_done;     /* out: LM iterations executed                       */
    int reserved;       /* out: accounting — (LM trials << 24) | block pairs of the Schur complement */
} svslam_ba_job;

int svslam_local_ba_batch(svslam_ctx *ctx, int njobs, svslam_ba_job *jobs,
                          const double cam_l[4], const double ext_l[7],
                          const double cam_r[4], const double ext_r[7],
                          int total_kf, double *poses, int total_lm,
                          double *pts, int total_obs, const int *obs_kf,
                          const int *obs_lm, const uint8_t *obs_is_right,
                          const float *obs_uv, double huber_delta, int iters,
                          double *edge_chi2);

/* The same call split in two, for a backend that runs beside the frontend the way
 * the reference's Backend thread does (src/backend.cpp:345-367, BackendLoop woken by
 * UpdateMap): submit copies the inputs, enqueues the solve on the context's stream
 * and returns; collect waits for it and writes poses / pts / edge_chi2 /
 * jobs[i].iters_done.  Between the two the context's staging memory belongs to the
 * batch: every other batched call on the same context fails until collect (use a
 * second context for the frontend).  collect takes the same njobs / totals.    */
int svslam_local_ba_submit(svslam_ctx *ctx, int njobs, const svslam_ba_job *jobs,
                           const double cam_l[4], const double ext_l[7],
                           const double cam_r[4], const double ext_r[7],
                           int total_kf, const double *poses, int total_lm,
                           const double *pts, int total_obs, const int *obs_kf,
                           const int *obs_lm, const uint8_t *obs_is_right,
                           const float *obs_uv, double huber_delta, int iters);
int svslam_local_ba_collect(svslam_ctx *ctx, int njobs, svslam_ba_job *jobs,
                            int total_kf, double *poses, int total_lm, double *pts,
                            int total_obs, double *edge_chi2);

/* ---- global pose-graph optimisation --------------------------------------------
 * Replaces the g2o problem of LoopClosure::PoseGraphOptimization (src/loopclosure.cpp:641-799: VertexPose per keyframe,
 * keyframe 0 fixed :701-704; EdgePoseGraph per odometry edge :720-735 and per loop edge :738-753, identity information, no
 * robust kernel; optimize(22) :758 under OptimizationAlgorithmLevenberg over LinearSolverDense :662-673) and the landmark
 * re-anchoring that follows it (:760-784).  One job is one graph: nkf vertices (SE(3) as everywhere here, ascending keyframe id)
 * and nedge edges (a, b, M) with residual log(M^-1 T_a T_b^-1) (g2o_types.h:247-262; Sophus' 6-vector, translation first;
 * formed as M^-1 (T_a T_b^-1): an odometry edge whose M is the host's T_a * T_b^-1 has residual exactly 0, so a graph without
 * loop edges returns its input bits) and update T <- exp(d) T (VertexPose::oplusImpl, g2o_types.h:42-49).  Vertices with
 * fixed[i] != 0 are constant.  LM control flow:
 * g2o's, exactly as svslam_local_ba_batch has it.  After the last iteration point p with anchor vertex k >= 0 becomes
 * T_k,new^-1 (T_k,old p) in f64 (also in a job without edges, where it is the identity up to rounding); anchor -1: untouched.
 * The reference hands g2o a dense 6N x 6N system ("Takes seconds to minutes", :655); here the system is never formed: with the
 * vertices in ascending id H is block tridiagonal plus one block per loop edge, and a block-skyline LDL^T (one wavefront per
 * job) factorises it inside each row's envelope.  Declared deviations: closed-form Jacobians where g2o differentiates
 * this edge numerically; an unpivoted factorisation where Eigen's dense Cholesky is used.
 * Errors, nothing written: an edge index outside [0, nkf); a == b; a job with vertices but none fixed; a job with edges but
 * no vertices; a job with more than 2^31 / 42 free vertices; jobs whose kf / edge / pt ranges do not ascend from job to job or overlap (gaps are allowed); a pose or measurement
 * quaternion whose squared norm is further than 2e-6 from 1; an anchor outside [-1, nkf); no memory for the solver scratch
 * (allocated inside the call on demand and kept; svslam_limits has no say in it, njobs is not bounded by max_jobs).
 * Valid no-ops: a job with nkf == 0 or nedge == 0 (poses as given, iters_done = n_trials = 0, chi2 = 0).
 * A job's result does not depend on the other jobs of the call, and two calls on the same inputs give the same bits.
 * svslam_lm_trace records the trials of jobs 0 .. max_jobs - 1 of this call in its six-double format.             */
typedef struct svslam_pg_job {
    int kf_ofs, nkf;        /* vertices, ascending keyframe id */
    int edge_ofs, nedge;
    int pt_ofs, npt;        /* landmarks to re-anchor; npt may be 0 */
    int iters_done;         /* out */
    int n_trials;           /* out: accepted + rejected */
    double chi2_before, chi2_after;   /* out */
} svslam_pg_job;

int svslam_pose_graph_batch(svslam_ctx *ctx, int njobs, svslam_pg_job *jobs,
                            int total_kf, double *poses /* in/out, 7 each */, const uint8_t *fixed,
                            int total_edges, const int *edge_a, const int *edge_b /* local to the job */,
                            const double *edge_meas /* 7 each */,
                            int total_pts, const int *pt_anchor /* local vertex or -1 */, double *pts /* in/out */,
                            int iters);

/* ---- local fusion: a verified loop corrects the active window ----------------------
 * The arithmetic of LoopClosure::LocalFusion (src/loopclosure.cpp:439-526), one job per closed loop; `cur` is the keyframe that
 * closed it, T_corr its corrected pose (svslam_loop_job::T_corr).  The landmark replacement that follows in the reference
 * (:530-573) is map bookkeeping and stays with the caller.
 *  1. corrected table (:451-467): row i < nkf is window keyframe i, corrected[i] = (T_i T_cur^-1) T_corr in that association;
 *     corrected[cur] = T_corr.  cur >= 0 is its index in the window; cur = -1: it has left the window, T_cur is given in the job and
 *     the table has one more row, number nkf, for it.
 *  2. landmarks (:470-503): landmark g of the call has the observations obs_kf[obs_ptr[g] .. obs_ptr[g + 1]) in list order; an entry is
 *     the table row of the observation's keyframe (a right-image observation counts, its frame is the keyframe), or -1 where the
 *     feature no longer names a live landmark or its frame has no row.  The FIRST entry k >= 0 moves the landmark:
 *     p' = corrected[k]^-1 (T_k p) with the old T_k; pt_kf[g] = k.  No such entry: the position is kept, pt_kf[g] = -1 and the job's
 *     n_unanchored counts it (the reference asserts and dereferences null there: declared deviation).
 *  3. last frame (:506-526): last >= 0 is its index in the window and T_last comes back as that row of the table; last = -1: it is no
 *     active keyframe and T_last becomes (T_last T_cur^-1) T_corr.
 * poses comes back as rows 0 .. nkf - 1 of the table (:511-519 writes the active keyframes only: an inactive cur is not written
 * anywhere).  All in f64 with the SE(3) operations of svslam_pose_graph_batch, no contraction: a job's result depends on nothing
 * but its inputs, and two calls give the same bits.
 * Errors, nothing written and nothing launched: a null array whose count is not 0; a negative count; jobs whose kf / pt ranges
 * leave the arrays, do not ascend from job to job or overlap (gaps are allowed and come back untouched); an obs_ptr that descends or
 * leaves obs_kf; an obs_kf outside [-1, nkf] (nkf only with cur = -1); cur or last outside [-1, nkf); a quaternion (window poses,
 * T_corr, T_cur with cur = -1, T_last with last = -1) whose squared norm is further than 2e-6 from 1; no memory for the call's
 * buffer (allocated on demand and kept; njobs is not bounded by max_jobs).  njobs == 0 is success.                             */
typedef struct svslam_lf_job {
    int kf_ofs, nkf;        /* the active window */
    int pt_ofs, npt;        /* the active landmarks; their observation lists are obs_ptr[pt_ofs .. pt_ofs + npt] */
    int cur;                /* index of cur in the window, or -1 */
    int last;               /* index of the frontend's last frame in the window, or -1 */
    double T_cur[7];        /* read when cur == -1 */
    double T_corr[7];
    double T_last[7];       /* in (read when last == -1) / out */
    int n_unanchored;       /* out */
    int reserved;
} svslam_lf_job;

int svslam_local_fusion_batch(svslam_ctx *ctx, int njobs, svslam_lf_job *jobs,
                              int total_kf, double *poses /* in/out, 7 each */,
                              int total_pts, double *pts /* in/out */, const int *obs_ptr /* total_pts + 1 */,
                              int total_obs, const int *obs_kf, int *pt_kf /* out, total_pts */);

/* ---- loop verification: Hamming match, PnP RANSAC, loop gates ---------------------
 * Replaces LoopClosure::KeypointMatchWithLoopCandid and LoopClosure::CalculatePose (src/loopclosure.cpp:286-437, called at :831-862).
 * One job is one keyframe pair of one stream: nc descriptors of the candidate (older) keyframe with the landmark of each one's
 * feature (has_xyz = 0 where the reference's map_point_.lock() fails), nq descriptors of the current keyframe with each one's pixel.
 * Match (:291-326): BruteForce-Hamming match(query = candidate, train = current) — every candidate row takes the nearest current
 * row over 256 bits, the lowest current index on a tie, no cross-check; thr = max(2 d_min, 30); matches with distance <= thr are
 * kept in ascending (candidate row, current row); fewer than min_matches: SVSLAM_LOOP_FEW_MATCHES (also nc == 0 or nq == 0, where
 * the reference dereferences min_element of an empty vector).  3-D filter (:340-371): matches without a landmark are dropped,
 * landmarks rounded to float (cv::Point3f); fewer than max(min_matches, 4): FEW_POINTS.  PnP RANSAC (:375-398) is this library's own
 * procedure: ransac_iters hypotheses, hypothesis i draws 4 distinct point indices from a stateless hash of (seed, i,
 * draw), P3P on the first three, the fourth chooses among the solutions, a degenerate sample gives no hypothesis; inlier: depth > 0
 * and squared reprojection error <= reproj_px^2; the winner has the most inliers (lowest i on a tie), all hypotheses are evaluated;
 * fewer than min_matches inliers or no hypothesis: FEW_INLIERS.  The inliers reported are the winner's, before the refinement: LM on
 * exp(d) T over them, squared pixel error, no robust kernel, g2o's control as svslam_local_ba_batch has it, 10 iterations.
 * Declared deviations from cv::solvePnPRansac: EPnP on 5 points there, cv::RNG, an early stop at confidence 0.99, no depth test,
 * solvePnP(ITERATIVE) from a DLT start as the refinement.  Gates (:400-436): T_corr = ext_l^-1 T_pnp, T_rel = T_corr T_cand^-1;
 * |log T_rel| > max_pose_distance: TOO_FAR; d = |log(T_cur T_corr^-1)| > max_pose_difference: TOO_DIFFERENT; else ACCEPTED with
 * need_correction = d > min_pose_difference (log: Sophus' 6-vector).
 * Every output is defined for every status: counts 0, poses the identity, d 0 where a stage was not reached.  A job's match list
 * (candidate row, current row, distance, inlier flag; rows local to the job) starts at its c_ofs in the four match arrays and has
 * n_matches entries; what lies behind them in the job's range is not specified.
 * Errors, nothing written: nc or nq above 1024; a pose or ext_l quaternion whose squared norm is further than 2e-6 from 1; jobs
 * whose c / q ranges do not ascend from job to job or overlap (gaps are allowed) or leave the arrays; ransac_iters outside
 * [1, 1024]; a negative min_matches or reproj_px; no memory for the call's buffer (allocated inside the call on demand and kept;
 * svslam_limits has no say in it, njobs is not bounded by max_jobs).  Valid no-ops: njobs == 0; a job with nc == 0 or nq == 0.
 * A job's result does not depend on the other jobs of the call, and two calls on the same inputs give the same bits.   */
enum { SVSLAM_LOOP_ACCEPTED = 0, SVSLAM_LOOP_FEW_MATCHES = 1, SVSLAM_LOOP_FEW_POINTS = 2, SVSLAM_LOOP_FEW_INLIERS = 3,
       SVSLAM_LOOP_TOO_FAR = 4, SVSLAM_LOOP_TOO_DIFFERENT = 5 };
typedef struct svslam_loop_job {
    int c_ofs, nc;          /* candidate rows: desc_c, xyz_c, has_xyz; the job's match list starts at c_ofs too */
    int q_ofs, nq;          /* current rows: desc_q, uv_q */
    double T_cur[7], T_cand[7];      /* Frame::Pose() of the two keyframes */
    int status;             /* out: SVSLAM_LOOP_* */
    int n_matches, n_points, n_inliers, need_correction, reserved;   /* out */
    double T_corr[7], T_rel[7], d;   /* out */
} svslam_loop_job;
typedef struct svslam_loop_params {
    double cam[4], ext_l[7];         /* the left camera */
    int min_matches;                 /* min_num_acceptable_keypoint_match */
    int ransac_iters;                /* 100 */
    double reproj_px;                /* 5.991, a pixel radius */
    double max_pose_distance;        /* max_pose_distance_between_loop_keyframes */
    double min_pose_difference, max_pose_difference;   /* m{in,ax}_pose_differnece_between_old_new */
    unsigned seed; int reserved;
} svslam_loop_params;
int svslam_loop_verify_batch(svslam_ctx *ctx, int njobs, svslam_loop_job *jobs, const svslam_loop_params *params,
                             int total_c, const uint8_t *desc_c /* 32 each */, const double *xyz_c /* 3 each */, const uint8_t *has_xyz,
                             int total_q, const uint8_t *desc_q /* 32 each */, const float *uv_q /* 2 each */,
                             int *match_c, int *match_q, int *match_dist, uint8_t *match_inlier /* out, total_c each */);

/* ---- loop-closure descriptors: BRIEF-256 at given points of a keyframe image ----------
 * Replaces LoopClosure::ExtractKeypointsDescriptor (src/loopclosure.cpp:131-171): cv::ORB::compute at provided keypoints, which carry
 * cv::KeyPoint's default angle of -1 degree, so no intensity-centroid angle enters; for the integer offsets of a table with |c| <= 13
 * that rotation rounds back to the table itself: plain BRIEF-256 on a blurred image.  One job is level 0 of one pyramid slot and a
 * range of points (x, y in xy).  The procedure, every step integer or written-out f32:
 *   filter   point i is kept iff edge <= x < w - edge and edge <= y < h - edge, compared in float; kept points keep their order; the
 *            kept rows of a job are the first n_desc rows of its range in desc, desc_pt[row] is the point's index inside the job;
 *            what lies behind those rows in the caller's arrays is left as it was.  Centre = round-half-to-even of (x, y).
 *   offsets  once per call: a = cosf(angle_deg (pi / 180)), b = sinf(..) in f32; ix = rint(px a - py b), iy = rint(px b + py a)
 *            for each of the 512 table points.
 *   blur     7 taps (18, 34, 49, 54, 49, 34, 18) / 256 = 256 g(sigma 2) rounded, the centre tap absorbing the remainder; separable;
 *            the horizontal sum is kept in full (<= 65280), the vertical sum over it, out = (v + 32768) >> 16.  Only pixels inside
 *            the image are read (see the refusals), so no border rule enters.
 *   tests    bit t (0 .. 255) = B(c + off[2t]) < B(c + off[2t + 1]), strict, on the blurred values; byte t / 8, bit t % 8.
 * Errors, nothing written: npts > 1024; ranges that do not ascend from job to job, overlap (gaps are allowed) or leave the arrays; a
 * slot out of range; edge < reach + 4, reach = the largest |ix|, |iy| after the rotation; reach > 24 (the wave's patch in LDS); a table
 * entry whose two points coincide; an angle that is not finite; no memory for the call's buffer (allocated inside the call on demand
 * and kept; svslam_limits has no say in it, njobs is not bounded by max_jobs).  Valid no-ops: njobs == 0, npts == 0, an image without
 * interior (w <= 2 edge).  Non-finite coordinates fail the filter.  A job's result does not depend on the other jobs of the call, and
 * two calls on the same inputs give the same bits.
 * The default table (pattern == NULL) is generated by a stateless hash (csrc/k_brief.h says how) and is NOT OpenCV's learned table; a
 * caller who has that one passes it.  svslam_brief_default_pattern copies the default out. */
typedef struct svslam_brief_job { int slot; int pt_ofs, npts; int n_desc /* out */; int reserved; } svslam_brief_job;
typedef struct svslam_brief_params {
    const int8_t *pattern;   /* [256][4] = x0,y0,x1,y1 per test; NULL: the library's default table */
    float angle_deg;         /* -1: cv::KeyPoint's default, what the reference's keypoints carry */
    int   edge;              /* 31: ORB's edgeThreshold */
} svslam_brief_params;
int svslam_brief_describe_batch(svslam_ctx *ctx, int njobs, svslam_brief_job *jobs, const svslam_brief_params *params,
                                int total_pts, const float *xy, uint8_t *desc /* [total_pts][32] */, int *desc_pt /* [total_pts] */);
int svslam_brief_default_pattern(int8_t out[1024]);

/* ---- ORB keypoint detector: oriented multi-scale FAST corners of a pyramid slot ----------
 * Replaces cv::ORB::create(num_features)->detect(img, kps, mask) of Frontend::DetectFeatures with keypoint_feature_detector: ORB
 * (src/frontend.cpp:20-33, :51).  ORB's defaults: scale factor 1.2f, 8 levels, edge threshold 31, first level 0, HARRIS_SCORE, patch
 * size 31, FAST threshold 20.  One job is level 0 of one pyramid slot (w x h, u8) and a range of rect centres (the existing features,
 * the rect_xy input and rule of svslam_gftt_batch).  OpenCV is on neither machine, so parity with it is unpinned; the contract is this
 * text and tests/ref_orb.py, met bit for bit, every step integer, written-out f32, or f64 on the host:
 *   levels   scale_L = (float)pow((double)1.2f, L); inv_L = 1.f / scale_L; w_L = rint((float)w inv_L), h_L alike, half to even
 *   quotas   factor = (float)(1.0 / (double)1.2f); nd = nfeatures (1 - factor) / (1 - (float)pow(factor, nlevels)) in f32, left to
 *            right; n_L = rint(nd), nd *= factor for L < nlevels - 1; n_last = max(nfeatures - sum, 0)
 *   pyramid  level L from level L - 1 by the bit-exact bilinear resize.  Per axis s = 1.0 / ((double)dst / (double)src),
 *            f = s (d + 0.5) - 0.5 in double, i = floor(f); i < 0: sample 0 with weight 256; i >= src - 1: sample src - 1 with weight
 *            256; else c1 = rint((f - i) 256), c0 = 256 - c1 on samples i, i + 1.  Horizontal t = p[i] c0 + p[i + 1] c1 kept in full,
 *            vertical v = t0 c0 + t1 c1, out = (v + 32768) >> 16
 *   mask     level 0: 255, and 0 inside the inclusive square [rint(pt - 10), rint(pt + 10)] of every rect centre, clipped to the
 *            image; level L >= 1: the same resize of the level L - 1 mask, then <= 254 becomes 0
 *   FAST     9 of 16 on the radius-3 circle at 3 <= x < w_L - 3, 3 <= y < h_L - 3, strict compares against v +- fast_threshold;
 *            score = the largest threshold at which the pixel is still a corner (max over the 16 arcs and both polarities of the
 *            arc's minimum signed difference, minus 1), 0 for a non-corner; a corner survives iff its score is strictly greater than
 *            its 8 neighbours' scores
 *   filters  border: edge <= x < w_L - edge, edge <= y < h_L - edge; then mask: mask_L[y][x] != 0
 *   cut 1    m = 2 n_L; with more than m survivors all with score >= the m-th largest are kept, ties included; m == 0: none
 *   Harris   7 x 7 block; per block pixel in int32 Ix = (p[+1] - p[-1]) 2 + (p[-row+1] - p[-row-1]) + (p[+row+1] - p[+row-1]),
 *            Iy = (p[+row] - p[-row]) 2 + (p[+row-1] - p[-row-1]) + (p[+row+1] - p[-row+1]); a += Ix Ix, b += Iy Iy, c += Ix Iy;
 *            scale = 1.f / (4 * 7 * 255.f), s4 = scale scale scale scale; response = ((float)a (float)b - (float)c (float)c -
 *            0.04f ((float)a + (float)b) ((float)a + (float)b)) s4 in f32, left to right, no contraction
 *   cut 2    with more than n_L points left all with response >= the n_L-th largest are kept (float compare, ties included)
 *   angle    intensity centroid over the circular patch of half-size 15 (umax: csrc/k_orb.h), m10 = sum u I, m01 = sum v I in int32;
 *            angle = fastAtan2((float)m01, (float)m10) in degrees, [0, 360): ax = |x|, ay = |y|; ax >= ay: c = ay / (ax +
 *            (float)DBL_EPSILON), a = (((p7 c c + p5) c c + p3) c c + p1) c; else c = ax / (ay + (float)DBL_EPSILON), a = 90 - the
 *            same; x < 0: a = 180 - a; y < 0: a = 360 - a; p1, p3, p5, p7 = 0.9997878412794807f, -0.3258083974640975f,
 *            0.1555786518463281f, -0.04432655554792128f, each times (float)(180 / pi); IEEE f32 division, no FMA
 *   output   x = (float)xi scale_L, y = (float)yi scale_L, size = 31 scale_L, angle, response, octave = L
 * Order (a declared deviation: OpenCV's comes out of nth_element and is unspecified): level ascending, row-major in level coordinates
 * inside a level.  Duplicates across levels are kept, as there.  n_found is the count these rules give, n_out = min(n_found, max_out);
 * the first n_out rows in that order are written to out[job][0 .. n_out), the rows behind them are left as they were.
 * Errors, nothing written: nfeatures < 1 (after the default) or above 2^24; nlevels outside 1..8; fast_threshold outside 1..254;
 * edge < 16 (the orientation reads radius 15, Harris radius 4); max_out < 1; a slot out of range; a rect range that leaves the array;
 * no memory for the call's buffer (allocated inside the call on demand and kept; a large call is split into chunks under a byte
 * budget; svslam_limits has no say in it, njobs is not bounded by max_jobs).  Valid no-ops: njobs == 0, an image none of whose levels
 * has an interior (w_L <= 2 edge or h_L <= 2 edge).  A rect centre that is not a number masks nothing.  A job's result does not depend
 * on the other jobs of the call, and two calls on the same inputs give the same bits.
 * svslam_orb_read_level is a test hook: image and mask (tight, w_L x h_L; either pointer may be NULL) of a level of a job of the last
 * call, as long as the job was in the last chunk of that call. */
typedef struct svslam_orb_job { int slot; int rect_ofs, nrect; int n_out, n_found /* out */; int reserved; } svslam_orb_job;
typedef struct svslam_orb_params { int nfeatures; int nlevels; int fast_threshold; int edge; } svslam_orb_params;   /* 0 in a field: ORB's default (500, 8, 20, 31) */
typedef struct svslam_orb_kp { float x, y, size, angle, response; int octave; } svslam_orb_kp;
int svslam_orb_detect_batch(svslam_ctx *ctx, int njobs, svslam_orb_job *jobs, const svslam_orb_params *params,
                            int total_rects, const float *rect_xy, int max_out, svslam_orb_kp *out /* [njobs][max_out] */);
int svslam_orb_read_level(svslam_ctx *ctx, int job, int level, uint8_t *img, uint8_t *mask, int *w, int *h);

/* ---- ORB descriptors: rBRIEF at each keypoint's angle and octave ------------------------------------------------
 * What cv::ORB::compute does with the keypoints cv::ORB::detect returned (LoopClosure::ExtractKeypointsDescriptor,
 * src/loopclosure.cpp:131-171): a freshly detected feature is described on pyramid level `octave` with the test table turned by its own
 * angle, a tracked one (cv::KeyPoint(pt, 7)) at -1 degree on level 0.  One job is level 0 of one pyramid slot and a range of
 * svslam_orb_kp, the detector's output struct; size and response are ignored.  The contract, restated in tests/ref_orb_desc.py and met
 * bit for bit; every step is integer, a written-out f32 step, or f64 on the host.  Parity with OpenCV is unpinned.
 *   levels    scale_L, inv_L = 1.f / scale_L, w_L, h_L are those of svslam_orb_detect_batch; level L comes from level L - 1 by the same
 *             bit-exact bilinear resize (the same functions of csrc/k_orb.h); no mask.  Only levels 1 .. Lmax are built, Lmax the largest
 *             octave among the call's points: a call whose points are all octave 0 launches no resize and reserves no level storage
 *   filter    in this order: a point is kept iff edge <= x < w - edge and edge <= y < h - edge (float compares on level-0 coordinates,
 *             as in svslam_brief_describe_batch); then cx = rint(x inv_L), cy = rint(y inv_L), one f32 product each, rounded half to
 *             even (inv_0 is exactly 1); on a level L >= 1 kept iff edge <= cx < w_L - edge and edge <= cy < h_L - edge (on level 0
 *             the first test is the whole filter, as in svslam_brief_describe_batch: x = w - edge - 0.01 is kept and its centre is
 *             w - edge, which edge >= reach + 4 keeps inside the image).  Kept points keep their order:
 *             the kept rows of a job are the first n_desc rows of its range in desc and desc_pt, desc_pt[row] = the point's index
 *             inside the job, rows behind n_desc are left as they were
 *   rotation  per point, on the host: r = angle * (float)(pi / 180) in f32, a = (float)cos((double)r), b = (float)sin((double)r);
 *             on the device, for each of the 512 table points: ix = rint(px a - py b), iy = rint(px b + py a), each product and each
 *             sum rounded to f32 on its own (no contraction), the result rounded half to even.  cos and sin stay on the host because
 *             the device's and the C library's differ in the last bit
 *   reach     per call, from the table alone: the largest over the 512 table points of the smallest integer m with m^2 >= px^2 + py^2.
 *             It bounds every rotated offset at every angle; 19 for the default table
 *   blur, tests, packing   svslam_brief_describe_batch's: taps 18, 34, 49, 54, 49, 34, 18, (v + 32768) >> 16, strict <, byte t / 8,
 *             bit t % 8, on the level-`octave` image around (cx, cy)
 * params: pattern NULL = the default table of svslam_brief_default_pattern, edge 0 = 31, nlevels 0 = 8.
 * Errors, nothing written: a job's range that leaves the arrays, ranges that do not ascend or overlap, a slot out of range, npts > 1024,
 * a table entry whose two points coincide, edge < reach + 4, reach > 24, nlevels outside 1..8, an octave outside 0 .. nlevels - 1 or a
 * non-finite angle (any finite float is accepted) at a point of a job, no memory for the call's buffer (allocated inside the call on demand and kept; a large call is
 * split into chunks under a byte budget, njobs is not bounded by max_jobs).  Valid no-ops: njobs == 0, npts == 0.  A point whose level
 * has no interior is dropped; non-finite coordinates fail the filter.  A job's result does not depend on the other jobs of the call,
 * and two calls on the same inputs give the same bits.
 * Declared deviations: (a) OpenCV sorts provided keypoints by level, the input order is kept here (the reference re-associates by
 * position); (b) a centre that fails the level-L border test is dropped where OpenCV would read its 32-pixel reflected border: a
 * detector keypoint never fails it (x = xi scale_L and rint(x inv_L) == xi there), a tracked one is octave 0.
 * Property: with the default table and every point at angle -1, octave 0, the rows are those of
 * svslam_brief_describe_batch(angle_deg = -1) bit for bit. */
typedef struct svslam_orb_desc_job { int slot; int pt_ofs, npts; int n_desc /* out */; int reserved; } svslam_orb_desc_job;
typedef struct svslam_orb_desc_params { const int8_t *pattern; int edge; int nlevels; int reserved; } svslam_orb_desc_params;   /* NULL / 0: default table, 31, 8 */
int svslam_orb_describe_batch(svslam_ctx *ctx, int njobs, svslam_orb_desc_job *jobs, const svslam_orb_desc_params *params,
                              int total_pts, const svslam_orb_kp *kps, uint8_t *desc /* [total_pts][32] */, int *desc_pt /* [total_pts] */);

/* ---- loop candidate search: a resident store of global image descriptors and the two-threshold rule ----------
 * Replaces stage 1 of the reference's loop closure, LoopClosure::LoopKeyframeCandidate (src/loopclosure.cpp:227-284) with
 * SimilarityScore (:173-180) and the normalisation of :128.  The global descriptor itself (the reference's MobileNetV2 vector of 1280
 * floats) is an input, or svslam_gdesc_* below; any vector of dim floats, 1 <= dim <= 4096, serves.  The store lives in the context, on the device:
 * nstreams x capacity normalised rows with their keyframe ids, ascending per stream.  Its layout is opaque.
 * The contract, met bit for bit by the kernel, its host build and tests/ref_loop_candidates.py; no tolerance anywhere:
 *   similarity  of two f32 vectors: 64 accumulators start at +0; accumulator l takes the elements e = l, l + 64, l + 128, ... below
 *               dim in that order, each step acc = acc + (a[e] * b[e]) with the product rounded to f32 and then the sum (no FMA);
 *               then six halving steps s = 32, 16, 8, 4, 2, 1: acc[l] += acc[l + s] for l < s; the similarity is acc[0].
 *   normalise   n2 = similarity(a, a); v[e] = a[e] / sqrtf(n2), IEEE square root and division.  n2 zero or not finite (a zero vector,
 *               an infinity or NaN in it, an overflow or underflow of the sum) is BAD_VECTOR; the reference would store NaNs.
 *               Stored rows are normalised at the append, a query inside the search call.
 *   selection   over the stream's stored rows in ascending keyframe id: a row with kf_id - id < min_gap is skipped (the reference
 *               hard-codes 20); best = the largest similarity that is > 0, the lowest id on a tie; n_weak counts the compared rows
 *               with sim > weak, strictly, the best included; n_compared counts the compared rows.  Then, in this order:
 *               NONE           no compared row has sim > 0 (the reference would fetch keyframe 0 and insert a null there)
 *               BELOW_STRONG   best < strong
 *               TOO_MANY_WEAK  n_weak > max_num_weak
 *               FOUND          otherwise; cand_kf = the best's id.
 *               Every output is defined for every status: cand_kf is -1 unless FOUND; best_sim / best_kf are 0 / -1 for NONE and
 *               BAD_VECTOR and the best otherwise; BAD_VECTOR (the query) has n_weak = n_compared = 0.
 * Against the reference: Eigen's vectorised a.transpose() * b sums in another order, so a similarity can differ from the reference's
 * by rounding, within (ceil(dim / 64) + 7) 2^-24 sum |a b| of the exact dot product each (tests/test_ref_loop_candidates.py derives
 * the bound); a threshold decision that close to the threshold can come out differently.
 *
 * svslam_loopdb_configure  allocates (or re-allocates) the store and empties it.  Refused: nstreams < 1, capacity < 1, dim outside
 *                          1 .. 4096; no device memory, which leaves the old store as it was.
 * svslam_loopdb_append_batch  normalises n vectors (vecs [n][dim]) and appends row i to streams[i] under kf_ids[i]; a stream may come
 *                          more than once in a call.  Refused as a whole, nothing written: an unknown stream, a negative id, an id not
 *                          above the stream's last one, a full stream, a BAD_VECTOR.  n == 0 is a valid no-op.
 * svslam_loop_candidates_batch  one job per stream per call, streams strictly ascending; vecs [njobs][dim] are the raw queries.
 *                          Refused, nothing written: an unconfigured store, an unknown or repeated or descending stream, a kf_id not
 *                          above the stream's last stored id, min_gap < 0, max_num_weak < 0, a threshold that is not finite.
 *                          njobs == 0 is a valid no-op.  A BAD_VECTOR query is that job's status, not a refusal.  A job's result does
 *                          not depend on the other jobs of the call; two calls on the same inputs give the same bits.
 * svslam_loopdb_count      the rows a stream holds.
 * svslam_loopdb_read       the first min(count, max_rows) ids and normalised rows of a stream, rows in the vector's own order.
 * The reference's thresholds (tests/golden/config-00.yaml): weak 0.93, strong 0.95, max_num_weak 3; min_gap 20. */
enum { SVSLAM_LC_FOUND = 0, SVSLAM_LC_NONE = 1, SVSLAM_LC_BELOW_STRONG = 2, SVSLAM_LC_TOO_MANY_WEAK = 3, SVSLAM_LC_BAD_VECTOR = 4 };
typedef struct svslam_lc_job {
    int stream, kf_id;                                        /* in */
    int status, cand_kf, best_kf, n_weak, n_compared;         /* out */
    float best_sim;                                           /* out */
} svslam_lc_job;
typedef struct svslam_lc_params { float weak, strong; int max_num_weak, min_gap; } svslam_lc_params;
int svslam_loopdb_configure(svslam_ctx *ctx, int nstreams, int capacity, int dim);
int svslam_loopdb_append_batch(svslam_ctx *ctx, int n, const int *streams, const int *kf_ids, const float *vecs /* [n][dim] */);
int svslam_loop_candidates_batch(svslam_ctx *ctx, int njobs, svslam_lc_job *jobs, const svslam_lc_params *params,
                                 const float *vecs /* [njobs][dim] */);
int svslam_loopdb_count(svslam_ctx *ctx, int stream, int *count);
int svslam_loopdb_read(svslam_ctx *ctx, int stream, int max_rows, int *kf_ids, float *vecs /* [max_rows][dim] */);

/* ---- global image descriptor: a small convolutional network on a keyframe image ----------
 * Replaces LoopClosure::ExtractFeatureVec (src/loopclosure.cpp:92-129): GaussianBlur(7 x 7), resize, blobFromImage and MobileNetV2 up to
 * the global average pool.  The network is a table of layers; its WEIGHTS are an input (the reference's ONNX file is not part of this
 * project; gdesc.py folds a torchvision state dict into params), the forward pass is this library's.  One job is level 0 of one
 * pyramid slot, exactly what svslam_brief_describe_batch reads.  The contract (csrc/k_global_desc.h), met bit for bit by
 * the kernels and their host build; every f32 output element is one chain in a fixed order, no split-K, no reassociation:
 *   prep     blur: separable integer taps (8, 28, 56, 72, 56, 28, 8) / 256 (OpenCV's table for ksize 7, sigma 0), the horizontal sum
 *            kept in full, the vertical sum over it, out = (v + 32768) >> 16, BORDER_REFLECT_101.
 *            resize to out_w x out_h: per axis scale = (double)src / dst, f = (float)((d + 0.5) scale - 0.5), s = floor(f), f -= s;
 *            s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; the second tap is min(s + 1, src - 1);
 *            c1 = rint(f 2048), c0 = rint((1 - f) 2048) (half to even); S = p[s] c0 + p[s + 1] c1 along x;
 *            out = (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2 along y.  Parity with OpenCV is not pinned.
 *            blob: x[c] = ((float)pix - mean[c]) * scale, c = 0, 1, 2, planar.  The defaults (prep == NULL) are the reference's call:
 *            224 x 224, mean (0.485, 0.456, 0.406), scale 1 / 255.
 *   CONV3    dense 3 x 3, pad 1, stride 1 or 2; weights [cout][cin][3][3]; acc = bias[co], acc = fmaf(w, x, acc) over (ci, ky, kx)
 *            row-major; a tap in the padding takes x = +0.0f and is part of the chain
 *   DW3      depthwise 3 x 3, pad 1, stride 1 or 2, cin == cout; weights [c][3][3]; acc = bias[c], the 9 taps in (ky, kx) order
 *   PW       1 x 1; weights [cout][cin]; acc = bias[co], acc = fmaf(w[co][ci], x[ci], acc), ci ascending
 *   AVGPOOL  global, the last layer: s = +0, s = s + x over the pixels in row-major order, s / (float)(H W)
 *   epilogue add_from >= 0 (PW with relu6 == 0 only; an earlier layer of the same C x H x W): one f32 add of that layer's output;
 *            then, if relu6, v = v > 0 ? v : +0 and v = v < 6 ? v : 6.  A 3 x 3 layer's output size is (n + 2 - 3) / stride + 1.
 * params holds, per layer in table order, the weights in the orders above followed by bias[cout]; AVGPOOL has none.
 * svslam_gdesc_configure   Refused, nothing changed and the old network kept: a table that does not chain (cin != the previous cout,
 *                          the first cin != 3), DW3 with cin != cout, a stride outside {1, 2}, a bad add_from, AVGPOOL missing or
 *                          not last, a final dim outside 1 .. 4096, nparams not the table's total, a weight / mean / scale that is
 *                          not finite, out_w or out_h < 1, no device memory.  workspace_bytes caps the activations of a chunk of
 *                          jobs (0: 256 MiB); a cap below one job's share still runs one job at a time.
 * svslam_gdesc_dim         cout of the last layer, 0 while no network is configured.
 * svslam_gdesc_describe_batch  vecs [njobs][dim], raw (the loop store normalises at its append and in its search).  Refused, vecs
 *                          untouched: no network, a slot out of range, an image below 4 x 4.  njobs == 0 is a valid no-op.  A job's
 *                          result does not depend on the chunk size or on the other jobs; two calls give the same bits.
 * svslam_gdesc_mobilenet_v2    the default table, 52 convolutions + the pool = 53 entries; returns the count, writes min(count, cap). */
enum { SVSLAM_GD_CONV3 = 0, SVSLAM_GD_DW3 = 1, SVSLAM_GD_PW = 2, SVSLAM_GD_AVGPOOL = 3 };
typedef struct svslam_gd_layer { int op, cin, cout, stride, relu6, add_from; } svslam_gd_layer;
typedef struct svslam_gd_prep { int out_w, out_h; float mean[3]; float scale; long long workspace_bytes; } svslam_gd_prep;
int svslam_gdesc_configure(svslam_ctx *ctx, int nlayers, const svslam_gd_layer *layers, const float *params, long long nparams,
                           const svslam_gd_prep *prep);
int svslam_gdesc_dim(svslam_ctx *ctx);
int svslam_gdesc_describe_batch(svslam_ctx *ctx, int njobs, const int *slots, float *vecs /* [njobs][dim] */);
int svslam_gdesc_mobilenet_v2(svslam_gd_layer *out, int cap);

/* ---- shared-map bundle adjustment (BASELINE config 5; not in the reference) -----------
 * ONE local-BA problem whose landmarks are sharded over the GPUs of a node: every rank holds all
 * nkf poses and its landmarks with their edges.  The rank opens its shard, then runs the pieces of
 * an LM trial; the host sums what the pieces hand out over the ranks (one RCCL all-reduce of
 * (6 nkf)^2 + 2 (6 nkf) + 1 doubles per trial — 3 781 at nkf = 10) and feeds the reduced camera
 * system back.  The LM control flow (g2o's, exactly as in svslam_local_ba_batch) lives in the
 * caller: stereovision-slam_amd/shared_ba.py.  io layout (svslam_sba_io_doubles(nkf) doubles):
 *   S[np*np] | bs[np] | bp[np] | diag(Hpp)[np] | scalars[8],  np = 6 nkf
 *   scalars: 0 chi2, 1 largest landmark diagonal, 2 Cholesky ok, 3 rho denominator (landmarks),
 *            4 rho denominator (poses, identical on every rank), 5 chi2 of the trial state
 * phase 1: diag(Hpp) and scalar 1 out.  phase 2 (lambda): S (without lambda I), bs, bp, scalar 0 out.
 * phase 3 (lambda): reduced S (with lambda I), bs, bp in; scalars 2-5 out; state updated.
 * phase 4: reject the trial (restore).  phase 5: finalise (per-edge chi2).                     */
int svslam_sba_io_doubles(int nkf);
int svslam_sba_open(svslam_ctx *ctx, const double cam_l[4], const double ext_l[7],
                    const double cam_r[4], const double ext_r[7], int nkf, const double *poses,
                    int nlm, const double *pts, int nobs, const int *obs_kf, const int *obs_lm,
                    const uint8_t *obs_is_right, const float *obs_uv, double huber_delta);
int svslam_sba_phase(svslam_ctx *ctx, int phase, double lambda, double *io);
int svslam_sba_close(svslam_ctx *ctx, double *poses, double *pts, double *edge_chi2);
/* The same optimisation as ONE call: the LM control flow runs inside the library, the reduced camera system is
 * all-reduced in place on the device buffer with RCCL (ncclAllReduce on the context's stream; librccl.so is bound
 * with dlopen at the first svslam_sba_comm_* call, nothing links it otherwise), two launches and one 64-byte
 * read-back per LM trial.  Communicator: rank 0 creates the 128-byte id, every rank receives it over any channel
 * and calls svslam_sba_comm_init; without a communicator svslam_sba_solve runs the single-rank problem.
 * trace (optional): 6 doubles per LM trial as svslam_lm_trace.  stats (optional, 4 doubles): trials, total ms,
 * ms per trial, bytes all-reduced per trial.                                                                 */
int svslam_device_count(void);      /* HIP devices visible to this process */
int svslam_sba_comm_unique_id(char out128[128]);
int svslam_sba_comm_init(svslam_ctx *ctx, int nranks, int rank, const char id128[128]);
int svslam_sba_comm_destroy(svslam_ctx *ctx);
int svslam_sba_solve(svslam_ctx *ctx, int iters, int *iters_done, double *lambda_out, double *trace, int trace_cap,
                     int *n_trace, double *stats);

/* test hook: accumulated per-phase ticks (wall_clock64, 100 MHz) of BA job 0;
 * out12[11] = LM trials.  enable=1 allocates the counters, out12 != NULL reads
 * and clears them.                                                            */
int svslam_ba_profile(svslam_ctx *ctx, int enable, long long *out12);

/* test hook: the Levenberg-Marquardt trajectory of the last svslam_pose_only_batch / svslam_local_ba_batch / svslam_pose_graph_batch call
 * on this context — one record of 6 doubles per LM trial, rejected trials included: iteration (pose-only:
 * 16 round + iteration), lambda of the trial, chi2 before, chi2 of the trial state, rho, accepted.  enable = 1
 * allocates the device buffer (kernels record while it exists), 0 frees it; out != NULL reads job `job`.    */
int svslam_lm_trace(svslam_ctx *ctx, int enable, int job, double *out, int cap_records, int *n_records);

/* ---- fused per-frame tracking (pyramid + LK + pose-only, one submission) --
 * The whole data-parallel part of Frontend::Track (src/frontend.cpp:645-663)
 * without a host round trip between TrackLastFrame and EstimateCurrentPose:
 * points that fail LK / leave the image are dropped on the device, the rest
 * that carry a map point (has_mp) become pose-only edges.                    */
typedef struct svslam_track_job {
    int    prev_slot, next_slot;
    int    pt_ofs, npts;
    double pose[7];     /* in: prior; out: refined                           */
    int    n_tracked;   /* out: status && in image                           */
    int    n_inlier;    /* out                                                */
} svslam_track_job;

int svslam_track_batch(svslam_ctx *ctx, int njobs, svslam_track_job *jobs,
                       const void *const *next_imgs, const int *strides,
                       int src_is_device, int total_pts, const double cam[4],
                       const float *prev_xy, float *next_xy,
                       const uint8_t *has_mp, const double *xyz,
                       uint8_t *status, uint8_t *outlier,
                       const svslam_lk_params *p, double chi2_th);

/* ---- the same with the features of the last frame resident in HBM ------------
 * svslam_track_batch makes the caller gather (position, map point, start guess) of
 * every feature of the last frame and scatter the survivors into the new frame
 * (src/frontend.cpp:331-347, :361-381, :546-553) — per-feature host work on every
 * frame.  Here the feature list of every stream's last frame lives in HBM: the call
 * reads it, tracks, optimises the pose and leaves the survivors (outlier edges
 * stripped of their map point) as the new list.  The caller only supplies the
 * predicted pose and gets counts back; the compacted survivors (xy, map point id) are
 * also returned for the frames the caller turns into keyframes.  After a keyframe has
 * added features / map points or the backend has moved them, the caller replaces the
 * stream's list with svslam_rtrack_upload.                                        */
typedef struct svslam_rtrack_job {
    int    stream;       /* resident slot, 0 .. max_streams-1                     */
    int    prev_slot, next_slot;
    int    pt_ofs, npts; /* npts = features of the last frame (the caller's count); pt_ofs:
                            where this job's survivors start in out_xy / out_mp   */
    double pose[7];      /* in: predicted T_cw; out: refined                      */
    double T_cam_w[7];   /* in: cam_left.pose * predicted T_cw (src/camera.cpp:74) */
    int    n_tracked;    /* out: survivors = features of the new frame            */
    int    n_edges;      /* out: survivors that carry a map point                 */
    int    n_outlier;    /* out: of those, classified outlier by the pose solve   */
    int    reserved;
} svslam_rtrack_job;

int svslam_rtrack_batch(svslam_ctx *ctx, int njobs, svslam_rtrack_job *jobs,
                        const void *const *next_imgs, const int *strides,
                        int src_is_device, int total_pts, const double cam[4],
                        float *out_xy, int *out_mp,
                        const svslam_lk_params *p, double chi2_th);
/* replaces the resident feature lists of n streams: stream i has counts[i] features at
 * xy/mp/xyz + ofs[i] (xyz is read only where mp >= 0)                               */
int svslam_rtrack_upload(svslam_ctx *ctx, int n, const int *streams, const int *ofs,
                         const int *counts, const float *xy, const int *mp,
                         const double *xyz);

/* ---- the map resident in HBM: the keyframe path without per-feature host work ------------------
 * With limits.device_map = 1 every resident stream (svslam_rtrack_*) also keeps its keyframe window, the features
 * of those keyframes, its landmarks and their observation counts on the device.  One call then runs everything
 * the reference does when a frame becomes a keyframe — Map::InsertKeyFrame / RemoveOldKeyframe / CleanMap
 * (src/map.cpp:53-181), SetObservationsForKeyFrame, DetectFeatures, FindFeaturesInRight, TriangulateNewPoints
 * (src/frontend.cpp:36-141, 251-320, 560-616; StereoInit / BuildInitMap :143-249 with is_init), Backend::Optimize
 * with its outlier handling and write-back (src/backend.cpp:22-246) — and leaves the keyframe's features as the
 * list the next frame tracks from.  The host supplies what is O(window): ids, the slot of the new keyframe and
 * the slot of the keyframe to retire (-1: none; the se3-log distance rule of RemoveOldKeyframe stays on the host),
 * and reads counts and the window's poses back.  mp values in the resident lists are landmark SLOTS here.       */
typedef struct svslam_dmap_job {
    int    stream, slot_cur, slot_right, is_init;  /* is_init: 0 keyframe of a tracked frame, 1 StereoInit, 2 no keyframe at all —
                                                      one local BA over the stream's window as it is (Backend::UpdateMap called from
                                                      outside the frontend, include/StereoVisionSLAM/backend.h:30): only stream, npts and
                                                      the BA outputs are used; such jobs do not share a call with keyframe jobs */
    int    kf_slot, remove_slot, kf_id, npts;   /* npts: features the frame has (tracked survivors); 0 at init   */
    long long frame_id;
    double pose[7];        /* in: T_cw (identity at init); out: after the local BA                              */
    double T_camr_w[7];    /* cam_right.pose * T_cw (src/camera.cpp:74)                                          */
    double T_wc[7];        /* inverse of pose (identity at init)                                                 */
    int    src_buf, dst_buf; /* filled by the library                                                            */
    int    stamp, corners_dropped; /* stamp: filled by the library; corners_dropped: out, surplus corners not appended (max_pts) */
    /* out */
    int    ok;             /* init: enough stereo matches (otherwise nothing was created); keyframe: 1           */
    int    n_features, n_corners, n_right_ok, n_tri_in, n_tri_ok;
    int    ba_nkf, ba_nlm, ba_nobs, ba_iters;
    int    flags;          /* 1 corners dropped (max_pts), 2 landmark slots exhausted, 4 BA skipped (max_obs)    */
    int    dead;
    int    ba_npair, ba_ntrial; /* accounting: (pose, landmark) block pairs of the Schur complement, LM trials (accepted + rejected) */
    int    ev_ofs, ev_n;   /* the landmarks this job freed: records [ev_ofs, ev_ofs + ev_n) of svslam_dmap_evicted()    */
    double win_pose[12][7];/* poses of the BA problem's keyframes after the solve ...                            */
    int    win_slot[12];   /* ... and their slots                                                                */
} svslam_dmap_job;

typedef struct svslam_dmap_params {
    int    num_features, num_features_init, num_active_keyframes, ba_iters;
    double max_triangulation_depth, chi2_th;
    int    ba_defer;       /* 1: the local BA of this call runs BESIDE what follows, on a second stream of the context (the
                              reference's backend thread, src/backend.cpp:250-287): the call returns once the keyframe is in
                              the map and its problem gathered; svslam_dmap_ba_collect applies the result — window poses,
                              landmark positions, outlier observations — later.  One deferred batch at a time. */
    int    reserved;
} svslam_dmap_params;
/* Applies the local BA a svslam_dmap_keyframe_batch call with ba_defer = 1 left running: waits for it, writes poses /
 * positions back into the device map, removes the outlier observations (src/backend.cpp:167-246) and refreshes the positions
 * in every job's resident feature list.  jobs_out (njobs as in that call, same order) receives the jobs with their BA
 * outputs (ba_*, win_pose / win_slot, pose).  Returns 0 and touches nothing when no batch is in flight (*njobs_inflight = 0). */
int svslam_dmap_ba_collect(svslam_ctx *ctx, int njobs, svslam_dmap_job *jobs_out, int *njobs_inflight);

int svslam_dmap_keyframe_batch(svslam_ctx *ctx, int njobs, svslam_dmap_job *jobs,
                               const void *const *left_imgs, const void *const *right_imgs, const int *strides,
                               int src_is_device, const double cam_l[4], const double ext_l[7],
                               const double cam_r[4], const double ext_r[7], const svslam_dmap_params *p);
/* The landmarks the LAST svslam_dmap_keyframe_batch freed from the device map (no observation left, outside the window,
 * not carried by tracking): id and last position.  Map::landmarks_ of the reference keeps every landmark for
 * saveSLAMOutputInFile (src/map.cpp:39-51, src/visual_odometry.cpp:226-304); a caller that writes landmarks.pcd archives
 * these.  *recs points into the context (valid until the next batch call); a job's records are unordered.             */
typedef struct svslam_dmap_evicted_rec { int id; float pos[3]; } svslam_dmap_evicted_rec;
int svslam_dmap_evicted(svslam_ctx *ctx, const svslam_dmap_evicted_rec **recs, int *n);
/* test / writer hook: one stream's window (max_kf entries; kf_frame < 0 = empty slot) and landmark arena
 * (max_lm entries; lm_id < 0 = free slot; lm_state 1 = active, 2 = outside the window)                           */
int svslam_dmap_read(svslam_ctx *ctx, int stream, long long *kf_frame, int *kf_id, double *kf_pose, int *kf_n,
                     int *lm_id, double *lm_pos, int *lm_obs, uint8_t *lm_state);

/* ---- test hooks: the kernels of the device map one at a time, on maps the test chose (tests/test_gpu_dmap_kernels.py) ----
 * Video drives the map only where natural runs go.  These hooks put one stream's map into any state and run ONE kernel of
 * the keyframe path on it, launched by the very lines svslam_dmap_keyframe_batch launches it with.  Nothing here is meant
 * for a caller that is not a test.
 *
 * One stream's whole map.  Per array: kf_* [max_kf], kf_pose [max_kf][7], f_* [max_kf][max_pts] (f_xy / f_xyr two floats per
 * feature; f_lm / f_lmr the landmark SLOT the left / right feature observes, -1 none; f_fl bit 0: right feature found),
 * lm_* [max_lm] (lm_pos [max_lm][3]; lm_stamp: last keyframe step whose tracked list named the landmark), next_lm_id [1].
 * A null member is skipped.  The write refuses kf_n outside [0, max_pts] and slots outside [-1, max_lm): the kernels index
 * with them.                                                                                                            */
typedef struct svslam_dmap_state {
    long long *kf_frame; int *kf_id; double *kf_pose; int *kf_n;
    float *f_xy, *f_xyr; int *f_lm, *f_lmr; uint8_t *f_fl;
    double *lm_pos; int *lm_id, *lm_obs; uint8_t *lm_state; int *lm_stamp, *next_lm_id;
} svslam_dmap_state;
int svslam_debug_dmap_write(svslam_ctx *ctx, int stream, const svslam_dmap_state *arrays);
int svslam_debug_dmap_read(svslam_ctx *ctx, int stream, svslam_dmap_state *arrays);
/* test hook: the resident feature list of `stream` as the next call would read it, max_pts entries each (null: skipped)  */
int svslam_debug_rtrack_read(svslam_ctx *ctx, int stream, float *xy, int *mp, double *xyz);

#define SVSLAM_DMAP_STAGE_BEGIN         0  /* k_dmap_begin:         in ev_quota; in/out evicted [njobs * ev_quota], ev_cursor [1]; the
                                              resident lists (svslam_rtrack_upload) are the tracked survivors                       */
#define SVSLAM_DMAP_STAGE_STEREO_PREP   1  /* k_dmap_stereo_prep:   in corners [njobs][max_corners][2], ncorners [njobs], cam_r;
                                              out lkjobs [njobs], prev_xy / next_xy [njobs][max_pts][2]                            */
#define SVSLAM_DMAP_STAGE_STEREO_FINISH 2  /* k_dmap_stereo_finish: in next_xy, status [njobs][max_pts], num_features_init, zmax;
                                              out trijobs [njobs], uv_l / uv_r [njobs][max_pts][2], tri_idx [njobs][max_pts]      */
#define SVSLAM_DMAP_STAGE_COMMIT        3  /* k_dmap_commit:        in tri_xyz [njobs][max_pts][3], tri_ok, tri_idx [njobs][max_pts];
                                              the jobs' n_tri_in, dead                                                              */
#define SVSLAM_DMAP_STAGE_BA_GATHER     4  /* k_dmap_ba_gather<threads>: in threads (512 | 1024), max_kf (<= 12), max_obs — the strides
                                              of: out badev [njobs][SVSLAM_DMAP_BADEV_INTS], poses [njobs][max_kf][7], pts [njobs]
                                              [max_lm][3], packed / edge_ref [njobs][max_obs], uv [njobs][max_obs][2], lm_slot_of
                                              [njobs][max_lm]; the jobs' flags, ba_*, win_slot                                      */
#define SVSLAM_DMAP_STAGE_BA_SCATTER    5  /* k_dmap_ba_scatter:    in badev (nkf, nlm, nobs, iters_done, ...), poses, pts, chi2
                                              [njobs][max_obs], edge_ref, lm_slot_of, max_kf, max_obs, chi2_th; the jobs' win_slot  */
#define SVSLAM_DMAP_STAGE_REFRESH       6  /* k_dmap_refresh:       the jobs' kf_slot, n_features; read back: svslam_debug_rtrack_read */
#define SVSLAM_DMAP_STAGE_REFRESH_XYZ   7  /* k_dmap_refresh_xyz:   the jobs' stream, npts                                         */
/* the gather's problem descriptor, one int each: kf_ofs, nkf, lm_ofs, nlm, obs_ofs, nobs, nblk, na, ncontrib, ntile, aux_ofs,
 * iters_done, rec_ofs, lay_nblk, lay_na, lay_ntile, nmv, reserved, lm_base, shmask, ntrial                               */
#define SVSLAM_DMAP_BADEV_INTS 21
/* Every array a stage names is copied to the device before the launch and back after it, whole, so a test that fills an
 * output with a pattern sees what the kernel did NOT write as well.  Arrays of other stages may be null.                  */
typedef struct svslam_dmap_stage_io {
    int    threads, max_kf, max_obs, ev_quota, max_corners, num_features_init;
    double zmax, chi2_th, cam_r[4];
    svslam_dmap_evicted_rec *evicted; int *ev_cursor;
    const float *corners; const int *ncorners;
    svslam_lk_job *lkjobs; float *prev_xy, *next_xy;
    const uint8_t *status; svslam_tri_job *trijobs; float *uv_l, *uv_r; int *tri_idx;
    const double *tri_xyz; const uint8_t *tri_ok;
    int *badev; double *poses, *pts; unsigned int *packed; float *uv; int *edge_ref, *lm_slot_of;
    const double *chi2;
} svslam_dmap_stage_io;
/* Runs stage `stage` for `njobs` jobs on distinct streams.  jobs goes to the device as the caller filled it (src_buf / dst_buf
 * are set to the stream's current resident buffer, as the keyframe call sets them; the stamp is the caller's) and comes back
 * as the kernel left it.  Indices a kernel would use unchecked (slots, counts, edge references) are validated first.       */
int svslam_debug_dmap_stage(svslam_ctx *ctx, int stage, int njobs, svslam_dmap_job *jobs, const svslam_dmap_stage_io *io);

/* host threads the library may use to prepare a batched call (per-problem BA structure
 * building); default 1.                                                        */
int svslam_set_host_threads(svslam_ctx *ctx, int n);
/* test hooks */
int svslam_debug_host_ns(svslam_ctx *ctx, long long *out8);
/* test hook: shard descriptors of the last low-latency local-BA call, 8 ints per shard (landmarks, edges, blocks, tiles,
 * solver: 2 = resident kernel / 1 = streaming kernel, active poses, mask of shards with edges, iterations) for `nproblems` problems */
int svslam_debug_ll_shards(svslam_ctx *ctx, int nproblems, int *out8, int *shards_per_problem);
/* test hook: the low-latency solver's residency guard (svslam_set_low_latency): shards per problem (0 = batch solver only),
 * problems one call may hand to it, CUs counted, co-resident solver workgroups per CU                                      */
int svslam_debug_ll_limits(svslam_ctx *ctx, int *out4);
/* test hook: the descriptors of the last svslam_local_ba_batch / svslam_local_ba_collect as the solver returned them, 8 ints per
 * problem: blocks, active poses, block pairs, LDS tiles, landmarks that go through the tiles, iterations, LM trials, flags
 * (bit 0: the edges arrived landmark-major with keyframes ascending, bit 1: the device build read them through its LDS edge
 * cache — the argument its last launch was given, bit 2: the structure was built on the host, SVSLAM_BA_HOST_BUILD).  `njobs`
 * must be that call's problem count.  Meant for calls the batch solver took: after a low-latency call the problems' own
 * descriptors carry no block, tile or pose counts (svslam_debug_ll_shards has the shards').                               */
int svslam_debug_ba_struct(svslam_ctx *ctx, int njobs, int *out8);
int svslam_debug_clock_mhz(svslam_ctx *ctx, int blocks, double ms, double *mhz);
/* test hook: `ncus` workgroups that each take one CU's whole LDS and spin for `ms` milliseconds, enqueued on the context's stream
 * (asynchronous; svslam_sync waits): those CUs cannot take a workgroup that needs LDS meanwhile.  What it shows
 * (tests/test_gpu_low_latency_pipeline.py): a launch of ANOTHER context whose workgroups do not all find a CU cannot
 * retire before the holders leave, whichever solver it uses — the give-up of the low-latency BA (SVSLAM_LL_TIMEOUT_US) bounds the
 * wait of partly resident problems on EACH OTHER, not the wait for foreign kernels                                             */
int svslam_debug_hold_cus(svslam_ctx *ctx, int ncus, double ms);

/* ---- device memory helpers for HBM-resident inputs (bench, pipelining) --- */
int svslam_dev_alloc(svslam_ctx *ctx, size_t bytes, void **out);
int svslam_dev_free(svslam_ctx *ctx, void *p);
int svslam_dev_upload(svslam_ctx *ctx, void *dst, const void *src, size_t bytes);
int svslam_dev_download(svslam_ctx *ctx, void *dst, const void *src, size_t bytes);
int svslam_sync(svslam_ctx *ctx);

/* ---- kernel timing (HIP events on the context's stream) -------------------
 * Accumulated per kernel family since the last reset; used by bench.py for
 * the roofline entry.  family: 0 pyramid, 1 lk, 2 gftt, 3 triangulate,
 * 4 pose_only, 5 local_ba, 6 stereo_bm (units = jobs), 12 cloud_filter (units = points; appended
 * after the last number in use, nothing moved), 13 pose_graph (units = jobs; appended after 12, nothing moved),
 * 14 loop_verify (units = jobs; appended after 13, nothing moved), 15 brief (units = points; appended after 14, nothing moved),
 * 16 loop_candidates (units = rows compared, summed over the jobs; appended after 15, nothing moved),
 * 17 global_desc (units = jobs; appended after 16, nothing moved),
 * 18 colour (the conversion kernel of svslam_pyramid_bgr_batch; units = images; appended after 17, nothing moved),
 * 19 local_fusion (units = jobs; appended after 18, nothing moved),
 * 20 orb (svslam_orb_detect_batch; units = jobs; appended after 19, nothing moved),
 * 21 orb_desc (svslam_orb_describe_batch; units = points; appended after 20, nothing moved).
 * Development families follow and are NOT stable numbers: with stereo_bm taking 6, the
 * per-kernel split moved from 6-9 to 7-10 and the local-BA solver interval from 10 to 11.
 * A caller that passed those raw numbers must move with them (Python addresses them by name). */
int svslam_timing_enable(svslam_ctx *ctx, int on);
int svslam_timing_reset(svslam_ctx *ctx);
int svslam_timing_get(svslam_ctx *ctx, int family, double *total_ms,
                      long long *launches, long long *units);

#ifdef __cplusplus
}
#endif
#endif /* SVSLAM_H */
