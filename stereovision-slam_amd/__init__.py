"""stereovision-slam_amd — MI355X-native hot path of StereoVision-SLAM.

Thin ctypes binding over the C ABI of lib/libsvslam_hip.so (include/svslam.h).
There is no CPU fallback: importing works anywhere (so the build can be checked
without a GPU), but creating a Context without a usable HIP device raises.
The package directory name contains a hyphen; load it with
``importlib.import_module("stereovision-slam_amd")``.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")

ABI_SYMBOLS = [
    "svslam_create", "svslam_destroy", "svslam_last_error", "svslam_build_info",
    "svslam_pyramid_batch", "svslam_pyramid_decimate_batch", "svslam_set_source_size", "svslam_set_low_latency", "svslam_set_pose_only_xtol", "svslam_get_pose_only_xtol", "svslam_pyramid_read",
    "svslam_pyramid_read_padded", "svslam_stereo_bm_batch", "svslam_stereo_bm_strip_rows", "svslam_dense_cloud_batch", "svslam_cloud_sor_batch", "svslam_cloud_voxel_grid", "svslam_debug_cloud_sor_climbs",
    "svslam_colour_reserve", "svslam_pyramid_bgr_batch", "svslam_colour_read", "svslam_dense_cloud_bgr_batch", "svslam_lk_batch", "svslam_gftt_batch", "svslam_gftt_eigmap", "svslam_triangulate_batch",
    "svslam_pose_only_batch", "svslam_local_ba_batch", "svslam_local_ba_submit", "svslam_local_ba_collect", "svslam_pose_graph_batch", "svslam_local_fusion_batch", "svslam_loop_verify_batch", "svslam_brief_describe_batch", "svslam_brief_default_pattern",
    "svslam_orb_detect_batch", "svslam_orb_read_level", "svslam_orb_describe_batch",
    "svslam_loopdb_configure", "svslam_loopdb_append_batch", "svslam_loop_candidates_batch", "svslam_loopdb_count", "svslam_loopdb_read",
    "svslam_gdesc_configure", "svslam_gdesc_dim", "svslam_gdesc_describe_batch", "svslam_gdesc_mobilenet_v2",
    "svslam_track_batch", "svslam_rtrack_batch", "svslam_rtrack_upload",
    "svslam_sba_io_doubles", "svslam_sba_open", "svslam_sba_phase", "svslam_sba_close",
    "svslam_device_count", "svslam_dmap_keyframe_batch", "svslam_dmap_ba_collect", "svslam_dmap_read", "svslam_dmap_evicted", "svslam_sba_comm_unique_id", "svslam_sba_comm_init", "svslam_sba_comm_destroy", "svslam_sba_solve",
    "svslam_dev_alloc", "svslam_dev_free", "svslam_dev_upload", "svslam_dev_download", "svslam_sync",
    "svslam_timing_enable", "svslam_timing_reset", "svslam_timing_get", "svslam_ba_profile",
    "svslam_set_host_threads", "svslam_debug_host_ns", "svslam_debug_ll_shards", "svslam_debug_ll_limits", "svslam_debug_ba_struct", "svslam_debug_clock_mhz", "svslam_debug_hold_cus", "svslam_lm_trace",
    "svslam_debug_dmap_write", "svslam_debug_dmap_read", "svslam_debug_rtrack_read", "svslam_debug_dmap_stage",
]

FAMILIES = {"pyramid": 0, "lk": 1, "gftt": 2, "triangulate": 3, "pose_only": 4, "local_ba": 5}
DENSE_FAMILIES = {"stereo_bm": 6}      # the dense-reconstruction program's kernels: not part of the per-frame loop bench.py sums over FAMILIES
DEBUG_FAMILIES = {"dbg0": 7, "dbg1": 8, "dbg2": 9, "dbg3": 10}     # per-kernel split (SVSLAM_TIMING_SPLIT=1), development
# intervals nested inside a family: the local-BA solver kernel alone (k_local_ba_t<0, 1, EID>, or the low-latency solver's kernels)
# inside "local_ba" (= map gather + structure build + solver + scatter)
KERNEL_FAMILIES = {"ba_solve": 11}
CLOUD_FAMILIES = {"cloud_filter": 12}      # the outlier removal and the voxel grid of the dense program (units = points); appended, nothing renumbered
# svslam_pose_graph_batch, svslam_loop_verify_batch (units = jobs), svslam_brief_describe_batch (units = points); appended after 12,
# 13 and 14, nothing renumbered; svslam_loop_candidates_batch (units = rows compared) appended after 15
# svslam_gdesc_describe_batch (units = jobs) appended after 16; svslam_local_fusion_batch (units = jobs) appended after 18 (colour)
LOOP_FAMILIES = {"pose_graph": 13, "loop_verify": 14, "brief": 15, "loop_candidates": 16, "global_desc": 17, "local_fusion": 19}
# svslam_pyramid_bgr_batch's conversion kernel (units = images), appended after 17; a dictionary of its own: the dense program's, not the per-frame loop's
COLOUR_FAMILIES = {"colour": 18}
# svslam_orb_detect_batch (units = jobs), appended after 19; a dictionary of its own: bench.py's sums over FAMILIES see nothing new
ORB_FAMILIES = {"orb": 20}
# svslam_orb_describe_batch (units = points), appended after 20
ORB_DESC_FAMILIES = {"orb_desc": 21}
# the HIP kernel(s) behind each timing family at the batch operating point (what a rocprofv3 --kernel-trace --stats row is named)
FAMILY_KERNELS = {"pyramid": ["k_pyr_fused"], "lk": ["k_lk"], "gftt": ["k_gftt_eig3", "k_gftt_select2"], "triangulate": ["k_triangulate"],
                  "pose_only": ["k_pose_only"], "local_ba": ["k_dmap_ba_gather", "k_ba_build", "k_local_ba_t", "k_dmap_ba_scatter"],
                  "ba_solve": ["k_local_ba_t"], "stereo_bm": ["k_bm_fill", "k_stereo_bm", "k_dense_cloud"],
                  "cloud_filter": ["k_cf_keys", "k_cf_gather", "k_cf_knn", "k_vg_keys", "k_vg_heads", "k_vg_starts", "k_vg_reduce"],
                  "pose_graph": ["k_pose_graph"], "local_fusion": ["k_local_fusion"], "loop_verify": ["k_loop_verify"], "brief": ["k_brief_filter", "k_brief_describe"],
                  "loop_candidates": ["k_lc_candidates"],
                  "colour": ["k_bgr_prepare"],
                  "orb_desc": ["k_orbd_resize", "k_orbd_filter", "k_orbd_describe"],
                  "orb": ["k_orb_fill", "k_orb_rects", "k_orb_resize", "k_orb_fast", "k_orb_select", "k_orb_emit"],
                  "global_desc": ["k_gd_prep", "k_gd_conv3", "k_gd_dw3", "k_gd_pw_mfma", "k_gd_pool"]}


class Limits(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_int), ("height", C.c_int), ("max_slots", C.c_int),
                ("max_jobs", C.c_int), ("max_pts", C.c_int), ("max_corners", C.c_int), ("max_kf", C.c_int),
                ("max_lm", C.c_int), ("max_obs", C.c_int), ("max_streams", C.c_int), ("device_map", C.c_int)]


class RtrackJob(C.Structure):
    _fields_ = [("stream", C.c_int), ("prev_slot", C.c_int), ("next_slot", C.c_int), ("pt_ofs", C.c_int),
                ("npts", C.c_int), ("pose", C.c_double * 7), ("T_cam_w", C.c_double * 7), ("n_tracked", C.c_int),
                ("n_edges", C.c_int), ("n_outlier", C.c_int), ("reserved", C.c_int)]


class LkJob(C.Structure):
    _fields_ = [("prev_slot", C.c_int), ("next_slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int)]


class LkParams(C.Structure):
    _fields_ = [("max_level", C.c_int), ("max_iter", C.c_int), ("epsilon", C.c_double),
                ("min_eig_thr", C.c_double), ("use_initial_flow", C.c_int)]


class GfttJob(C.Structure):
    _fields_ = [("slot", C.c_int), ("rect_ofs", C.c_int), ("nrect", C.c_int)]


class TriJob(C.Structure):
    _fields_ = [("pt_ofs", C.c_int), ("npts", C.c_int), ("T_wc", C.c_double * 7), ("zmax", C.c_double)]


class PoseJob(C.Structure):
    _fields_ = [("pt_ofs", C.c_int), ("npts", C.c_int), ("pose", C.c_double * 7), ("n_inlier", C.c_int),
                ("reserved", C.c_int)]


class BaJob(C.Structure):
    _fields_ = [("kf_ofs", C.c_int), ("nkf", C.c_int), ("lm_ofs", C.c_int), ("nlm", C.c_int),
                ("obs_ofs", C.c_int), ("nobs", C.c_int), ("iters_done", C.c_int), ("reserved", C.c_int)]


class PgJob(C.Structure):
    _fields_ = [("kf_ofs", C.c_int), ("nkf", C.c_int), ("edge_ofs", C.c_int), ("nedge", C.c_int), ("pt_ofs", C.c_int),
                ("npt", C.c_int), ("iters_done", C.c_int), ("n_trials", C.c_int), ("chi2_before", C.c_double),
                ("chi2_after", C.c_double)]


class LfJob(C.Structure):
    _fields_ = [("kf_ofs", C.c_int), ("nkf", C.c_int), ("pt_ofs", C.c_int), ("npt", C.c_int), ("cur", C.c_int), ("last", C.c_int),
                ("T_cur", C.c_double * 7), ("T_corr", C.c_double * 7), ("T_last", C.c_double * 7), ("n_unanchored", C.c_int),
                ("reserved", C.c_int)]


class LoopJob(C.Structure):
    _fields_ = [("c_ofs", C.c_int), ("nc", C.c_int), ("q_ofs", C.c_int), ("nq", C.c_int), ("T_cur", C.c_double * 7),
                ("T_cand", C.c_double * 7), ("status", C.c_int), ("n_matches", C.c_int), ("n_points", C.c_int), ("n_inliers", C.c_int),
                ("need_correction", C.c_int), ("reserved", C.c_int), ("T_corr", C.c_double * 7), ("T_rel", C.c_double * 7), ("d", C.c_double)]


class LoopParams(C.Structure):
    _fields_ = [("cam", C.c_double * 4), ("ext_l", C.c_double * 7), ("min_matches", C.c_int), ("ransac_iters", C.c_int),
                ("reproj_px", C.c_double), ("max_pose_distance", C.c_double), ("min_pose_difference", C.c_double),
                ("max_pose_difference", C.c_double), ("seed", C.c_uint), ("reserved", C.c_int)]


LOOP_STATUS = ("ACCEPTED", "FEW_MATCHES", "FEW_POINTS", "FEW_INLIERS", "TOO_FAR", "TOO_DIFFERENT")
# the reference's constants (src/loopclosure.cpp:381) and the values of its config for the loop keys
LOOP_DEFAULTS = dict(min_matches=20, ransac_iters=100, reproj_px=5.991, max_pose_distance=20.0, min_pose_difference=1.0,
                     max_pose_difference=50.0, seed=0)


class LcJob(C.Structure):
    _fields_ = [("stream", C.c_int), ("kf_id", C.c_int), ("status", C.c_int), ("cand_kf", C.c_int), ("best_kf", C.c_int),
                ("n_weak", C.c_int), ("n_compared", C.c_int), ("best_sim", C.c_float)]


class LcParams(C.Structure):
    _fields_ = [("weak", C.c_float), ("strong", C.c_float), ("max_num_weak", C.c_int), ("min_gap", C.c_int)]


LC_STATUS = ("FOUND", "NONE", "BELOW_STRONG", "TOO_MANY_WEAK", "BAD_VECTOR")
# potential_loop_weak_threshold, potential_loop_strong_threshold, max_num_weak_threshold of the reference's configuration; the gap is
# the literal of src/loopclosure.cpp:244
LC_DEFAULTS = dict(weak=0.93, strong=0.95, max_num_weak=3, min_gap=20)


class GdLayer(C.Structure):
    _fields_ = [("op", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("stride", C.c_int), ("relu6", C.c_int), ("add_from", C.c_int)]


class GdPrep(C.Structure):
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("mean", C.c_float * 3), ("scale", C.c_float), ("workspace_bytes", C.c_longlong)]


GD_OPS = ("CONV3", "DW3", "PW", "AVGPOOL")
# the reference's blobFromImage call (src/loopclosure.cpp:103-105): it subtracts 0.485 from a 0 .. 255 value
GD_PREP_DEFAULTS = dict(out_w=224, out_h=224, mean=(0.485, 0.456, 0.406), scale=1.0 / 255.0, workspace_bytes=0)


def gd_layer_array(layers):
    """[(op, cin, cout, stride, relu6, add_from)] -> a ctypes array of svslam_gd_layer"""
    arr = (GdLayer * max(len(layers), 1))()
    for i, l in enumerate(layers):
        arr[i] = GdLayer(*[int(v) for v in l])
    return arr


def gd_prep_struct(prep):
    """None (the reference's call) or a dict over GD_PREP_DEFAULTS -> svslam_gd_prep or None"""
    if prep is None:
        return None
    unknown = set(prep) - set(GD_PREP_DEFAULTS)
    if unknown:
        raise TypeError("global descriptor: unknown prep key(s) %s" % sorted(unknown))
    p = dict(GD_PREP_DEFAULTS); p.update(prep)
    return GdPrep(int(p["out_w"]), int(p["out_h"]), (C.c_float * 3)(*[float(m) for m in p["mean"]]), float(p["scale"]),
                  int(p["workspace_bytes"]))


class BriefJob(C.Structure):
    _fields_ = [("slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int), ("n_desc", C.c_int), ("reserved", C.c_int)]


class BriefParams(C.Structure):
    _fields_ = [("pattern", C.c_void_p), ("angle_deg", C.c_float), ("edge", C.c_int)]


class OrbJob(C.Structure):
    _fields_ = [("slot", C.c_int), ("rect_ofs", C.c_int), ("nrect", C.c_int), ("n_out", C.c_int), ("n_found", C.c_int), ("reserved", C.c_int)]


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("nlevels", C.c_int), ("fast_threshold", C.c_int), ("edge", C.c_int)]


class OrbDescJob(C.Structure):
    _fields_ = [("slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int), ("n_desc", C.c_int), ("reserved", C.c_int)]


class OrbDescParams(C.Structure):
    _fields_ = [("pattern", C.c_void_p), ("edge", C.c_int), ("nlevels", C.c_int), ("reserved", C.c_int)]


# svslam_orb_kp as a structured array's row
ORB_KP = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])


def orb_keypoints(kp):
    """keypoints as an ORB_KP array: one already, or rows of (x, y, angle, octave)"""
    if isinstance(kp, np.ndarray) and kp.dtype == ORB_KP:
        return np.ascontiguousarray(kp).reshape(-1)
    rows = np.asarray(kp, np.float64).reshape(-1, 4)
    out = np.zeros(len(rows), ORB_KP)
    out["x"], out["y"], out["angle"], out["octave"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3].astype(np.int32)
    return out


class BmParams(C.Structure):
    _fields_ = [("num_disparities", C.c_int), ("block_size", C.c_int), ("pre_filter_cap", C.c_int),
                ("texture_threshold", C.c_int), ("uniqueness_ratio", C.c_int), ("reserved", C.c_int)]


class BmJob(C.Structure):
    _fields_ = [("slot_left", C.c_int), ("slot_right", C.c_int)]


class DenseJob(C.Structure):
    _fields_ = [("slot_left", C.c_int), ("slot_right", C.c_int), ("pt_ofs", C.c_int), ("n_points", C.c_int),
                ("T_cw", C.c_double * 7)]


class TrackJob(C.Structure):
    _fields_ = [("prev_slot", C.c_int), ("next_slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int),
                ("pose", C.c_double * 7), ("n_tracked", C.c_int), ("n_inlier", C.c_int)]


class DmapJob(C.Structure):
    """svslam_dmap_job"""
    _fields_ = [("stream", C.c_int), ("slot_cur", C.c_int), ("slot_right", C.c_int), ("is_init", C.c_int),
                ("kf_slot", C.c_int), ("remove_slot", C.c_int), ("kf_id", C.c_int), ("npts", C.c_int), ("frame_id", C.c_longlong),
                ("pose", C.c_double * 7), ("T_camr_w", C.c_double * 7), ("T_wc", C.c_double * 7), ("src_buf", C.c_int), ("dst_buf", C.c_int),
                ("stamp", C.c_int), ("corners_dropped", C.c_int), ("ok", C.c_int), ("n_features", C.c_int), ("n_corners", C.c_int),
                ("n_right_ok", C.c_int), ("n_tri_in", C.c_int), ("n_tri_ok", C.c_int), ("ba_nkf", C.c_int), ("ba_nlm", C.c_int),
                ("ba_nobs", C.c_int), ("ba_iters", C.c_int), ("flags", C.c_int), ("dead", C.c_int), ("ba_npair", C.c_int),
                ("ba_ntrial", C.c_int), ("ev_ofs", C.c_int), ("ev_n", C.c_int), ("win_pose", (C.c_double * 7) * 12),
                ("win_slot", C.c_int * 12)]


class DmapParams(C.Structure):
    _fields_ = [("num_features", C.c_int), ("num_features_init", C.c_int), ("num_active_keyframes", C.c_int), ("ba_iters", C.c_int),
                ("max_triangulation_depth", C.c_double), ("chi2_th", C.c_double), ("ba_defer", C.c_int), ("reserved", C.c_int)]


# test hooks of the device map (svslam_debug_dmap_*): the arrays of one stream's map, (name, dtype, shape in terms of KW, NF, NL)
DMAP_STATE_FIELDS = (("kf_frame", np.int64, "K"), ("kf_id", np.int32, "K"), ("kf_pose", np.float64, "K7"), ("kf_n", np.int32, "K"),
                     ("f_xy", np.float32, "KF2"), ("f_xyr", np.float32, "KF2"), ("f_lm", np.int32, "KF"), ("f_lmr", np.int32, "KF"),
                     ("f_fl", np.uint8, "KF"), ("lm_pos", np.float64, "L3"), ("lm_id", np.int32, "L"), ("lm_obs", np.int32, "L"),
                     ("lm_state", np.uint8, "L"), ("lm_stamp", np.int32, "L"), ("next_lm_id", np.int32, "1"))
DMAP_STAGES = {"begin": 0, "stereo_prep": 1, "stereo_finish": 2, "commit": 3, "ba_gather": 4, "ba_scatter": 5, "refresh": 6, "refresh_xyz": 7}
DMAP_BADEV_INTS = 21
DMAP_BADEV = ("kf_ofs", "nkf", "lm_ofs", "nlm", "obs_ofs", "nobs", "nblk", "na", "ncontrib", "ntile", "aux_ofs", "iters_done", "rec_ofs",
              "lay_nblk", "lay_na", "lay_ntile", "nmv", "reserved", "lm_base", "shmask", "ntrial")


class DmapState(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in DMAP_STATE_FIELDS]


class DmapStageIO(C.Structure):
    _fields_ = [("threads", C.c_int), ("max_kf", C.c_int), ("max_obs", C.c_int), ("ev_quota", C.c_int), ("max_corners", C.c_int),
                ("num_features_init", C.c_int), ("zmax", C.c_double), ("chi2_th", C.c_double), ("cam_r", C.c_double * 4)] + \
               [(name, C.c_void_p) for name in ("evicted", "ev_cursor", "corners", "ncorners", "lkjobs", "prev_xy", "next_xy", "status",
                                                "trijobs", "uv_l", "uv_r", "tri_idx", "tri_xyz", "tri_ok", "badev", "poses", "pts",
                                                "packed", "uv", "edge_ref", "lm_slot_of", "chi2")]


_lib = None


def build(force=False, verbose=False):
    """Compile every native library of the package (hipcc, gfx950)."""
    return _build.build_all(force=force, verbose=verbose)


def lib_path():
    return os.path.join(LIB_DIR, "libsvslam_hip.so")


def load():
    """dlopen libsvslam_hip.so; raises if it has not been built."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError("libsvslam_hip.so is missing: run stereovision-slam_amd/build.py "
                               "(there is no CPU fallback)")
        L = C.CDLL(p)
        L.svslam_last_error.restype = C.c_char_p
        L.svslam_build_info.restype = C.c_char_p
        L.svslam_last_error.argtypes = [C.c_void_p]
        L.svslam_destroy.argtypes = [C.c_void_p]
        L.svslam_destroy.restype = None
        L.svslam_set_pose_only_xtol.argtypes = [C.c_void_p, C.c_double]
        L.svslam_get_pose_only_xtol.argtypes = [C.c_void_p]
        L.svslam_get_pose_only_xtol.restype = C.c_double
        L.svslam_cloud_sor_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svslam_cloud_voxel_grid.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.svslam_gdesc_configure.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.svslam_gdesc_describe_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.svslam_gdesc_dim.argtypes = [C.c_void_p]
        L.svslam_orb_detect_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.svslam_orb_describe_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svslam_orb_read_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.svslam_dev_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.svslam_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        L.svslam_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.svslam_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a, cols):
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols)


def _d(a):
    return np.ascontiguousarray(a, np.float64)


IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


class Context:
    """One svslam_ctx: own HIP stream, resident pyramid slots, staging arena."""

    def __init__(self, width, height, max_slots=4, max_jobs=1, max_pts=512, max_corners=150, max_kf=10,
                 max_lm=2048, max_obs=8192, device=0, max_streams=0, device_map=0):
        self.L = load()
        self.lim = Limits(device, width, height, max_slots, max_jobs, max_pts, max_corners, max_kf, max_lm,
                          max_obs, max_streams, device_map)
        self.h = C.c_void_p()
        rc = self.L.svslam_create(C.byref(self.lim), C.byref(self.h))
        if rc != 0:
            msg = self.L.svslam_last_error(self.h).decode() if self.h else "no HIP device / bad limits"
            if self.h:
                self.L.svslam_destroy(self.h)
                self.h = C.c_void_p()
            raise RuntimeError("svslam_create failed (%d): %s" % (rc, msg))
        self.width, self.height = width, height
        self._owned = True

    @classmethod
    def borrow(cls, handle, width, height):
        """wrap an svslam_ctx owned by someone else (e.g. the host pipeline)"""
        self = cls.__new__(cls)
        self.L = load()
        self.h = C.c_void_p(handle)
        self.width, self.height = width, height
        self._owned = False
        return self

    def close(self):
        if self.h and getattr(self, "_owned", False):
            self.L.svslam_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.svslam_last_error(self.h).decode()))

    # ---- device memory -------------------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.svslam_dev_alloc(self.h, nbytes, C.byref(p)), "dev_alloc")
        return p.value

    def dev_free(self, ptr):
        self._chk(self.L.svslam_dev_free(self.h, C.c_void_p(ptr)), "dev_free")

    def dev_upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.svslam_dev_upload(self.h, C.c_void_p(ptr), _p(arr), arr.nbytes), "dev_upload")

    def dev_download(self, ptr, arr):
        self._chk(self.L.svslam_dev_download(self.h, _p(arr), C.c_void_p(ptr), arr.nbytes), "dev_download")

    def sync(self):
        self._chk(self.L.svslam_sync(self.h), "sync")

    # ---- timing ----------------------------------------------------------
    def ll_limits(self):
        """test hook (svslam_debug_ll_limits): [shards per problem, problems per call, CUs counted, solver workgroups per CU]"""
        o = (C.c_int * 4)()
        self._chk(self.L.svslam_debug_ll_limits(self.h, o), "debug_ll_limits")
        return [int(v) for v in o]

    def hold_cus(self, ncus, ms):
        """test hook (svslam_debug_hold_cus): ncus workgroups take a CU's LDS each and spin for ms; asynchronous"""
        self._chk(self.L.svslam_debug_hold_cus(self.h, int(ncus), C.c_double(ms)), "debug_hold_cus")

    def clock_mhz(self, blocks=1, ms=1.0):
        """effective shader clock seen by a wave that spins for `ms` of the constant 100 MHz counter (svslam_debug_clock_mhz)"""
        mhz = C.c_double(0)
        self._chk(self.L.svslam_debug_clock_mhz(self.h, blocks, C.c_double(ms), C.byref(mhz)), "debug_clock_mhz")
        return mhz.value

    def host_counters(self):
        """test hook (svslam_debug_host_ns): 8 host-side counters since the last call; [6] = local-BA problems the
        low-latency solver took"""
        o = (C.c_longlong * 8)()
        self._chk(self.L.svslam_debug_host_ns(self.h, o), "debug_host_ns")
        return [int(v) for v in o]

    def ll_shards(self, nproblems=1):
        """test hook (svslam_debug_ll_shards): [nproblems, W, 8] ints of the last low-latency local-BA call — landmarks,
        edges, blocks, tiles, solver (2 resident / 1 streaming), active poses, shard mask, iterations"""
        w = C.c_int(0)
        out = np.zeros((nproblems * 16, 8), np.int32)
        self._chk(self.L.svslam_debug_ll_shards(self.h, nproblems, _p(out), C.byref(w)), "debug_ll_shards")
        return out[:nproblems * w.value].reshape(nproblems, w.value, 8).copy()

    BA_STRUCT_FIELDS = ("nblk", "na", "ncontrib", "ntile", "nmv", "iters_done", "ntrial", "flags")

    def ba_struct(self, njobs=1):
        """test hook (svslam_debug_ba_struct): [njobs, 8] ints of the last local-BA call — blocks, active poses, block pairs,
        tiles, landmarks in the tiles, iterations, LM trials, flags (1 edges arrived in order, 2 edge cache used, 4 host build)"""
        out = np.zeros((njobs, 8), np.int32)
        self._chk(self.L.svslam_debug_ba_struct(self.h, njobs, _p(out)), "debug_ba_struct")
        return out

    def low_latency(self, on=True):
        """latency shape of the serial kernels (svslam_set_low_latency): a few jobs per launch"""
        self._chk(self.L.svslam_set_low_latency(self.h, 1 if on else 0), "set_low_latency")

    def pose_only_xtol(self, xtol):
        """parameter tolerance of the pose-only LM (svslam_set_pose_only_xtol); 0 = g2o's schedule to the last trial"""
        self._chk(self.L.svslam_set_pose_only_xtol(self.h, C.c_double(xtol)), "set_pose_only_xtol")

    def pose_only_xtol_effective(self):
        """the tolerance the context uses (svslam_get_pose_only_xtol)"""
        return float(self.L.svslam_get_pose_only_xtol(self.h))

    def timing(self, on=True):
        self.L.svslam_timing_enable(self.h, 1 if on else 0)
        self.L.svslam_timing_reset(self.h)

    def timing_get(self, family):
        ms, n, u = C.c_double(), C.c_longlong(), C.c_longlong()
        fam = next(t[family] for t in (FAMILIES, KERNEL_FAMILIES, DENSE_FAMILIES, CLOUD_FAMILIES, LOOP_FAMILIES, COLOUR_FAMILIES, ORB_FAMILIES, ORB_DESC_FAMILIES, DEBUG_FAMILIES) if family in t)
        self._chk(self.L.svslam_timing_get(self.h, fam, C.byref(ms), C.byref(n), C.byref(u)), "timing")
        return ms.value, n.value, u.value

    def ba_profile(self, enable=True, read=False):
        out = (C.c_longlong * 12)()
        self._chk(self.L.svslam_ba_profile(self.h, 1 if enable else 0, out if read else None), "ba_profile")
        return list(out)

    def lm_trace(self, enable=True, job=None, cap=408):
        """test hook: record / read the LM trajectory [ntrials, 6] of the last pose-only / local-BA call (svslam_lm_trace)"""
        if job is None:
            self._chk(self.L.svslam_lm_trace(self.h, 1 if enable else 0, 0, None, 0, None), "lm_trace")
            return None
        out = np.zeros((cap, 6)); n = C.c_int(0)
        self._chk(self.L.svslam_lm_trace(self.h, 1, job, _p(out), cap, C.byref(n)), "lm_trace")
        return out[:n.value].copy()

    # ---- pyramids --------------------------------------------------------
    def pyramid(self, slots, imgs, device=False, strides=None, decimate_from=None):
        n = len(slots)
        sl = (C.c_int * n)(*slots)
        keep = []
        if device:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in imgs])
            st = (C.c_int * n)(*(strides or [self.width if decimate_from is None else decimate_from[0]] * n))
        else:
            keep = [np.ascontiguousarray(im, np.uint8) for im in imgs]
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in keep])
            st = (C.c_int * n)(*[im.shape[1] for im in keep])
        if decimate_from is None:
            rc = self.L.svslam_pyramid_batch(self.h, n, sl, ptrs, st, 1 if device else 0)
        else:
            rc = self.L.svslam_pyramid_decimate_batch(self.h, n, sl, ptrs, st, decimate_from[0], decimate_from[1],
                                                      1 if device else 0)
        self._chk(rc, "pyramid")

    def pyramid_read(self, slot, level):
        w, h = C.c_int(), C.c_int()
        self._chk(self.L.svslam_pyramid_read(self.h, slot, level, None, C.byref(w), C.byref(h)), "pyramid_read")
        out = np.zeros((h.value, w.value), np.uint8)
        self._chk(self.L.svslam_pyramid_read(self.h, slot, level, _p(out), C.byref(w), C.byref(h)), "pyramid_read")
        return out

    def pyramid_read_padded(self, slot, level):
        """the level with its stored 16-px REFLECT_101 border"""
        w, h = C.c_int(), C.c_int()
        self._chk(self.L.svslam_pyramid_read(self.h, slot, level, None, C.byref(w), C.byref(h)), "pyramid_read")
        out = np.zeros((h.value + 32, w.value + 32), np.uint8)
        self._chk(self.L.svslam_pyramid_read_padded(self.h, slot, level, _p(out)), "pyramid_read_padded")
        return out

    # ---- dense stereo ----------------------------------------------------
    @staticmethod
    def _bm_params(num_disparities=128, block_size=15, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15):
        return BmParams(num_disparities, block_size, pre_filter_cap, texture_threshold, uniqueness_ratio, 0)

    def stereo_bm(self, jobs, **params):
        """cv::StereoBM on level 0 of pyramid slots.  jobs: list of (slot_left, slot_right); params: num_disparities 128,
        block_size 15, pre_filter_cap 31, texture_threshold 10, uniqueness_ratio 15.  returns int16 [njobs, h, w] of
        16 x disparity, -16 where there is none."""
        n = len(jobs)
        arr = (BmJob * max(n, 1))(*[BmJob(int(l), int(r)) for l, r in jobs])
        out = np.zeros((n, self.height, self.width), np.int16)
        prm = self._bm_params(**params)
        self._chk(self.L.svslam_stereo_bm_batch(self.h, n, arr, C.byref(prm), _p(out)), "stereo_bm_batch")
        return out

    def stereo_bm_strip_rows(self, njobs, **params):
        """test hook: the strip height (16, 8 or 4 output rows per workgroup; 0 on the early-out) a call of njobs jobs runs with"""
        prm = self._bm_params(**params)
        th = self.L.svslam_stereo_bm_strip_rows(self.h, int(njobs), C.byref(prm))
        if th < 0:
            self._chk(th, "stereo_bm_strip_rows")
        return th

    def dense_cloud(self, jobs, cam_l, ext_l, baseline, min_depth=1.0, max_pts_per_job=None, **params):
        """the matcher + src/dense_reconstruction.cpp:116-173.  jobs: list of (slot_left, slot_right, T_cw[7] or None).
        returns per job (xyz float32 [n, 3] in the map frame, pix int32 [n] = y * width + x, disp int16 [h, w]), the
        points in the reference's order (x outer, y inner)."""
        n = len(jobs)
        cap = self.width * self.height if max_pts_per_job is None else int(max_pts_per_job)
        arr = (DenseJob * max(n, 1))()
        for i, (sl, sr, T) in enumerate(jobs):
            arr[i] = DenseJob(int(sl), int(sr), i * cap, 0, (C.c_double * 7)(*(IDENT if T is None else _d(T))))
        xyz = np.zeros((max(n * cap, 1), 3), np.float32); pix = np.zeros(max(n * cap, 1), np.int32)
        disp = np.zeros((n, self.height, self.width), np.int16)
        prm = self._bm_params(**params)
        self._chk(self.L.svslam_dense_cloud_batch(self.h, n, arr, _p(_d(cam_l)), _p(_d(ext_l)), C.c_double(baseline), C.byref(prm),
                                                  C.c_double(min_depth), cap, _p(xyz), _p(pix), _p(disp)), "dense_cloud_batch")
        return [(xyz[j.pt_ofs:j.pt_ofs + j.n_points].copy(), pix[j.pt_ofs:j.pt_ofs + j.n_points].copy(), disp[i].copy())
                for i, j in enumerate(arr[:n])]

    # ---- colour input of the dense program ---------------------------------
    def colour_reserve(self, n):
        """n colour planes [height, width, 3] (b, g, r) on the device (svslam_colour_reserve); 0 frees, a new count drops the contents"""
        self._chk(self.L.svslam_colour_reserve(self.h, int(n)), "colour_reserve")

    def pyramid_bgr(self, slots, planes, imgs, device=False, strides=None):
        """packed BGR images -> pyramid slots (from the grey image, made on the device) and colour planes (svslam_pyramid_bgr_batch).
        planes: a plane per image, -1 keeps no colour.  imgs: uint8 [H, W, 3], all of one shape: the context's, or one that
        halves to it (then dst(x, y) = src(2x, 2y)).  device=True: imgs are (pointer, H, W) of images in device memory,
        strides their bytes per row (default 3 W)."""
        n = len(slots)
        if len(planes) != n or len(imgs) != n:
            raise ValueError("slots, planes and imgs differ in length")
        sl = (C.c_int * max(n, 1))(*[int(v) for v in slots]); pl = (C.c_int * max(n, 1))(*[int(v) for v in planes])
        keep = []
        if device:
            shapes = {(int(h), int(w)) for _, h, w in imgs}
            ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(int(p)) for p, _, _ in imgs])
            st = [3 * int(w) for _, _, w in imgs] if strides is None else [int(v) for v in strides]
        else:
            # a view whose pixels are packed keeps its row stride; anything else is copied tight
            keep = [im if isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.strides[1:] == (3, 1) and im.strides[0] >= 3 * im.shape[1]
                    else np.ascontiguousarray(im, np.uint8) for im in imgs]
            if any(im.ndim != 3 or im.shape[2] != 3 for im in keep):
                raise ValueError("pyramid_bgr takes uint8 [H, W, 3] images")
            shapes = {im.shape[:2] for im in keep}
            ptrs = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in keep])
            st = [im.strides[0] for im in keep]
        if len(shapes) > 1:
            raise ValueError("the images of one call have one shape")
        sh, sw = shapes.pop() if shapes else (self.height, self.width)
        self._chk(self.L.svslam_pyramid_bgr_batch(self.h, n, sl, pl, ptrs, (C.c_int * max(n, 1))(*st), int(sw), int(sh), 1 if device else 0), "pyramid_bgr_batch")

    def colour_read(self, plane):
        """test hook (svslam_colour_read): a colour plane, uint8 [height, width, 3]"""
        out = np.zeros((self.height, self.width, 3), np.uint8)
        self._chk(self.L.svslam_colour_read(self.h, int(plane), _p(out)), "colour_read")
        return out

    def dense_cloud_bgr(self, jobs, cam_l, ext_l, baseline, min_depth=1.0, max_pts_per_job=None, **params):
        """dense_cloud with the colour of every point (svslam_dense_cloud_bgr_batch).  jobs: list of (slot_left, slot_right, plane,
        T_cw[7] or None).  returns per job (xyz, pix, bgr uint8 [n, 3], disp); xyz, pix and disp are dense_cloud's."""
        n = len(jobs)
        cap = self.width * self.height if max_pts_per_job is None else int(max_pts_per_job)
        arr = (DenseJob * max(n, 1))()
        for i, (sl, sr, _, T) in enumerate(jobs):
            arr[i] = DenseJob(int(sl), int(sr), i * cap, 0, (C.c_double * 7)(*(IDENT if T is None else _d(T))))
        pl = (C.c_int * max(n, 1))(*[int(j[2]) for j in jobs])
        xyz = np.zeros((max(n * cap, 1), 3), np.float32); pix = np.zeros(max(n * cap, 1), np.int32)
        bgr = np.zeros((max(n * cap, 1), 3), np.uint8)
        disp = np.zeros((n, self.height, self.width), np.int16)
        prm = self._bm_params(**params)
        self._chk(self.L.svslam_dense_cloud_bgr_batch(self.h, n, arr, _p(_d(cam_l)), _p(_d(ext_l)), C.c_double(baseline), C.byref(prm),
                                                      C.c_double(min_depth), cap, pl, _p(xyz), _p(pix), _p(bgr), _p(disp)), "dense_cloud_bgr_batch")
        return [(xyz[j.pt_ofs:j.pt_ofs + j.n_points].copy(), pix[j.pt_ofs:j.pt_ofs + j.n_points].copy(),
                 bgr[j.pt_ofs:j.pt_ofs + j.n_points].copy(), disp[i].copy()) for i, j in enumerate(arr[:n])]

    # ---- cloud filters ---------------------------------------------------
    def cloud_sor(self, clouds, mean_k=50, stddev_mul=1.0):
        """pcl::StatisticalOutlierRemoval on a list of [n, 3] float32 clouds, one batched call (svslam_cloud_sor_batch).
        returns per cloud (keep bool [n], mean_dist float32 [n], threshold float; NaN and all kept below mean_k + 1 points)"""
        cl = [_f32(x, 3) for x in clouds]
        ofs = np.zeros(len(cl) + 1, np.int64)
        ofs[1:] = np.cumsum([len(x) for x in cl])
        n = int(ofs[-1])
        xyz = np.ascontiguousarray(np.concatenate(cl)) if n else np.zeros((1, 3), np.float32)
        keep = np.zeros(max(n, 1), np.uint8); md = np.zeros(max(n, 1), np.float32); thr = np.zeros(max(len(cl), 1))
        self._chk(self.L.svslam_cloud_sor_batch(self.h, len(cl), _p(ofs), _p(xyz), int(mean_k), C.c_double(stddev_mul), _p(keep), _p(md),
                                                _p(thr)), "cloud_sor_batch")
        return [(keep[a:b].astype(bool), md[a:b].copy(), float(thr[i])) for i, (a, b) in enumerate(zip(ofs[:-1], ofs[1:]))]

    def cloud_sor_climbs(self):
        """measurement hook (svslam_debug_cloud_sor_climbs): (queries, queries that scanned more than their first block) since the last call"""
        q, k = C.c_longlong(), C.c_longlong()
        self._chk(self.L.svslam_debug_cloud_sor_climbs(self.h, C.byref(q), C.byref(k)), "debug_cloud_sor_climbs")
        return q.value, k.value

    def cloud_voxel_grid(self, xyz, rgb, leaf=0.02):
        """pcl::VoxelGrid (svslam_cloud_voxel_grid): xyz float32 [n, 3], rgb uint8 [n, 3] -> (xyz, rgb, overflowed); overflowed:
        PCL's int32 index guard tripped, the output is the input"""
        xyz = _f32(xyz, 3); rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        n = len(xyz)
        if len(rgb) != n:
            raise ValueError("xyz and rgb differ in length")
        oxyz = np.zeros((max(n, 1), 3), np.float32); orgb = np.zeros((max(n, 1), 3), np.uint8)
        m, over = C.c_int64(0), C.c_int(0)
        self._chk(self.L.svslam_cloud_voxel_grid(self.h, n, _p(xyz), _p(rgb), C.c_double(leaf), _p(oxyz), _p(orgb), C.byref(m), C.byref(over)),
                  "cloud_voxel_grid")
        return oxyz[:m.value].copy(), orgb[:m.value].copy(), bool(over.value)

    # ---- LK --------------------------------------------------------------
    def lk(self, jobs, params=None):
        """jobs: list of (prev_slot, next_slot, prev_xy[n,2], next_xy_guess[n,2]).
        returns list of (next_xy, status, err)."""
        n = len(jobs)
        arr = (LkJob * n)()
        prevs, nexts, ofs = [], [], 0
        for i, (ps, ns, p, q) in enumerate(jobs):
            p = _f32(p, 2); q = _f32(q, 2)
            arr[i] = LkJob(ps, ns, ofs, p.shape[0])
            ofs += p.shape[0]
            prevs.append(p); nexts.append(q)
        prev = np.concatenate(prevs) if prevs else np.zeros((0, 2), np.float32)
        nxt = np.concatenate(nexts).copy() if nexts else np.zeros((0, 2), np.float32)
        prev = np.ascontiguousarray(prev); nxt = np.ascontiguousarray(nxt)
        status = np.zeros(max(ofs, 1), np.uint8)
        err = np.zeros(max(ofs, 1), np.float32)
        prm = params or LkParams(3, 30, 0.01, 1e-4, 1)
        self._chk(self.L.svslam_lk_batch(self.h, n, arr, ofs, _p(prev), _p(nxt), _p(status), _p(err), C.byref(prm)),
                  "lk_batch")
        out = []
        for j in arr:
            s = slice(j.pt_ofs, j.pt_ofs + j.npts)
            out.append((nxt[s].copy(), status[s].copy(), err[s].copy()))
        return out

    # ---- GFTT ------------------------------------------------------------
    def gftt(self, jobs, max_corners=150, quality=0.01, min_dist=20.0):
        """jobs: list of (slot, rect_xy[n,2] or None). returns list of corners[k,2]."""
        n = len(jobs)
        arr = (GfttJob * n)()
        rects, ofs = [], 0
        for i, (slot, r) in enumerate(jobs):
            r = np.zeros((0, 2), np.float32) if r is None else _f32(r, 2)
            arr[i] = GfttJob(slot, ofs, r.shape[0])
            ofs += r.shape[0]
            rects.append(r)
        rect = np.ascontiguousarray(np.concatenate(rects)) if ofs else np.zeros((1, 2), np.float32)
        out = np.zeros((n, max_corners, 2), np.float32)
        cnt = np.zeros(n, np.int32)
        self._chk(self.L.svslam_gftt_batch(self.h, n, arr, ofs, _p(rect), max_corners, C.c_double(quality),
                                           C.c_double(min_dist), _p(out), _p(cnt)), "gftt_batch")
        return [out[i, :cnt[i]].copy() for i in range(n)]

    def gftt_eigmap(self, slot):
        out = np.zeros((self.height, self.width), np.float32)
        self._chk(self.L.svslam_gftt_eigmap(self.h, slot, _p(out)), "gftt_eigmap")
        return out

    # ---- triangulation -----------------------------------------------------
    def triangulate(self, jobs, cam_l, ext_l, cam_r, ext_r):
        """jobs: list of (uv_l[n,2], uv_r[n,2], T_wc[7] or None, zmax). returns list of (xyz, ok)."""
        n = len(jobs)
        arr = (TriJob * n)()
        ls, rs, ofs = [], [], 0
        for i, (ul, ur, T, zmax) in enumerate(jobs):
            ul = _f32(ul, 2); ur = _f32(ur, 2)
            T = IDENT if T is None else _d(T)
            arr[i] = TriJob(ofs, ul.shape[0], (C.c_double * 7)(*T), float(zmax))
            ofs += ul.shape[0]
            ls.append(ul); rs.append(ur)
        if ofs == 0:
            return [(np.zeros((0, 3)), np.zeros(0, np.uint8)) for _ in jobs]
        L_ = np.ascontiguousarray(np.concatenate(ls)); R_ = np.ascontiguousarray(np.concatenate(rs))
        xyz = np.zeros((ofs, 3)); ok = np.zeros(ofs, np.uint8)
        self._chk(self.L.svslam_triangulate_batch(self.h, n, arr, ofs, _p(_d(cam_l)), _p(_d(ext_l)), _p(_d(cam_r)),
                                                  _p(_d(ext_r)), _p(L_), _p(R_), _p(xyz), _p(ok)), "triangulate")
        return [(xyz[j.pt_ofs:j.pt_ofs + j.npts].copy(), ok[j.pt_ofs:j.pt_ofs + j.npts].copy()) for j in arr]

    # ---- pose-only ---------------------------------------------------------
    def pose_only(self, jobs, cam, chi2_th=5.991, rounds=4, iters=10):
        """jobs: list of (pose[7], xyz[n,3], uv[n,2]). returns list of (pose, outlier, n_inlier)."""
        n = len(jobs)
        arr = (PoseJob * n)()
        xs, us, ofs = [], [], 0
        for i, (T, xyz, uv) in enumerate(jobs):
            xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3); uv = _f32(uv, 2)
            arr[i] = PoseJob(ofs, xyz.shape[0], (C.c_double * 7)(*_d(T)), 0, 0)
            ofs += xyz.shape[0]
            xs.append(xyz); us.append(uv)
        X = np.ascontiguousarray(np.concatenate(xs)) if ofs else np.zeros((1, 3))
        U = np.ascontiguousarray(np.concatenate(us)) if ofs else np.zeros((1, 2), np.float32)
        outl = np.zeros(max(ofs, 1), np.uint8)
        self._chk(self.L.svslam_pose_only_batch(self.h, n, arr, ofs, _p(_d(cam)), _p(X), _p(U), _p(outl),
                                                C.c_double(chi2_th), rounds, iters), "pose_only")
        return [(np.array(j.pose[:]), outl[j.pt_ofs:j.pt_ofs + j.npts].copy(), j.n_inlier) for j in arr]

    # ---- local BA ------------------------------------------------------------
    def local_ba(self, jobs, cam_l, ext_l, cam_r, ext_r, huber_delta=5.991, iters=10, split=False, between=None):
        """jobs: list of (poses[k,7], pts[m,3], obs_kf, obs_lm, obs_is_right, obs_uv).
        returns list of (poses, pts, edge_chi2, iters_done).  split=True goes through
        svslam_local_ba_submit / _collect (between() runs while the batch is in flight)."""
        n = len(jobs)
        arr = (BaJob * n)()
        P, X, K_, L_, R_, U = [], [], [], [], [], []
        ko = lo = oo = 0
        for i, (poses, pts, okf, olm, ori, ouv) in enumerate(jobs):
            poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
            pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
            okf = np.ascontiguousarray(okf, np.int32); olm = np.ascontiguousarray(olm, np.int32)
            ori = np.ascontiguousarray(ori, np.uint8); ouv = _f32(ouv, 2)
            arr[i] = BaJob(ko, poses.shape[0], lo, pts.shape[0], oo, okf.shape[0], 0, 0)
            ko += poses.shape[0]; lo += pts.shape[0]; oo += okf.shape[0]
            P.append(poses); X.append(pts); K_.append(okf); L_.append(olm); R_.append(ori); U.append(ouv)
        P = np.ascontiguousarray(np.concatenate(P)); X = np.ascontiguousarray(np.concatenate(X))
        K_ = np.ascontiguousarray(np.concatenate(K_)); L_ = np.ascontiguousarray(np.concatenate(L_))
        R_ = np.ascontiguousarray(np.concatenate(R_)); U = np.ascontiguousarray(np.concatenate(U))
        chi2 = np.zeros(max(oo, 1))
        if split:
            self._chk(self.L.svslam_local_ba_submit(self.h, n, arr, _p(_d(cam_l)), _p(_d(ext_l)), _p(_d(cam_r)),
                                                    _p(_d(ext_r)), ko, _p(P), lo, _p(X), oo, _p(K_), _p(L_), _p(R_),
                                                    _p(U), C.c_double(huber_delta), iters), "local_ba_submit")
            if between is not None:
                between()
            self._chk(self.L.svslam_local_ba_collect(self.h, n, arr, ko, _p(P), lo, _p(X), oo, _p(chi2)), "local_ba_collect")
        else:
            self._chk(self.L.svslam_local_ba_batch(self.h, n, arr, _p(_d(cam_l)), _p(_d(ext_l)), _p(_d(cam_r)),
                                                   _p(_d(ext_r)), ko, _p(P), lo, _p(X), oo, _p(K_), _p(L_), _p(R_),
                                                   _p(U), C.c_double(huber_delta), iters, _p(chi2)), "local_ba")
        out = []
        for j in arr:
            out.append((P[j.kf_ofs:j.kf_ofs + j.nkf].copy(), X[j.lm_ofs:j.lm_ofs + j.nlm].copy(),
                        chi2[j.obs_ofs:j.obs_ofs + j.nobs].copy(), j.iters_done))
        return out

    # ---- global pose-graph optimisation ----------------------------------------
    def pose_graph(self, jobs, iters=22):
        """LoopClosure::PoseGraphOptimization for every job in one call (svslam_pose_graph_batch).
        jobs: list of dicts with poses[n,7], fixed[n], edges = (a, b, meas[e,7]) or None, and optionally pts[m,3] with
        anchor[m] (vertex a point keeps its coordinates relative to, or -1).
        returns a list of dicts: poses, pts, iters, trials, chi2_before, chi2_after."""
        n = len(jobs)
        arr = (PgJob * n)()
        P, F, A, B, M, X, AN = [], [], [], [], [], [], []
        ko = eo = po = 0
        for i, job in enumerate(jobs):
            poses = np.ascontiguousarray(job["poses"], np.float64).reshape(-1, 7)
            fixed = np.ascontiguousarray(job["fixed"], np.uint8).reshape(-1)
            if len(fixed) != len(poses):
                raise ValueError("pose_graph: job %d has %d poses and %d fixed flags" % (i, len(poses), len(fixed)))
            edges = job.get("edges")
            if edges is None:
                ea = eb = np.zeros(0, np.int32); meas = np.zeros((0, 7))
            else:
                ea = np.ascontiguousarray(edges[0], np.int32).reshape(-1); eb = np.ascontiguousarray(edges[1], np.int32).reshape(-1)
                meas = np.ascontiguousarray(edges[2], np.float64).reshape(-1, 7)
                if not (len(ea) == len(eb) == len(meas)):
                    raise ValueError("pose_graph: job %d: edge arrays of different lengths" % i)
            pts = job.get("pts")
            pts = np.zeros((0, 3)) if pts is None else np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
            anchor = job.get("anchor")
            anchor = np.zeros(0, np.int32) if anchor is None else np.ascontiguousarray(anchor, np.int32).reshape(-1)
            if len(anchor) != len(pts):
                raise ValueError("pose_graph: job %d has %d points and %d anchors" % (i, len(pts), len(anchor)))
            arr[i] = PgJob(ko, len(poses), eo, len(ea), po, len(pts), 0, 0, 0.0, 0.0)
            ko += len(poses); eo += len(ea); po += len(pts)
            P.append(poses); F.append(fixed); A.append(ea); B.append(eb); M.append(meas); X.append(pts); AN.append(anchor)
        cat = lambda v, shape, dt: np.ascontiguousarray(np.concatenate(v)) if v else np.zeros(shape, dt)
        P = cat(P, (0, 7), np.float64); F = cat(F, 0, np.uint8); A = cat(A, 0, np.int32); B = cat(B, 0, np.int32)
        M = cat(M, (0, 7), np.float64); X = cat(X, (0, 3), np.float64); AN = cat(AN, 0, np.int32)
        self._chk(self.L.svslam_pose_graph_batch(self.h, n, arr, ko, _p(P), _p(F), eo, _p(A), _p(B), _p(M), po, _p(AN), _p(X),
                                                 int(iters)), "pose_graph")
        return [dict(poses=P[j.kf_ofs:j.kf_ofs + j.nkf].copy(), pts=X[j.pt_ofs:j.pt_ofs + j.npt].copy(), iters=j.iters_done,
                     trials=j.n_trials, chi2_before=j.chi2_before, chi2_after=j.chi2_after) for j in arr]

    # ---- local fusion after a closed loop ---------------------------------------
    def local_fusion(self, jobs):
        """steps 1-3 of LoopClosure::LocalFusion for every job in one call (svslam_local_fusion_batch).
        jobs: list of dicts with poses[n,7] (the active window), cur (index in the window, or -1 with T_cur[7]), T_corr[7],
        last (index in the window, or -1 with T_last[7]), pts[m,3], obs_ptr[m+1] and obs_kf[obs_ptr[m]] (per observation in list
        order the row of its keyframe in the corrected table: window index, n for a cur outside the window, -1 for none).
        returns a list of dicts: poses, T_last, pts, pt_kf (the row a landmark moved with, or -1), n_unanchored."""
        n = len(jobs)
        arr = (LfJob * max(n, 1))()
        P, X, OP, OK = [], [], [np.zeros(1, np.int32)], []
        ko = po = oo = 0
        for i, job in enumerate(jobs):
            poses = np.ascontiguousarray(job["poses"], np.float64).reshape(-1, 7)
            pts = job.get("pts")
            pts = np.zeros((0, 3)) if pts is None else np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
            ptr = job.get("obs_ptr")
            ptr = np.zeros(1, np.int64) if ptr is None else np.asarray(ptr, np.int64).reshape(-1)
            okf = job.get("obs_kf")
            okf = np.zeros(0, np.int32) if okf is None else np.ascontiguousarray(okf, np.int32).reshape(-1)
            if len(ptr) != len(pts) + 1 or ptr[0] != 0 or ptr[-1] != len(okf):
                raise ValueError("local_fusion: job %d: obs_ptr does not index %d points and %d observations" % (i, len(pts), len(okf)))
            cur, last = int(job["cur"]), int(job["last"])
            arr[i].kf_ofs, arr[i].nkf, arr[i].pt_ofs, arr[i].npt, arr[i].cur, arr[i].last = ko, len(poses), po, len(pts), cur, last
            arr[i].T_corr = (C.c_double * 7)(*_d(job["T_corr"]).reshape(7))
            if cur < 0:
                arr[i].T_cur = (C.c_double * 7)(*_d(job["T_cur"]).reshape(7))
            if last < 0:
                arr[i].T_last = (C.c_double * 7)(*_d(job["T_last"]).reshape(7))
            P.append(poses); X.append(pts); OP.append((ptr[1:] + oo).astype(np.int32)); OK.append(okf)
            ko += len(poses); po += len(pts); oo += len(okf)
        cat = lambda v, shape, dt: np.ascontiguousarray(np.concatenate(v)) if v else np.zeros(shape, dt)
        P = cat(P, (0, 7), np.float64); X = cat(X, (0, 3), np.float64); OP = cat(OP, 1, np.int32); OK = cat(OK, 0, np.int32)
        K = np.full(po, -1, np.int32)
        self._chk(self.L.svslam_local_fusion_batch(self.h, n, arr, ko, _p(P), po, _p(X), _p(OP), oo, _p(OK), _p(K)), "local_fusion")
        return [dict(poses=P[j.kf_ofs:j.kf_ofs + j.nkf].copy(), T_last=np.array(j.T_last), pts=X[j.pt_ofs:j.pt_ofs + j.npt].copy(),
                     pt_kf=K[j.pt_ofs:j.pt_ofs + j.npt].copy(), n_unanchored=j.n_unanchored) for j in arr[:n]]

    # ---- loop verification -----------------------------------------------------
    def loop_verify(self, jobs, cam, ext_l, **params):
        """LoopClosure::KeypointMatchWithLoopCandid + CalculatePose for every job in one call (svslam_loop_verify_batch).
        jobs: list of dicts with desc_c [nc, 32] u8, desc_q [nq, 32] u8, xyz_c [nc, 3], has_xyz [nc], uv_q [nq, 2], T_cur[7], T_cand[7].
        params: min_matches, ransac_iters, reproj_px, max_pose_distance, min_pose_difference, max_pose_difference, seed (LOOP_DEFAULTS).
        returns a list of dicts: status (index into LOOP_STATUS), n_matches, n_points, n_inliers, T_corr, T_rel, d, need_correction,
        matches [n_matches, 4] = candidate row, current row, Hamming distance, inlier flag."""
        unknown = set(params) - set(LOOP_DEFAULTS)
        if unknown:
            raise TypeError("loop_verify: unknown parameter(s) %s" % sorted(unknown))
        p = dict(LOOP_DEFAULTS); p.update(params)
        n = len(jobs)
        arr = (LoopJob * n)()
        DC, XC, HX, DQ, UV = [], [], [], [], []
        co = qo = 0
        for i, job in enumerate(jobs):
            dc = np.ascontiguousarray(job["desc_c"], np.uint8).reshape(-1, 32); dq = np.ascontiguousarray(job["desc_q"], np.uint8).reshape(-1, 32)
            xc = np.ascontiguousarray(job["xyz_c"], np.float64).reshape(-1, 3); hx = np.ascontiguousarray(job["has_xyz"], np.uint8).reshape(-1)
            uv = _f32(job["uv_q"], 2)
            if len(xc) != len(dc) or len(hx) != len(dc):
                raise ValueError("loop_verify: job %d has %d candidate descriptors, %d landmarks and %d flags" % (i, len(dc), len(xc), len(hx)))
            if len(uv) != len(dq):
                raise ValueError("loop_verify: job %d has %d current descriptors and %d pixels" % (i, len(dq), len(uv)))
            arr[i].c_ofs, arr[i].nc, arr[i].q_ofs, arr[i].nq = co, len(dc), qo, len(dq)
            arr[i].T_cur = (C.c_double * 7)(*_d(job["T_cur"]).reshape(7)); arr[i].T_cand = (C.c_double * 7)(*_d(job["T_cand"]).reshape(7))
            co += len(dc); qo += len(dq)
            DC.append(dc); XC.append(xc); HX.append(hx); DQ.append(dq); UV.append(uv)
        cat = lambda v, shape, dt: np.ascontiguousarray(np.concatenate(v)) if v else np.zeros(shape, dt)
        DC = cat(DC, (0, 32), np.uint8); XC = cat(XC, (0, 3), np.float64); HX = cat(HX, 0, np.uint8)
        DQ = cat(DQ, (0, 32), np.uint8); UV = cat(UV, (0, 2), np.float32)
        P = LoopParams((C.c_double * 4)(*_d(cam).reshape(4)), (C.c_double * 7)(*_d(ext_l).reshape(7)), int(p["min_matches"]),
                       int(p["ransac_iters"]), float(p["reproj_px"]), float(p["max_pose_distance"]), float(p["min_pose_difference"]),
                       float(p["max_pose_difference"]), int(p["seed"]) & 0xFFFFFFFF, 0)
        mc = np.zeros(co, np.int32); mq = np.zeros(co, np.int32); md = np.zeros(co, np.int32); mi = np.zeros(co, np.uint8)
        self._chk(self.L.svslam_loop_verify_batch(self.h, n, arr, C.byref(P), co, _p(DC), _p(XC), _p(HX), qo, _p(DQ), _p(UV),
                                                  _p(mc), _p(mq), _p(md), _p(mi)), "loop_verify")
        out = []
        for j in arr:
            s = slice(j.c_ofs, j.c_ofs + j.n_matches)
            out.append(dict(status=j.status, n_matches=j.n_matches, n_points=j.n_points, n_inliers=j.n_inliers,
                            need_correction=bool(j.need_correction), T_corr=np.array(j.T_corr), T_rel=np.array(j.T_rel), d=j.d,
                            matches=np.stack([mc[s], mq[s], md[s], mi[s]], axis=1).astype(np.int64)))
        return out

    # ---- loop-closure descriptors ------------------------------------------------
    def brief_default_pattern(self):
        """the library's default table of 256 tests, [256, 4] int8 = x0, y0, x1, y1 (svslam_brief_default_pattern)"""
        out = np.zeros((256, 4), np.int8)
        if self.L.svslam_brief_default_pattern(_p(out)) != 0:
            raise RuntimeError("brief_default_pattern failed")
        return out

    def brief_describe(self, jobs, xy=None, pattern=None, angle_deg=-1.0, edge=31):
        """BRIEF-256 at points of level 0 of pyramid slots, all jobs in one call (svslam_brief_describe_batch).
        jobs: list of (slot, xy [n, 2]) with xy=None, or list of (slot, pt_ofs, npts) into the shared array xy [total, 2].
        pattern: [256, 4] int8 or None for the default table.
        returns per job (desc [n_desc, 32] u8, desc_pt [n_desc] int32 = index of the row's point inside the job, n_desc)."""
        n = len(jobs)
        arr = (BriefJob * n)()
        if xy is None:
            parts, o = [], 0
            for i, (slot, pts) in enumerate(jobs):
                pts = _f32(pts, 2)
                arr[i].slot, arr[i].pt_ofs, arr[i].npts = int(slot), o, len(pts)
                o += len(pts); parts.append(pts)
            XY = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2), np.float32)
        else:
            XY = _f32(xy, 2)
            for i, (slot, ofs, npts) in enumerate(jobs):
                arr[i].slot, arr[i].pt_ofs, arr[i].npts = int(slot), int(ofs), int(npts)
        total = len(XY)
        pat = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, np.int8)
            if pat.size != 1024:
                raise ValueError("brief_describe: the table has %d entries, not 256 x 4" % pat.size)
        P = BriefParams(pat.ctypes.data if pat is not None else None, float(angle_deg), int(edge))
        desc = np.zeros((total, 32), np.uint8); dpt = np.zeros(total, np.int32)
        self._chk(self.L.svslam_brief_describe_batch(self.h, n, arr, C.byref(P), total, _p(XY), _p(desc), _p(dpt)), "brief_describe")
        return [(desc[j.pt_ofs:j.pt_ofs + j.n_desc].copy(), dpt[j.pt_ofs:j.pt_ofs + j.n_desc].copy(), j.n_desc) for j in arr]

    # ---- ORB detector --------------------------------------------------------------
    def orb_detect(self, jobs, max_out=2000, nfeatures=0, nlevels=0, fast_threshold=0, edge=0):
        """ORB keypoints of level 0 of pyramid slots, all jobs in one call (svslam_orb_detect_batch).
        jobs: list of (slot, rect_xy [n, 2] or None), the rects being the centres of the existing features (as for gftt).
        A parameter of 0 is ORB's default (500, 8, 20, 31).
        returns per job (keypoints, n_found): a structured array (ORB_KP) of the first min(n_found, max_out) keypoints, level
        ascending and row-major inside a level, and the count the rules give."""
        n = len(jobs)
        arr = (OrbJob * max(n, 1))()
        rects, ofs = [], 0
        for i, (slot, r) in enumerate(jobs):
            r = np.zeros((0, 2), np.float32) if r is None else _f32(r, 2)
            arr[i].slot, arr[i].rect_ofs, arr[i].nrect = int(slot), ofs, r.shape[0]
            ofs += r.shape[0]
            rects.append(r)
        rect = np.ascontiguousarray(np.concatenate(rects)) if ofs else np.zeros((1, 2), np.float32)
        out = np.zeros((max(n, 1), max(int(max_out), 1)), ORB_KP)
        P = OrbParams(int(nfeatures), int(nlevels), int(fast_threshold), int(edge))
        self._chk(self.L.svslam_orb_detect_batch(self.h, n, arr, C.byref(P), ofs, _p(rect), int(max_out), _p(out)), "orb_detect")
        return [(out[i, :arr[i].n_out].copy(), int(arr[i].n_found)) for i in range(n)]

    def orb_read_level(self, job, level):
        """test hook: (image, mask) of a pyramid level of a job of the last orb_detect call (svslam_orb_read_level)"""
        w, h = C.c_int(0), C.c_int(0)
        self._chk(self.L.svslam_orb_read_level(self.h, int(job), int(level), None, None, C.byref(w), C.byref(h)), "orb_read_level")
        img = np.zeros((h.value, w.value), np.uint8); mask = np.zeros((h.value, w.value), np.uint8)
        self._chk(self.L.svslam_orb_read_level(self.h, int(job), int(level), _p(img), _p(mask), C.byref(w), C.byref(h)), "orb_read_level")
        return img, mask

    def orb_describe(self, jobs, pattern=None, edge=0, nlevels=0):
        """ORB descriptors at keypoints of pyramid slots, each at its own angle and octave, all jobs in one call
        (svslam_orb_describe_batch).  jobs: list of (slot, keypoints), keypoints a structured array (ORB_KP, what orb_detect
        returns) or rows of (x, y, angle, octave).  pattern: [256, 4] int8 or None for the default table; edge, nlevels 0: 31, 8.
        returns per job (desc [n_desc, 32] u8, desc_pt [n_desc] int32 = index of the row's point inside the job, n_desc)."""
        n = len(jobs)
        arr = (OrbDescJob * max(n, 1))()
        parts, o = [], 0
        for i, (slot, kp) in enumerate(jobs):
            kp = orb_keypoints(kp)
            arr[i].slot, arr[i].pt_ofs, arr[i].npts = int(slot), o, len(kp)
            o += len(kp); parts.append(kp)
        KP = np.ascontiguousarray(np.concatenate(parts)) if o else np.zeros(1, ORB_KP)
        pat = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, np.int8)
            if pat.size != 1024:
                raise ValueError("orb_describe: the table has %d entries, not 256 x 4" % pat.size)
        P = OrbDescParams(pat.ctypes.data if pat is not None else None, int(edge), int(nlevels), 0)
        desc = np.zeros((max(o, 1), 32), np.uint8); dpt = np.zeros(max(o, 1), np.int32)
        self._chk(self.L.svslam_orb_describe_batch(self.h, n, arr, C.byref(P), o, _p(KP), _p(desc), _p(dpt)), "orb_describe")
        return [(desc[j.pt_ofs:j.pt_ofs + j.n_desc].copy(), dpt[j.pt_ofs:j.pt_ofs + j.n_desc].copy(), j.n_desc) for j in arr[:n]]

    # ---- loop candidate search ---------------------------------------------------
    def loopdb_configure(self, nstreams, capacity, dim=1280):
        """allocate (or re-allocate) and empty the context's store of global descriptors (svslam_loopdb_configure)"""
        self._chk(self.L.svslam_loopdb_configure(self.h, int(nstreams), int(capacity), int(dim)), "loopdb_configure")
        self._lc_dim = int(dim)

    def _lc_vecs(self, vecs, n, what):
        dim = getattr(self, "_lc_dim", None)
        if dim is None:
            raise RuntimeError("%s: the store is not configured" % what)
        v = np.ascontiguousarray(vecs, np.float32).reshape(-1, dim) if n else np.zeros((0, dim), np.float32)
        if len(v) != n:
            raise ValueError("%s: %d vectors of %d floats for %d rows" % (what, len(v), dim, n))
        return v

    def loopdb_append(self, streams, kf_ids, vecs):
        """normalise and append vecs [n, dim]: row i to streams[i] under kf_ids[i] (svslam_loopdb_append_batch); refused as a whole"""
        s = np.ascontiguousarray(streams, np.int32).reshape(-1); k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        if len(s) != len(k):
            raise ValueError("loopdb_append: %d streams and %d ids" % (len(s), len(k)))
        v = self._lc_vecs(vecs, len(s), "loopdb_append")
        self._chk(self.L.svslam_loopdb_append_batch(self.h, len(s), _p(s), _p(k), _p(v)), "loopdb_append")

    def loop_candidates(self, jobs, vecs, **params):
        """LoopClosure::LoopKeyframeCandidate for one keyframe per stream, all in one call (svslam_loop_candidates_batch).
        jobs: [(stream, kf_id)], streams ascending; vecs [njobs, dim] raw global descriptors.
        params: weak, strong, max_num_weak, min_gap (LC_DEFAULTS).
        returns a list of dicts: status (index into LC_STATUS), cand_kf, best_sim, best_kf, n_weak, n_compared."""
        unknown = set(params) - set(LC_DEFAULTS)
        if unknown:
            raise TypeError("loop_candidates: unknown parameter(s) %s" % sorted(unknown))
        p = dict(LC_DEFAULTS); p.update(params)
        n = len(jobs)
        arr = (LcJob * max(n, 1))()
        for i, (s, k) in enumerate(jobs):
            arr[i].stream, arr[i].kf_id = int(s), int(k)
        v = self._lc_vecs(vecs, n, "loop_candidates") if n else np.zeros((0, 1), np.float32)
        P = LcParams(float(p["weak"]), float(p["strong"]), int(p["max_num_weak"]), int(p["min_gap"]))
        self._chk(self.L.svslam_loop_candidates_batch(self.h, n, arr, C.byref(P), _p(v)), "loop_candidates")
        return [dict(status=arr[i].status, cand_kf=arr[i].cand_kf, best_sim=np.float32(arr[i].best_sim), best_kf=arr[i].best_kf,
                     n_weak=arr[i].n_weak, n_compared=arr[i].n_compared) for i in range(n)]

    def loopdb_count(self, stream):
        n = C.c_int(0)
        self._chk(self.L.svslam_loopdb_count(self.h, int(stream), C.byref(n)), "loopdb_count")
        return n.value

    def loopdb_read(self, stream):
        """(kf_ids [n] int32, rows [n, dim] float32): what a stream holds, normalised (svslam_loopdb_read)"""
        n = self.loopdb_count(stream)
        ids = np.zeros(n, np.int32); rows = np.zeros((n, self._lc_dim), np.float32)
        self._chk(self.L.svslam_loopdb_read(self.h, int(stream), n, _p(ids), _p(rows)), "loopdb_read")
        return ids, rows

    # ---- global image descriptor -------------------------------------------------
    def gdesc_configure(self, layers, params, prep=None):
        """configure the context's descriptor network (svslam_gdesc_configure).  layers: [(op, cin, cout, stride, relu6, add_from)]
        (gdesc.mobilenet_v2_layers() is the reference's); params: the weights and biases, one f32 array in table order;
        prep: None for the reference's call or a dict over GD_PREP_DEFAULTS"""
        arr = gd_layer_array(layers)
        prm = np.ascontiguousarray(params, np.float32).reshape(-1)
        P = gd_prep_struct(prep)
        self._chk(self.L.svslam_gdesc_configure(self.h, len(layers), C.cast(arr, C.c_void_p), _p(prm), prm.size,
                                                C.cast(C.pointer(P), C.c_void_p) if P is not None else None), "gdesc_configure")

    def gdesc_dim(self):
        """floats per descriptor, 0 while no network is configured (svslam_gdesc_dim)"""
        return int(self.L.svslam_gdesc_dim(self.h))

    def gdesc_describe(self, slots):
        """the raw descriptors [n, dim] f32 of level 0 of the given pyramid slots, all in one call (svslam_gdesc_describe_batch)"""
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros((len(sl), max(self.gdesc_dim(), 1)), np.float32)
        self._chk(self.L.svslam_gdesc_describe_batch(self.h, len(sl), _p(sl), _p(out)), "gdesc_describe")
        return out[:, :self.gdesc_dim()] if self.gdesc_dim() else out[:, :0]

    # ---- shared-map BA (one rank's shard; the LM driver is shared_ba.py) ---------
    def sba_open(self, cam_l, ext_l, cam_r, ext_r, poses, pts, okf, olm, ori, ouv, huber_delta=5.991):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7); pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        okf = np.ascontiguousarray(okf, np.int32); olm = np.ascontiguousarray(olm, np.int32)
        ori = np.ascontiguousarray(ori, np.uint8); ouv = _f32(ouv, 2)
        self._sba = (poses.shape[0], pts.shape[0], okf.shape[0])
        self._chk(self.L.svslam_sba_open(self.h, _p(_d(cam_l)), _p(_d(ext_l)), _p(_d(cam_r)), _p(_d(ext_r)), poses.shape[0], _p(poses),
                                         pts.shape[0], _p(pts), okf.shape[0], _p(okf), _p(olm), _p(ori), _p(ouv),
                                         C.c_double(huber_delta)), "sba_open")
        return self.L.svslam_sba_io_doubles(poses.shape[0])

    def sba_phase(self, phase, lam, io):
        self._chk(self.L.svslam_sba_phase(self.h, phase, C.c_double(lam), _p(io)), "sba_phase")
        return io

    def sba_comm_init(self, nranks, rank, id128):
        """RCCL communicator of this context's rank for svslam_sba_solve (id128: sba_comm_unique_id() of rank 0)"""
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(self.L.svslam_sba_comm_init(self.h, nranks, rank, buf), "sba_comm_init")

    def sba_comm_destroy(self):
        self._chk(self.L.svslam_sba_comm_destroy(self.h), "sba_comm_destroy")

    def sba_solve(self, iters=10):
        """the LM loop of the open shard inside the library (svslam_sba_solve): returns (iterations, lambda,
        trace[ntrials, 6], stats dict)"""
        it = C.c_int(0); lam = C.c_double(0); nt = C.c_int(0)
        cap = 10 * max(iters, 1) + 2
        tr = np.zeros((cap, 6)); st = np.zeros(4)
        self._chk(self.L.svslam_sba_solve(self.h, iters, C.byref(it), C.byref(lam), _p(tr), cap, C.byref(nt), _p(st)), "sba_solve")
        return it.value, lam.value, tr[:nt.value].copy(), dict(trials=int(st[0]), ms=float(st[1]), ms_per_trial=float(st[2]),
                                                                 allreduce_bytes_per_trial=int(st[3]))

    def sba_close(self):
        nkf, nlm, nobs = self._sba
        poses = np.zeros((nkf, 7)); pts = np.zeros((nlm, 3)); chi2 = np.zeros(max(nobs, 1))
        self._chk(self.L.svslam_sba_close(self.h, _p(poses), _p(pts), _p(chi2)), "sba_close")
        return poses, pts, chi2[:nobs]

    def dmap_read(self, stream, max_kf, max_lm):
        """test hook: one stream's device-resident window and landmark arena (svslam_dmap_read)"""
        d = dict(kf_frame=np.zeros(max_kf, np.int64), kf_id=np.zeros(max_kf, np.int32), kf_pose=np.zeros((max_kf, 7)),
                 kf_n=np.zeros(max_kf, np.int32), lm_id=np.zeros(max_lm, np.int32), lm_pos=np.zeros((max_lm, 3)),
                 lm_obs=np.zeros(max_lm, np.int32), lm_state=np.zeros(max_lm, np.uint8))
        self._chk(self.L.svslam_dmap_read(self.h, stream, _p(d["kf_frame"]), _p(d["kf_id"]), _p(d["kf_pose"]), _p(d["kf_n"]),
                                          _p(d["lm_id"]), _p(d["lm_pos"]), _p(d["lm_obs"]), _p(d["lm_state"])), "dmap_read")
        return d

    def dmap_state_shapes(self):
        KW, NF, NL = self.lim.max_kf, self.lim.max_pts, self.lim.max_lm
        dims = {"K": (KW,), "K7": (KW, 7), "KF": (KW, NF), "KF2": (KW, NF, 2), "L": (NL,), "L3": (NL, 3), "1": (1,)}
        return {name: (dt, dims[sh]) for name, dt, sh in DMAP_STATE_FIELDS}

    def _dmap_state(self, arrays):
        st = DmapState()
        for name, (dt, shape) in self.dmap_state_shapes().items():
            a = arrays[name]
            if a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("dmap state: %s must be a contiguous %s array of shape %s" % (name, np.dtype(dt).name, shape))
            setattr(st, name, a.ctypes.data)
        return st

    def dmap_state_read(self, stream):
        """test hook: every array of one stream's device-resident map (svslam_debug_dmap_read), a dict by the header's names"""
        d = {name: np.zeros(shape, dt) for name, (dt, shape) in self.dmap_state_shapes().items()}
        self._chk(self.L.svslam_debug_dmap_read(self.h, stream, C.byref(self._dmap_state(d))), "debug_dmap_read")
        return d

    def dmap_state_write(self, stream, arrays):
        """test hook: seeds one stream's device-resident map (svslam_debug_dmap_write) from a dict as dmap_state_read returns it"""
        self._chk(self.L.svslam_debug_dmap_write(self.h, stream, C.byref(self._dmap_state(arrays))), "debug_dmap_write")

    def rtrack_read(self, stream):
        """test hook: the resident feature list of a stream, max_pts entries (svslam_debug_rtrack_read)"""
        n = self.lim.max_pts
        xy = np.zeros((n, 2), np.float32); mp = np.zeros(n, np.int32); xyz = np.zeros((n, 3))
        self._chk(self.L.svslam_debug_rtrack_read(self.h, stream, _p(xy), _p(mp), _p(xyz)), "debug_rtrack_read")
        return xy, mp, xyz

    def dmap_stage(self, stage, jobs, arrays=None, **scalars):
        """test hook: one kernel of the keyframe path alone (svslam_debug_dmap_stage).  jobs: a ctypes array of DmapJob, updated in
        place; arrays: {member of svslam_dmap_stage_io: contiguous numpy array of the header's size}, updated in place; scalars: its
        int / double members (cam_r: four doubles)."""
        io = DmapStageIO()
        for k, v in scalars.items():
            if k == "cam_r":
                io.cam_r = (C.c_double * 4)(*[float(x) for x in v])
            else:
                setattr(io, k, v)
        n, NF, NL = len(jobs), self.lim.max_pts, self.lim.max_lm
        P, E, MK = n * NF, n * max(io.max_obs, 1), io.max_kf
        nbytes = dict(evicted=16 * n * io.ev_quota, ev_cursor=4, corners=8 * n * io.max_corners, ncorners=4 * n, lkjobs=16 * n, prev_xy=8 * P,
                      next_xy=8 * P, status=P, trijobs=C.sizeof(TriJob) * n, uv_l=8 * P, uv_r=8 * P, tri_idx=4 * P, tri_xyz=24 * P, tri_ok=P,
                      badev=4 * DMAP_BADEV_INTS * n, poses=56 * n * MK, pts=24 * n * NL, packed=4 * E, uv=8 * E, edge_ref=4 * E,
                      lm_slot_of=4 * n * NL, chi2=8 * E)
        for k, a in (arrays or {}).items():
            if not a.flags.c_contiguous or a.nbytes != nbytes[k]:
                raise ValueError("dmap_stage: %s must be contiguous and hold %d bytes, not %d" % (k, nbytes[k], a.nbytes))
            setattr(io, k, a.ctypes.data)
        self._chk(self.L.svslam_debug_dmap_stage(self.h, DMAP_STAGES[stage], len(jobs), jobs, C.byref(io)), "debug_dmap_stage(%s)" % stage)

    # ---- resident tracking -----------------------------------------------------
    def rtrack_upload(self, lists):
        """lists: [(stream, xy[n,2], mp[n], xyz[n,3])] -> replaces the resident feature lists"""
        n = len(lists)
        streams = (C.c_int * n)(*[l[0] for l in lists])
        cnt = [len(l[2]) for l in lists]
        ofs = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32) if n else np.zeros(0, np.int32)
        xy = np.ascontiguousarray(np.concatenate([_f32(l[1], 2) for l in lists]))
        mp = np.ascontiguousarray(np.concatenate([np.asarray(l[2], np.int32) for l in lists]))
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(l[3], np.float64).reshape(-1, 3) for l in lists]))
        self._chk(self.L.svslam_rtrack_upload(self.h, n, streams, _p(ofs), (C.c_int * n)(*cnt), _p(xy), _p(mp), _p(xyz)),
                  "rtrack_upload")

    def rtrack(self, jobs, cam, params=None, chi2_th=5.991):
        """jobs: [(stream, prev_slot, next_slot, next_img, pose[7], T_cam_w[7], npts)].
        returns list of dict(xy, mp, pose, n_tracked, n_edges, n_outlier)."""
        n = len(jobs)
        arr = (RtrackJob * n)()
        ofs, keep = 0, []
        for i, (sid, ps, ns, img, T, Tc, npts) in enumerate(jobs):
            arr[i] = RtrackJob(sid, ps, ns, ofs, npts, (C.c_double * 7)(*_d(T)), (C.c_double * 7)(*_d(Tc)), 0, 0, 0, 0)
            ofs += npts
            keep.append(np.ascontiguousarray(img, np.uint8))
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in keep]); st = (C.c_int * n)(*[im.shape[1] for im in keep])
        xy = np.zeros((max(ofs, 1), 2), np.float32); mp = np.zeros(max(ofs, 1), np.int32)
        prm = params or LkParams(3, 30, 0.01, 1e-4, 1)
        self._chk(self.L.svslam_rtrack_batch(self.h, n, arr, ptrs, st, 0, ofs, _p(_d(cam)), _p(xy), _p(mp), C.byref(prm),
                                             C.c_double(chi2_th)), "rtrack")
        out = []
        for j in arr:
            s = slice(j.pt_ofs, j.pt_ofs + j.n_tracked)
            out.append(dict(xy=xy[s].copy(), mp=mp[s].copy(), pose=np.array(list(j.pose)), n_tracked=j.n_tracked,
                            n_edges=j.n_edges, n_outlier=j.n_outlier))
        return out

    # ---- fused tracking --------------------------------------------------------
    def track(self, jobs, cam, params=None, chi2_th=5.991, device=False):
        """jobs: list of (prev_slot, next_slot, next_img, pose[7], prev_xy, guess_xy, has_mp, xyz).
        returns list of dict(next_xy, status, outlier, pose, n_tracked, n_inlier)."""
        n = len(jobs)
        arr = (TrackJob * n)()
        keep, prevs, nexts, mps, xs, ofs = [], [], [], [], [], 0
        for i, (ps, ns, img, T, p, q, mp, xyz) in enumerate(jobs):
            p = _f32(p, 2); q = _f32(q, 2)
            arr[i] = TrackJob(ps, ns, ofs, p.shape[0], (C.c_double * 7)(*_d(T)), 0, 0)
            ofs += p.shape[0]
            prevs.append(p); nexts.append(q)
            mps.append(np.ascontiguousarray(mp, np.uint8)); xs.append(np.ascontiguousarray(xyz, np.float64).reshape(-1, 3))
            keep.append(img if device else np.ascontiguousarray(img, np.uint8))
        if device:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in keep]); st = (C.c_int * n)(*[self.width] * n)
        else:
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in keep]); st = (C.c_int * n)(*[im.shape[1] for im in keep])
        prev = np.ascontiguousarray(np.concatenate(prevs)); nxt = np.ascontiguousarray(np.concatenate(nexts)).copy()
        mp = np.ascontiguousarray(np.concatenate(mps)); X = np.ascontiguousarray(np.concatenate(xs))
        status = np.zeros(max(ofs, 1), np.uint8); outl = np.zeros(max(ofs, 1), np.uint8)
        prm = params or LkParams(3, 30, 0.01, 1e-4, 1)
        self._chk(self.L.svslam_track_batch(self.h, n, arr, ptrs, st, 1 if device else 0, ofs, _p(_d(cam)), _p(prev),
                                            _p(nxt), _p(mp), _p(X), _p(status), _p(outl), C.byref(prm),
                                            C.c_double(chi2_th)), "track_batch")
        out = []
        for j in arr:
            s = slice(j.pt_ofs, j.pt_ofs + j.npts)
            out.append(dict(next_xy=nxt[s].copy(), status=status[s].copy(), outlier=outl[s].copy(),
                            pose=np.array(j.pose[:]), n_tracked=j.n_tracked, n_inlier=j.n_inlier))
        return out


# ---- synthetic stream (CPU generator; HIP generator is in libsvslam_hip.so) ----
class SynthView(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("R", C.c_float * 9), ("C", C.c_double * 3), ("seed", C.c_uint32), ("noise_seed", C.c_uint32),
                ("scale", C.c_float)]


KITTI00_HALF_CAM = (718.856 * 0.5, 718.856 * 0.5, 607.1928 * 0.5, 185.2157 * 0.5)
KITTI00_BASELINE = 0.537166
_synth = None


def sba_comm_unique_id():
    """the 128-byte RCCL id rank 0 hands to every rank (svslam_sba_comm_unique_id)"""
    buf = (C.c_char * 128)()
    if load().svslam_sba_comm_unique_id(buf) != 0:
        raise RuntimeError("svslam_sba_comm_unique_id failed (librccl.so missing?)")
    return bytes(buf.raw)


def synth_lib():
    global _synth
    if _synth is None:
        p = os.path.join(LIB_DIR, "libsvslam_synth.so")
        if not os.path.exists(p):
            _build.build_synth()
        _synth = C.CDLL(p)
    return _synth


def synth_pair(seed, frame, w=620, h=188, cam=KITTI00_HALF_CAM, baseline=KITTI00_BASELINE):
    left = np.zeros((h, w), np.uint8); right = np.zeros((h, w), np.uint8)
    camv = (C.c_double * 4)(*cam)
    synth_lib().svs_synth_render_pair(C.c_uint32(seed), frame, w, h, camv, C.c_double(baseline), _p(left), _p(right), w)
    return left, right


def synth_gt(seed, frame):
    T = np.zeros(7)
    synth_lib().svs_synth_gt(C.c_uint32(seed), frame, _p(T))
    return T


def synth_views(seed, frame, cam=KITTI00_HALF_CAM, baseline=KITTI00_BASELINE):
    vl, vr = SynthView(), SynthView()
    camv = (C.c_double * 4)(*cam)
    synth_lib().svs_synth_make_views(C.c_uint32(seed), frame, camv, C.c_double(baseline), C.byref(vl), C.byref(vr))
    return vl, vr


def synth_render_streams_device(seeds, frame0, nframes, w, h, d_left, d_right, device=0, cam=KITTI00_HALF_CAM,
                                baseline=KITTI00_BASELINE, block=4096, sampled=False):
    """render frames [frame0, frame0 + nframes) of every stream in `seeds` into the device buffers
    d_left / d_right, laid out [stream][nframes][h*w]; a few launches per `block` images.  sampled: only the pixels
    (2x, 2y), each replicated into its 2x2 block — for full-size frames that the pipeline decimates by 1/2 (src_width /
    src_height), whose results are then bit-identical to those of a full render, at a quarter of the rendering work."""
    n = len(seeds)
    render = load().svslam_synth_render_batch_sampled if sampled else load().svslam_synth_render_batch
    per = max(1, block // max(nframes, 1))            # streams per launch
    camv = (C.c_double * 4)(*cam)
    img = w * h
    for s0 in range(0, n, per):
        m = min(per, n - s0)
        sd = (C.c_uint32 * m)(*[int(x) & 0xFFFFFFFF for x in seeds[s0:s0 + m]])
        vl = (SynthView * (m * nframes))(); vr = (SynthView * (m * nframes))()
        synth_lib().svs_synth_make_views_batch(m, sd, frame0, nframes, camv, C.c_double(baseline), vl, vr)
        for arr, base in ((vl, d_left), (vr, d_right)):
            rc = render(device, m * nframes, arr, w, h, C.c_void_p(base + s0 * nframes * img))
            if rc != 0:
                raise RuntimeError("svslam_synth_render_batch failed (%d)" % rc)


def synth_render_device(views, w, h, d_out, device=0):
    """render len(views) images into the device buffer d_out (tight w*h each)."""
    n = len(views)
    arr = (SynthView * n)(*views)
    rc = load().svslam_synth_render_batch(device, n, arr, w, h, C.c_void_p(d_out))
    if rc != 0:
        raise RuntimeError("svslam_synth_render_batch failed (%d)" % rc)
