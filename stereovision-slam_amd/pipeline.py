"""ctypes binding of the C++ host pipeline (lib/libsvslam_pipeline.so): the
reference's Frontend/Backend/Map logic driving the HIP kernels, S streams in
lockstep.  `lib` may be overridden by tests with the CPU twin built under
oracle/ (same C API, oracle kernels) — the product never does that."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class PipeConfig(C.Structure):
    _fields_ = [("num_features", C.c_int), ("num_features_init", C.c_int), ("num_features_tracking", C.c_int),
                ("num_features_tracking_bad", C.c_int), ("num_features_needed_for_keyframe", C.c_int),
                ("max_triangulation_depth", C.c_double), ("num_active_keyframes", C.c_int), ("backend_on", C.c_int),
                ("chi2_th", C.c_double), ("width", C.c_int), ("height", C.c_int), ("cam_l", C.c_double * 4),
                ("ext_l", C.c_double * 7), ("cam_r", C.c_double * 4), ("ext_r", C.c_double * 7),
                ("max_lm", C.c_int), ("max_obs", C.c_int), ("host_threads", C.c_int),
                ("src_width", C.c_int), ("src_height", C.c_int), ("resident_track", C.c_int),
                ("low_latency", C.c_int), ("max_pts", C.c_int), ("device_map", C.c_int), ("backend_lag", C.c_int)]


class FrameResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("status", C.c_int), ("is_keyframe", C.c_int), ("n_features", C.c_int),
                ("n_inliers", C.c_int), ("frame_id", C.c_longlong), ("keyframe_id", C.c_longlong)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in
                ("frames", "keyframes", "track_pts", "pose_edges", "gftt_calls", "gftt_rects", "corners", "right_pts",
                 "tri_pts", "ba_calls", "ba_edges", "ba_kf", "ba_lm", "ba_iters", "pyr_left", "pyr_right", "ns_step",
                 "ns_kernel_calls", "corners_dropped", "ba_skipped", "ba_pairs", "ba_trials", "lm_total", "lm_resident", "lm_full")]


RESULT_DTYPE = np.dtype([("pose", np.float64, 7), ("status", np.int32), ("is_keyframe", np.int32),
                         ("n_features", np.int32), ("n_inliers", np.int32), ("frame_id", np.int64),
                         ("keyframe_id", np.int64)])
assert RESULT_DTYPE.itemsize == C.sizeof(FrameResult)


def tune_allocator(lib=None):
    """process-wide malloc settings for many-stream hosts (svs_pipe_tune_allocator)"""
    (_bind(lib) if lib is not None else product_lib()).svs_pipe_tune_allocator()


def default_config(width=620, height=188, cam=(359.428, 359.428, 303.5964, 92.60785), baseline=0.537166, **kw):
    """config/stereo_slam_configs/config-00.yaml of the reference + KITTI-00 halved calibration"""
    c = PipeConfig()
    c.num_features = 150; c.num_features_init = 50; c.num_features_tracking = 50
    c.num_features_tracking_bad = 20; c.num_features_needed_for_keyframe = 80
    c.max_triangulation_depth = 300.0; c.num_active_keyframes = 10; c.backend_on = 1; c.chi2_th = 5.991
    c.width = width; c.height = height
    c.cam_l = (C.c_double * 4)(*cam); c.cam_r = (C.c_double * 4)(*cam)
    c.ext_l = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    c.ext_r = (C.c_double * 7)(0, 0, 0, 1, -baseline, 0, 0)
    c.max_lm = 4096; c.max_obs = 16384; c.host_threads = 1
    c.src_width = 0; c.src_height = 0; c.resident_track = 1; c.low_latency = 0; c.max_pts = 512; c.device_map = 0; c.backend_lag = 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def load_yaml_config(path, **kw):
    """reads the scalar keys of a reference stereo_slam_configs/*.yaml (OpenCV FileStorage subset)"""
    vals = {}
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line or line.startswith("%") or ":" not in line:
                continue
            k, v = line.split(":", 1)
            vals[k.strip()] = v.strip()
    c = default_config(**kw)
    for k in ("num_features", "num_features_init", "num_features_tracking", "num_features_tracking_bad",
              "num_features_needed_for_keyframe", "num_active_keyframes", "backend_on"):
        if k in vals:
            setattr(c, k, int(float(vals[k])))
    for k in ("max_triangulation_depth", "chi2_th"):
        if k in vals:
            setattr(c, k, float(vals[k]))
    return c


class LoopQuery(C.Structure):
    _fields_ = [("stream", C.c_int), ("kf_id", C.c_longlong), ("cand_kf_id", C.c_longlong), ("n_desc_q", C.c_int), ("n_idx_q", C.c_int),
                ("desc_q", C.c_void_p), ("feat_q", C.c_void_p), ("n_desc_c", C.c_int), ("n_idx_c", C.c_int), ("desc_c", C.c_void_p),
                ("feat_c", C.c_void_p)]


class LoopResult(C.Structure):
    _fields_ = [("status", C.c_int), ("n_matches", C.c_int), ("n_points", C.c_int), ("n_inliers", C.c_int), ("need_correction", C.c_int),
                ("reserved", C.c_int), ("T_corr", C.c_double * 7), ("T_rel", C.c_double * 7), ("d", C.c_double)]


class LoopPair(C.Structure):
    _fields_ = [("stream", C.c_int), ("kf_id", C.c_longlong), ("cand_kf_id", C.c_longlong)]


class LoopDetectParams(C.Structure):
    _fields_ = [("weak", C.c_float), ("strong", C.c_float), ("max_num_weak", C.c_int), ("min_gap", C.c_int),
                ("keyframes_to_ignore_after_loop", C.c_longlong)]


class LoopDetection(C.Structure):
    _fields_ = [("is_keyframe", C.c_int), ("skipped", C.c_int), ("searched", C.c_int), ("verified", C.c_int), ("stored", C.c_int),
                ("reserved", C.c_int), ("kf_id", C.c_longlong), ("cand_status", C.c_int), ("cand_kf", C.c_int), ("best_kf", C.c_int),
                ("n_weak", C.c_int), ("n_compared", C.c_int), ("best_sim", C.c_float), ("loop", LoopResult)]


class FusionJob(C.Structure):
    _fields_ = [("stream", C.c_int), ("npairs", C.c_int), ("kf_id", C.c_longlong), ("cand_kf_id", C.c_longlong), ("pair_ofs", C.c_longlong),
                ("T_corr", C.c_double * 7)]


class FusionStats(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("fused", "nkf", "npt", "n_unanchored", "pairs", "merged", "revived", "repointed", "same_deleted", "reserved")]


def _fusion_dict(r):
    return {k: getattr(r, k) for k, _ in FusionStats._fields_ if k not in ("fused", "reserved")}


def _bind(L):
    L.svs_pipe_create.restype = C.c_void_p
    L.svs_pipe_create.argtypes = [C.POINTER(PipeConfig), C.c_int, C.c_int]
    L.svs_pipe_destroy.argtypes = [C.c_void_p]
    L.svs_pipe_destroy.restype = None
    L.svs_pipe_last_error.restype = C.c_char_p
    L.svs_pipe_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.svs_pipe_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int,
                                      C.c_int, C.c_void_p]
    L.svs_pipe_counters_get.argtypes = [C.c_void_p, C.POINTER(Counters)]
    L.svs_pipe_save_outputs.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    L.svs_pipe_flush.argtypes = [C.c_void_p]
    L.svs_pipe_map_snapshot.restype = C.c_longlong
    L.svs_pipe_map_snapshot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    L.svs_pipe_tune_allocator.restype = None
    L.svs_pipe_backend_ctx.restype = C.c_void_p
    L.svs_pipe_backend_ctx.argtypes = [C.c_void_p]
    L.svs_pipe_kernel_ctx.restype = C.c_void_p
    L.svs_pipe_kernel_ctx.argtypes = [C.c_void_p]
    if hasattr(L, "svs_pipe_set_detector"):
        L.svs_pipe_set_detector.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "svs_pipe_add_loop_edge"):        # product library only (the CPU twins have no pose-graph provider)
        L.svs_pipe_add_loop_edge.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
        L.svs_pipe_pose_graph_optimization.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(L, "svs_pipe_verify_loops"):
        L.svs_pipe_verify_loops.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svs_pipe_keep_keyframe_features.argtypes = [C.c_void_p, C.c_int]
        L.svs_pipe_keyframe_features.restype = C.c_longlong
        L.svs_pipe_keyframe_features.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
    if hasattr(L, "svs_pipe_describe_new_keyframes"):
        L.svs_pipe_describe_new_keyframes.argtypes = [C.c_void_p, C.c_void_p]
        L.svs_pipe_keyframe_descriptors.restype = C.c_longlong
        L.svs_pipe_keyframe_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong]
        L.svs_pipe_verify_loops_stored.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    if hasattr(L, "svs_pipe_describe_new_keyframes_oriented"):
        L.svs_pipe_describe_new_keyframes_oriented.argtypes = [C.c_void_p, C.c_void_p]
        L.svs_pipe_keyframe_keypoints.restype = C.c_longlong
        L.svs_pipe_keyframe_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong]
    if hasattr(L, "svs_pipe_detect_loops"):
        L.svs_pipe_loopdb_configure.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.svs_pipe_detect_loops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svs_pipe_loop_matches.restype = C.c_longlong
        if hasattr(L, "svs_pipe_gdesc_configure"):
            L.svs_pipe_gdesc_configure.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
            L.svs_pipe_gdesc_dim.argtypes = [C.c_void_p]
            L.svs_pipe_describe_global_new_keyframes.argtypes = [C.c_void_p, C.c_void_p]
        L.svs_pipe_loop_matches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.svs_pipe_loopdb_ids.restype = C.c_longlong
        L.svs_pipe_loopdb_ids.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.svs_pipe_last_closed_keyframe.restype = C.c_longlong
        L.svs_pipe_last_closed_keyframe.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "svs_pipe_local_fusion"):
        L.svs_pipe_local_fusion.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svs_pipe_detect_loops_fused.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.svs_pipe_all_landmarks.restype = C.c_longlong
        L.svs_pipe_all_landmarks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.svs_pipe_last_frame.restype = C.c_longlong
        L.svs_pipe_last_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


_product = None


def product_lib():
    global _product
    if _product is None:
        # always the product library next to this file (no environment override: the CPU twin under oracle/ has the same C
        # API and must never be loadable as the product; A/B scripts pass `lib=` to Pipeline explicitly)
        p = os.path.join(HERE, "lib", "libsvslam_pipeline.so")
        if not os.path.exists(p):
            raise RuntimeError("libsvslam_pipeline.so is missing: run stereovision-slam_amd/build.py")
        _product = _bind(C.CDLL(p))
    return _product


DETECTORS = {"GFTT": 0, "ORB": 1}


class Pipeline:
    def __init__(self, cfg=None, nstreams=1, device=0, lib=None, detector=None):
        """detector: None (GFTT, the setter is not called), "GFTT" or "ORB" (svs_pipe_set_detector; ORB: host map only)"""
        self.L = _bind(lib) if lib is not None else product_lib()
        self.cfg = cfg or default_config()
        self.n = nstreams
        self.h = self.L.svs_pipe_create(C.byref(self.cfg), nstreams, device)
        if not self.h:
            raise RuntimeError("svs_pipe_create failed: " + self.L.svs_pipe_last_error().decode())
        if detector is not None:
            try:
                self.set_detector(detector)
            except Exception:
                self.close()
                raise

    def set_detector(self, detector):
        """which detector DetectFeatures runs, before the first frame: "GFTT" / 0 or "ORB" / 1"""
        kind = DETECTORS[detector.upper()] if isinstance(detector, str) else int(detector)
        if self.L.svs_pipe_set_detector(self.h, kind) != 0:
            raise RuntimeError("svs_pipe_set_detector refused: " + self.L.svs_pipe_last_error().decode())

    def close(self):
        if self.h:
            self.L.svs_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, lefts, rights, device=False):
        """one frame per stream; lefts/rights: lists of np.uint8 images (or device pointers)"""
        n = self.n
        if device:
            lp = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in lefts])
            rp = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in rights])
        else:
            keep = [np.ascontiguousarray(a, np.uint8) for a in list(lefts) + list(rights)]
            lp = (C.c_void_p * n)(*[a.ctypes.data for a in keep[:n]])
            rp = (C.c_void_p * n)(*[a.ctypes.data for a in keep[n:]])
        out = np.zeros(n, RESULT_DTYPE)
        rc = self.L.svs_pipe_step(self.h, lp, rp, 1 if device else 0, out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError("svs_pipe_step failed: " + self.L.svs_pipe_last_error().decode())
        return out

    def run_device(self, left_base, right_base, stream_stride, frame_stride, first_frame, nframes, want_results=True, out=None):
        """out: a caller-owned [nframes, n] RESULT_DTYPE array to fill (e.g. allocated and touched ahead of a measurement)"""
        if out is not None:
            assert out.shape == (nframes, self.n) and out.dtype == RESULT_DTYPE and out.flags.c_contiguous
            want_results = True
        elif want_results:
            out = np.zeros((nframes, self.n), RESULT_DTYPE)
        rc = self.L.svs_pipe_run_device(self.h, C.c_void_p(left_base), C.c_void_p(right_base), stream_stride,
                                        frame_stride, first_frame, nframes,
                                        out.ctypes.data_as(C.c_void_p) if want_results else None)
        if rc != 0:
            raise RuntimeError("svs_pipe_run_device failed: " + self.L.svs_pipe_last_error().decode())
        return out

    def flush(self):
        """complete a backend optimisation that is still in flight (backend_on == 2)"""
        if self.L.svs_pipe_flush(self.h) != 0:
            raise RuntimeError("svs_pipe_flush failed: " + self.L.svs_pipe_last_error().decode())

    def counters(self):
        c = Counters()
        self.L.svs_pipe_counters_get(self.h, C.byref(c))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def save_outputs(self, stream, out_dir, dataset_dir="./data/dataset/sequences/00", left_cam_index=0):
        """keyframes.txt + landmarks.pcd in the reference's formats"""
        rc = self.L.svs_pipe_save_outputs(self.h, stream, out_dir.encode(), dataset_dir.encode(), left_cam_index)
        if rc != 0:
            raise RuntimeError("svs_pipe_save_outputs failed (%d)" % rc)

    def add_loop_edge(self, stream, kf_id, loop_kf_id, T_rel):
        """records that keyframe kf_id closes a loop with the older keyframe loop_kf_id; T_rel = T_kf * T_loop^-1 (double[7])"""
        T = np.ascontiguousarray(T_rel, np.float64).reshape(7)
        if self.L.svs_pipe_add_loop_edge(self.h, stream, C.c_longlong(kf_id), C.c_longlong(loop_kf_id), T.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("svs_pipe_add_loop_edge refused: " + self.L.svs_pipe_last_error().decode())

    def pose_graph_optimization(self, streams=None, iters=22):
        """LoopClosure::PoseGraphOptimization for the given streams (default: all) in one kernel call; returns one dict per stream
        (nkf, nedge, npt, iters, trials, chi2_before, chi2_after)"""
        ss = list(range(self.n)) if streams is None else list(streams)
        arr = (C.c_int * max(len(ss), 1))(*ss)
        st = np.zeros((max(len(ss), 1), 7))
        if self.L.svs_pipe_pose_graph_optimization(self.h, len(ss), arr, int(iters), st.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("svs_pipe_pose_graph_optimization failed: " + self.L.svs_pipe_last_error().decode())
        keys = ("nkf", "nedge", "npt", "iters", "trials")
        return [dict({k: int(r[i]) for i, k in enumerate(keys)}, chi2_before=float(r[5]), chi2_after=float(r[6])) for r in st[:len(ss)]]

    def keep_keyframe_features(self, on=True):
        """keyframes that leave the window from now on keep their feature lists (verify_loops reads the candidate keyframe's)"""
        self.L.svs_pipe_keep_keyframe_features(self.h, 1 if on else 0)

    def keyframe_features(self, stream, kf_id):
        """the left features of a keyframe, read-only (svs_pipe_keyframe_features): dict(xy [n, 2], mp [n] landmark id or -1,
        outlier [n], has_xyz [n], xyz [n, 3] — the landmark position verify_loops would gather — and pose[7])"""
        n = self.L.svs_pipe_keyframe_features(self.h, stream, C.c_longlong(kf_id), None, 0, None)
        if n < 0:
            raise RuntimeError("svs_pipe_keyframe_features refused: " + self.L.svs_pipe_last_error().decode())
        out = np.zeros((max(n, 1), 8)); pose = np.zeros(7)
        if self.L.svs_pipe_keyframe_features(self.h, stream, C.c_longlong(kf_id), out.ctypes.data_as(C.c_void_p), n, pose.ctypes.data_as(C.c_void_p)) != n:
            raise RuntimeError("svs_pipe_keyframe_features changed size between two calls")
        out = out[:n]
        return dict(xy=out[:, :2].astype(np.float32), mp=out[:, 2].astype(np.int64), outlier=out[:, 3] != 0, has_xyz=out[:, 4] != 0,
                    xyz=out[:, 5:8].copy(), pose=pose)

    def verify_loops(self, queries, **params):
        """LoopClosure::KeypointMatchWithLoopCandid + CalculatePose for every query in one kernel call (svs_pipe_verify_loops); every
        ACCEPTED pair is recorded as a loop edge for pose_graph_optimization.  queries: dicts with stream, kf_id, cand_kf_id, desc_q
        [nq, 32] u8 and feat_q [nq] (desc_feat_indx) of the keyframe, desc_c / feat_c of the older candidate keyframe.  params: as
        Context.loop_verify (LOOP_DEFAULTS).  Returns one dict per query: status, n_matches, n_points, n_inliers, need_correction,
        T_corr, T_rel, d, matches [n_matches, 4] (candidate row, current row, distance, inlier)."""
        import importlib
        _svs = importlib.import_module(__package__)          # LOOP_DEFAULTS, LoopParams: the binding of include/svslam.h
        unknown = set(params) - set(_svs.LOOP_DEFAULTS)
        if unknown:
            raise TypeError("verify_loops: unknown parameter(s) %s" % sorted(unknown))
        p = dict(_svs.LOOP_DEFAULTS); p.update(params)
        n = len(queries)
        qs = (LoopQuery * max(n, 1))()
        keep = []
        for i, q in enumerate(queries):
            a = [np.ascontiguousarray(q["desc_q"], np.uint8).reshape(-1, 32), np.ascontiguousarray(q["feat_q"], np.int32).reshape(-1),
                 np.ascontiguousarray(q["desc_c"], np.uint8).reshape(-1, 32), np.ascontiguousarray(q["feat_c"], np.int32).reshape(-1)]
            keep.append(a)
            qs[i] = LoopQuery(int(q["stream"]), int(q["kf_id"]), int(q["cand_kf_id"]), len(a[0]), len(a[1]), a[0].ctypes.data, a[1].ctypes.data,
                              len(a[2]), len(a[3]), a[2].ctypes.data, a[3].ctypes.data)
        P = _svs.LoopParams((C.c_double * 4)(), (C.c_double * 7)(), int(p["min_matches"]), int(p["ransac_iters"]), float(p["reproj_px"]),
                            float(p["max_pose_distance"]), float(p["min_pose_difference"]), float(p["max_pose_difference"]),
                            int(p["seed"]) & 0xFFFFFFFF, 0)
        res = (LoopResult * max(n, 1))()
        rows = sum(len(a[2]) for a in keep)
        m4 = np.zeros((max(rows, 1), 4), np.int32)
        if self.L.svs_pipe_verify_loops(self.h, n, qs, C.byref(P), res, m4.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("svs_pipe_verify_loops refused: " + self.L.svs_pipe_last_error().decode())
        out = []; row = 0
        for i in range(n):
            r = res[i]
            out.append(dict(status=r.status, n_matches=r.n_matches, n_points=r.n_points, n_inliers=r.n_inliers,
                            need_correction=bool(r.need_correction), T_corr=np.array(r.T_corr), T_rel=np.array(r.T_rel), d=r.d,
                            matches=m4[row:row + r.n_matches].astype(np.int64)))
            row += len(keep[i][2])
        return out

    def describe_new_keyframes(self, pattern=None, angle_deg=-1.0, edge=31, oriented=False, nlevels=0):
        """LoopClosure::ExtractKeypointsDescriptor for every stream whose last step made a keyframe (svs_pipe_describe_new_keyframes):
        BRIEF-256 at the keyframe's non-outlier left features, stored with the keyframe.  Call it after step() and before the next
        one.  pattern / angle_deg / edge: as Context.brief_describe.  Returns the number of keyframes described.
        oriented=True (svs_pipe_describe_new_keyframes_oriented): every feature at its own angle and octave, as Context.orb_describe
        (angle_deg is not used; nlevels 0 is 8)."""
        import importlib
        _svs = importlib.import_module(__package__)
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8)
        if pat is not None and pat.size != 1024:
            raise ValueError("describe_new_keyframes: the table has %d entries, not 256 x 4" % pat.size)
        if oriented:
            if not hasattr(self.L, "svs_pipe_describe_new_keyframes_oriented"):
                raise RuntimeError("describe_new_keyframes(oriented=True): this pipeline library has no oriented descriptors")
            P = _svs.OrbDescParams(None if pat is None else pat.ctypes.data, int(edge), int(nlevels), 0)
            n = self.L.svs_pipe_describe_new_keyframes_oriented(self.h, C.byref(P))
            if n < 0:
                raise RuntimeError("svs_pipe_describe_new_keyframes_oriented refused: " + self.L.svs_pipe_last_error().decode())
            return n
        P = _svs.BriefParams(None if pat is None else pat.ctypes.data, float(angle_deg), int(edge))
        n = self.L.svs_pipe_describe_new_keyframes(self.h, C.byref(P))
        if n < 0:
            raise RuntimeError("svs_pipe_describe_new_keyframes refused: " + self.L.svs_pipe_last_error().decode())
        return n

    def keyframe_keypoints(self, stream, kf_id):
        """x, y, angle, octave of every left feature of a keyframe (svs_pipe_keyframe_keypoints), [n, 4] f32 in the order of
        keyframe_features: what describe_new_keyframes(oriented=True) describes"""
        n = self.L.svs_pipe_keyframe_keypoints(self.h, int(stream), C.c_longlong(kf_id), None, 0)
        if n < 0:
            raise RuntimeError("svs_pipe_keyframe_keypoints refused: " + self.L.svs_pipe_last_error().decode())
        rows = np.zeros((n, 4), np.float32)
        if n and self.L.svs_pipe_keyframe_keypoints(self.h, int(stream), C.c_longlong(kf_id), rows.ctypes.data_as(C.c_void_p), n) != n:
            raise RuntimeError("svs_pipe_keyframe_keypoints changed size between two calls")
        return rows

    def keyframe_descriptors(self, stream, kf_id):
        """the stored descriptors of a keyframe (svs_pipe_keyframe_descriptors): desc [n, 32] u8 and feat [n] int32, the index of each
        row's feature in keyframe_features(stream, kf_id).  Raises for a keyframe that was never described."""
        n = self.L.svs_pipe_keyframe_descriptors(self.h, stream, C.c_longlong(kf_id), None, None, 0)
        if n < 0:
            raise RuntimeError("svs_pipe_keyframe_descriptors refused: " + self.L.svs_pipe_last_error().decode())
        desc = np.zeros((n, 32), np.uint8); feat = np.zeros(n, np.int32)
        if n and self.L.svs_pipe_keyframe_descriptors(self.h, stream, C.c_longlong(kf_id), desc.ctypes.data_as(C.c_void_p),
                                                      feat.ctypes.data_as(C.c_void_p), n) != n:
            raise RuntimeError("svs_pipe_keyframe_descriptors changed size between two calls")
        return desc, feat

    def verify_loops_stored(self, pairs, **params):
        """verify_loops on the descriptors describe_new_keyframes stored (svs_pipe_verify_loops_stored).  pairs: (stream, kf_id,
        cand_kf_id) each.  params and the result: as verify_loops."""
        import importlib
        _svs = importlib.import_module(__package__)
        unknown = set(params) - set(_svs.LOOP_DEFAULTS)
        if unknown:
            raise TypeError("verify_loops_stored: unknown parameter(s) %s" % sorted(unknown))
        p = dict(_svs.LOOP_DEFAULTS); p.update(params)
        n = len(pairs)
        ps = (LoopPair * max(n, 1))()
        for i, (s, kf, cand) in enumerate(pairs):
            ps[i] = LoopPair(int(s), int(kf), int(cand))
        P = _svs.LoopParams((C.c_double * 4)(), (C.c_double * 7)(), int(p["min_matches"]), int(p["ransac_iters"]), float(p["reproj_px"]),
                            float(p["max_pose_distance"]), float(p["min_pose_difference"]), float(p["max_pose_difference"]),
                            int(p["seed"]) & 0xFFFFFFFF, 0)
        rows_of = []
        for s, kf, cand in pairs:
            k = self.L.svs_pipe_keyframe_descriptors(self.h, int(s), C.c_longlong(int(cand)), None, None, 0)
            if k < 0:
                raise RuntimeError("svs_pipe_verify_loops_stored refused: " + self.L.svs_pipe_last_error().decode())
            rows_of.append(k)
        rows = sum(rows_of)
        res = (LoopResult * max(n, 1))()
        m4 = np.zeros((max(rows, 1), 4), np.int32)
        if self.L.svs_pipe_verify_loops_stored(self.h, n, ps, C.byref(P), res, m4.ctypes.data_as(C.c_void_p), rows) != 0:
            raise RuntimeError("svs_pipe_verify_loops_stored refused: " + self.L.svs_pipe_last_error().decode())
        out = []; row = 0
        for i in range(n):
            r = res[i]
            out.append(dict(status=r.status, n_matches=r.n_matches, n_points=r.n_points, n_inliers=r.n_inliers,
                            need_correction=bool(r.need_correction), T_corr=np.array(r.T_corr), T_rel=np.array(r.T_rel), d=r.d,
                            matches=m4[row:row + r.n_matches].astype(np.int64)))
            row += rows_of[i]
        return out

    def loopdb_configure(self, capacity, dim=1280):
        """the store of global image descriptors detect_loops searches (svs_pipe_loopdb_configure): capacity rows of dim floats per stream"""
        if self.L.svs_pipe_loopdb_configure(self.h, int(capacity), int(dim)) != 0:
            raise RuntimeError("svs_pipe_loopdb_configure refused: " + self.L.svs_pipe_last_error().decode())
        self._lc_dim = int(dim)

    def configure_global_descriptor(self, layers, params, prep=None):
        """the network behind the global image descriptor (svs_pipe_gdesc_configure): layers as Context.gdesc_configure
        (gdesc.mobilenet_v2_layers() is the reference's), params one f32 array in table order, prep None for the reference's call or a
        dict over GD_PREP_DEFAULTS.  With a network configured detect_loops needs no vecs."""
        import importlib
        _svs = importlib.import_module(__package__)
        arr = _svs.gd_layer_array(layers)
        prm = np.ascontiguousarray(params, np.float32).reshape(-1)
        P = _svs.gd_prep_struct(prep)
        if self.L.svs_pipe_gdesc_configure(self.h, len(layers), C.cast(arr, C.c_void_p), prm.ctypes.data_as(C.c_void_p), prm.size,
                                           C.cast(C.pointer(P), C.c_void_p) if P is not None else None) != 0:
            raise RuntimeError("svs_pipe_gdesc_configure refused: " + self.L.svs_pipe_last_error().decode())

    def global_descriptor_dim(self):
        return int(self.L.svs_pipe_gdesc_dim(self.h))

    def describe_global_new_keyframes(self):
        """LoopClosure::ExtractFeatureVec for every stream whose last step made a keyframe (svs_pipe_describe_global_new_keyframes):
        (vecs [nstreams, dim] raw, rows of the other streams zero; the number of rows computed).  Works with device_map = 1."""
        v = np.zeros((self.n, max(self.global_descriptor_dim(), 1)), np.float32)
        n = self.L.svs_pipe_describe_global_new_keyframes(self.h, v.ctypes.data_as(C.c_void_p))
        if n < 0:
            raise RuntimeError("svs_pipe_describe_global_new_keyframes refused: " + self.L.svs_pipe_last_error().decode())
        return v, n

    def local_fusion(self, jobs):
        """LoopClosure::LocalFusion for every job in one kernel call (svs_pipe_local_fusion), for a loop verified elsewhere (e.g.
        verify_loops_stored): the active window, the active landmarks and the last frame move with the keyframe's corrected pose,
        then the loop keyframe's landmarks replace the current keyframe's.  jobs: dicts with stream, kf_id, cand_kf_id, T_corr[7]
        and pairs [(feature index in the loop keyframe, feature index in the keyframe)].  Returns one dict of statistics per job:
        nkf, npt, n_unanchored, pairs, merged, revived, repointed, same_deleted.  A refusal changes nothing for any job."""
        n = len(jobs)
        arr = (FusionJob * max(n, 1))()
        pairs = []
        for i, j in enumerate(jobs):
            pr = np.asarray(j.get("pairs", ()), np.int64).reshape(-1, 2)
            arr[i] = FusionJob(int(j["stream"]), len(pr), int(j["kf_id"]), int(j["cand_kf_id"]), len(pairs),
                               (C.c_double * 7)(*np.ascontiguousarray(j["T_corr"], np.float64).reshape(7)))
            pairs.extend((int(a), int(b)) for a, b in pr)
        P = np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2)) if pairs else np.zeros((1, 2), np.int32)
        st = (FusionStats * max(n, 1))()
        if self.L.svs_pipe_local_fusion(self.h, n, arr, P.ctypes.data_as(C.c_void_p), st) != 0:
            raise RuntimeError("svs_pipe_local_fusion refused: " + self.L.svs_pipe_last_error().decode())
        return [_fusion_dict(st[i]) for i in range(n)]

    def all_landmarks(self, stream=0):
        """Map::landmarks_ of a stream, id-ascending (svs_pipe_all_landmarks): dict(id [n], xyz [n, 3], observed_times [n], active [n],
        anchor_kf [n]); dead landmarks come from the archive (float positions)"""
        n = self.L.svs_pipe_all_landmarks(self.h, int(stream), None, 0)
        if n < 0:
            raise RuntimeError("svs_pipe_all_landmarks refused: " + self.L.svs_pipe_last_error().decode())
        out = np.zeros((max(n, 1), 7))
        if self.L.svs_pipe_all_landmarks(self.h, int(stream), out.ctypes.data_as(C.c_void_p), n) != n:
            raise RuntimeError("svs_pipe_all_landmarks changed size between two calls")
        out = out[:n]
        return dict(id=out[:, 0].astype(np.int64), xyz=out[:, 1:4].copy(), observed_times=out[:, 4].astype(np.int64), active=out[:, 5] != 0,
                    anchor_kf=out[:, 6].astype(np.int64))

    def last_frame(self, stream=0):
        """(pose[7], keyframe id or -1) of the frontend's last frame of a stream (svs_pipe_last_frame)"""
        pose = np.zeros(7)
        k = self.L.svs_pipe_last_frame(self.h, int(stream), pose.ctypes.data_as(C.c_void_p))
        if k < -1:
            raise RuntimeError("svs_pipe_last_frame refused: " + self.L.svs_pipe_last_error().decode())
        return pose, int(k)

    def detect_loops(self, vecs=None, keyframes_to_ignore_after_loop=5, weak=None, strong=None, max_num_weak=None, min_gap=None, local_fusion=False,
                     **loop_params):
        """LoopClosure::AddNewKeyFrame + one turn of LoopClosurePipeline for every stream whose last step made a keyframe
        (svs_pipe_detect_loops), after describe_new_keyframes: skip rule, candidate search, verification, loop edge, store update.
        vecs: [nstreams, dim] global descriptors (rows of streams without a new keyframe are not read), or None: the network set by
        configure_global_descriptor computes them.  weak, strong, max_num_weak,
        min_gap: LC_DEFAULTS; loop_params: as verify_loops.  Returns one dict per stream: is_keyframe, skipped, searched, verified,
        stored, kf_id, cand (status, cand_kf, best_sim, best_kf, n_weak, n_compared) or None, loop (as verify_loops) or None.
        local_fusion=True (svs_pipe_detect_loops_fused): every stream whose pair was ACCEPTED with need_correction is fused
        (LoopClosure::LocalFusion) in one more kernel call; the dicts gain fused and fusion (the statistics of local_fusion, or None).
        Off (the default) this is the call it was."""
        import importlib
        _svs = importlib.import_module(__package__)
        unknown = set(loop_params) - set(_svs.LOOP_DEFAULTS)
        if unknown:
            raise TypeError("detect_loops: unknown parameter(s) %s" % sorted(unknown))
        p = dict(_svs.LOOP_DEFAULTS); p.update(loop_params)
        c = dict(_svs.LC_DEFAULTS)
        c.update({k: v for k, v in dict(weak=weak, strong=strong, max_num_weak=max_num_weak, min_gap=min_gap).items() if v is not None})
        ns = self.n
        v = None if vecs is None else np.ascontiguousarray(vecs, np.float32).reshape(ns, getattr(self, "_lc_dim", -1))     # unconfigured: the library refuses
        D = LoopDetectParams(float(c["weak"]), float(c["strong"]), int(c["max_num_weak"]), int(c["min_gap"]), int(keyframes_to_ignore_after_loop))
        P = _svs.LoopParams((C.c_double * 4)(), (C.c_double * 7)(), int(p["min_matches"]), int(p["ransac_iters"]), float(p["reproj_px"]),
                            float(p["max_pose_distance"]), float(p["min_pose_difference"]), float(p["max_pose_difference"]),
                            int(p["seed"]) & 0xFFFFFFFF, 0)
        res = (LoopDetection * ns)()
        fs = (FusionStats * ns)()
        if local_fusion:
            if self.L.svs_pipe_detect_loops_fused(self.h, v.ctypes.data_as(C.c_void_p) if v is not None else None, C.byref(D), C.byref(P), 1, res, fs) != 0:
                raise RuntimeError("svs_pipe_detect_loops_fused refused: " + self.L.svs_pipe_last_error().decode())
        elif self.L.svs_pipe_detect_loops(self.h, v.ctypes.data_as(C.c_void_p) if v is not None else None, C.byref(D), C.byref(P), res) != 0:
            raise RuntimeError("svs_pipe_detect_loops refused: " + self.L.svs_pipe_last_error().decode())
        out = []
        for s in range(ns):
            r = res[s]
            d = dict(is_keyframe=bool(r.is_keyframe), skipped=bool(r.skipped), searched=bool(r.searched), verified=bool(r.verified),
                     stored=bool(r.stored), kf_id=r.kf_id, cand=None, loop=None)
            if r.searched:
                d["cand"] = dict(status=r.cand_status, cand_kf=r.cand_kf, best_sim=np.float32(r.best_sim), best_kf=r.best_kf, n_weak=r.n_weak,
                                 n_compared=r.n_compared)
            if r.verified:
                l = r.loop
                m4 = np.zeros((max(l.n_matches, 1), 4), np.int32)
                if self.L.svs_pipe_loop_matches(self.h, s, m4.ctypes.data_as(C.c_void_p), l.n_matches) != l.n_matches:
                    raise RuntimeError("svs_pipe_loop_matches: " + self.L.svs_pipe_last_error().decode())
                d["loop"] = dict(status=l.status, n_matches=l.n_matches, n_points=l.n_points, n_inliers=l.n_inliers,
                                 need_correction=bool(l.need_correction), T_corr=np.array(l.T_corr), T_rel=np.array(l.T_rel), d=l.d,
                                 matches=m4[:l.n_matches].astype(np.int64))
            if local_fusion:
                d["fused"] = bool(fs[s].fused)
                d["fusion"] = _fusion_dict(fs[s]) if fs[s].fused else None
            out.append(d)
        return out

    def loopdb_ids(self, stream):
        """the keyframe ids a stream's store holds (svs_pipe_loopdb_ids)"""
        n = self.L.svs_pipe_loopdb_ids(self.h, int(stream), None, 0)
        if n < 0:
            raise RuntimeError("svs_pipe_loopdb_ids refused: " + self.L.svs_pipe_last_error().decode())
        ids = np.zeros(n, np.int32)
        if n and self.L.svs_pipe_loopdb_ids(self.h, int(stream), ids.ctypes.data_as(C.c_void_p), n) != n:
            raise RuntimeError("svs_pipe_loopdb_ids refused: " + self.L.svs_pipe_last_error().decode())
        return ids

    def last_closed_keyframe(self, stream):
        return self.L.svs_pipe_last_closed_keyframe(self.h, int(stream))

    def map_snapshot(self, stream=0):
        """the host map of one stream after the last step (svs_pipe_map_snapshot): active keyframe ids and poses, active landmarks
        with position, observation counter and observation list [(keyframe id, 0 left / 1 right, feature index)]"""
        ni = self.L.svs_pipe_map_snapshot(self.h, stream, None, 0, None, 0)
        if ni < 0:
            raise RuntimeError("svs_pipe_map_snapshot: %d (-2: the map of this pipeline lives on the device)" % ni)
        ints = np.zeros(ni, np.int64)
        dbl = np.zeros(7 * ni, np.float64)
        if self.L.svs_pipe_map_snapshot(self.h, stream, ints.ctypes.data_as(C.c_void_p), ni, dbl.ctypes.data_as(C.c_void_p), dbl.size) != ni:
            raise RuntimeError("svs_pipe_map_snapshot changed size between two calls")
        o = d = 0
        nk = int(ints[o]); o += 1
        kf = [int(v) for v in ints[o:o + nk]]; o += nk
        poses = {k: dbl[d + 7 * i:d + 7 * i + 7].copy() for i, k in enumerate(kf)}; d += 7 * nk
        nl = int(ints[o]); o += 1
        lms = []
        for _ in range(nl):
            mid, times, no = (int(v) for v in ints[o:o + 3]); o += 3
            obs = tuple((int(ints[o + 3 * i]), int(ints[o + 3 * i + 1]), int(ints[o + 3 * i + 2])) for i in range(no)); o += 3 * no
            lms.append((mid, times, obs, tuple(float(v) for v in dbl[d:d + 3]))); d += 3
        return {"active_keyframes": kf, "landmarks": lms, "keyframe_poses": poses}

    def kernel_ctx(self):
        return self.L.svs_pipe_kernel_ctx(self.h)

    def backend_ctx(self):
        return self.L.svs_pipe_backend_ctx(self.h)


# ---- trajectory error (the reference has no evaluator) -----------------
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def camera_centres(poses_cw):
    """T_cw poses [n,7] -> camera centres in world [n,3]"""
    out = np.zeros((len(poses_cw), 3))
    for i, T in enumerate(poses_cw):
        out[i] = -quat_to_R(T[:4]).T @ T[4:]
    return out


def ate_rmse(est_cw, gt_cw):
    """RMSE of camera-centre error after rigid (SE3, no scale) alignment (Horn / Kabsch)"""
    a = camera_centres(est_cw); b = camera_centres(gt_cw)
    ma, mb = a.mean(0), b.mean(0)
    Hm = (a - ma).T @ (b - mb)
    U, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    al = (a - ma) @ R.T + mb
    return float(np.sqrt(((al - b) ** 2).sum(1).mean()))
