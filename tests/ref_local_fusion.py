"""LoopClosure::LocalFusion in plain Python: the contract of svslam_local_fusion_batch and of Pipeline::LocalFusion.

Written from the reference's src/loopclosure.cpp:439-582 (LocalFusion), :584-639 (LoopClosureUpdate), :340-366 (what KeypointMatches_
holds), src/mappoint.cpp:22-36 (AddObservation) and src/map.cpp:42-51 (RemoveLandmark), and from nothing else.  `cur` is the
keyframe that closed the loop, `cand` the loop keyframe, T_corr = current_frame_corrected_pose_.

  1 corrected poses (:451-467)   corrected[cur] = T_corr; for every ACTIVE keyframe i != cur: corrected[i] = (T_i * T_cur^-1) * T_corr,
                                 in that association.  cur has its entry whether it is still active or not.
  2 active landmarks (:470-503)  walk the observation list in list order; the first observation whose feature is alive, whose
                                 feature still names a live landmark (any: map_point_.lock()) and whose frame has an entry moves the
                                 landmark: p' = corrected[k]^-1 * (T_k * p) with the OLD T_k.  Right-image observations count.  The
                                 reference asserts that one is found; here such a landmark stays and is counted (n_unanchored).
  3 last frame (:506-526)        not an active keyframe: T_f <- (T_f * T_cur^-1) * T_corr; an active keyframe: step 4 wrote it.
                                 relative_motion is not touched.
  4 write-back (:511-519)        the active keyframes only; relative_pose_pkf is NOT refreshed.
  5 replacement (:530-573)       over KeypointMatches_, a std::set<pair<cand feature, cur feature>>: ascending lexicographic order,
                                 every pair on the map as the pairs before it left it.  mp_loop = landmark of cand.left[ci]; gone:
                                 nothing.  mp_curr = landmark of cur.left[qi].  Alive: each of its observations, in order, is added
                                 to mp_loop (observed_times + 1) and re-pointed to mp_loop, then Map::RemoveLandmark(mp_curr) erases
                                 it from landmarks_ and active_landmarks_ — it is destroyed, every feature that still names it has an
                                 expired pointer.  Not alive: cur.left[qi] names mp_loop, no observation is added.
                                 mp_loop is mp_curr: the observations are appended to themselves, then the landmark is removed — it
                                 is deleted and all its features expire (the reference's quirk, kept).  mp_loop is not made active.

The arithmetic (fuse) is numpy f64 in the kernel's operation order: se3_mul / se3_inv / se3_act of tests/ref_pose_graph.py are the
operations of csrc/k_pose_graph.h.  The bookkeeping (local_fusion) runs over the object graph of tests/ref_glue.py."""
import numpy as np

from ref_pose_graph import se3_act, se3_inv, se3_mul


# ---------------------------------------------------------------- steps 1-3 on arrays: what the kernel computes
def corrected(T, T_cur, T_corr):
    """(T * T_cur^-1) * T_corr (:462-464, :507 + :524)"""
    return se3_mul(se3_mul(T, se3_inv(T_cur)), T_corr)


def fuse(job):
    """job: the dict Context.local_fusion takes — poses [n, 7], cur (window index or -1 with T_cur), T_corr, last (window index or -1
    with T_last), pts [m, 3], obs_ptr [m + 1], obs_kf (row of the corrected table per observation, -1 for none; row n is a cur
    outside the window).  Returns what it returns: poses, T_last, pts, pt_kf, n_unanchored."""
    poses = np.array(job["poses"], np.float64).reshape(-1, 7)
    n = len(poses)
    cur, last = int(job["cur"]), int(job["last"])
    T_corr = np.array(job["T_corr"], np.float64)
    T_cur = poses[cur].copy() if cur >= 0 else np.array(job["T_cur"], np.float64)
    table = np.zeros((n + 1, 7))
    table[n] = T_corr
    for i in range(n):
        table[i] = T_corr if i == cur else corrected(poses[i], T_cur, T_corr)
    old = np.concatenate([poses, T_cur[None]])
    pts = np.array(job["pts"] if job.get("pts") is not None else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    ptr = np.asarray(job["obs_ptr"] if job.get("obs_ptr") is not None else [0]).reshape(-1)
    okf = np.asarray(job["obs_kf"] if job.get("obs_kf") is not None else [], np.int64).reshape(-1)
    pt_kf = np.full(len(pts), -1, np.int32)
    unanchored = 0
    for p in range(len(pts)):
        k = next((int(v) for v in okf[ptr[p]:ptr[p + 1]] if v >= 0), -1)
        pt_kf[p] = k
        if k < 0:
            unanchored += 1
            continue
        pts[p] = se3_act(se3_inv(table[k]), se3_act(old[k], pts[p]))
    if last >= 0:
        T_last = table[last].copy()
    else:
        T_last = corrected(np.array(job["T_last"], np.float64), T_cur, T_corr)
    return dict(poses=table[:n].copy(), T_last=T_last, pts=pts, pt_kf=pt_kf, n_unanchored=unanchored)


# ---------------------------------------------------------------- steps 1-5 on ref_glue's object graph
def lock(the_map, mp):
    """weak_ptr<MapPoint>::lock(): Map::landmarks_ is the only owner, so a landmark erased from it is destroyed"""
    return mp if mp is not None and the_map.landmarks.get(mp.id) is mp else None


def add_observation(mp, feat):
    """src/mappoint.cpp:22-36, with the first_valid_obs_ rule ref_glue leaves out: set when it is expired and the feature is no outlier"""
    mp.observations.append(feat)
    mp.observed_times += 1
    if getattr(mp, "first_valid_obs", None) is None and not feat.outlier:
        mp.first_valid_obs = feat


def remove_landmark(the_map, mp, frames):
    """src/map.cpp:42-51.  The landmark is destroyed: every feature of `frames` (all keyframes and the frames tracking still
    holds) that names it is left with an expired pointer, which ref_glue writes as None"""
    the_map.landmarks.pop(mp.id, None)
    the_map.active_landmarks.pop(mp.id, None)
    for fr in frames:
        for f in list(fr.feature_left) + list(fr.feature_right):
            if f is not None and f.map_point is mp:
                f.map_point = None


def gather(the_map, last_frame, cur, T_corr):
    """the job `fuse` takes, read off the graph: window in ascending keyframe id, active landmarks in ascending id"""
    kf_ids = sorted(the_map.active_keyframes)
    row = {k: i for i, k in enumerate(kf_ids)}
    cur_row = row.get(cur.keyframe_id, -1)
    if cur_row < 0:
        row[cur.keyframe_id] = len(kf_ids)
    lm_ids = sorted(the_map.active_landmarks)
    ptr, okf = [0], []
    for m in lm_ids:
        for f in the_map.active_landmarks[m].observations:
            ok = f is not None and lock(the_map, f.map_point) is not None and f.frame is not None and f.frame.is_keyframe
            okf.append(row.get(f.frame.keyframe_id, -1) if ok else -1)
        ptr.append(len(okf))
    last_row = row.get(last_frame.keyframe_id, -1) if last_frame.is_keyframe and last_frame.keyframe_id in the_map.active_keyframes else -1
    job = dict(poses=np.array([the_map.active_keyframes[k].pose for k in kf_ids]).reshape(-1, 7), cur=cur_row, T_cur=cur.pose.copy(),
               T_corr=np.array(T_corr, np.float64), last=last_row, T_last=last_frame.pose.copy(),
               pts=np.array([the_map.active_landmarks[m].pos for m in lm_ids]).reshape(-1, 3), obs_ptr=np.array(ptr), obs_kf=np.array(okf, np.int64))
    return job, kf_ids, lm_ids


def local_fusion(the_map, last_frame, cur, cand, T_corr, matches, frames=()):
    """LocalFusion on the graph.  matches: pairs (feature index in cand.feature_left, feature index in cur.feature_left); frames:
    the frames besides the map's keyframes whose features may name landmarks (the frontend's last and current frame).
    Returns the statistics Pipeline::LocalFusion reports."""
    job, kf_ids, lm_ids = gather(the_map, last_frame, cur, T_corr)
    out = fuse(job)
    for i, m in enumerate(lm_ids):                                       # step 2
        the_map.active_landmarks[m].pos = out["pts"][i].copy()
    for i, k in enumerate(kf_ids):                                       # step 4
        the_map.active_keyframes[k].pose = out["poses"][i].copy()
    if job["last"] < 0:                                                  # step 3
        last_frame.pose = out["T_last"].copy()
    everywhere = list(the_map.keyframes.values()) + [f for f in frames if f is not None]
    st = dict(nkf=len(kf_ids), npt=len(lm_ids), n_unanchored=out["n_unanchored"], pairs=0, merged=0, repointed=0, same_deleted=0)
    for ci, qi in sorted(set((int(a), int(b)) for a, b in matches)):      # step 5
        st["pairs"] += 1
        mp_loop = lock(the_map, cand.feature_left[ci].map_point)
        if mp_loop is None:
            continue
        mp_curr = lock(the_map, cur.feature_left[qi].map_point)
        if mp_curr is not None:
            for f in list(mp_curr.observations):                         # GetObs() returns a copy of the list
                if f is not None:
                    add_observation(mp_loop, f)
                    f.map_point = mp_loop
                    st["repointed"] += 1
            remove_landmark(the_map, mp_curr, everywhere)
            if mp_curr is mp_loop:
                st["same_deleted"] += 1
            else:
                st["merged"] += 1
        else:
            cur.feature_left[qi].map_point = mp_loop
            st["repointed"] += 1
    return st
