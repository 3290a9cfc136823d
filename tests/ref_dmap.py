"""A plain model of the device-resident map (include/svslam.h, svslam_dmap_*; csrc/k_dmap.h is the code under test).

Written from the reference, not from the kernels: Map::InsertKeyFrame / RemoveOldKeyframe / CleanMap (src/map.cpp:53-181),
DetectFeatures / FindFeaturesInRight / BuildInitMap / StereoInit / TriangulateNewPoints / SetObservationsForKeyFrame
(src/frontend.cpp:36-141, 216-320, 560-616) and Backend::Optimize (src/backend.cpp:39-246).  Landmarks are a dict by id,
a landmark's observations a list in chronological order (keyframe id ascending, left before right: the order AddObservation
is called in), the problem of Optimize the two loops of backend.cpp:83-160, its threshold the loop of :167-193.  Nothing here
scans, sorts bitonically or computes with slots: slots appear only where a model is read from the arena arrays
(MapModel.from_state) and written back over them (MapModel.to_state).

What the project adds on top of the reference, as the header states it:
  * fixed capacities: max_pts features per keyframe (surplus corners dropped, flag 1), max_lm landmark slots (flag 2),
    max_obs edges / max_kf keyframes of a local BA (flag 4: the keyframe goes without one);
  * a new landmark takes the lowest free slot, in creation order; its id is next_lm_id + its rank among the call's new ones;
  * a landmark outside the window (CleanMap took it from active_landmarks_) with no observation, which the tracked list of
    THIS step does not name (lm_stamp != the step's stamp), leaves the map: at most `quota` of them per call, handed over as
    (id, float32 position).  WHICH of the candidates go when there are more is the implementation's business:
    check_eviction() asserts the contract and applies the set the device chose.

The map arrays ("state") are the dict Context.dmap_state_read returns."""
import numpy as np

FLAG_CORNERS_DROPPED, FLAG_LM_FULL, FLAG_BA_SKIPPED = 1, 2, 4
FL_RIGHT_OK = 1


def f32(x):
    return np.float32(x)


# ---------------------------------------------------------------------------------------------- the map as containers
class Feature:
    """one left feature of a keyframe and, where FindFeaturesInRight found it, its right twin (feature_right_[i])"""
    __slots__ = ("xy", "xyr", "lm", "lmr", "fl")

    def __init__(self, xy, xyr=None, lm=None, lmr=None, fl=0):
        self.xy = (f32(xy[0]), f32(xy[1]))
        self.xyr = None if xyr is None else (f32(xyr[0]), f32(xyr[1]))       # None: never written (the arena keeps what it had)
        self.lm, self.lmr, self.fl = lm, lmr, fl                             # landmark ids (None: map_point_ expired)


class Keyframe:
    __slots__ = ("slot", "frame_id", "kf_id", "pose", "feats")

    def __init__(self, slot, frame_id, kf_id, pose, feats):
        self.slot, self.frame_id, self.kf_id, self.pose, self.feats = slot, int(frame_id), int(kf_id), [float(v) for v in pose], feats

    @property
    def active(self):
        return self.frame_id >= 0


class Landmark:
    __slots__ = ("id", "slot", "pos", "obs", "active", "stamp")

    def __init__(self, id_, slot, pos, active, stamp):
        self.id, self.slot, self.pos, self.active, self.stamp = int(id_), slot, [float(v) for v in pos], active, int(stamp)
        self.obs = []          # (keyframe id, 0 left / 1 right, keyframe slot, feature index), chronological


def check_preconditions(state):
    """What the kernels take for granted (k_dmap.h: "a landmark is named by one feature of a frame at most", observations
    are implicit).  A case that breaks one of these tests nothing: it fails here, on the CPU.
    ONE feature: its left side, its right side or both.  The reference cannot produce anything else — a right feature gets its
    map point with the left feature of the same index (frontend.cpp:183-186, :299-302) — and the gather's fill relies on it
    (two features of one keyframe naming one landmark, one on each side, would take the same edge position)."""
    KW, NF = state["f_lm"].shape
    NL = state["lm_id"].shape[0]
    live = state["lm_id"] >= 0
    ids = state["lm_id"][live]
    assert len(set(ids.tolist())) == len(ids), "landmark ids are not unique"
    assert np.array_equal(state["lm_state"] == 0, ~live), "state is 0 exactly where id is -1"
    assert (state["lm_state"] <= 2).all()
    act = state["kf_frame"] >= 0
    kid = state["kf_id"][act]
    assert len(set(kid.tolist())) == len(kid), "keyframe ids of the window are not unique"
    assert ((state["kf_n"] >= 0) & (state["kf_n"] <= NF)).all()
    count = np.zeros(NL, np.int64)
    for k in np.flatnonzero(act):
        n = int(state["kf_n"][k])
        left = {int(l): i for i, l in enumerate(state["f_lm"][k, :n]) if l >= 0}
        for i, l in enumerate(state["f_lmr"][k, :n]):
            assert l < 0 or left.get(int(l), i) == i, "keyframe slot %d: landmark slot %d is named by two features (%d left, %d right)" % (k, l, left[int(l)], i)
        for name in ("f_lm", "f_lmr"):
            links = state[name][k, :n]
            assert ((links >= -1) & (links < NL)).all()
            named = links[links >= 0]
            assert len(set(named.tolist())) == len(named), "keyframe slot %d: a landmark is named twice on one side" % k
            assert live[named].all(), "keyframe slot %d names a free landmark slot" % k
            np.add.at(count, named, 1)
    assert np.array_equal(count[live], state["lm_obs"][live].astype(np.int64)), "lm_obs != features of active keyframes naming the landmark"
    # every slot's link arrays stay inside the arena, stale ones included (the write hook refuses others)
    assert ((state["f_lm"] >= -1) & (state["f_lm"] < NL) & (state["f_lmr"] >= -1) & (state["f_lmr"] < NL)).all()


class MapModel:
    """one stream's map: keyframes by slot (active or not), landmarks by id"""

    def __init__(self):
        self.kfs, self.lms, self.next_lm_id = {}, {}, 0
        self.KW = self.NF = self.NL = 0
        self.evicted = []

    # ---- arena -> model ------------------------------------------------------------------------
    @classmethod
    def from_state(cls, state, open_slots=()):
        """active keyframes (and the slots of `open_slots`: the keyframe a StereoInit is filling is not in the map yet) with their
        kf_n features; live landmarks; observations rebuilt in the order the reference's lists have them"""
        check_preconditions(state)
        m = cls()
        m.KW, m.NF = state["f_lm"].shape
        m.NL = state["lm_id"].shape[0]
        m.next_lm_id = int(state["next_lm_id"][0])
        id_of = {}
        for l in range(m.NL):
            if state["lm_id"][l] >= 0:
                lm = Landmark(state["lm_id"][l], l, state["lm_pos"][l], state["lm_state"][l] == 1, state["lm_stamp"][l])
                m.lms[lm.id] = lm
                id_of[l] = lm.id
        for k in range(m.KW):
            if state["kf_frame"][k] < 0 and k not in open_slots:
                continue
            feats = []
            for i in range(int(state["kf_n"][k])):
                a, b = int(state["f_lm"][k, i]), int(state["f_lmr"][k, i])
                feats.append(Feature(state["f_xy"][k, i], state["f_xyr"][k, i], id_of.get(a), id_of.get(b), int(state["f_fl"][k, i])))
            m.kfs[k] = Keyframe(k, state["kf_frame"][k], state["kf_id"][k], state["kf_pose"][k], feats)
        for kf in sorted((kf for kf in m.kfs.values() if kf.active), key=lambda kf: kf.kf_id):      # chronological
            for side in (0, 1):                                                                    # left before right
                for i, ft in enumerate(kf.feats):
                    lid = ft.lm if side == 0 else ft.lmr
                    if lid is not None:
                        m.lms[lid].obs.append((kf.kf_id, side, kf.slot, i))
        for lm in m.lms.values():
            lm.obs.sort(key=lambda o: (o[0], o[1]))
        return m

    # ---- model -> arena (over the arrays the model was read from) --------------------------------
    def to_state(self, base):
        out = {k: v.copy() for k, v in base.items()}
        for lm in self.evicted:                                  # the slot is marked free; what the landmark last held stays behind
            out["lm_obs"][lm.slot] = len(lm.obs); out["lm_stamp"][lm.slot] = lm.stamp; out["lm_pos"][lm.slot] = lm.pos
            out["lm_id"][lm.slot] = -1
            out["lm_state"][lm.slot] = 0
        for lm in self.lms.values():
            l = lm.slot
            out["lm_id"][l] = lm.id; out["lm_pos"][l] = lm.pos; out["lm_obs"][l] = len(lm.obs)
            out["lm_state"][l] = 1 if lm.active else 2; out["lm_stamp"][l] = lm.stamp
        for k, kf in self.kfs.items():
            if kf.feats is None:
                out["kf_frame"][k] = -1
                continue
            out["kf_frame"][k] = kf.frame_id; out["kf_id"][k] = kf.kf_id; out["kf_pose"][k] = kf.pose; out["kf_n"][k] = len(kf.feats)
            for i, ft in enumerate(kf.feats):
                out["f_xy"][k, i] = ft.xy
                if ft.xyr is not None:
                    out["f_xyr"][k, i] = ft.xyr
                out["f_lm"][k, i] = -1 if ft.lm is None else self.lms[ft.lm].slot
                out["f_lmr"][k, i] = -1 if ft.lmr is None else self.lms[ft.lmr].slot
                out["f_fl"][k, i] = ft.fl
        out["next_lm_id"][0] = self.next_lm_id
        return out

    def active_keyframes(self):
        """Map::active_keyframes_: id-ordered"""
        return sorted((kf for kf in self.kfs.values() if kf.active), key=lambda kf: kf.kf_id)

    def active_landmarks(self):
        """Map::active_landmarks_: id-ordered (ids are unsigned)"""
        return sorted((lm for lm in self.lms.values() if lm.active), key=lambda lm: lm.id)

    def _remove_observation(self, lm, kf_id, side):
        lm.obs = [o for o in lm.obs if not (o[0] == kf_id and o[1] == side)]

    # ---- Map::InsertKeyFrame / RemoveOldKeyframe / CleanMap + SetObservationsForKeyFrame ----------
    def begin(self, job, tracked_xy, tracked_slots):
        """job: dict(is_init, kf_slot, remove_slot, kf_id, frame_id, pose, npts, stamp); tracked_*: the resident list (positions,
        landmark SLOTS, -1 none).  Returns the job's outputs and the eviction candidates (ids)."""
        outs = dict(ok=0 if job["is_init"] else 1, dead=0, flags=0, n_corners=0, n_right_ok=0, n_tri_in=0, n_tri_ok=0, ba_nkf=0, ba_nlm=0,
                    ba_nobs=0, ba_iters=0, n_features=job["npts"], corners_dropped=0, ev_ofs=0, ev_n=0, ba_npair=0, ba_ntrial=0)
        if job["is_init"]:
            return outs, []
        if job["remove_slot"] >= 0:                              # RemoveOldKeyframe: the host chose which (map.cpp:137-165)
            old = self.kfs[job["remove_slot"]]
            for ft in old.feats:
                if ft.lm is not None:
                    self._remove_observation(self.lms[ft.lm], old.kf_id, 0)
            for ft in old.feats:
                if ft.lmr is not None:
                    self._remove_observation(self.lms[ft.lmr], old.kf_id, 1)
            old.frame_id, old.feats = -1, None                 # (the arena keeps what the slot held; only the frame id says "empty")
            for lm in self.lms.values():                         # CleanMap: landmarks nobody observes leave active_landmarks_
                if lm.active and not lm.obs:
                    lm.active = False
        id_at = {lm.slot: lm.id for lm in self.lms.values()}
        feats = []
        for i in range(job["npts"]):
            s = int(tracked_slots[i])
            feats.append(Feature(tracked_xy[i], None, id_at[s] if s >= 0 else None, None, 0))
        kf = Keyframe(job["kf_slot"], job["frame_id"], job["kf_id"], job["pose"], feats)
        self.kfs[kf.slot] = kf
        for i, ft in enumerate(feats):                           # SetObservationsForKeyFrame (frontend.cpp:560-574)
            if ft.lm is not None:
                lm = self.lms[ft.lm]
                lm.obs.append((kf.kf_id, 0, kf.slot, i))
                lm.stamp = job["stamp"]
        cands = [lm.id for lm in self.lms.values() if not lm.active and not lm.obs and lm.stamp != job["stamp"]]
        return outs, cands

    def check_eviction(self, cands, quota, records, state_after):
        """the contract of the hand-over: `records` [(id, x, y, z float32)] is a subset of the candidates of size min(candidates, quota),
        each record is (id, float32(pos)), the freed slots are marked free, every other candidate is untouched.  Applies the set."""
        want = min(len(cands), quota)
        assert len(records) == want, (len(records), want)
        ids = [int(r[0]) for r in records]
        assert len(set(ids)) == len(ids) and set(ids) <= set(cands)
        for r in records:
            lm = self.lms[int(r[0])]
            assert [f32(v) for v in lm.pos] == [f32(r[1]), f32(r[2]), f32(r[3])], (lm.id, lm.pos, r)
            assert state_after["lm_id"][lm.slot] == -1 and state_after["lm_state"][lm.slot] == 0
        for i in ids:
            self.evicted.append(self.lms.pop(i))
        return set(ids)

    # ---- DetectFeatures' append (frontend.cpp:52-66) + the start guesses of FindFeaturesInRight (:79-103) ----
    def stereo_prep(self, job, corners, T_camr_w, cam_r):
        """corners: the detector's list, strongest first.  Returns outputs, prev_xy, next_xy (lists of float32 pairs)"""
        kf = self.kfs[job["kf_slot"]]
        assert len(kf.feats) == job["npts"]
        room = self.NF - job["npts"]
        take, outs = len(corners), {}
        if take > room:                                          # the keyframe's feature list is full: the weakest corners go
            kept = max(room, 0)
            outs["flags"] = job.get("flags", 0) | FLAG_CORNERS_DROPPED
            outs["corners_dropped"] = take - kept
            take = kept
        for c in corners[:take]:
            kf.feats.append(Feature(c, None, None, None, 0))
        outs.update(n_corners=take, n_features=len(kf.feats))
        prev, nxt = [], []
        for ft in kf.feats:
            prev.append(ft.xy)
            if ft.lm is not None:                                # camera_right_->world2pixel(mp->pos_, Pose())
                u, v = project(T_camr_w, cam_r, self.lms[ft.lm].pos)
                nxt.append((f32(u), f32(v)))
            else:
                nxt.append(ft.xy)
        return outs, prev, nxt

    # ---- right features (frontend.cpp:111-135), StereoInit's count (:227), the pairs to triangulate (:155-161 / :267-273) ----
    def stereo_finish(self, job, next_xy, status, w, h, num_features_init):
        kf = self.kfs[job["kf_slot"]]
        assert len(kf.feats) == job["n_features"]
        good = 0
        for i, ft in enumerate(kf.feats):
            x, y = f32(next_xy[i][0]), f32(next_xy[i][1])
            ok = bool(status[i]) and y >= 0 and y < f32(h) and x >= 0 and x < f32(w)
            ft.fl = FL_RIGHT_OK if ok else 0
            ft.xyr = (x, y) if ok else (f32(0), f32(0))
            good += 1 if ok else 0
        dead = bool(job["is_init"]) and good < num_features_init
        tri = []
        if not dead:
            for i, ft in enumerate(kf.feats):
                if ft.fl & FL_RIGHT_OK and (job["is_init"] or ft.lm is None):
                    tri.append(i)
        outs = dict(n_right_ok=good, dead=1 if dead else 0, n_tri_in=len(tri))
        if job["is_init"]:
            outs["ok"] = 0 if dead else 1
        return outs, tri

    # ---- new landmarks (frontend.cpp:176-191 / :289-305); StereoInit's keyframe (:195-197) ----
    def commit(self, job, tri_idx, tri_ok, tri_xyz):
        if job["dead"]:
            return {}
        kf = self.kfs[job["kf_slot"]]
        taken = {lm.slot for lm in self.lms.values()}
        free = [l for l in range(self.NL) if l not in taken]     # ascending: the lowest free slot first
        accepted = [q for q in range(job["n_tri_in"]) if tri_ok[q]]
        made = 0
        for rank, q in enumerate(accepted):
            if rank >= len(free):
                break                                            # max_lm landmark slots: the rest are not created
            lm = Landmark(self.next_lm_id + rank, free[rank], tri_xyz[q], True, job["stamp"])
            i = int(tri_idx[q])
            lm.obs = [(job["kf_id"], 0, kf.slot, i), (job["kf_id"], 1, kf.slot, i)]
            self.lms[lm.id] = lm
            kf.feats[i].lm = kf.feats[i].lmr = lm.id
            made += 1
        outs = dict(n_tri_ok=made)
        if len(accepted) > len(free):
            outs["flags"] = job.get("flags", 0) | FLAG_LM_FULL
        self.next_lm_id += made
        if job["is_init"]:
            kf.frame_id, kf.kf_id, kf.pose = int(job["frame_id"]), int(job["kf_id"]), [float(v) for v in job["pose"]]
        return outs

    # ---- Backend::Optimize's problem (backend.cpp:39-160) ----
    def ba_problem(self, max_kf, max_obs):
        """vertices and edges in the order the loops of backend.cpp create them; None when over a capacity"""
        kfs = self.active_keyframes()
        local = {kf.kf_id: a for a, kf in enumerate(kfs)}
        verts, edges = [], []
        for lm in self.active_landmarks():
            for (kf_id, side, slot, i) in lm.obs:
                if not verts or verts[-1] is not lm:
                    verts.append(lm)                             # a landmark becomes a vertex with its first observation (:118-130)
                ft = self.kfs[slot].feats[i]
                edges.append(dict(v=len(verts) - 1, a=local[kf_id], right=side, uv=ft.xy if side == 0 else ft.xyr, kf_slot=slot, feat=i))
        skipped = len(edges) > max_obs or len(kfs) > max_kf
        return dict(kfs=kfs, verts=verts, edges=edges, skipped=skipped)

    # ---- outlier threshold, observations removed, write-back (backend.cpp:167-246) ----
    def ba_apply(self, job, prob, chi2, poses, pts, iters_done, chi2_th, ncontrib=0, ntrial=0):
        """prob: ba_problem()'s; chi2 per edge, poses per keyframe, pts per vertex: the solver's.  Returns the job's outputs."""
        edges = prob["edges"]
        if job["dead"] or not edges:
            return {}
        if iters_done < 0:
            return dict(ba_iters=-1)
        th, iteration = float(chi2_th), 0
        while iteration < 5:
            cnt_outlier = sum(1 for e in range(len(edges)) if chi2[e] > th)
            cnt_inlier = len(edges) - cnt_outlier
            inlier_ratio = cnt_inlier / float(cnt_inlier + cnt_outlier)
            if inlier_ratio > 0.5:
                break
            th *= 2
            iteration += 1
        for e, ed in enumerate(edges):
            if chi2[e] > th:
                ft = self.kfs[ed["kf_slot"]].feats[ed["feat"]]
                lid = ft.lmr if ed["right"] else ft.lm
                if ed["right"]:
                    ft.lmr = None
                else:
                    ft.lm = None
                if lid is not None:
                    self._remove_observation(self.lms[lid], self.kfs[ed["kf_slot"]].kf_id, ed["right"])
        outs = dict(ba_iters=iters_done, ba_npair=ncontrib, ba_ntrial=ntrial, win_pose={})
        for a, kf in enumerate(prob["kfs"]):
            kf.pose = [float(v) for v in poses[a]]
            outs["win_pose"][a] = kf.pose
            if kf.slot == job["kf_slot"]:
                outs["pose"] = kf.pose
        for v, lm in enumerate(prob["verts"]):
            lm.pos = [float(x) for x in pts[v]]
        return outs

    # ---- the keyframe's features as the list the next frame tracks from ----
    def resident_list(self, kf_slot):
        """[(xy, landmark slot or -1, position or (0, 0, 1))]"""
        out = []
        for ft in self.kfs[kf_slot].feats:
            if ft.lm is not None:
                out.append((ft.xy, self.lms[ft.lm].slot, self.lms[ft.lm].pos))
            else:
                out.append((ft.xy, -1, [0.0, 0.0, 1.0]))
        return out

    def position_at(self, slot):
        for lm in self.lms.values():
            if lm.slot == slot:
                return lm.pos
        raise KeyError(slot)


def project(T, cam, X):
    """Camera::world2pixel in doubles: Sophus' SE3 * point is Eigen's quaternion action t = 2 q_v x p, p + w t + q_v x t, plus the
    translation; then fx X / Z + cx.  T = (qx qy qz qw tx ty tz), cam = (fx fy cx cy); plain IEEE doubles, no fused operations."""
    qx, qy, qz, qw, tx, ty, tz = [float(v) for v in T]
    x, y, z = [float(v) for v in X]
    ux = qy * z - qz * y; uy = qz * x - qx * z; uz = qx * y - qy * x
    ux += ux; uy += uy; uz += uz
    p0 = x + qw * ux + (qy * uz - qz * uy)
    p1 = y + qw * uy + (qz * ux - qx * uz)
    p2 = z + qw * uz + (qx * uy - qy * ux)
    p0 += tx; p1 += ty; p2 += tz
    return float(cam[0]) * p0 / p2 + float(cam[2]), float(cam[1]) * p1 / p2 + float(cam[3])
