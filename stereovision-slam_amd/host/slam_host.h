// slam_host.h — host side of the drop-in: the reference's Frontend / Backend /
// Map / Frame / Feature / MapPoint logic restated over flat arrays and staged so
// that S independent streams advance in lockstep and every library call site of
// the reference becomes ONE batched C-ABI call for all streams.
//
// Mirrors (file:line into the reference):
//   Frontend::AddFrame/Track/StereoInit/...      src/frontend.cpp:143-721
//   Backend::Optimize gather / scatter           src/backend.cpp:39-246
//   Map::InsertKeyFrame/RemoveOldKeyframe/CleanMap  src/map.cpp:21-181
//   MapPoint::AddObservation/RemoveObservation   src/mappoint.cpp:22-78
//   Frame / Feature id factories                 src/frame.cpp:22-35
// Differences, all deliberate: the pointer graph (shared_ptr /
// weak_ptr) is replaced by indices; unordered_map iteration is replaced by
// ascending-id order; BA runs synchronously inside UpdateMap() (the reference's
// free-running backend thread makes it nondeterministic); viewer and
// loop closure are off.
//
// The kernel provider K exposes the batched entry points of include/svslam.h;
// this header never names an implementation.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <iomanip>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/svslam.h"
#include "se3.h"
#include "thread_pool.h"

namespace svs {

struct Config {                       // config/stereo_slam_configs/config-00.yaml
    int num_features = 150;
    int num_features_init = 50;
    int num_features_tracking = 50;
    int num_features_tracking_bad = 20;
    int num_features_needed_for_keyframe = 80;
    double max_triangulation_depth = 300.0;
    int num_active_keyframes = 10;
    int backend_on = 1;
    int src_width = 0, src_height = 0;   // > 0: input frames are full resolution, decimated into the pyramid
    int resident_track = 1;              // last-frame features stay in device memory (needs backend_on <= 1)
    double chi2_th = 5.991;
    int width = 620, height = 188;
    Camera cam_l, cam_r;
    // Capacities of the kernel provider per stream (0 = unlimited).  The reference has no such
    // limits; a stream that would exceed one is handled on its own BEFORE any shared state is
    // touched, so the other streams of the lockstep batch never notice: surplus new corners are
    // not appended (max_pts), an over-sized local BA is skipped for this keyframe (max_kf /
    // max_lm / max_obs) — the reference's own backend drops optimisation requests too (lossy
    // notify).  Counters::corners_dropped / ba_skipped report how often.
    int max_pts = 0, max_kf = 0, max_lm = 0, max_obs = 0;
    // 1: the kernel provider keeps every stream's map (window, keyframe features, landmarks, observation counts) in
    // device memory and runs the whole keyframe path there (K::dmap_keyframe); the host keeps O(window) per stream —
    // the keyframes' ids, slots and poses.  Needs resident_track and backend_on == 1.
    int device_map = 0;
    // backend_on >= 2: frames a submitted local BA may stay in flight before its result is applied.  1 = the result
    // lands exactly one frame late (round 2).  The reference's backend thread takes several frame times (g2o on the
    // CPU) and its result lands whenever it is done; a fixed lag keeps that overlap AND reproducibility: a lone
    // camera's frame then costs the tracking chain only, the 1.3-ms BA of a keyframe runs beside the next frames.
    // A new keyframe always collects the optimisation in flight first.
    int backend_lag = 1;
};

enum class FrontendStatus { INITING = 0, TRACKING_GOOD = 1, TRACKING_BAD = 2, LOST = 3 };

struct Feature {
    float x = 0, y = 0;
    long mp = -1;        // map point id, -1 == expired weak_ptr
    bool outlier = false;
    // cv::KeyPoint's octave and angle of position_ (src/frontend.cpp:51-58): what ORB::detect gave a freshly detected feature; a tracked
    // one is cv::KeyPoint(pt, 7) (:374), angle -1 and octave 0, and so is a GFTT corner.  Both live in what was the struct's padding
    int8_t octave = 0;
    float angle = -1.f;
};
static_assert(sizeof(Feature) == 24, "angle and octave live in Feature's padding: the host map pays nothing for them");

struct Frame {
    long id = 0;
    long keyframe_id = 0;
    bool is_keyframe = false;
    SE3 pose;                         // T_cw
    std::vector<Feature> left, right; // right[i] pairs with left[i]
    std::vector<uint8_t> right_ok;    // 0 == nullptr in the reference
    Frame *prev_keyframe = nullptr;
    SE3 relative_pose_pkf;
    Frame *loop_keyframe = nullptr;   // loop_keyframe_ / loop_relative_pose_ of the reference (include/StereoVisionSLAM/frame.h): the older
    SE3 loop_relative_pose;           // keyframe a loop detector matched this one with, and T_this * T_loop^-1 as it measured it
    int ba_local = -1;                // index in the current BA problem (scratch of Backend::Optimize)
    int dslot = -1;                   // device_map: slot of this keyframe in the provider's window arena
    // descriptor_ / desc_feat_indx_ of the reference (LoopClosure::ExtractKeypointsDescriptor): 32 bytes a row, and the index in
    // `left` of the feature each row describes.  Empty until Pipeline::DescribeNewKeyframes is asked; kept when the keyframe leaves
    // the window.  described: the keyframe was described (possibly with zero rows)
    std::vector<uint8_t> desc;
    std::vector<int> desc_feat_indx;
    bool described = false;
    bool loop_checked = false;        // Pipeline::DetectLoops has handled this keyframe (skipped, searched, stored or not)
};

struct ObsRef {
    Frame *frame;
    int idx;
    bool is_left;
    bool operator==(const ObsRef &o) const { return frame == o.frame && idx == o.idx && is_left == o.is_left; }
};

// Observation list of a landmark: most landmarks of a local window are seen from one or two
// keyframes (2-4 observations), so the first 6 live inside the MapPoint (one cache line
// pair, no second pointer chase in the BA gather); the rest spill to the heap.
class ObsList {
public:
    size_t size() const { return n_; }
    const ObsRef &operator[](size_t i) const { return i < kInline ? in_[i] : more_[i - kInline]; }
    void push_back(const ObsRef &o)
    {
        if (n_ < kInline) in_[n_] = o; else more_.push_back(o);
        ++n_;
    }
    void erase_at(size_t i)                 // order-preserving, like std::list::remove
    {
        for (size_t k = i; k + 1 < n_; ++k) at(k) = at(k + 1);
        --n_;
        if (n_ >= kInline) more_.pop_back();
    }
    void clear() { n_ = 0; more_.clear(); }
    struct It {
        const ObsList *l; size_t i;
        bool operator!=(const It &o) const { return i != o.i; }
        void operator++() { ++i; }
        const ObsRef &operator*() const { return (*l)[i]; }
    };
    It begin() const { return It{ this, 0 }; }
    It end() const { return It{ this, n_ }; }
private:
    static constexpr size_t kInline = 6;
    ObsRef &at(size_t i) { return i < kInline ? in_[i] : more_[i - kInline]; }
    ObsRef in_[kInline];
    std::vector<ObsRef> more_;
    size_t n_ = 0;
};

struct MapPoint {
    long id = 0;
    double pos[3] = { 0, 0, 0 };
    bool is_outlier = false;
    bool active = false;               // member of Map::active_landmarks_
    bool in_limbo = false;             // listed in Map::limbo_ (unobserved, outside the window)
    int observed_times = 0;
    long seen_stamp = -1;              // keyframe id at which a live feature list last named this landmark (Map::ReleaseRetired)
    ObsList observations;
    // first_valid_obs_ of the reference (src/mappoint.cpp:31-35, 60-76): the observation whose keyframe a pose-graph optimisation
    // re-anchors this landmark to (src/loopclosure.cpp:767-775).  Only its frame pointer is ever dereferenced (keyframes live for
    // the whole run); has_anchor == false is the reference's expired weak_ptr.
    ObsRef anchor = { nullptr, 0, true };
    bool has_anchor = false;
    long anchor_kf() const { return has_anchor ? anchor.frame->keyframe_id : -1; }
};

struct LandmarkRecord { long id; double pos[3]; int observed_times; bool active; long anchor_kf = -1; };   // what the map hands to writers / viewers

inline Feature &feat_of(const ObsRef &r) { return r.is_left ? r.frame->left[r.idx] : r.frame->right[r.idx]; }

// ------------------------------------------------------------------ Map
// The reference keeps four unordered_maps (src/map.h:15-16).  Ids come from monotonically
// increasing factories, so "all" containers are append-only arrays indexed by id and the
// "active" containers are id-sorted vectors: no node allocation on the per-frame path.
class Map {
public:
    explicit Map(int num_active) : num_active_keyframes_(num_active) {}

    // Map::landmarks_ (src/map.h:15) keeps every landmark ever created, but only saveSLAMOutputInFile
    // (src/visual_odometry.cpp:226-304) ever reads the ones that left the window — their positions.  A landmark is
    // DEAD once nothing can reach it again: no observation (observed_times == 0: no active keyframe's feature names
    // it) and not named by the feature list tracking carries forward (ids enter that list only at keyframes and it
    // only shrinks in between).  Dead landmarks are spilled to an append-only archive of (id, float xyz, anchor keyframe id) — 20 bytes
    // instead of ~190 — and their MapPoint object is reused: the host store stays bounded on long runs (VERDICT r2:
    // 4.9 KB per frame -> 600 GB for 10 k frames at 12 288 streams).  Behaviour is unchanged: a dead landmark is
    // unreachable by construction; `point()` of its id gives nullptr, which every caller already treats as "no map
    // point" (an expired weak_ptr in the reference).
    MapPoint *CreateNewMappoint()       // src/mappoint.cpp:88-98 (per-stream factory)
    {
        MapPoint *m;
        if (!free_.empty()) {
            m = free_.back(); free_.pop_back();
            m->is_outlier = false; m->active = false; m->in_limbo = false; m->observed_times = 0; m->seen_stamp = -1; m->observations.clear(); m->has_anchor = false;
        } else { pool_.emplace_back(); m = &pool_.back(); }
        m->id = next_id_++;
        slots_.push_back(m);
        return m;
    }
    MapPoint *point(long id)
    {
        if (id < base_id_) {                         // covers id == -1 (no map point) and evicted ids below the window
            if (revived_.empty() || id < 0) return nullptr;
            auto it = revived_.find(id);             // ... unless a loop brought one back (Revive): empty on a run without loops
            return it == revived_.end() ? nullptr : it->second;
        }
        return slots_[(size_t)(id - base_id_)];
    }
    // Map::RemoveLandmark (src/map.cpp:42-51): erased from landmarks_ and active_landmarks_, which destroys it.  The slot becomes
    // null and the landmark is NOT archived (SaveOutputs writes landmarks_, which no longer has it); features keep the stale id,
    // and point(id) == nullptr is their expired weak_ptr.  The object is recycled.
    void RemoveLandmark(MapPoint *m)
    {
        if (!m) return;
        if (m->active) { active_landmarks_.erase(std::remove(active_landmarks_.begin(), active_landmarks_.end(), m), active_landmarks_.end()); m->active = false; }
        if (m->in_limbo) { limbo_.erase(std::remove(limbo_.begin(), limbo_.end(), m), limbo_.end()); m->in_limbo = false; }
        Unslot(m);
        m->observations.clear(); m->observed_times = 0;
        free_.push_back(m);
    }
    // A dead landmark back from its 20-byte archive record, for LocalFusion: in the reference Map::landmarks_ still owns it, so the
    // loop keyframe's feature can lock it.  Old id, the archived position widened to double (declared deviation: the reference
    // still has the double; the error is at most half an f32 ulp), no observations, not active, the anchor rebuilt from the
    // record's keyframe id (only the frame pointer of an anchor is ever dereferenced; its feature index is -1, which no real
    // observation has, so RemoveObservation's `anchor == f` can never take it for one of the list).  The record is superseded: the id is listed
    // once everywhere.  It waits in limbo like any unobserved landmark outside the window: observed again it leaves limbo, named
    // by nothing it is archived again at the next keyframe.  nullptr: the id is live already, or found in no record (keep_archive
    // off, or removed by an earlier fusion) - the reference's expired pointer.
    MapPoint *Revive(long id)
    {
        if (id < 0 || id >= next_id_ || point(id)) return nullptr;
        auto a = archive_.begin();
        while (a != archive_.end() && (long)a->id != id) ++a;
        if (a == archive_.end()) return nullptr;
        MapPoint *m;
        if (!free_.empty()) { m = free_.back(); free_.pop_back(); } else { pool_.emplace_back(); m = &pool_.back(); }
        m->id = id; m->is_outlier = false; m->active = false; m->in_limbo = false; m->observed_times = 0; m->seen_stamp = -1; m->observations.clear();
        for (int k = 0; k < 3; ++k) m->pos[k] = (double)a->pos[k];
        m->has_anchor = a->anchor_kf >= 0 && (size_t)a->anchor_kf < keyframes_.size();
        m->anchor = ObsRef{ m->has_anchor ? keyframes_[(size_t)a->anchor_kf] : nullptr, -1, true };
        archive_.erase(a);
        if (id >= base_id_) slots_[(size_t)(id - base_id_)] = m; else revived_[id] = m;
        ToLimbo(m);
        return m;
    }
    size_t num_revived_below_base() const { return revived_.size(); }
    // Map::landmarks_ still holds the id: live, or dead with an archive record (in the reference a dead landmark is an ordinary
    // member of landmarks_ that nothing observes).  Known, DropArchived and Revive scan the archive linearly, once per feature that
    // names a dead landmark: fine for a call that runs once per closed loop, not for a per-frame path
    bool Known(long id)
    {
        if (id < 0) return false;
        if (point(id)) return true;
        for (const ArchivedLandmark &a : archive_) if ((long)a.id == id) return true;
        return false;
    }
    // Map::RemoveLandmark of a dead landmark: its archive record goes, nothing else refers to it.  False: no record of that id
    bool DropArchived(long id)
    {
        for (auto a = archive_.begin(); a != archive_.end(); ++a)
            if ((long)a->id == id) { archive_.erase(a); return true; }
        return false;
    }
    size_t num_landmarks() const { return (size_t)next_id_; }                 // Map::landmarks_.size()
    size_t num_resident_landmarks() const { return pool_.size() - free_.size(); }
    void set_keep_archive(bool on) { keep_archive_ = on; }
    // on: a keyframe keeps its feature lists when it leaves the window, as the reference's do for good (LoopClosure reads
    // feature_left_ of old keyframes, src/loopclosure.cpp:343-346); off (default): they go back to the allocator
    void set_keep_features(bool on) { keep_features_ = on; }
    // device-map mode: a landmark the provider freed from its map (K::dmap_evicted) joins the same 20-byte archive (without an anchor)
    void ArchiveEvicted(int id, const float *pos) { if (keep_archive_) archive_.push_back(ArchivedLandmark{ (uint32_t)id, { pos[0], pos[1], pos[2] }, -1 }); }
    size_t num_archived() const { return archive_.size(); }
    // every landmark ever created, id-ascending (live ones with their current position, evicted ones as archived)
    std::vector<LandmarkRecord> AllLandmarks() const
    {
        std::vector<LandmarkRecord> o;
        o.reserve(archive_.size() + slots_.size());
        for (const ArchivedLandmark &a : archive_) o.push_back(LandmarkRecord{ (long)a.id, { a.pos[0], a.pos[1], a.pos[2] }, 0, false, (long)a.anchor_kf });
        for (const auto &r : revived_) { const MapPoint *m = r.second; o.push_back(LandmarkRecord{ m->id, { m->pos[0], m->pos[1], m->pos[2] }, m->observed_times, m->active, m->anchor_kf() }); }
        for (const MapPoint *m : slots_)
            if (m) o.push_back(LandmarkRecord{ m->id, { m->pos[0], m->pos[1], m->pos[2] }, m->observed_times, m->active, m->anchor_kf() });
        std::sort(o.begin(), o.end(), [](const LandmarkRecord &a, const LandmarkRecord &b) { return a.id < b.id; });
        return o;
    }

    void InsertMapPoint(MapPoint *mp)   // src/map.cpp:69-74
    {
        // landmarks_[id] = mp is implicit (slots_); ids are new, so appending keeps id order
        mp->active = true;
        active_landmarks_.push_back(mp);
    }
    void InsertKeyFrame(Frame *frame)   // src/map.cpp:53-67
    {
        current_frame_ = frame;
        keyframes_.push_back(frame);              // keyframe_id == index
        active_keyframes_.push_back(frame);
        if ((int)active_keyframes_.size() > num_active_keyframes_) RemoveOldKeyframe();
    }
    void AddObservation(MapPoint *mp, const ObsRef &f)   // src/mappoint.cpp:22-36
    {
        mp->observations.push_back(f);
        mp->observed_times++;
        if (!mp->has_anchor && !feat_of(f).outlier) { mp->anchor = f; mp->has_anchor = true; }      // :31-35
    }
    void RemoveObservation(MapPoint *mp, const ObsRef &f) // src/mappoint.cpp:38-78
    {
        if (!mp) return;
        for (size_t i = 0; i < mp->observations.size(); ++i) {
            if (mp->observations[i] == f) {
                mp->observations.erase_at(i);
                Feature &ft = feat_of(f);
                if (ft.outlier) ft.mp = -1;
                mp->observed_times--;
                if (mp->observed_times == 0 && !mp->active) ToLimbo(mp);   // re-observed after it left the window, now unobserved again
                break;
            }
        }
        // :60-76 — the anchor observation has become an outlier: the first remaining observation that is none and still names a
        // landmark takes over; with none left the anchor stays what it was (the reference keeps the stale feature)
        if (mp->has_anchor && mp->anchor == f && feat_of(f).outlier)
            for (size_t i = 0; i < mp->observations.size(); ++i) {
                const Feature &o = feat_of(mp->observations[i]);
                if (!o.outlier && o.mp >= 0) { mp->anchor = mp->observations[i]; break; }
            }
    }
    // every landmark SaveOutputs writes, archived ones first, then the revived ones below the id window, then the live ones: position and anchor keyframe (-1: none) out, the
    // re-anchored positions back in the same order (Pipeline::PoseGraphOptimization)
    void CollectAnchored(std::vector<double> &pts, std::vector<int> &anchor) const
    {
        for (const ArchivedLandmark &a : archive_) { for (int k = 0; k < 3; ++k) pts.push_back((double)a.pos[k]); anchor.push_back(a.anchor_kf); }
        for (const auto &r : revived_) { for (int k = 0; k < 3; ++k) pts.push_back(r.second->pos[k]); anchor.push_back((int)r.second->anchor_kf()); }
        for (const MapPoint *m : slots_) if (m) { for (int k = 0; k < 3; ++k) pts.push_back(m->pos[k]); anchor.push_back((int)m->anchor_kf()); }
    }
    // id -> archived float position of every dead landmark (Pipeline::VerifyLoops builds it once per call and stream; deque
    // elements do not move)
    void ArchiveIndex(std::unordered_map<long, const float *> &idx) const
    {
        idx.reserve(archive_.size());
        for (const ArchivedLandmark &a : archive_) idx[(long)a.id] = a.pos;
    }
    void StoreAnchored(const double *pts)
    {
        for (ArchivedLandmark &a : archive_) { for (int k = 0; k < 3; ++k) a.pos[k] = (float)pts[k]; pts += 3; }
        for (auto &r : revived_) { for (int k = 0; k < 3; ++k) r.second->pos[k] = pts[k]; pts += 3; }
        for (MapPoint *m : slots_) if (m) { for (int k = 0; k < 3; ++k) m->pos[k] = pts[k]; pts += 3; }
    }
    void CleanMap()                     // src/map.cpp:21-40
    {
        size_t keep = 0;
        for (MapPoint *m : active_landmarks_) {
            if (m->observed_times == 0) { m->active = false; ToLimbo(m); }   // out of the window; dead unless tracking still carries it
            else active_landmarks_[keep++] = m;
        }
        active_landmarks_.resize(keep);
    }
    // which keyframe leaves the window (src/map.cpp:76-120): the nearest one if it is closer than 0.2, else the farthest
    static Frame *ChooseKeyframeToRemove(const std::vector<Frame *> &active, Frame *current)
    {
        double max_dis = 0, min_dis = 999999;
        Frame *max_kf = nullptr, *min_kf = nullptr;
        SE3 Twc = current->pose.inverse();
        for (Frame *kf : active) {
            if (kf == current) continue;
            double dis = (kf->pose * Twc).log_norm();
            if (dis > max_dis) { max_dis = dis; max_kf = kf; }
            if (dis < min_dis) { min_dis = dis; min_kf = kf; }
        }
        const double min_dis_th = 0.2;
        // The reference indexes active_keyframes_ with the ids it found, default id 0 if no distance qualified (NaN after a
        // diverged pose: neither comparison holds; all distances exactly 0 still set min_kf_id): `.at(0)` removes keyframe 0
        // while it is in the window and throws std::out_of_range once it has left — the reference run ends there
        // (src/map.cpp:127-134; tests/ref_glue.py, the second reading, keeps that behaviour as a KeyError).  Declared
        // deviation: here the window always shrinks — the oldest active keyframe that is not the current one goes.
        Frame *rm = (min_dis < min_dis_th) ? min_kf : max_kf;
        if (!rm)
            for (Frame *kf : active) if (kf != current) { rm = kf; break; }
        return rm;
    }
    void RemoveOldKeyframe()            // src/map.cpp:76-181
    {
        if (!current_frame_) return;
        Frame *rm = ChooseKeyframeToRemove(active_keyframes_, current_frame_);
        if (!rm) return;
        active_keyframes_.erase(std::remove(active_keyframes_.begin(), active_keyframes_.end(), rm), active_keyframes_.end());
        for (size_t i = 0; i < rm->left.size(); ++i)
            if (rm->left[i].mp >= 0) RemoveObservation(point(rm->left[i].mp), ObsRef{ rm, (int)i, true });
        for (size_t i = 0; i < rm->right.size(); ++i) {
            if (!rm->right_ok[i]) continue;
            if (rm->right[i].mp >= 0) RemoveObservation(point(rm->right[i].mp), ObsRef{ rm, (int)i, false });
        }
        CleanMap();
        retired_.push_back(rm);
    }
    // The map no longer refers to the features of a keyframe that left the window (its
    // observations were removed above; Map::keyframes_ keeps the frame for its pose), so their
    // lists can go back to the allocator and the next keyframe reuses the memory instead of
    // faulting in fresh pages.  The caller decides when: a local BA still in flight holds
    // ObsRefs into the frames of the window it was gathered from.
    // `carried`: the feature list of the newest frame (what tracking carries forward from here), `stamp`: any number
    // that grows from call to call.  Landmarks in limbo (unobserved, outside the window) that the list does not
    // name are dead: archived and recycled.
    void ReleaseRetired(const std::vector<Feature> *carried = nullptr, long stamp = 0)
    {
        if (!keep_features_)
            for (Frame *rm : retired_) {
                std::vector<Feature>().swap(rm->left);
                std::vector<Feature>().swap(rm->right);
                std::vector<uint8_t>().swap(rm->right_ok);
            }
        retired_.clear();
        if (!carried || limbo_.empty()) return;
        for (const Feature &f : *carried)
            if (MapPoint *m = point(f.mp)) m->seen_stamp = stamp;
        size_t keep = 0;
        for (MapPoint *m : limbo_) {
            if (m->observed_times > 0 || m->active) { m->in_limbo = false; continue; }   // observed again: RemoveObservation brings it back
            if (m->seen_stamp == stamp) { limbo_[keep++] = m; continue; }                  // tracking still carries it
            m->in_limbo = false;
            Evict(m);
        }
        limbo_.resize(keep);
        // slide the id window past leading evicted ids
        size_t lead = 0;
        while (lead < slots_.size() && !slots_[lead]) ++lead;
        if (lead >= 1024 && lead * 2 >= slots_.size()) { slots_.erase(slots_.begin(), slots_.begin() + (long)lead); base_id_ += (long)lead; }
    }

    std::vector<Frame *> keyframes_, active_keyframes_;   // id-ascending
    std::vector<MapPoint *> active_landmarks_;            // id-ascending

private:
    struct ArchivedLandmark { uint32_t id; float pos[3]; int32_t anchor_kf; };     // 20 bytes; anchor_kf: MapPoint::anchor_kf() when it died
    void ToLimbo(MapPoint *m) { if (!m->in_limbo) { m->in_limbo = true; limbo_.push_back(m); } }
    void Evict(MapPoint *m)
    {
        if (keep_archive_) archive_.push_back(ArchivedLandmark{ (uint32_t)m->id, { (float)m->pos[0], (float)m->pos[1], (float)m->pos[2] }, (int32_t)m->anchor_kf() });
        Unslot(m);
        free_.push_back(m);
    }
    void Unslot(MapPoint *m) { if (m->id >= base_id_) slots_[(size_t)(m->id - base_id_)] = nullptr; else revived_.erase(m->id); }
    std::deque<MapPoint> pool_;               // MapPoint objects, recycled through free_
    std::vector<MapPoint *> free_, limbo_;    // limbo_: unobserved and outside the window, possibly still tracked
    std::vector<MapPoint *> slots_;           // id - base_id_ -> MapPoint (nullptr: evicted)
    std::map<long, MapPoint *> revived_;      // revived landmarks whose id the window has slid past (Revive); empty unless a loop was fused
    long base_id_ = 0, next_id_ = 0;
    std::deque<ArchivedLandmark> archive_;    // (a deque: grows by 512-byte blocks, no doubling reallocation)
    bool keep_archive_ = true, keep_features_ = false;
    std::vector<Frame *> retired_;            // left the window, feature lists not yet released
    Frame *current_frame_ = nullptr;
    int num_active_keyframes_;
};

// ------------------------------------------------------------------ per-stream state
struct FrameResult {
    double pose[7];
    int status;
    int is_keyframe;
    int n_features;
    int n_inliers;
    long frame_id;
    long keyframe_id;
};

struct Counters {                      // workload accounting for the roofline
    long long frames = 0, keyframes = 0;
    long long track_pts = 0, pose_edges = 0;
    long long gftt_calls = 0, gftt_rects = 0, corners = 0;
    long long right_pts = 0, tri_pts = 0;
    long long ba_calls = 0, ba_edges = 0, ba_kf = 0, ba_lm = 0, ba_iters = 0;
    long long ba_pairs = 0, ba_trials = 0;        // block pairs of the Schur complements, LM trials (the flop accounting of bench.py)
    long long pyr_left = 0, pyr_right = 0;
    long long ns_step = 0, ns_kernel_calls = 0;   // wall time inside step() / inside the C-ABI calls
    long long corners_dropped = 0, ba_skipped = 0; // per-stream capacity events (Config::max_*)
    // device-resident map: keyframes whose new landmarks did not all find a slot (there max_lm is the number of LIVE landmark
    // slots of a stream — active, observed-inactive, tracked, evictions waiting for the hand-over list — not the size of one BA
    // problem; the surplus points are not created and the run leaves the reference's), and the landmarks it did create
    long long lm_full = 0, lm_created_dev = 0;
};

// BA job bookkeeping between gather and scatter (per stream, reused)
struct BaGather {                // what Backend::Optimize keeps between building the problem and reading it back
    std::vector<Frame *> kfs;
    std::vector<MapPoint *> lms;
    std::vector<ObsRef> edge_feat;
    int nkf_ub = 0, nlm_ub = 0, nobs_ub = 0;     // sizes reserved for this problem in the batch arrays
    void clear() { kfs.clear(); lms.clear(); edge_feat.clear(); }
};

struct Stream {
    explicit Stream(const Config &c) : map(c.num_active_keyframes) {}
    Map map;
    FrontendStatus status = FrontendStatus::INITING;
    Frame *current = nullptr, *last = nullptr;
    std::unique_ptr<Frame> cur_owned, last_owned;       // non-keyframes
    std::vector<std::unique_ptr<Frame>> kf_store;        // keyframes live forever (Map::keyframes_)
    SE3 relative_motion;
    int tracking_inliers = 0;
    Frame *frontend_current_kf = nullptr, *frontend_prev_kf = nullptr;
    long frame_factory_id = 0, kf_factory_id = 0;
    int slot_prev = 0, slot_cur = 1, slot_right = 2;
    bool is_new_kf = false, init_ok = false;
    int dev_feat = 0;                    // features of the last frame held by the kernel provider (resident mode)
    // scratch between stages (per stream: the stages run one thread per stream)
    std::vector<int> tri_idx;
    BaGather ba;
    long long c_pose_edges = 0, c_keyframes = 0, c_corners = 0, c_dropped = 0;   // merged into Counters after the step
};

// ------------------------------------------------------------------ the staged pipeline
// Every stage has the shape  [serial: sizes -> offsets]  [parallel over streams: fill the
// batched arrays]  [ONE C-ABI call for all streams]  [parallel over streams: consume].
// does the kernel provider offer the ORB detector (HipKernels::orb_detect)?  The providers of the CPU twins do not.
template <class K> constexpr auto provider_has_orb(int) -> decltype(&K::orb_detect, true) { return true; }
template <class K> constexpr bool provider_has_orb(long) { return false; }
// and the oriented descriptors (HipKernels::orb_describe)?
template <class K> constexpr auto provider_has_orb_describe(int) -> decltype(&K::orb_describe, true) { return true; }
template <class K> constexpr bool provider_has_orb_describe(long) { return false; }

template <class K>
class Pipeline {
public:
    Pipeline(const Config &cfg, K &kernels, int nstreams, int host_threads = 1)
        : cfg_(cfg), k_(kernels), pool_(host_threads)
    {
        for (int s = 0; s < nstreams; ++s) {
            streams_.emplace_back(new Stream(cfg));
            streams_.back()->slot_prev = 3 * s;
            streams_.back()->slot_cur = 3 * s + 1;
            streams_.back()->slot_right = 3 * s + 2;
        }
        cfg_.cam_l.k4(cam_l_); cfg_.cam_r.k4(cam_r_);
    }
    ~Pipeline()
    {
        if (std::getenv("SVS_PIPE_PROFILE")) {
            const char *nm[9] = { "begin", "track-prep", "track-finish", "detect", "right", "tri", "ba-gather", "ba-scatter", "end" };
            double fr = (double)std::max<long long>(cnt_.frames / std::max(1, nstreams()), 1);
            std::fprintf(stderr, "[pipe %d streams, %d host threads] host ms/step:", nstreams(), pool_.size());
            for (int i = 0; i < 9; ++i) std::fprintf(stderr, " %s %.3f", nm[i], st_[i] / 1e6 / fr);
            std::fprintf(stderr, " | step %.3f abi %.3f\n", cnt_.ns_step / 1e6 / fr, cnt_.ns_kernel_calls / 1e6 / fr);
        }
    }
    int nstreams() const { return (int)streams_.size(); }
    const Counters &counters() const { return cnt_; }
    Stream &stream(int s) { return *streams_[s]; }
    bool map_on_host() const { return !(cfg_.device_map && cfg_.resident_track); }   // (svs_pipe_map_snapshot)
    // Which detector DetectFeatures runs: 0 = GFTT (src/frontend.cpp:24, the default), 1 = ORB (:20-33).  A setter and not a field
    // of the configuration, whose layout the CPU twin shares.  False (last_error(), nothing changed): another kind, a call after the
    // first frame, a provider without orb_detect, or ORB with device_map / resident_track: there GFTT is fused into the keyframe chain.
    bool SetDetector(int kind)
    {
        if (kind != 0 && kind != 1) return refuse("SetDetector: the detector is 0 (GFTT) or 1 (ORB)");
        if (cnt_.frames > 0) return refuse("SetDetector: the detector is chosen before the first frame");
        if (kind == 1) {
            if (!provider_has_orb<K>(0)) return refuse("SetDetector: this kernel provider has no ORB detector");
            if (cfg_.device_map || cfg_.resident_track)
                return refuse("SetDetector: the ORB detector runs on the host-map path only (device_map and resident_track off)");
        }
        detector_ = kind;
        return true;
    }
    int detector() const { return detector_; }

    // Frontend::AddFrame for every stream (src/frontend.cpp:690-721), in lockstep.
    // left/right: one image pointer per stream (host or device memory).
    void step(const void *const *left, const void *const *right, const int *strides, int is_device,
              FrameResult *out)
    {
        const int S = nstreams();
        const long long t_step0 = now_ns();
        std::vector<int> TS, IS, KS;
        long long t_b = now_ns();
        for (int s = 0; s < S; ++s) {
            Stream &st = *streams_[s];
            // Frame::CreateFrame (src/frame.cpp:22-28)
            st.cur_owned.reset(new Frame());
            st.current = st.cur_owned.get();
            st.current->id = st.frame_factory_id++;
            st.is_new_kf = false; st.init_ok = false;
            std::swap(st.slot_prev, st.slot_cur);   // last frame's pyramid becomes "prev"
            if (st.status == FrontendStatus::INITING) IS.push_back(s);
            else if (st.status == FrontendStatus::LOST) { st.dev_feat = 0; /* Reset(): not implemented upstream (:723-731); the frame gets no features */ }
            else TS.push_back(s);
        }
        cnt_.frames += S;
        st_[0] += now_ns() - t_b;
        if (!TS.empty()) {
            if (resident()) {
                TrackResidentRun(TS, left, strides, is_device);
                { STimer t_(st_[2]); pool_.parallel_for((int)TS.size(), [&](int i) { TrackFinishResident(TS[i], i); }); }
            } else {
                TrackPrepareAndRun(TS, left, strides, is_device);
                { STimer t_(st_[2]); pool_.parallel_for((int)TS.size(), [&](int i) { TrackFinish(TS[i], i); }); }
            }
            for (int s : TS) if (streams_[s]->is_new_kf) KS.push_back(s);
        }
        std::vector<int> DS = IS;                 // streams that detect this frame
        DS.insert(DS.end(), KS.begin(), KS.end());
        std::vector<int> MS;                      // streams that triangulate + BA
        if (device_map()) {
            // backend_on 2: the local BA of the last keyframe step runs beside the tracking (a second stream of the provider's
            // context); its result lands backend_lag frames later, or before the next keyframe step touches the map
            if (dm_inflight_ && (++ba_age_ >= std::max(1, cfg_.backend_lag) || !DS.empty())) DmCollect();
            if (!DS.empty()) KeyframeOnDevice(IS, KS, left, right, strides, is_device, MS);
        } else if (!DS.empty()) {
            BuildPyramids(IS, DS, left, right, strides, is_device);
            DetectFeatures(DS);
            FindFeaturesInRight(DS);
            for (int s : IS) {
                Stream &st = *streams_[s];
                int good = 0;
                for (uint8_t ok : st.current->right_ok) good += ok ? 1 : 0;
                if (good >= cfg_.num_features_init) { st.init_ok = true; MS.push_back(s); }   // :227
            }
            MS.insert(MS.end(), KS.begin(), KS.end());
            if (!MS.empty()) Triangulate(MS);
        }
        // Backend::UpdateMap (src/frontend.cpp:281 / src/backend.cpp:14-18).  backend_on 1: the
        // optimisation completes before the next frame (deterministic stand-in for "the backend
        // thread was fast").  backend_on 2: it runs beside the next frame's Track() like the
        // reference's Backend thread, and its result lands after that frame — always exactly one
        // frame late, so runs stay reproducible.
        if (device_map()) {
            // everything below happened on the device
        } else if (cfg_.backend_on == 1 && backend_enabled_) {
            for (int s : MS) ReleaseRetired(*streams_[s]);           // nothing in flight
            if (!MS.empty()) { BackendSubmit(MS); BackendCollect(); }
        } else if (cfg_.backend_on >= 2 && backend_enabled_) {
            if (ba_inflight_ && (++ba_age_ >= std::max(1, cfg_.backend_lag) || !MS.empty()))
                BackendCollect();                                    // may still touch frames retired this step
            for (int s : MS) ReleaseRetired(*streams_[s]);
            if (!MS.empty()) { BackendSubmit(MS); ba_age_ = 0; }
        } else {
            BackendCollect();
            for (int s : MS) ReleaseRetired(*streams_[s]);
        }
        // frames whose feature list or map points changed on the host (init, keyframes, BA) replace
        // the resident copy; every other frame's list never left the device
        if (resident() && !device_map() && !DS.empty()) UploadFeatures(DS);
        if (on_keyframe) for (int s : MS) on_keyframe(s, *streams_[s]->current);
        long long t_e = now_ns();
        for (int s : TS) {
            Stream &st = *streams_[s];
            st.relative_motion = st.current->pose * st.last->pose.inverse();   // src/frontend.cpp:685
        }
        for (int s = 0; s < S; ++s) {
            Stream &st = *streams_[s];
            FrameResult &r = out[s];
            std::memcpy(r.pose, st.current->pose.v, sizeof(r.pose));
            r.status = (int)st.status;
            r.is_keyframe = st.current->is_keyframe ? 1 : 0;
            r.n_features = resident() ? st.dev_feat : (int)st.current->left.size();
            r.n_inliers = st.tracking_inliers;
            r.frame_id = st.current->id;
            r.keyframe_id = st.current->is_keyframe ? st.current->keyframe_id : -1;
            // last_frame_ = current_frame_ (src/frontend.cpp:718)
            st.last = st.current;
            st.last_owned = std::move(st.cur_owned);   // null if the frame moved into kf_store
            cnt_.pose_edges += st.c_pose_edges; cnt_.keyframes += st.c_keyframes; cnt_.corners += st.c_corners;
            cnt_.corners_dropped += st.c_dropped;
            st.c_pose_edges = st.c_keyframes = st.c_corners = st.c_dropped = 0;
        }
        st_[8] += now_ns() - t_e;
        cnt_.ns_step += now_ns() - t_step0;
    }

    // VisualOdometry::saveSLAMOutputInFile (src/visual_odometry.cpp:198-310): keyframes.txt
    // (dataset dir, left camera index, then `frame_id r00 r01 r02 tx r10 ... tz` of T_cw per
    // keyframe in keyframe order, default ostream precision) and landmarks.pcd in the layout
    // of pcl::io::savePCDFileASCII (float x y z, precision 8).  Consumed by the reference's
    // DenseReconstruction::Initialize (src/dense_reconstruction.cpp:35-74).
    bool SaveOutputs(int s, const std::string &dir, const std::string &dataset_dir, int left_cam_index)
    {
        Stream &st = *streams_[s];
        std::ofstream pcd(dir + "/landmarks.pcd");
        if (!pcd) return false;
        std::vector<LandmarkRecord> all = AllLandmarks(s);
        const size_t n = all.size();
        pcd << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\n"
            << "COUNT 1 1 1\nWIDTH " << n << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << n << "\nDATA ascii\n";
        pcd << std::setprecision(8);
        for (const LandmarkRecord &m : all) pcd << (float)m.pos[0] << " " << (float)m.pos[1] << " " << (float)m.pos[2] << "\n";
        std::ofstream kf(dir + "/keyframes.txt");
        if (!kf) return false;
        kf << dataset_dir << std::endl << left_cam_index << std::endl;
        for (const Frame *f : st.map.keyframes_) {
            const double *q = f->pose.v;
            const double x = q[0], y = q[1], z = q[2], w = q[3];
            const double R[9] = { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) };
            kf << f->id << " ";
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) {
                    kf << (j < 3 ? R[i * 3 + j] : q[4 + i]);
                    if (i * 4 + j < 11) kf << " "; else kf << std::endl;
                }
        }
        return true;
    }

    // Map::landmarks_ of stream s (src/map.h:15): every landmark ever created, id-ascending — wherever the map lives
    std::vector<LandmarkRecord> AllLandmarks(int s)
    {
        Stream &st = *streams_[s];
        std::vector<LandmarkRecord> all = st.map.AllLandmarks();
        if (device_map()) {
            // the map lives in the provider's memory: the archive of what it freed (above) + the landmarks it still holds
            const int NL = cfg_.max_lm;
            std::vector<int> id((size_t)NL), obs((size_t)NL);
            std::vector<double> pos(3 * (size_t)NL);
            std::vector<uint8_t> stt((size_t)NL);
            check(k_.dmap_read(s, nullptr, nullptr, nullptr, nullptr, id.data(), pos.data(), obs.data(), stt.data()), "dmap_read");
            for (int l = 0; l < NL; ++l)
                if (id[(size_t)l] >= 0) all.push_back(LandmarkRecord{ id[(size_t)l], { pos[3 * (size_t)l], pos[3 * (size_t)l + 1], pos[3 * (size_t)l + 2] }, obs[(size_t)l], stt[(size_t)l] == 1 });
            std::sort(all.begin(), all.end(), [](const LandmarkRecord &a, const LandmarkRecord &b) { return a.id < b.id; });
        }
        return all;
    }
    bool MapOnDevice() const { return device_map(); }

    // Frame::loop_keyframe_ / loop_relative_pose_ as LoopClosure sets them after a confirmed loop (src/loopclosure.cpp:598-606): at
    // most one loop per keyframe, a later call replaces it.  T_rel = T_kf * T_loop^-1 as measured.  Refused (false, last_error()):
    // a stream or an id that is not a keyframe of it, loop_kf_id >= kf_id, a rotation that is not a unit quaternion.
    bool AddLoopEdge(int s, long kf_id, long loop_kf_id, const SE3 &T_rel)
    {
        if (s < 0 || s >= nstreams()) return refuse("AddLoopEdge: no such stream");
        std::vector<Frame *> &kfs = streams_[s]->map.keyframes_;
        if (kf_id < 0 || kf_id >= (long)kfs.size() || loop_kf_id < 0 || loop_kf_id >= (long)kfs.size()) return refuse("AddLoopEdge: not a keyframe id of this stream");
        if (loop_kf_id >= kf_id) return refuse("AddLoopEdge: the loop keyframe must be older than the keyframe");
        const double *q = T_rel.v;
        if (!(std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 2e-6)) return refuse("AddLoopEdge: the relative pose's quaternion is not of unit length");
        kfs[(size_t)kf_id]->loop_keyframe = kfs[(size_t)loop_kf_id];
        kfs[(size_t)kf_id]->loop_relative_pose = T_rel;
        return true;
    }
    // LoopClosure::PoseGraphOptimization (src/loopclosure.cpp:641-799) for the given streams in ONE call of the kernel provider:
    // per stream every keyframe a vertex (keyframe 0 fixed, :701-704), an edge (kf, prev, relative_pose_pkf) per keyframe with a
    // previous one (:720-735) and (kf, loop, loop_relative_pose) where AddLoopEdge set one (:738-753), every landmark SaveOutputs
    // writes re-anchored to the keyframe of its first valid observation (:760-784); then the poses are written back (:787-790)
    // and relative_pose_pkf recomputed from them like after a local BA (src/backend.cpp:243-245).  A local BA in flight is
    // collected first.  False (last_error()): device_map = 1 (nothing done), an unknown stream, the provider's refusal.
    struct PoseGraphStats { int nkf, nedge, npt, iters, trials; double chi2_before, chi2_after; };
    bool PoseGraphOptimization(const std::vector<int> &streams, int iters = 22, std::vector<PoseGraphStats> *stats = nullptr)
    {
        if (device_map()) return refuse("PoseGraphOptimization: with device_map = 1 the landmarks live on the device without anchors; not supported yet");
        for (int s : streams) if (s < 0 || s >= nstreams()) return refuse("PoseGraphOptimization: no such stream");
        Flush();
        const int n = (int)streams.size();
        std::vector<svslam_pg_job> jobs((size_t)n);
        std::vector<double> poses, meas, pts;
        std::vector<uint8_t> fixed;
        std::vector<int> ea, eb, anchor;
        for (int j = 0; j < n; ++j) {
            Map &m = streams_[streams[(size_t)j]]->map;
            svslam_pg_job &J = jobs[(size_t)j];
            std::memset(&J, 0, sizeof(J));
            J.kf_ofs = (int)fixed.size(); J.edge_ofs = (int)ea.size(); J.pt_ofs = (int)anchor.size();
            for (const Frame *kf : m.keyframes_) {                      // keyframe_id == index
                poses.insert(poses.end(), kf->pose.v, kf->pose.v + 7);
                fixed.push_back(kf->keyframe_id == 0 ? 1 : 0);
                if (kf->prev_keyframe) { ea.push_back((int)kf->keyframe_id); eb.push_back((int)kf->prev_keyframe->keyframe_id); meas.insert(meas.end(), kf->relative_pose_pkf.v, kf->relative_pose_pkf.v + 7); }
                if (kf->loop_keyframe) { ea.push_back((int)kf->keyframe_id); eb.push_back((int)kf->loop_keyframe->keyframe_id); meas.insert(meas.end(), kf->loop_relative_pose.v, kf->loop_relative_pose.v + 7); }
            }
            m.CollectAnchored(pts, anchor);
            J.nkf = (int)fixed.size() - J.kf_ofs; J.nedge = (int)ea.size() - J.edge_ofs; J.npt = (int)anchor.size() - J.pt_ofs;
        }
        if (k_.pose_graph(n, jobs.data(), (int)fixed.size(), poses.data(), fixed.data(), (int)ea.size(), ea.data(), eb.data(), meas.data(),
                          (int)anchor.size(), anchor.data(), pts.data(), iters) != 0)
            return refuse(std::string("PoseGraphOptimization: ") + k_.last_error());
        for (int j = 0; j < n; ++j) {
            Map &m = streams_[streams[(size_t)j]]->map;
            const svslam_pg_job &J = jobs[(size_t)j];
            for (size_t i = 0; i < m.keyframes_.size(); ++i) m.keyframes_[i]->pose = SE3(poses.data() + 7 * ((size_t)J.kf_ofs + i));
            for (Frame *kf : m.keyframes_) if (kf->prev_keyframe) kf->relative_pose_pkf = kf->pose * kf->prev_keyframe->pose.inverse();
            m.StoreAnchored(pts.data() + 3 * (size_t)J.pt_ofs);
            if (stats) stats->push_back(PoseGraphStats{ J.nkf, J.nedge, J.npt, J.iters_done, J.n_trials, J.chi2_before, J.chi2_after });
        }
        return true;
    }
    // LoopClosure::KeypointMatchWithLoopCandid + CalculatePose (src/loopclosure.cpp:286-437, as called at :831-862) for every query
    // in ONE call of the kernel provider.  A query names a keyframe and an older candidate keyframe of one stream and brings the
    // 256-bit descriptors of both with desc_feat_indx, the reference's map from descriptor row to index in feature_left_.  The
    // current keyframe's pixels come from kf->left; the candidate's landmarks from Map::point(id), or for a dead landmark from the
    // stream's archive (a float position: what the reference's cv::Point3f cast keeps anyway); mp == -1 or an id found in neither
    // place (keep_archive off) is has_xyz = 0, the reference's expired weak_ptr.  Every ACCEPTED result is recorded with
    // AddLoopEdge(stream, kf, cand, T_rel).  LocalFusion (:439-582) is not done here (Pipeline::LocalFusion, or DetectLoops with
    // local_fusion): the result carries T_corr, need_correction and the matches (descriptor rows) for it.  A local BA in flight is collected first.  False (last_error(), nothing done):
    // device_map = 1, an unknown stream, ids that are not keyframes, cand >= kf, a desc_feat_indx entry out of range or repeated,
    // negative counts or null arrays, the provider's refusal.
    struct LoopQuery {
        int stream; long kf_id, cand_kf_id;
        int nq; const uint8_t *desc_q; int nfq; const int *feat_q;      // current keyframe: descriptors [nq][32], desc_feat_indx [nfq], nfq == nq
        int nc; const uint8_t *desc_c; int nfc; const int *feat_c;      // candidate keyframe
    };
    struct LoopResult {
        int status = 0, n_matches = 0, n_points = 0, n_inliers = 0; bool need_correction = false;
        SE3 T_corr, T_rel; double d = 0;
        std::vector<int> match_c, match_q, match_dist;          // descriptor rows; the features are feat_c[match_c[i]], feat_q[match_q[i]]
        std::vector<uint8_t> match_inlier;
    };
    bool VerifyLoops(const std::vector<LoopQuery> &queries, const svslam_loop_params &params, std::vector<LoopResult> *results)
    {
        if (device_map()) return refuse("VerifyLoops: with device_map = 1 the landmarks live on the device without anchors; not supported yet");
        for (const LoopQuery &q : queries) {
            if (q.stream < 0 || q.stream >= nstreams()) return refuse("VerifyLoops: no such stream");
            const std::vector<Frame *> &kfs = streams_[q.stream]->map.keyframes_;
            if (q.kf_id < 0 || q.kf_id >= (long)kfs.size() || q.cand_kf_id < 0 || q.cand_kf_id >= (long)kfs.size()) return refuse("VerifyLoops: not a keyframe id of this stream");
            if (q.cand_kf_id >= q.kf_id) return refuse("VerifyLoops: the candidate keyframe must be older than the keyframe");
            if (q.nq < 0 || q.nc < 0 || q.nq != q.nfq || q.nc != q.nfc) return refuse("VerifyLoops: the descriptor count and the index count differ");
            if ((q.nq > 0 && (!q.desc_q || !q.feat_q)) || (q.nc > 0 && (!q.desc_c || !q.feat_c))) return refuse("VerifyLoops: null descriptors or desc_feat_indx");
            for (int side = 0; side < 2; ++side) {
                const int n = side ? q.nc : q.nq; const int *idx = side ? q.feat_c : q.feat_q;
                const size_t nf = kfs[(size_t)(side ? q.cand_kf_id : q.kf_id)]->left.size();
                if (n > 0 && nf == 0) return refuse("VerifyLoops: the keyframe's feature list was released when it left the window (SetKeepKeyframeFeatures)");
                std::vector<uint8_t> seen(nf, 0);
                for (int i = 0; i < n; ++i) {
                    if (idx[i] < 0 || (size_t)idx[i] >= nf) return refuse("VerifyLoops: a desc_feat_indx entry is not a feature of its keyframe");
                    if (seen[(size_t)idx[i]]) return refuse("VerifyLoops: a desc_feat_indx entry is repeated");
                    seen[(size_t)idx[i]] = 1;
                }
            }
        }
        Flush();
        const int n = (int)queries.size();
        std::vector<svslam_loop_job> jobs((size_t)n);
        std::vector<uint8_t> desc_c, desc_q, has;
        std::vector<double> xyz;
        std::vector<float> uv;
        ArchiveCache archive;
        for (int j = 0; j < n; ++j) {
            const LoopQuery &q = queries[(size_t)j];
            Map &m = streams_[q.stream]->map;
            const Frame *kf = m.keyframes_[(size_t)q.kf_id], *cand = m.keyframes_[(size_t)q.cand_kf_id];
            svslam_loop_job &J = jobs[(size_t)j];
            std::memset(&J, 0, sizeof(J));
            J.c_ofs = (int)has.size(); J.nc = q.nc; J.q_ofs = (int)(uv.size() / 2); J.nq = q.nq;
            std::memcpy(J.T_cur, kf->pose.v, sizeof(J.T_cur)); std::memcpy(J.T_cand, cand->pose.v, sizeof(J.T_cand));
            if (q.nq) desc_q.insert(desc_q.end(), q.desc_q, q.desc_q + 32 * (size_t)q.nq);
            if (q.nc) desc_c.insert(desc_c.end(), q.desc_c, q.desc_c + 32 * (size_t)q.nc);
            for (int i = 0; i < q.nq; ++i) { const Feature &f = kf->left[(size_t)q.feat_q[i]]; uv.push_back(f.x); uv.push_back(f.y); }
            for (int i = 0; i < q.nc; ++i) {
                const long id = cand->left[(size_t)q.feat_c[i]].mp;
                double p[3] = { 0, 0, 0 };
                const uint8_t ok = LandmarkPosition(q.stream, id, archive, p) ? 1 : 0;
                xyz.push_back(p[0]); xyz.push_back(p[1]); xyz.push_back(p[2]); has.push_back(ok);
            }
        }
        svslam_loop_params P = params;
        std::memcpy(P.cam, cam_l_, sizeof(P.cam)); std::memcpy(P.ext_l, cfg_.cam_l.pose.v, sizeof(P.ext_l));
        const int tc = (int)has.size(), tq = (int)(uv.size() / 2);
        std::vector<int> mc((size_t)tc), mq((size_t)tc), md((size_t)tc);
        std::vector<uint8_t> mi((size_t)tc);
        if (k_.loop_verify(n, jobs.data(), &P, tc, desc_c.data(), xyz.data(), has.data(), tq, desc_q.data(), uv.data(), mc.data(), mq.data(), md.data(), mi.data()) != 0)
            return refuse(std::string("VerifyLoops: ") + k_.last_error());
        if (results) results->clear();
        for (int j = 0; j < n; ++j) {
            const svslam_loop_job &J = jobs[(size_t)j];
            if (J.status == SVSLAM_LOOP_ACCEPTED) AddLoopEdge(queries[(size_t)j].stream, queries[(size_t)j].kf_id, queries[(size_t)j].cand_kf_id, SE3(J.T_rel));
            if (!results) continue;
            LoopResult R;
            R.status = J.status; R.n_matches = J.n_matches; R.n_points = J.n_points; R.n_inliers = J.n_inliers; R.need_correction = J.need_correction != 0;
            R.T_corr = SE3(J.T_corr); R.T_rel = SE3(J.T_rel); R.d = J.d;
            R.match_c.assign(mc.begin() + J.c_ofs, mc.begin() + J.c_ofs + J.n_matches); R.match_q.assign(mq.begin() + J.c_ofs, mq.begin() + J.c_ofs + J.n_matches);
            R.match_dist.assign(md.begin() + J.c_ofs, md.begin() + J.c_ofs + J.n_matches); R.match_inlier.assign(mi.begin() + J.c_ofs, mi.begin() + J.c_ofs + J.n_matches);
            results->push_back(std::move(R));
        }
        return true;
    }
    // Keyframes that leave the window from now on keep their feature lists (Map::set_keep_features): VerifyLoops needs the
    // candidate's.  Off by default: the host store of a long run stays as small as before.
    void SetKeepKeyframeFeatures(bool on) { for (auto &st : streams_) st->map.set_keep_features(on); }
    // the position VerifyLoops uses for landmark `id` of stream s: the live landmark's, else the archived float one; false: id == -1
    // or found in neither place.  The archive's id index of a stream is built when its first dead landmark is asked for.
    typedef std::unordered_map<int, std::unordered_map<long, const float *>> ArchiveCache;
    bool LandmarkPosition(int s, long id, ArchiveCache &cache, double *p)
    {
        if (id < 0) return false;
        Map &m = streams_[s]->map;
        if (const MapPoint *mp = m.point(id)) { p[0] = mp->pos[0]; p[1] = mp->pos[1]; p[2] = mp->pos[2]; return true; }
        auto it = cache.find(s);
        if (it == cache.end()) { it = cache.emplace(s, std::unordered_map<long, const float *>()).first; m.ArchiveIndex(it->second); }
        auto a = it->second.find(id);
        if (a == it->second.end()) return false;
        p[0] = a->second[0]; p[1] = a->second[1]; p[2] = a->second[2];
        return true;
    }
    // the left features of a keyframe, read-only: what a descriptor front end samples at, and what VerifyLoops would gather for
    // them.  8 doubles each: x, y, landmark id or -1, outlier flag, has_xyz, X, Y, Z.  pose7 (optional): the keyframe's pose.
    bool KeyframeFeatures(int s, long kf_id, std::vector<double> *out8, double *pose7)
    {
        if (device_map()) return refuse("KeyframeFeatures: with device_map = 1 the keyframes' features live on the device");
        if (s < 0 || s >= nstreams()) return refuse("KeyframeFeatures: no such stream");
        const std::vector<Frame *> &kfs = streams_[s]->map.keyframes_;
        if (kf_id < 0 || kf_id >= (long)kfs.size()) return refuse("KeyframeFeatures: not a keyframe id of this stream");
        Flush();
        ArchiveCache archive;
        out8->clear();
        for (const Feature &f : kfs[(size_t)kf_id]->left) {
            double p[3] = { 0, 0, 0 };
            const bool ok = LandmarkPosition(s, f.mp, archive, p);
            const double row[8] = { f.x, f.y, (double)f.mp, f.outlier ? 1.0 : 0.0, ok ? 1.0 : 0.0, p[0], p[1], p[2] };
            out8->insert(out8->end(), row, row + 8);
        }
        if (pose7) std::memcpy(pose7, kfs[(size_t)kf_id]->pose.v, 56);
        return true;
    }
    // LoopClosure::ExtractKeypointsDescriptor (src/loopclosure.cpp:131-171) for every stream whose last step made a keyframe that has
    // no descriptors yet: BRIEF-256 (svslam_brief_describe_batch) at the non-outlier left features (:142-148) of the
    // keyframe, on level 0 of slot_cur, where the keyframe's left image still is until the stream's next step.  ONE provider call
    // for all streams.  Frame::desc_feat_indx[row] is the feature's own index: the reference recovers it by comparing positions
    // (:154-165), which maps two features at one pixel to the first of them.  The reference describes in its loop-closure thread,
    // some frames later, when the backend may have flagged more outliers; here it is right after the keyframe's step.  A local BA
    // in flight is collected first (the provider's context is its until then).  params: nullptr for the default table, -1 degree,
    // edge 31.  n_described (optional): keyframes described by this call.  False (last_error(), nothing stored): device_map = 1,
    // the provider's refusal (e.g. more than 1024 non-outlier features).
    bool DescribeNewKeyframes(const svslam_brief_params *params = nullptr, int *n_described = nullptr)
    {
        if (n_described) *n_described = 0;
        if (device_map()) return refuse("DescribeNewKeyframes: with device_map = 1 the keyframes' features live on the device; not supported yet");
        Flush();
        DescribeSet D;
        CollectUndescribed(D);
        if (D.kfs.empty()) return true;
        const int total = (int)D.feats.size();
        std::vector<svslam_brief_job> jobs(D.kfs.size());
        for (size_t j = 0; j < jobs.size(); ++j) { std::memset(&jobs[j], 0, sizeof(jobs[j])); jobs[j].slot = D.slot[j]; jobs[j].pt_ofs = D.ofs[j]; jobs[j].npts = (int)D.sel[j].size(); }
        std::vector<float> xy(2 * (size_t)total + 2);
        for (int i = 0; i < total; ++i) { xy[2 * (size_t)i] = D.feats[(size_t)i]->x; xy[2 * (size_t)i + 1] = D.feats[(size_t)i]->y; }
        svslam_brief_params P;
        if (params) P = *params; else { P.pattern = nullptr; P.angle_deg = -1.0f; P.edge = 31; }
        std::vector<uint8_t> desc(32 * (size_t)total + 1);
        std::vector<int> dpt((size_t)total + 1);
        if (k_.brief_describe((int)jobs.size(), jobs.data(), &P, total, xy.data(), desc.data(), dpt.data()) != 0)
            return refuse(std::string("DescribeNewKeyframes: ") + k_.last_error());
        for (size_t j = 0; j < jobs.size(); ++j) StoreDescriptors(D, j, jobs[j].n_desc, desc, dpt);
        if (n_described) *n_described = (int)D.kfs.size();
        return true;
    }
    // DescribeNewKeyframes with every feature described at its own angle and octave (svslam_orb_describe_batch): what
    // cv::ORB::compute does with Feature::position_ when the detector is ORB.  The same selection rule, storage and refusals; a
    // tracked feature and a GFTT corner carry -1 degree and octave 0, so with GFTT the rows are DescribeNewKeyframes' rows.
    // params: nullptr for the default table, edge 31, 8 levels.  Instantiated only where it is called: the provider needs orb_describe.
    bool DescribeNewKeyframesOriented(const svslam_orb_desc_params *params = nullptr, int *n_described = nullptr)
    {
        if (n_described) *n_described = 0;
        if (device_map()) return refuse("DescribeNewKeyframesOriented: with device_map = 1 the keyframes' features live on the device; not supported yet");
        Flush();
        DescribeSet D;
        CollectUndescribed(D);
        if (D.kfs.empty()) return true;
        const int total = (int)D.feats.size();
        std::vector<svslam_orb_desc_job> jobs(D.kfs.size());
        for (size_t j = 0; j < jobs.size(); ++j) { std::memset(&jobs[j], 0, sizeof(jobs[j])); jobs[j].slot = D.slot[j]; jobs[j].pt_ofs = D.ofs[j]; jobs[j].npts = (int)D.sel[j].size(); }
        std::vector<svslam_orb_kp> kps((size_t)total + 1);
        for (int i = 0; i < total; ++i) { const Feature &F = *D.feats[(size_t)i]; kps[(size_t)i] = svslam_orb_kp{ F.x, F.y, 0.f, F.angle, 0.f, (int)F.octave }; }
        svslam_orb_desc_params P;
        if (params) P = *params; else std::memset(&P, 0, sizeof(P));
        std::vector<uint8_t> desc(32 * (size_t)total + 1);
        std::vector<int> dpt((size_t)total + 1);
        if (k_.orb_describe((int)jobs.size(), jobs.data(), &P, total, kps.data(), desc.data(), dpt.data()) != 0)
            return refuse(std::string("DescribeNewKeyframesOriented: ") + k_.last_error());
        for (size_t j = 0; j < jobs.size(); ++j) StoreDescriptors(D, j, jobs[j].n_desc, desc, dpt);
        if (n_described) *n_described = (int)D.kfs.size();
        return true;
    }
    // what both describe calls share.  CollectUndescribed: every stream whose last step made a keyframe that has no descriptors yet,
    // its slot, the indices of its non-outlier left features (sel) and those features in one list, job j's from ofs[j] on.
    // StoreDescriptors: the first n_desc rows of job j become the keyframe's; desc_feat_indx[row] = the feature's own index.
    struct DescribeSet {
        std::vector<Frame *> kfs;
        std::vector<int> slot, ofs;
        std::vector<std::vector<int>> sel;
        std::vector<const Feature *> feats;
    };
    void CollectUndescribed(DescribeSet &D)
    {
        for (auto &stp : streams_) {
            Frame *f = stp->last;
            if (!f || !f->is_keyframe || f->described) continue;
            D.kfs.push_back(f); D.slot.push_back(stp->slot_cur); D.ofs.push_back((int)D.feats.size());
            D.sel.emplace_back();
            for (size_t i = 0; i < f->left.size(); ++i)
                if (!f->left[i].outlier) { D.sel.back().push_back((int)i); D.feats.push_back(&f->left[i]); }
        }
    }
    static void StoreDescriptors(const DescribeSet &D, size_t j, int n_desc, const std::vector<uint8_t> &desc, const std::vector<int> &dpt)
    {
        Frame *f = D.kfs[j];
        const size_t o = (size_t)D.ofs[j];
        f->desc.assign(desc.begin() + 32 * o, desc.begin() + 32 * (o + (size_t)n_desc));
        f->desc_feat_indx.resize((size_t)n_desc);
        for (int r = 0; r < n_desc; ++r) f->desc_feat_indx[(size_t)r] = D.sel[j][(size_t)dpt[o + (size_t)r]];
        f->described = true;
    }
    // x, y, angle, octave of every left feature of a keyframe, in the order of keyframe_features: what a test compares the stored rows
    // with.  rows: [n][4] floats or nullptr; returns n, or -1 for a bad stream / id
    long KeyframeKeypoints(int s, long kf_id, float *rows, long cap)
    {
        if (s < 0 || s >= nstreams()) { refuse("KeyframeKeypoints: no such stream"); return -1; }
        const std::vector<Frame *> &kfs = streams_[s]->map.keyframes_;
        if (kf_id < 0 || kf_id >= (long)kfs.size()) { refuse("KeyframeKeypoints: not a keyframe id of this stream"); return -1; }
        const Frame *f = kfs[(size_t)kf_id];
        const long n = (long)f->left.size();
        if (rows && cap >= n)
            for (long i = 0; i < n; ++i) {
                const Feature &F = f->left[(size_t)i];
                rows[4 * i] = F.x; rows[4 * i + 1] = F.y; rows[4 * i + 2] = F.angle; rows[4 * i + 3] = (float)F.octave;
            }
        return n;
    }
    // the stored descriptors of a keyframe, read-only: rows of 32 bytes and desc_feat_indx.  False: a bad stream / id, or a keyframe
    // that was never described (which is not a keyframe described with zero rows)
    bool KeyframeDescriptors(int s, long kf_id, const std::vector<uint8_t> **desc, const std::vector<int> **feat)
    {
        if (s < 0 || s >= nstreams()) return refuse("KeyframeDescriptors: no such stream");
        const std::vector<Frame *> &kfs = streams_[s]->map.keyframes_;
        if (kf_id < 0 || kf_id >= (long)kfs.size()) return refuse("KeyframeDescriptors: not a keyframe id of this stream");
        const Frame *f = kfs[(size_t)kf_id];
        if (!f->described) return refuse("KeyframeDescriptors: the keyframe was never described (DescribeNewKeyframes after its step)");
        if (desc) *desc = &f->desc;
        if (feat) *feat = &f->desc_feat_indx;
        return true;
    }
    // VerifyLoops on the descriptors DescribeNewKeyframes stored: the queries are built from Frame::desc / desc_feat_indx of both
    // keyframes and handed to VerifyLoops unchanged.  False (nothing done): what VerifyLoops refuses, and a keyframe that was never
    // described.
    struct LoopPair { int stream; long kf_id, cand_kf_id; };
    bool VerifyLoopsStored(const std::vector<LoopPair> &pairs, const svslam_loop_params &params, std::vector<LoopResult> *results)
    {
        std::vector<LoopQuery> qs;
        for (const LoopPair &p : pairs) {
            if (p.stream < 0 || p.stream >= nstreams()) return refuse("VerifyLoopsStored: no such stream");
            const std::vector<Frame *> &kfs = streams_[p.stream]->map.keyframes_;
            if (p.kf_id < 0 || p.kf_id >= (long)kfs.size() || p.cand_kf_id < 0 || p.cand_kf_id >= (long)kfs.size())
                return refuse("VerifyLoopsStored: not a keyframe id of this stream");
            const Frame *q = kfs[(size_t)p.kf_id], *c = kfs[(size_t)p.cand_kf_id];
            if (!q->described || !c->described) return refuse("VerifyLoopsStored: a keyframe of the pair was never described (DescribeNewKeyframes after its step)");
            const int nq = (int)q->desc_feat_indx.size(), nc = (int)c->desc_feat_indx.size();
            qs.push_back(LoopQuery{ p.stream, p.kf_id, p.cand_kf_id, nq, q->desc.data(), nq, q->desc_feat_indx.data(), nc, c->desc.data(), nc, c->desc_feat_indx.data() });
        }
        return VerifyLoops(qs, params, results);
    }
    // The network behind the global image descriptor (svslam_gdesc_configure): a table of layers, its parameters and the
    // preprocessing (nullptr: the reference's call).  Replaces the network configured before; a refusal keeps that one.
    bool ConfigureGlobalDescriptor(int nlayers, const svslam_gd_layer *layers, const float *params, long long nparams, const svslam_gd_prep *prep = nullptr)
    {
        Flush();
        if (k_.gdesc_configure(nlayers, layers, params, nparams, prep) != 0) return refuse(std::string("ConfigureGlobalDescriptor: ") + k_.last_error());
        gd_dim_ = k_.gdesc_dim();
        return true;
    }
    int GlobalDescriptorDim() const { return gd_dim_; }
    // LoopClosure::ExtractFeatureVec (src/loopclosure.cpp:92-129) for every stream whose last step made a keyframe: the configured
    // network on level 0 of slot_cur, where the keyframe's left image still is until the stream's next step (the window of
    // DescribeNewKeyframes).  ONE provider call for all streams.  vecs becomes [nstreams][dim], raw; the rows of the other streams
    // are zero.  The kernels read only the image, so this works with device_map = 1 as well.  n_described (optional): rows
    // computed.  False (last_error(), vecs untouched): no network configured, the provider's refusal.
    bool DescribeGlobalNewKeyframes(std::vector<float> *vecs, int *n_described = nullptr) { return DescribeGlobal(vecs, n_described, false); }
    // The store of global image descriptors DetectLoops searches (svslam_loopdb_configure): capacity rows of dim floats
    // for every stream, emptied.  Every stream's last_closed is forgotten with it.
    bool ConfigureLoopStore(int capacity, int dim)
    {
        Flush();
        if (k_.loopdb_configure(nstreams(), capacity, dim) != 0) return refuse(std::string("ConfigureLoopStore: ") + k_.last_error());
        lc_dim_ = dim; lc_capacity_ = capacity;
        lc_last_closed_.assign((size_t)nstreams(), -1);
        return true;
    }
    // LoopClosure::LocalFusion (src/loopclosure.cpp:439-582, as LoopClosureUpdate calls it at :625) for every job in ONE call of the
    // kernel provider (DESIGN 15 has the rules).  A job names the keyframe that closed a loop, the loop keyframe, the corrected
    // pose and KeypointMatches_ as pairs (feature index in cand->left, feature index in kf->left).  A local BA in flight is
    // collected first; then, per job,
    //   1-3  the provider moves the active window, the active landmarks and the last frame (local_fusion: the first-valid-observation
    //        search runs there; the host hands it, per observation in list order, the row of its keyframe or -1)
    //   4    the active keyframes take their corrected poses (an inactive kf is not written; relative_pose_pkf and relative_motion
    //        are NOT refreshed: the stale edge is what a later pose-graph run distributes)
    //   5    the pairs in ascending (ci, qi), each on the map as the pairs before it left it: the candidate's landmark, revived
    //        from the archive when it is dead (Map::Revive), takes over the observations of the current feature's landmark, which
    //        is removed (Map::RemoveLandmark; a dead one has no observation to move and only loses its archive record) - or, where
    //        that one has expired, the feature is pointed at it.  The same landmark on
    //        both sides is deleted (the reference's quirk).  The candidate's landmark is not made active.
    // In resident mode the stream's feature list on the provider is uploaded again afterwards.
    // False (last_error(), NOTHING changed for any job of the call): device_map = 1, an unknown stream, two jobs on one stream, ids
    // that are not keyframes, cand >= kf, a keyframe whose feature list was released, a pair's index out of range, a repeated pair, a
    // T_corr that is no unit quaternion, resident tracking where the last frame is not kf, the provider's refusal.
    struct FusionJob { int stream = 0; long kf_id = -1, cand_kf_id = -1; SE3 T_corr; std::vector<std::pair<int, int>> pairs; };
    struct FusionStats { int nkf = 0, npt = 0, n_unanchored = 0, pairs = 0, merged = 0, revived = 0, repointed = 0, same_deleted = 0; };
    bool LocalFusion(const std::vector<FusionJob> &jobs, std::vector<FusionStats> *stats)
    {
        if (device_map()) return refuse("LocalFusion: with device_map = 1 the landmarks live on the device without anchors; not supported yet");
        const int n = (int)jobs.size();
        std::vector<std::vector<std::pair<int, int>>> order((size_t)n);
        for (int j = 0; j < n; ++j) {
            const FusionJob &F = jobs[(size_t)j];
            if (F.stream < 0 || F.stream >= nstreams()) return refuse("LocalFusion: no such stream");
            for (int i = 0; i < j; ++i) if (jobs[(size_t)i].stream == F.stream) return refuse("LocalFusion: two jobs on one stream");
            const Stream &st = *streams_[F.stream];
            const std::vector<Frame *> &kfs = st.map.keyframes_;
            if (F.kf_id < 0 || F.kf_id >= (long)kfs.size() || F.cand_kf_id < 0 || F.cand_kf_id >= (long)kfs.size()) return refuse("LocalFusion: not a keyframe id of this stream");
            if (F.cand_kf_id >= F.kf_id) return refuse("LocalFusion: the loop keyframe must be older than the keyframe");
            const double *q = F.T_corr.v;
            if (!(std::fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 2e-6)) return refuse("LocalFusion: the corrected pose's quaternion is not of unit length");
            const Frame *kf = kfs[(size_t)F.kf_id], *cand = kfs[(size_t)F.cand_kf_id];
            if (!F.pairs.empty() && (kf->left.empty() || cand->left.empty()))
                return refuse("LocalFusion: the keyframe's feature list was released when it left the window (SetKeepKeyframeFeatures)");
            std::vector<std::pair<int, int>> &o = order[(size_t)j];
            o = F.pairs;
            std::sort(o.begin(), o.end());                                // std::set<pair<cand feature, cur feature>>: ascending lexicographic
            for (size_t i = 0; i < o.size(); ++i) {
                if (o[i].first < 0 || (size_t)o[i].first >= cand->left.size() || o[i].second < 0 || (size_t)o[i].second >= kf->left.size())
                    return refuse("LocalFusion: a pair's index is not a feature of its keyframe");
                if (i > 0 && o[i] == o[i - 1]) return refuse("LocalFusion: a pair is repeated");
            }
            if (resident() && st.last != kf)
                return refuse("LocalFusion: with resident tracking the last frame's features are held only by the kernel provider once it is not the keyframe itself; call it after the keyframe's step");
        }
        Flush();
        // gather
        std::vector<svslam_lf_job> lj((size_t)n);
        std::vector<double> poses, pts;
        std::vector<int> obs_ptr(1, 0), obs_kf, pt_kf;
        for (int j = 0; j < n; ++j) {
            const FusionJob &F = jobs[(size_t)j];
            Stream &st = *streams_[F.stream];
            Map &m = st.map;
            const Frame *kf = m.keyframes_[(size_t)F.kf_id];
            svslam_lf_job &J = lj[(size_t)j];
            std::memset(&J, 0, sizeof(J));
            J.kf_ofs = (int)(poses.size() / 7); J.nkf = (int)m.active_keyframes_.size(); J.pt_ofs = (int)(pts.size() / 3); J.npt = (int)m.active_landmarks_.size();
            J.cur = J.last = -1;
            for (int i = 0; i < J.nkf; ++i) {
                const Frame *a = m.active_keyframes_[(size_t)i];
                poses.insert(poses.end(), a->pose.v, a->pose.v + 7);
                if (a == kf) J.cur = i;
                if (a == st.last) J.last = i;
            }
            std::memcpy(J.T_cur, kf->pose.v, 56); std::memcpy(J.T_corr, F.T_corr.v, 56); std::memcpy(J.T_last, st.last->pose.v, 56);
            auto row_of = [&](const Frame *f) {
                for (int i = 0; i < J.nkf; ++i) if (m.active_keyframes_[(size_t)i] == f) return i;
                return (J.cur < 0 && f == kf) ? J.nkf : -1;
            };
            for (MapPoint *mp : m.active_landmarks_) {
                pts.insert(pts.end(), mp->pos, mp->pos + 3);
                for (const ObsRef &o : mp->observations)
                    obs_kf.push_back(m.Known(feat_of(o).mp) ? row_of(o.frame) : -1);      // the feature still names A landmark of the map
                obs_ptr.push_back((int)obs_kf.size());
            }
        }
        pt_kf.assign(pts.size() / 3 + 1, -1);
        poses.push_back(0); pts.push_back(0); obs_kf.push_back(0);           // data() of an empty vector may be null
        if (k_.local_fusion(n, lj.data(), (int)(poses.size() / 7), poses.data(), (int)(pts.size() / 3), pts.data(), obs_ptr.data(),
                            (int)obs_kf.size() - 1, obs_kf.data(), pt_kf.data()) != 0)
            return refuse(std::string("LocalFusion: ") + k_.last_error());
        // write back, then the replacement
        if (stats) stats->clear();
        std::vector<int> up;
        for (int j = 0; j < n; ++j) {
            const FusionJob &F = jobs[(size_t)j];
            Stream &st = *streams_[F.stream];
            Map &m = st.map;
            Frame *kf = m.keyframes_[(size_t)F.kf_id], *cand = m.keyframes_[(size_t)F.cand_kf_id];
            const svslam_lf_job &J = lj[(size_t)j];
            FusionStats S;
            S.nkf = J.nkf; S.npt = J.npt; S.n_unanchored = J.n_unanchored;
            for (int i = 0; i < J.npt; ++i) std::memcpy(m.active_landmarks_[(size_t)i]->pos, &pts[3 * ((size_t)J.pt_ofs + (size_t)i)], 24);
            for (int i = 0; i < J.nkf; ++i) m.active_keyframes_[(size_t)i]->pose = SE3(&poses[7 * ((size_t)J.kf_ofs + (size_t)i)]);
            if (J.last < 0) st.last->pose = SE3(J.T_last);
            for (const std::pair<int, int> &pr : order[(size_t)j]) {
                ++S.pairs;
                const long lid = cand->left[(size_t)pr.first].mp;
                MapPoint *mp_loop = m.point(lid);
                if (!mp_loop && (mp_loop = m.Revive(lid))) ++S.revived;
                if (!mp_loop) continue;
                Feature &fq = kf->left[(size_t)pr.second];
                MapPoint *mp_curr = m.point(fq.mp);
                if (mp_curr) {
                    std::vector<ObsRef> obs;                              // GetObs() hands out a copy: mp_loop may be mp_curr
                    for (const ObsRef &o : mp_curr->observations) obs.push_back(o);
                    for (const ObsRef &o : obs) { m.AddObservation(mp_loop, o); feat_of(o).mp = mp_loop->id; ++S.repointed; }
                    if (mp_curr == mp_loop) ++S.same_deleted; else ++S.merged;
                    m.RemoveLandmark(mp_curr);
                } else if (m.DropArchived(fq.mp)) ++S.merged;             // a dead landmark: no observation to move, nothing re-pointed, removed
                else { fq.mp = mp_loop->id; ++S.repointed; }
            }
            if (stats) stats->push_back(S);
            up.push_back(F.stream);
        }
        if (resident() && !up.empty()) UploadFeatures(up);
        return true;
    }

    // LoopClosure::AddNewKeyFrame (src/loopclosure.cpp:182-198) and one turn of LoopClosurePipeline (:801-872) for every stream whose
    // last step made a keyframe, synchronously, after DescribeNewKeyframes.  vecs holds one global descriptor of dim floats per
    // stream, [nstreams][dim]; the rows of streams without a new keyframe are not read.
    //   1. kf_id - last_closed <= keyframes_to_ignore_after_loop: skipped, never stored (:191-196)
    //   2. ONE loop_candidates call for all remaining streams (LoopKeyframeCandidate, :227-284)
    //   3. ONE VerifyLoopsStored call for the jobs that came back FOUND (:835-840)
    //   4. an ACCEPTED pair is a loop edge already (VerifyLoops records it); it sets the stream's last_closed and is NOT stored (:861, :868)
    //   5. every other keyframe is appended to the store, in one call (:870)
    // A keyframe whose vector cannot be normalised (BAD_VECTOR) is not stored either; the reference would store NaNs.  LocalFusion
    // (:858) is done only when LoopDetectParams::local_fusion asks for it; the result carries the LoopResult for it either way.  A keyframe is handled once: a second call after the same step
    // finds nothing to do.  False (last_error(), nothing done): device_map = 1, a store that was not configured, a new keyframe
    // that was never described, a stream whose store is full, the provider's refusal.
    // vecs == nullptr: the vectors are computed here by the configured network (ConfigureGlobalDescriptor), for the keyframes this
    // call handles; refused when no network is configured, or when the store's dim is not the network's.
    // local_fusion (default off: the call is what it was): the call ends with ONE LocalFusion call for every stream whose pair was
    // ACCEPTED with need_correction (LoopClosureUpdate, :594-597, :858); its pairs are the match rows whose candidate feature had a
    // landmark (KeypointMatches_, :340-366), mapped through desc_feat_indx.  LoopDetection::fused / fusion report it.
    struct LoopDetectParams { svslam_lc_params cand; svslam_loop_params verify; long keyframes_to_ignore_after_loop; bool local_fusion = false; };
    struct LoopDetection {
        bool is_keyframe = false, skipped = false, searched = false, verified = false, stored = false;
        long kf_id = -1;
        svslam_lc_job cand = {};          // status, cand_kf, best_sim, best_kf, n_weak, n_compared when searched
        LoopResult loop;                  // when verified
        bool fused = false;               // LoopDetectParams::local_fusion: LocalFusion ran for this stream
        FusionStats fusion;               // when fused
    };
    bool DetectLoops(const float *vecs, const LoopDetectParams &params, std::vector<LoopDetection> *results)
    {
        if (device_map()) return refuse("DetectLoops: with device_map = 1 the keyframes' features live on the device; not supported yet");
        if (lc_dim_ == 0) return refuse("DetectLoops: the store was not configured (ConfigureLoopStore)");
        std::vector<float> own;
        if (!vecs) {
            if (gd_dim_ == 0) return refuse("DetectLoops: no descriptors were given and no network is configured (ConfigureGlobalDescriptor)");
            if (gd_dim_ != lc_dim_) return refuse("DetectLoops: the store's dim is not the configured network's");
            if (!DescribeGlobal(&own, nullptr, true)) return false;
            vecs = own.data();
        }
        const int ns = nstreams();
        std::vector<LoopDetection> out((size_t)ns);
        std::vector<Frame *> fresh((size_t)ns, nullptr);
        for (int s = 0; s < ns; ++s) {
            Frame *f = streams_[s]->last;
            if (!f || !f->is_keyframe || f->loop_checked) continue;
            if (!f->described) return refuse("DetectLoops: the new keyframe was never described (DescribeNewKeyframes after its step)");
            int count = 0;
            if (k_.loopdb_count(s, &count) != 0) return refuse(std::string("DetectLoops: ") + k_.last_error());
            if (count >= lc_capacity_) return refuse("DetectLoops: the stream's store is full");
            fresh[(size_t)s] = f;
        }
        Flush();
        std::vector<svslam_lc_job> jobs;
        std::vector<float> q;
        for (int s = 0; s < ns; ++s) {
            Frame *f = fresh[(size_t)s];
            if (!f) continue;
            LoopDetection &D = out[(size_t)s];
            D.is_keyframe = true; D.kf_id = f->keyframe_id;
            const long closed = lc_last_closed_[(size_t)s];
            if (closed >= 0 && f->keyframe_id - closed <= params.keyframes_to_ignore_after_loop) { D.skipped = true; continue; }
            svslam_lc_job J;
            std::memset(&J, 0, sizeof(J));
            J.stream = s; J.kf_id = (int)f->keyframe_id;
            jobs.push_back(J);
            q.insert(q.end(), vecs + (size_t)s * lc_dim_, vecs + ((size_t)s + 1) * lc_dim_);
        }
        if (!jobs.empty() && k_.loop_candidates((int)jobs.size(), jobs.data(), &params.cand, q.data()) != 0)
            return refuse(std::string("DetectLoops: ") + k_.last_error());
        std::vector<LoopPair> pairs;
        for (const svslam_lc_job &J : jobs) {
            out[(size_t)J.stream].searched = true; out[(size_t)J.stream].cand = J;
            if (J.status == SVSLAM_LC_FOUND) pairs.push_back(LoopPair{ J.stream, (long)J.kf_id, (long)J.cand_kf });
        }
        std::vector<LoopResult> rs;
        if (!pairs.empty() && !VerifyLoopsStored(pairs, params.verify, &rs)) return false;
        for (size_t i = 0; i < pairs.size(); ++i) {
            LoopDetection &D = out[(size_t)pairs[i].stream];
            D.verified = true; D.loop = std::move(rs[i]);
            if (D.loop.status == SVSLAM_LOOP_ACCEPTED) lc_last_closed_[(size_t)pairs[i].stream] = pairs[i].kf_id;
        }
        std::vector<int> as, ak;
        std::vector<float> av;
        for (size_t j = 0; j < jobs.size(); ++j) {
            const LoopDetection &D = out[(size_t)jobs[j].stream];
            if (jobs[j].status == SVSLAM_LC_BAD_VECTOR || (D.verified && D.loop.status == SVSLAM_LOOP_ACCEPTED)) continue;
            as.push_back(jobs[j].stream); ak.push_back(jobs[j].kf_id);
            av.insert(av.end(), q.begin() + (long)(j * (size_t)lc_dim_), q.begin() + (long)((j + 1) * (size_t)lc_dim_));
        }
        if (!as.empty() && k_.loopdb_append((int)as.size(), as.data(), ak.data(), av.data()) != 0)
            return refuse(std::string("DetectLoops: ") + k_.last_error());
        for (int s : as) out[(size_t)s].stored = true;
        for (int s = 0; s < ns; ++s) if (fresh[(size_t)s]) fresh[(size_t)s]->loop_checked = true;
        if (params.local_fusion) {
            std::vector<FusionJob> fj;
            ArchiveCache archive;
            for (size_t i = 0; i < pairs.size(); ++i) {
                const LoopDetection &D = out[(size_t)pairs[i].stream];
                if (D.loop.status != SVSLAM_LOOP_ACCEPTED || !D.loop.need_correction) continue;
                const std::vector<Frame *> &kfs = streams_[pairs[i].stream]->map.keyframes_;
                const Frame *kf = kfs[(size_t)pairs[i].kf_id], *cand = kfs[(size_t)pairs[i].cand_kf_id];
                FusionJob F;
                F.stream = pairs[i].stream; F.kf_id = pairs[i].kf_id; F.cand_kf_id = pairs[i].cand_kf_id; F.T_corr = D.loop.T_corr;
                for (size_t r = 0; r < D.loop.match_c.size(); ++r) {
                    const int ci = cand->desc_feat_indx[(size_t)D.loop.match_c[r]], qi = kf->desc_feat_indx[(size_t)D.loop.match_q[r]];
                    double p[3];
                    if (LandmarkPosition(F.stream, cand->left[(size_t)ci].mp, archive, p)) F.pairs.emplace_back(ci, qi);      // has_xyz
                }
                fj.push_back(std::move(F));
            }
            std::vector<FusionStats> fs;
            if (!fj.empty()) {
                // the detection itself has taken effect by now (loop edges, the store): the caller gets its results with the refusal
                if (!LocalFusion(fj, &fs)) { last_detections_ = out; if (results) *results = std::move(out); return false; }
                for (size_t i = 0; i < fj.size(); ++i) { out[(size_t)fj[i].stream].fused = true; out[(size_t)fj[i].stream].fusion = fs[i]; }
            }
        }
        last_detections_ = out;
        if (results) *results = std::move(out);
        return true;
    }
    // what the last DetectLoops call returned (the C API reads a stream's matches from here)
    const std::vector<LoopDetection> &LastDetections() const { return last_detections_; }
    long LastClosedKeyframe(int s) const { return s >= 0 && (size_t)s < lc_last_closed_.size() ? lc_last_closed_[(size_t)s] : -1; }
    const std::string &last_error() const { return refusal_; }

private:
    bool refuse(const std::string &why) { refusal_ = why; return false; }
    std::string refusal_;
    int gd_dim_ = 0;               // floats per global descriptor of the configured network (0: none)
    // unchecked_only: the keyframes DetectLoops has not handled yet
    bool DescribeGlobal(std::vector<float> *vecs, int *n_described, bool unchecked_only)
    {
        if (n_described) *n_described = 0;
        if (!vecs) return refuse("DescribeGlobalNewKeyframes: null output");
        if (gd_dim_ == 0) return refuse("DescribeGlobalNewKeyframes: no network is configured (ConfigureGlobalDescriptor)");
        Flush();
        std::vector<int> slots, who;
        for (int s = 0; s < nstreams(); ++s) {
            const Frame *f = streams_[s]->last;
            if (!f || !f->is_keyframe || (unchecked_only && f->loop_checked)) continue;
            slots.push_back(streams_[s]->slot_cur); who.push_back(s);
        }
        std::vector<float> rows(slots.size() * (size_t)gd_dim_ + 1);
        if (!slots.empty() && k_.gdesc_describe((int)slots.size(), slots.data(), rows.data()) != 0)
            return refuse(std::string("DescribeGlobalNewKeyframes: ") + k_.last_error());
        vecs->assign((size_t)nstreams() * (size_t)gd_dim_, 0.f);
        for (size_t j = 0; j < who.size(); ++j)
            std::memcpy(vecs->data() + (size_t)who[j] * gd_dim_, rows.data() + j * (size_t)gd_dim_, sizeof(float) * (size_t)gd_dim_);
        if (n_described) *n_described = (int)who.size();
        return true;
    }
    // DetectLoops: the store's shape (0: not configured), the keyframe that last closed a loop per stream (-1: none), the last results
    int lc_dim_ = 0, lc_capacity_ = 0;
    std::vector<long> lc_last_closed_;
    std::vector<LoopDetection> last_detections_;
    void check(int rc, const char *what)
    {
        if (rc != 0) throw std::runtime_error(std::string(what) + " failed: " + k_.last_error());
    }
    static long long now_ns()
    {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    struct STimer {            // host-side stage profile (SVS_PIPE_PROFILE=1 prints it at destruction)
        long long &acc; long long t0;
        explicit STimer(long long &a) : acc(a), t0(now_ns()) {}
        ~STimer() { acc += now_ns() - t0; }
    };
    struct KTimer {            // accumulates the wall time of one C-ABI call
        Counters &c; long long t0;
        explicit KTimer(Counters &cc) : c(cc), t0(now_ns()) {}
        ~KTimer() { c.ns_kernel_calls += now_ns() - t0; }
    };

    // ---- Track(): constant-velocity prior + TrackLastFrame + EstimateCurrentPose
    void TrackPrepareAndRun(const std::vector<int> &TS, const void *const *left, const int *strides, int is_device)
    {
        const int n = (int)TS.size();
        long long t_p = now_ns();
        jobs_track_.resize(n);
        imgs_.resize(n); strides_.resize(n);
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[TS[i]];
            svslam_track_job &j = jobs_track_[i];
            j.prev_slot = st.slot_prev; j.next_slot = st.slot_cur;
            j.pt_ofs = ofs; j.npts = (int)st.last->left.size();
            j.n_tracked = 0; j.n_inlier = 0;
            ofs += j.npts;
            imgs_[i] = left[TS[i]];
            strides_[i] = strides ? strides[TS[i]] : (cfg_.src_width > 0 ? cfg_.src_width : cfg_.width);
        }
        const size_t tot = (size_t)std::max(ofs, 1);
        prev_xy_.resize(2 * tot); next_xy_.resize(2 * tot); has_mp_.resize(tot); xyz_.resize(3 * tot);
        status_.assign(tot, 0); outlier_.assign(tot, 0);
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[TS[i]];
            Frame *cur = st.current, *last = st.last;
            cur->pose = st.relative_motion * last->pose;            // :655
            svslam_track_job &j = jobs_track_[i];
            std::memcpy(j.pose, cur->pose.v, sizeof(j.pose));
            size_t g = (size_t)j.pt_ofs;
            const SE3 T_caml_w = cfg_.cam_l.pose * cur->pose;        // pose_ * T_c_w, once per frame
            const std::vector<Feature> &LF = last->left;
            for (size_t fi = 0; fi < LF.size(); ++fi) {             // :331-347
                const Feature &f = LF[fi];
                if (fi + 8 < LF.size() && LF[fi + 8].mp >= 0) __builtin_prefetch(st.map.point(LF[fi + 8].mp), 0, 1);
                prev_xy_[2 * g] = f.x; prev_xy_[2 * g + 1] = f.y;
                MapPoint *mp = st.map.point(f.mp);
                if (mp) {
                    double uv[2];
                    cfg_.cam_l.project(T_caml_w, mp->pos, uv);
                    next_xy_[2 * g] = (float)uv[0]; next_xy_[2 * g + 1] = (float)uv[1];
                    has_mp_[g] = 1;
                    xyz_[3 * g] = mp->pos[0]; xyz_[3 * g + 1] = mp->pos[1]; xyz_[3 * g + 2] = mp->pos[2];
                } else {
                    next_xy_[2 * g] = f.x; next_xy_[2 * g + 1] = f.y;
                    has_mp_[g] = 0;
                    xyz_[3 * g] = 0; xyz_[3 * g + 1] = 0; xyz_[3 * g + 2] = 1;
                }
                ++g;
            }
        });
        st_[1] += now_ns() - t_p;
        svslam_lk_params prm = { 3, 30, 0.01, 1e-4, 1 };            // :353-357
        { KTimer kt_(cnt_); check(k_.track(n, jobs_track_.data(), imgs_.data(), strides_.data(), is_device, ofs, cam_l_,
                       prev_xy_.data(), next_xy_.data(), has_mp_.data(), xyz_.data(), status_.data(),
                       outlier_.data(), &prm, 5.991), "track"); }
        cnt_.track_pts += ofs; cnt_.pyr_left += n;
    }

    bool resident() const { return cfg_.resident_track && (cfg_.backend_on <= 1 || cfg_.device_map); }
    bool device_map() const { return cfg_.device_map && cfg_.resident_track; }

    // ---- the keyframe path with the map in device memory: InsertKeyframe (:576-643) / StereoInit (:216-249) and
    // Backend::Optimize as ONE call of the kernel provider.  The host keeps the window's frames (ids, poses, slots):
    // it picks the keyframe to retire (Map::ChooseKeyframeToRemove) and a free slot for the new one.
    void KeyframeOnDevice(const std::vector<int> &IS, const std::vector<int> &KS, const void *const *left,
                          const void *const *right, const int *strides, int is_device, std::vector<int> &MS)
    {
        long long t_h = now_ns();
        std::vector<int> DS = IS;
        DS.insert(DS.end(), KS.begin(), KS.end());
        const int n = (int)DS.size();
        jobs_dm_.assign((size_t)n, svslam_dmap_job());
        dm_left_.resize(n); dm_right_.resize(n); strides_.resize(n);
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            const bool init = i < (int)IS.size();
            Frame *cur = st.current;
            svslam_dmap_job &j = jobs_dm_[i];
            std::memset(&j, 0, sizeof(j));
            j.stream = DS[i]; j.slot_cur = st.slot_cur; j.slot_right = st.slot_right; j.is_init = init ? 1 : 0;
            j.frame_id = cur->id; j.remove_slot = -1;
            if (init) {
                j.kf_slot = FreeWindowSlot(st); j.kf_id = (int)st.kf_factory_id; j.npts = 0;
            } else {
                // Frame::SetKeyFrame + Map::InsertKeyFrame (src/map.cpp:53-67) on the host mirror
                cur->is_keyframe = true;
                cur->keyframe_id = st.kf_factory_id++;
                st.kf_store.push_back(std::move(st.cur_owned));
                st.map.keyframes_.push_back(cur);
                st.map.active_keyframes_.push_back(cur);
                st.c_keyframes++;
                if ((int)st.map.active_keyframes_.size() > cfg_.num_active_keyframes) {
                    Frame *rm = Map::ChooseKeyframeToRemove(st.map.active_keyframes_, cur);
                    if (rm) {
                        j.remove_slot = rm->dslot; rm->dslot = -1;
                        auto &ak = st.map.active_keyframes_;
                        ak.erase(std::remove(ak.begin(), ak.end(), rm), ak.end());
                    }
                }
                cur->dslot = j.kf_slot = FreeWindowSlot(st, j.remove_slot);
                j.kf_id = (int)cur->keyframe_id; j.npts = st.dev_feat;
                st.frontend_prev_kf = st.frontend_current_kf;
                st.frontend_current_kf = cur;
                cur->prev_keyframe = st.frontend_prev_kf;
                if (st.frontend_prev_kf) cur->relative_pose_pkf = cur->pose * st.frontend_prev_kf->pose.inverse();
            }
            std::memcpy(j.pose, cur->pose.v, sizeof(j.pose));
            const SE3 T_camr_w = cfg_.cam_r.pose * cur->pose;
            std::memcpy(j.T_camr_w, T_camr_w.v, sizeof(j.T_camr_w));
            const SE3 Twc = init ? SE3() : cur->pose.inverse();       // :261
            std::memcpy(j.T_wc, Twc.v, sizeof(j.T_wc));
            dm_left_[i] = left[DS[i]]; dm_right_[i] = right[DS[i]];
            strides_[i] = strides ? strides[DS[i]] : (cfg_.src_width > 0 ? cfg_.src_width : cfg_.width);
        });
        svslam_dmap_params prm{};
        prm.num_features = cfg_.num_features; prm.num_features_init = cfg_.num_features_init;
        prm.num_active_keyframes = cfg_.num_active_keyframes; prm.ba_iters = (backend_enabled_ && cfg_.backend_on >= 1) ? 10 : 0;   // src/backend.cpp:163
        prm.max_triangulation_depth = cfg_.max_triangulation_depth; prm.chi2_th = cfg_.chi2_th;
        prm.ba_defer = 0; prm.reserved = 0;
        st_[6] += now_ns() - t_h;
        // a provider call holds at most dm_chunk_ jobs (its staging memory is sized for that); with the backend beside the
        // frontend (backend_on 2) the LAST call's local BA is left running (one deferred batch at a time; the calls before
        // it, if any — only a start-up with more than dm_chunk_ streams has them — complete theirs at once)
        int defer_from = n;
        for (int c0 = 0; c0 < n; c0 += dm_chunk_) {
            const int m = std::min(dm_chunk_, n - c0);
            prm.ba_defer = (cfg_.backend_on >= 2 && prm.ba_iters > 0 && c0 + m >= n) ? 1 : 0;
            if (prm.ba_defer) defer_from = c0;
            KTimer kt_(cnt_);
            check(k_.dmap_keyframe(m, jobs_dm_.data() + c0, dm_left_.data() + c0, dm_right_.data() + c0, strides_.data() + c0, is_device,
                                   cam_l_, cfg_.cam_l.pose.v, cam_r_, cfg_.cam_r.pose.v, &prm), "dmap_keyframe");
            // Map::landmarks_ keeps every landmark (src/map.cpp:39-51): what the provider freed goes to the stream's archive
            const svslam_dmap_evicted_rec *ev = nullptr; int nev = 0;
            check(k_.dmap_evicted(&ev, &nev), "dmap_evicted");
            for (int i = c0; i < c0 + m && nev > 0; ++i) {
                const svslam_dmap_job &j = jobs_dm_[i];
                Map &mp = streams_[DS[i]]->map;
                for (int e = j.ev_ofs; e < j.ev_ofs + j.ev_n && e < nev; ++e) mp.ArchiveEvicted(ev[e].id, ev[e].pos);
            }
        }
        t_h = now_ns();
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[DS[i]];
            const svslam_dmap_job &j = jobs_dm_[i];
            Frame *cur = st.current;
            const bool init = j.is_init != 0;
            cnt_.gftt_calls++; cnt_.gftt_rects += j.npts; cnt_.right_pts += j.n_features; cnt_.pyr_right++;
            st.c_corners += j.n_corners;
            if (init) cnt_.pyr_left++;
            st.c_dropped += j.corners_dropped;
            st.dev_feat = j.n_features;
            if (init) {
                if (!j.ok) continue;                                  // StereoInit failed (:227): try again with the next frame
                st.init_ok = true;
                // StereoInit :232-246 + BuildInitMap :195-203
                st.frontend_current_kf = cur;
                cur->is_keyframe = true;
                cur->keyframe_id = st.kf_factory_id++;
                cur->dslot = j.kf_slot;
                st.kf_store.push_back(std::move(st.cur_owned));
                st.map.keyframes_.push_back(cur);
                st.map.active_keyframes_.push_back(cur);
                st.c_keyframes++;
                st.status = FrontendStatus::TRACKING_GOOD;
            }
            MS.push_back(DS[i]);
            cnt_.tri_pts += j.n_tri_in;
            if (j.flags & 4) cnt_.ba_skipped++;
            if (j.flags & 2) cnt_.lm_full++;
            cnt_.lm_created_dev += j.n_tri_ok;
            if (prm.ba_iters > 0 && i < defer_from) ApplyDeviceBa(st, j);
        }
        if (defer_from < n) {                  // the deferred batch: its jobs and streams wait for DmCollect
            dm_pending_.assign(jobs_dm_.begin() + defer_from, jobs_dm_.end());
            dm_pending_streams_.assign(DS.begin() + defer_from, DS.end());
            dm_inflight_ = true; ba_age_ = 0;
        }
        st_[7] += now_ns() - t_h;
    }
    // Backend::Optimize's write-back on the host mirror (:224-246): counters, the window's poses
    void ApplyDeviceBa(Stream &st, const svslam_dmap_job &j)
    {
        if (j.flags & 4) return;
        cnt_.ba_calls++; cnt_.ba_edges += j.ba_nobs; cnt_.ba_kf += j.ba_nkf; cnt_.ba_lm += j.ba_nlm; cnt_.ba_iters += j.ba_iters;
        cnt_.ba_pairs += j.ba_npair; cnt_.ba_trials += j.ba_ntrial;
        for (int a = 0; a < j.ba_nkf; ++a)
            for (Frame *kf : st.map.active_keyframes_)
                if (kf->dslot == j.win_slot[a]) { kf->pose = SE3(j.win_pose[a]); break; }
        for (Frame *kf : st.map.active_keyframes_)
            if (kf->keyframe_id != 0 && kf->prev_keyframe) kf->relative_pose_pkf = kf->pose * kf->prev_keyframe->pose.inverse();
    }
    // the deferred local BA of the device map lands (svslam_dmap_ba_collect)
    void DmCollect()
    {
        if (!dm_inflight_) return;
        dm_inflight_ = false;
        int nin = 0;
        { KTimer kt_(cnt_); check(k_.dmap_ba_collect((int)dm_pending_.size(), dm_pending_.data(), &nin), "dmap_ba_collect"); }
        long long t_h = now_ns();
        for (size_t i = 0; i < dm_pending_.size(); ++i) {
            if (dm_pending_[i].is_init && !dm_pending_[i].ok) continue;
            ApplyDeviceBa(*streams_[dm_pending_streams_[i]], dm_pending_[i]);
        }
        st_[7] += now_ns() - t_h;
    }
    int FreeWindowSlot(const Stream &st, int just_freed = -1) const
    {
        if (just_freed >= 0) return just_freed;
        unsigned used = 0;
        for (const Frame *kf : st.map.active_keyframes_) if (kf->dslot >= 0) used |= 1u << kf->dslot;
        for (int k = 0; k < cfg_.num_active_keyframes + 1; ++k) if (!(used & (1u << k))) return k;
        return 0;
    }

    // ---- Track() with the last frame's features resident in the kernel provider's memory: the
    // gather of :331-347 and the scatter of :361-381 / :546-553 run on the device, the host
    // supplies the predicted pose and reads counts (and, for keyframes, the survivor list).
    void TrackResidentRun(const std::vector<int> &TS, const void *const *left, const int *strides, int is_device)
    {
        const int n = (int)TS.size();
        long long t_p = now_ns();
        jobs_rt_.resize(n);
        imgs_.resize(n); strides_.resize(n);
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[TS[i]];
            svslam_rtrack_job &j = jobs_rt_[i];
            Frame *cur = st.current, *last = st.last;
            cur->pose = st.relative_motion * last->pose;            // :655
            const SE3 T_caml_w = cfg_.cam_l.pose * cur->pose;
            j.stream = TS[i]; j.prev_slot = st.slot_prev; j.next_slot = st.slot_cur;
            j.pt_ofs = ofs; j.npts = st.dev_feat;
            std::memcpy(j.pose, cur->pose.v, sizeof(j.pose));
            std::memcpy(j.T_cam_w, T_caml_w.v, sizeof(j.T_cam_w));
            j.n_tracked = j.n_edges = j.n_outlier = 0; j.reserved = 0;
            ofs += j.npts;
            imgs_[i] = left[TS[i]];
            strides_[i] = strides ? strides[TS[i]] : (cfg_.src_width > 0 ? cfg_.src_width : cfg_.width);
        }
        const size_t tot = (size_t)std::max(ofs, 1);
        const bool want_lists = !device_map();      // with the map on the device nobody on the host reads the survivors
        if (want_lists) { next_xy_.resize(2 * tot); rt_mp_.resize(tot); }
        st_[1] += now_ns() - t_p;
        svslam_lk_params prm = { 3, 30, 0.01, 1e-4, 1 };            // :353-357
        { KTimer kt_(cnt_); check(k_.rtrack(n, jobs_rt_.data(), imgs_.data(), strides_.data(), is_device, ofs, cam_l_,
                       want_lists ? next_xy_.data() : nullptr, want_lists ? rt_mp_.data() : nullptr, &prm, 5.991), "rtrack"); }
        cnt_.track_pts += ofs; cnt_.pyr_left += n;
    }

    void TrackFinishResident(int s, int i)
    {
        Stream &st = *streams_[s];
        const svslam_rtrack_job &j = jobs_rt_[i];
        Frame *cur = st.current;
        st.dev_feat = j.n_tracked;
        st.c_pose_edges += j.n_edges;
        cur->pose = SE3(j.pose);                                   // :542
        st.tracking_inliers = j.n_edges - j.n_outlier;             // :556
        if (st.tracking_inliers > cfg_.num_features_tracking) st.status = FrontendStatus::TRACKING_GOOD;
        else if (st.tracking_inliers > cfg_.num_features_tracking_bad) st.status = FrontendStatus::TRACKING_BAD;
        else st.status = FrontendStatus::LOST;                     // :665-679
        if (st.tracking_inliers >= cfg_.num_features_needed_for_keyframe) return;
        if (device_map()) { st.is_new_kf = true; return; }          // InsertKeyframe runs on the device (KeyframeOnDevice)
        // InsertKeyframe :576-616 — only now does the host need the frame's features
        cur->left.reserve((size_t)j.n_tracked + (size_t)cfg_.num_features);
        for (int r = 0; r < j.n_tracked; ++r) {
            Feature f;
            f.x = next_xy_[2 * ((size_t)j.pt_ofs + r)]; f.y = next_xy_[2 * ((size_t)j.pt_ofs + r) + 1];
            f.mp = rt_mp_[(size_t)j.pt_ofs + r];
            cur->left.push_back(f);
        }
        MakeKeyFrame(st);
        st.frontend_prev_kf = st.frontend_current_kf;
        st.frontend_current_kf = cur;
        cur->prev_keyframe = st.frontend_prev_kf;
        cur->relative_pose_pkf = cur->pose * st.frontend_prev_kf->pose.inverse();
        for (size_t k = 0; k < cur->left.size(); ++k)               // SetObservationsForKeyFrame :560-574
            if (cur->left[k].mp >= 0) st.map.AddObservation(st.map.point(cur->left[k].mp), ObsRef{ cur, (int)k, true });
        st.is_new_kf = true;
    }

    void UploadFeatures(const std::vector<int> &DS)
    {
        const int n = (int)DS.size();
        up_stream_.resize(n); up_ofs_.resize(n); up_cnt_.resize(n);
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            up_stream_[i] = DS[i]; up_ofs_[i] = ofs; up_cnt_[i] = (int)streams_[DS[i]]->current->left.size();
            ofs += up_cnt_[i];
        }
        const size_t tot = (size_t)std::max(ofs, 1);
        up_xy_.resize(2 * tot); up_mp_.resize(tot); up_xyz_.resize(3 * tot);
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            size_t g = (size_t)up_ofs_[i];
            for (const Feature &f : st.current->left) {
                up_xy_[2 * g] = f.x; up_xy_[2 * g + 1] = f.y; up_mp_[g] = (int)f.mp;
                const MapPoint *mp = st.map.point(f.mp);
                if (mp) { up_xyz_[3 * g] = mp->pos[0]; up_xyz_[3 * g + 1] = mp->pos[1]; up_xyz_[3 * g + 2] = mp->pos[2]; }
                else { up_xyz_[3 * g] = 0; up_xyz_[3 * g + 1] = 0; up_xyz_[3 * g + 2] = 1; }
                ++g;
            }
            st.dev_feat = up_cnt_[i];
        });
        { KTimer kt_(cnt_); check(k_.rtrack_upload(n, up_stream_.data(), up_ofs_.data(), up_cnt_.data(), up_xy_.data(),
                                                   up_mp_.data(), up_xyz_.data()), "rtrack_upload"); }
    }

    // sets st.is_new_kf if the frame became a keyframe
    void TrackFinish(int s, int i)
    {
        Stream &st = *streams_[s];
        const svslam_track_job &j = jobs_track_[i];
        Frame *cur = st.current, *last = st.last;
        // TrackLastFrame :361-381 (status already includes the in-image test)
        int n_edges = 0, n_outlier = 0;
        cur->left.reserve((size_t)j.npts + (size_t)cfg_.num_features);
        for (int p = 0; p < j.npts; ++p) {
            const int g = j.pt_ofs + p;
            if (!status_[g]) continue;
            Feature f;
            f.x = next_xy_[2 * g]; f.y = next_xy_[2 * g + 1];
            f.mp = last->left[p].mp;
            // EstimateCurrentPose :546-553: outliers lose their map point
            if (f.mp >= 0) {
                ++n_edges;
                if (outlier_[g]) { f.mp = -1; ++n_outlier; }
            }
            cur->left.push_back(f);
        }
        st.c_pose_edges += n_edges;
        cur->pose = SE3(j.pose);                                   // :542
        st.tracking_inliers = n_edges - n_outlier;                 // :556
        if (st.tracking_inliers > cfg_.num_features_tracking) st.status = FrontendStatus::TRACKING_GOOD;
        else if (st.tracking_inliers > cfg_.num_features_tracking_bad) st.status = FrontendStatus::TRACKING_BAD;
        else st.status = FrontendStatus::LOST;                     // :665-679
        // InsertKeyframe :576-616
        if (st.tracking_inliers >= cfg_.num_features_needed_for_keyframe) return;
        MakeKeyFrame(st);
        st.frontend_prev_kf = st.frontend_current_kf;
        st.frontend_current_kf = cur;
        cur->prev_keyframe = st.frontend_prev_kf;
        cur->relative_pose_pkf = cur->pose * st.frontend_prev_kf->pose.inverse();
        // SetObservationsForKeyFrame :560-574
        for (size_t k = 0; k < cur->left.size(); ++k)
            if (cur->left[k].mp >= 0) st.map.AddObservation(st.map.point(cur->left[k].mp), ObsRef{ cur, (int)k, true });
        st.is_new_kf = true;
    }

    // safe point of a keyframe step (no BA in flight that holds pointers into the map): retired keyframes give
    // their feature lists back, landmarks nothing can reach any more are archived (Map::ReleaseRetired)
    void ReleaseRetired(Stream &st) { st.map.ReleaseRetired(&st.current->left, st.current->id); }

    void MakeKeyFrame(Stream &st)
    {
        Frame *cur = st.current;
        cur->is_keyframe = true;                                   // Frame::SetKeyFrame
        cur->keyframe_id = st.kf_factory_id++;
        st.kf_store.push_back(std::move(st.cur_owned));            // Map::keyframes_ keeps it alive
        st.map.InsertKeyFrame(cur);
        st.c_keyframes++;
    }

    void BuildPyramids(const std::vector<int> &IS, const std::vector<int> &DS, const void *const *left,
                       const void *const *right, const int *strides, int is_device)
    {
        std::vector<int> slots; imgs_.clear(); strides_.clear();
        for (int s : IS) {
            slots.push_back(streams_[s]->slot_cur); imgs_.push_back(left[s]);
            strides_.push_back(strides ? strides[s] : (cfg_.src_width > 0 ? cfg_.src_width : cfg_.width));
        }
        for (int s : DS) {
            slots.push_back(streams_[s]->slot_right); imgs_.push_back(right[s]);
            strides_.push_back(strides ? strides[s] : (cfg_.src_width > 0 ? cfg_.src_width : cfg_.width));
        }
        { KTimer kt_(cnt_); check(k_.pyramid((int)slots.size(), slots.data(), imgs_.data(), strides_.data(), is_device), "pyramid"); }
        cnt_.pyr_left += (long long)IS.size(); cnt_.pyr_right += (long long)DS.size();
    }

    // keypoint_feature_detector: ORB (src/frontend.cpp:20-33, :51): cv::ORB::create(num_features)->detect(img, kps, mask) through the
    // provider's orb_detect with the rects DetectFeatures has filled; (x, y) of the keypoints are appended under the same max_pts /
    // c_dropped rule as the corners, with their angle and octave (DescribeNewKeyframesOriented reads them); size and response are not stored.
    // Keypoints the rules give beyond the call's 2 num_features rows (score and response ties) count as dropped.
    void DetectOrb(const std::vector<int> &DS, int n, int ofs)
    {
        if constexpr (provider_has_orb<K>(0)) {
            const int max_out = 2 * cfg_.num_features;
            jobs_orb_.resize((size_t)n);
            for (int i = 0; i < n; ++i) {
                std::memset(&jobs_orb_[(size_t)i], 0, sizeof(svslam_orb_job));
                jobs_orb_[(size_t)i].slot = jobs_gftt_[i].slot; jobs_orb_[(size_t)i].rect_ofs = jobs_gftt_[i].rect_ofs; jobs_orb_[(size_t)i].nrect = jobs_gftt_[i].nrect;
            }
            kps_orb_.resize((size_t)n * max_out);
            svslam_orb_params P;
            P.nfeatures = cfg_.num_features; P.nlevels = 0; P.fast_threshold = 0; P.edge = 0;          // ORB's defaults
            { KTimer kt_(cnt_); check(k_.orb_detect(n, jobs_orb_.data(), &P, ofs, rects_.data(), max_out, kps_orb_.data()), "orb_detect"); }
            long long t_h3 = now_ns();
            pool_.parallel_for(n, [&](int i) {
                Stream &st = *streams_[DS[i]];
                int take = jobs_orb_[(size_t)i].n_out;
                st.c_dropped += jobs_orb_[(size_t)i].n_found - take;
                if (cfg_.max_pts > 0) {                                  // capacity of the kernel provider
                    const int room = std::max(0, cfg_.max_pts - (int)st.current->left.size());
                    if (take > room) { st.c_dropped += take - room; take = room; }
                }
                for (int c = 0; c < take; ++c) {
                    Feature f;
                    f.x = kps_orb_[(size_t)i * max_out + c].x;
                    f.y = kps_orb_[(size_t)i * max_out + c].y;
                    f.angle = kps_orb_[(size_t)i * max_out + c].angle;
                    f.octave = (int8_t)kps_orb_[(size_t)i * max_out + c].octave;
                    st.current->left.push_back(f);
                }
                st.c_corners += take;
            });
            cnt_.gftt_calls += n; cnt_.gftt_rects += ofs;
            st_[3] += now_ns() - t_h3;
        } else {
            (void)DS; (void)n; (void)ofs;
            throw std::runtime_error("this kernel provider has no ORB detector");
        }
    }

    // Frontend::DetectFeatures :36-70
    void DetectFeatures(const std::vector<int> &DS)
    {
        long long t_h3 = now_ns();
        const int n = (int)DS.size();
        jobs_gftt_.resize(n);
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[DS[i]];
            jobs_gftt_[i].slot = st.slot_cur;
            jobs_gftt_[i].rect_ofs = ofs;
            jobs_gftt_[i].nrect = (int)st.current->left.size();
            ofs += jobs_gftt_[i].nrect;
        }
        rects_.resize(2 * (size_t)std::max(ofs, 1));
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            size_t g = (size_t)jobs_gftt_[i].rect_ofs;
            for (const Feature &f : st.current->left) { rects_[2 * g] = f.x; rects_[2 * g + 1] = f.y; ++g; }
        });
        if (detector_ == 1) { st_[3] += now_ns() - t_h3; DetectOrb(DS, n, ofs); return; }
        corners_.assign((size_t)n * cfg_.num_features * 2, 0.f);
        ncorners_.assign((size_t)n, 0);
        st_[3] += now_ns() - t_h3;
        { KTimer kt_(cnt_); check(k_.gftt(n, jobs_gftt_.data(), ofs, rects_.data(), cfg_.num_features, 0.01, 20.0, corners_.data(),
                      ncorners_.data()), "gftt"); }                 // :24
        t_h3 = now_ns();
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            int take = ncorners_[i];
            if (cfg_.max_pts > 0) {                                  // capacity of the kernel provider
                const int room = std::max(0, cfg_.max_pts - (int)st.current->left.size());
                if (take > room) { st.c_dropped += take - room; take = room; }
            }
            for (int c = 0; c < take; ++c) {
                Feature f;
                f.x = corners_[((size_t)i * cfg_.num_features + c) * 2];
                f.y = corners_[((size_t)i * cfg_.num_features + c) * 2 + 1];
                st.current->left.push_back(f);
            }
            st.c_corners += take;
        });
        cnt_.gftt_calls += n; cnt_.gftt_rects += ofs;
        st_[3] += now_ns() - t_h3;
    }

    // Frontend::FindFeaturesInRight :72-141
    void FindFeaturesInRight(const std::vector<int> &DS)
    {
        long long t_h4 = now_ns();
        const int n = (int)DS.size();
        jobs_lk_.resize(n);
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[DS[i]];
            jobs_lk_[i].prev_slot = st.slot_cur; jobs_lk_[i].next_slot = st.slot_right;
            jobs_lk_[i].pt_ofs = ofs; jobs_lk_[i].npts = (int)st.current->left.size();
            ofs += jobs_lk_[i].npts;
        }
        const size_t tot = (size_t)std::max(ofs, 1);
        prev_xy_.resize(2 * tot); next_xy_.resize(2 * tot);
        status_.assign(tot, 0); err_.assign(tot, 0.f);
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            Frame *cur = st.current;
            size_t g = (size_t)jobs_lk_[i].pt_ofs;
            const SE3 T_camr_w = cfg_.cam_r.pose * cur->pose;
            for (const Feature &f : cur->left) {
                prev_xy_[2 * g] = f.x; prev_xy_[2 * g + 1] = f.y;
                MapPoint *mp = st.map.point(f.mp);
                if (mp) {
                    double uv[2];
                    cfg_.cam_r.project(T_camr_w, mp->pos, uv);
                    next_xy_[2 * g] = (float)uv[0]; next_xy_[2 * g + 1] = (float)uv[1];
                } else { next_xy_[2 * g] = f.x; next_xy_[2 * g + 1] = f.y; }
                ++g;
            }
        });
        st_[4] += now_ns() - t_h4;
        svslam_lk_params prm = { 3, 30, 0.01, 1e-4, 1 };            // :105-109
        { KTimer kt_(cnt_); check(k_.lk(n, jobs_lk_.data(), ofs, prev_xy_.data(), next_xy_.data(), status_.data(), err_.data(), &prm), "lk"); }
        t_h4 = now_ns();
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[DS[i]];
            Frame *cur = st.current;
            cur->right.assign(cur->left.size(), Feature());
            cur->right_ok.assign(cur->left.size(), 0);
            for (int p = 0; p < jobs_lk_[i].npts; ++p) {
                const int g = jobs_lk_[i].pt_ofs + p;
                const float x = next_xy_[2 * g], y = next_xy_[2 * g + 1];
                if (status_[g] && y >= 0 && y < (float)cfg_.height && x >= 0 && x < (float)cfg_.width) {  // :115-118
                    cur->right[p].x = x; cur->right[p].y = y;
                    cur->right_ok[p] = 1;
                }
            }
        });
        cnt_.right_pts += ofs;
        st_[4] += now_ns() - t_h4;
    }

    // BuildInitMap :143-214 / TriangulateNewPoints :251-320
    void Triangulate(const std::vector<int> &MS)
    {
        long long t_h5 = now_ns();
        const int n = (int)MS.size();
        jobs_tri_.resize(n);
        // which pairs go in: decided per stream, then laid out
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            Frame *cur = st.current;
            const bool init = !st.is_new_kf;
            st.tri_idx.clear();
            for (size_t p = 0; p < cur->left.size(); ++p) {
                if (!cur->right_ok[p]) continue;
                if (!init && cur->left[p].mp >= 0) continue;        // :272
                st.tri_idx.push_back((int)p);
            }
        });
        int ofs = 0;
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[MS[i]];
            const bool init = !st.is_new_kf;
            svslam_tri_job &j = jobs_tri_[i];
            j.pt_ofs = ofs; j.npts = (int)st.tri_idx.size();
            SE3 Twc = init ? SE3() : st.current->pose.inverse();    // :261
            std::memcpy(j.T_wc, Twc.v, sizeof(j.T_wc));
            j.zmax = init ? 0.0 : cfg_.max_triangulation_depth;     // :174 vs :286-288
            ofs += j.npts;
        }
        const size_t tot = (size_t)std::max(ofs, 1);
        uv_l_.resize(2 * tot); uv_r_.resize(2 * tot);
        tri_xyz_.assign(3 * tot, 0.0); tri_ok_.assign(tot, 0);
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            Frame *cur = st.current;
            size_t g = (size_t)jobs_tri_[i].pt_ofs;
            for (int p : st.tri_idx) {
                uv_l_[2 * g] = cur->left[p].x; uv_l_[2 * g + 1] = cur->left[p].y;
                uv_r_[2 * g] = cur->right[p].x; uv_r_[2 * g + 1] = cur->right[p].y;
                ++g;
            }
        });
        st_[5] += now_ns() - t_h5;
        if (ofs > 0) {
            KTimer kt_(cnt_);
            check(k_.triangulate(n, jobs_tri_.data(), ofs, cam_l_, cfg_.cam_l.pose.v, cam_r_, cfg_.cam_r.pose.v,
                                 uv_l_.data(), uv_r_.data(), tri_xyz_.data(), tri_ok_.data()), "triangulate");
        }
        cnt_.tri_pts += ofs;
        t_h5 = now_ns();
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            Frame *cur = st.current;
            const bool init = !st.is_new_kf;
            for (int q = 0; q < jobs_tri_[i].npts; ++q) {
                const int g = jobs_tri_[i].pt_ofs + q;
                if (!tri_ok_[g]) continue;
                const int p = st.tri_idx[q];
                MapPoint *mp = st.map.CreateNewMappoint();
                mp->pos[0] = tri_xyz_[3 * g]; mp->pos[1] = tri_xyz_[3 * g + 1]; mp->pos[2] = tri_xyz_[3 * g + 2];
                st.map.AddObservation(mp, ObsRef{ cur, p, true });
                st.map.AddObservation(mp, ObsRef{ cur, p, false });
                cur->left[p].mp = mp->id;
                cur->right[p].mp = mp->id;
                st.map.InsertMapPoint(mp);
            }
            if (init) {
                // StereoInit :232-246 + BuildInitMap :195-203
                st.frontend_current_kf = cur;
                MakeKeyFrame(st);
                st.status = FrontendStatus::TRACKING_GOOD;
            }
        });
        st_[5] += now_ns() - t_h5;
    }

    // Backend::UpdateMap -> Optimize (src/backend.cpp:9-248): gather + enqueue ...
    void BackendSubmit(const std::vector<int> &MS_all)
    {
        long long t_h6 = now_ns();
        ba_ms_ = MS_all;
        std::vector<int> &MS = ba_ms_;
        int n = (int)MS.size();
        // Gather per stream (:39-160), in parallel, STRAIGHT into the batch arrays the provider reads: pass 0
        // bounds every problem's sizes (and pulls its landmarks into cache), a prefix sum places the problems,
        // pass 1 fills them.  A problem may use less than its reservation (outlier features, landmarks without a
        // live observation): the jobs carry offsets, gaps are never read.
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            BaGather &g = st.ba;
            const std::vector<MapPoint *> &AL = st.map.active_landmarks_;
            size_t max_obs = 0;
            for (size_t li = 0; li < AL.size(); ++li) {
                if (li + 8 < AL.size()) {                            // the landmarks are scattered over the pool
                    __builtin_prefetch(AL[li + 8], 0, 1);
                    __builtin_prefetch(reinterpret_cast<const char *>(AL[li + 8]) + 64, 0, 1);
                }
                max_obs += AL[li]->observations.size();
            }
            g.nkf_ub = (int)st.map.active_keyframes_.size(); g.nlm_ub = (int)AL.size(); g.nobs_ub = (int)max_obs;
            if (cfg_.max_lm > 0) g.nlm_ub = std::min(g.nlm_ub, cfg_.max_lm + 1);
            if (cfg_.max_obs > 0) g.nobs_ub = std::min(g.nobs_ub, cfg_.max_obs + 1);
        });
        jobs_ba_.resize(n);
        int ko = 0, lo = 0, oo = 0;
        for (int i = 0; i < n; ++i) {
            const BaGather &g = streams_[MS[i]]->ba;
            svslam_ba_job &j = jobs_ba_[i];
            j.kf_ofs = ko; j.lm_ofs = lo; j.obs_ofs = oo;
            j.nkf = j.nlm = j.nobs = 0; j.iters_done = 0; j.reserved = 0;
            ko += g.nkf_ub; lo += g.nlm_ub; oo += g.nobs_ub;
        }
        // (the bounds are already clamped to capacity + 1 below: a problem that will be dropped as over capacity
        // reserves no more than a problem that just fits, so it cannot push the batch past the provider's arena)
        ba_poses_.resize(7 * (size_t)std::max(ko, 1)); ba_pts_.resize(3 * (size_t)std::max(lo, 1));
        ba_okf_.resize((size_t)std::max(oo, 1)); ba_olm_.resize((size_t)std::max(oo, 1));
        ba_right_.resize((size_t)std::max(oo, 1)); ba_uv_.resize(2 * (size_t)std::max(oo, 1));
        ba_chi2_.resize((size_t)std::max(oo, 1));
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            BaGather &g = st.ba;
            svslam_ba_job &j = jobs_ba_[i];
            g.clear();
            double *__restrict o_poses = &ba_poses_[7 * (size_t)j.kf_ofs];
            for (Frame *kf : st.map.active_keyframes_) {             // :39-66
                kf->ba_local = (int)g.kfs.size();
                std::memcpy(o_poses + 7 * g.kfs.size(), kf->pose.v, 7 * sizeof(double));
                g.kfs.push_back(kf);
            }
            const std::vector<MapPoint *> &AL = st.map.active_landmarks_;
            g.lms.resize(AL.size()); g.edge_feat.resize((size_t)g.nobs_ub);
            const int lm_room = g.nlm_ub; const size_t obs_room = (size_t)g.nobs_ub;   // writes stop at the reservation, counting goes on
            MapPoint **__restrict o_lms = g.lms.data();
            double *__restrict o_pts = &ba_pts_[3 * (size_t)j.lm_ofs];
            int *__restrict o_kf = &ba_okf_[(size_t)j.obs_ofs], *__restrict o_lm = &ba_olm_[(size_t)j.obs_ofs];
            uint8_t *__restrict o_right = &ba_right_[(size_t)j.obs_ofs];
            float *__restrict o_uv = &ba_uv_[2 * (size_t)j.obs_ofs];
            ObsRef *__restrict o_ef = g.edge_feat.data();
            int nl = 0; size_t ne = 0;
            for (size_t li = 0; li < AL.size(); ++li) {              // :83-160
                MapPoint *mp = AL[li];
                if (mp->is_outlier) continue;
                int lm_local = -1;
                const size_t nob = mp->observations.size();
                for (size_t oi = 0; oi < nob; ++oi) {
                    const ObsRef &ob = mp->observations[oi];
                    const Feature &ft = feat_of(ob);
                    if (ft.outlier) continue;
                    if (lm_local < 0) {                              // vertex even if no edge follows (:118-130)
                        lm_local = nl++;
                        if (lm_local < lm_room) {
                            o_lms[lm_local] = mp;
                            o_pts[3 * lm_local] = mp->pos[0]; o_pts[3 * lm_local + 1] = mp->pos[1]; o_pts[3 * lm_local + 2] = mp->pos[2];
                        }
                    }
                    const int kl = ob.frame->ba_local;
                    if (kl < 0) continue;                            // frame not in the active window (:133)
                    if (ne < obs_room) {
                        o_kf[ne] = kl; o_lm[ne] = lm_local;
                        o_right[ne] = ob.is_left ? 0 : 1;
                        o_uv[2 * ne] = ft.x; o_uv[2 * ne + 1] = ft.y;
                        o_ef[ne] = ob;
                    }
                    ++ne;
                }
            }
            g.lms.resize((size_t)std::min(nl, lm_room)); g.edge_feat.resize(std::min(ne, obs_room));
            j.nkf = (int)g.kfs.size(); j.nlm = nl; j.nobs = (int)ne;      // beyond the reservation = over capacity: dropped below
            for (size_t e = 0; e < std::min(ne, obs_room); ++e) ba_chi2_[(size_t)j.obs_ofs + e] = 0.0;
            for (Frame *kf : g.kfs) kf->ba_local = -1;
        });
        // a problem beyond the provider's capacity is dropped for this keyframe, alone
        {
            size_t keep = 0;
            for (int i = 0; i < n; ++i) {
                const svslam_ba_job &j = jobs_ba_[i];
                const bool fits = (cfg_.max_kf <= 0 || j.nkf <= cfg_.max_kf) && (cfg_.max_lm <= 0 || j.nlm <= cfg_.max_lm) &&
                                  (cfg_.max_obs <= 0 || j.nobs <= cfg_.max_obs);
                if (fits) { MS[keep] = MS[i]; jobs_ba_[keep] = j; ++keep; } else cnt_.ba_skipped++;
            }
            MS.resize(keep); jobs_ba_.resize(keep);
            n = (int)keep;
            if (n == 0) { st_[6] += now_ns() - t_h6; return; }
        }
        st_[6] += now_ns() - t_h6;
        if (const char *dump = std::getenv("SVS_DUMP_BA")) DumpBaProblem(dump, 0);   // development hook
        { KTimer kt_(cnt_); check(k_.local_ba_submit(n, jobs_ba_.data(), cam_l_, cfg_.cam_l.pose.v, cam_r_, cfg_.cam_r.pose.v, ko,
                          ba_poses_.data(), lo, ba_pts_.data(), oo, ba_okf_.data(), ba_olm_.data(), ba_right_.data(),
                          ba_uv_.data(), cfg_.chi2_th, 10), "local_ba_submit"); }   // :150-164
        ba_ko_ = ko; ba_lo_ = lo; ba_oo_ = oo;
        ba_inflight_ = true;
    }

    // development hook: writes job i of the batch being submitted when its window is full
    // (int32 nkf nlm nobs | f64 poses[7 nkf] pts[3 nlm] | i32 okf[nobs] olm[nobs] | u8 right[nobs] | f32 uv[2 nobs]).
    // A '%' in the path makes it a printf pattern for a running number (one file per full-window keyframe:
    // tests/golden/make_ba_golden.py captures its problems this way), otherwise the file is overwritten.
    void DumpBaProblem(const char *path, int i)
    {
        const svslam_ba_job &j = jobs_ba_[(size_t)i];
        if (j.nkf < cfg_.num_active_keyframes) return;
        char name[1024];
        if (std::strchr(path, '%')) { std::snprintf(name, sizeof(name), path, dump_seq_++); path = name; }
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        const int hdr[3] = { j.nkf, j.nlm, j.nobs };
        f.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
        f.write(reinterpret_cast<const char *>(&ba_poses_[7 * (size_t)j.kf_ofs]), sizeof(double) * 7 * j.nkf);
        f.write(reinterpret_cast<const char *>(&ba_pts_[3 * (size_t)j.lm_ofs]), sizeof(double) * 3 * j.nlm);
        f.write(reinterpret_cast<const char *>(&ba_okf_[(size_t)j.obs_ofs]), sizeof(int) * j.nobs);
        f.write(reinterpret_cast<const char *>(&ba_olm_[(size_t)j.obs_ofs]), sizeof(int) * j.nobs);
        f.write(reinterpret_cast<const char *>(&ba_right_[(size_t)j.obs_ofs]), (size_t)j.nobs);
        f.write(reinterpret_cast<const char *>(&ba_uv_[2 * (size_t)j.obs_ofs]), sizeof(float) * 2 * j.nobs);
    }

    // ... wait for the solve and write it back to the map (src/backend.cpp:167-246)
    void BackendCollect()
    {
        if (!ba_inflight_) return;
        ba_inflight_ = false;
        const std::vector<int> &MS = ba_ms_;
        const int n = (int)MS.size();
        { KTimer kt_(cnt_); check(k_.local_ba_collect(n, jobs_ba_.data(), ba_ko_, ba_poses_.data(), ba_lo_, ba_pts_.data(),
                          ba_oo_, ba_chi2_.data()), "local_ba_collect"); }
        long long t_h6 = now_ns();
        for (int i = 0; i < n; ++i) {
            const svslam_ba_job &j = jobs_ba_[i];
            cnt_.ba_calls++; cnt_.ba_edges += j.nobs; cnt_.ba_kf += j.nkf; cnt_.ba_lm += j.nlm;
            cnt_.ba_iters += j.iters_done;
            cnt_.ba_pairs += (long long)((unsigned)j.reserved & 0x00ffffffu); cnt_.ba_trials += (long long)((unsigned)j.reserved >> 24);
        }
        pool_.parallel_for(n, [&](int i) {
            Stream &st = *streams_[MS[i]];
            BaGather &g = st.ba;
            const svslam_ba_job &j = jobs_ba_[i];
            // :167-193 threshold doubling
            double chi2_th = cfg_.chi2_th;
            int cnt_outlier = 0, cnt_inlier = 0, iteration = 0;
            while (iteration < 5) {
                cnt_outlier = 0; cnt_inlier = 0;
                for (int e = 0; e < j.nobs; ++e) {
                    if (ba_chi2_[j.obs_ofs + e] > chi2_th) cnt_outlier++; else cnt_inlier++;
                }
                double inlier_ratio = cnt_inlier / double(cnt_inlier + cnt_outlier);
                if (inlier_ratio > 0.5) break;
                chi2_th *= 2; iteration++;
            }
            // :197-213
            for (int e = 0; e < j.nobs; ++e) {
                const ObsRef &ob = g.edge_feat[e];
                Feature &ft = feat_of(ob);
                if (ba_chi2_[j.obs_ofs + e] > chi2_th) {
                    ft.outlier = true;
                    MapPoint *mp = st.map.point(ft.mp);
                    if (mp) st.map.RemoveObservation(mp, ob);
                } else ft.outlier = false;
            }
            // :224-231
            for (int k = 0; k < j.nkf; ++k) g.kfs[k]->pose = SE3(&ba_poses_[(size_t)(j.kf_ofs + k) * 7]);
            for (int l = 0; l < j.nlm; ++l) std::memcpy(g.lms[l]->pos, &ba_pts_[(size_t)(j.lm_ofs + l) * 3], 24);
            // :235-246
            for (Frame *kf : g.kfs) {
                if (kf->keyframe_id == 0) continue;
                if (kf->prev_keyframe) kf->relative_pose_pkf = kf->pose * kf->prev_keyframe->pose.inverse();
            }
        });
        st_[7] += now_ns() - t_h6;
    }

public:
    // completes a backend optimisation that is still in flight (backend_on 2)
    void Flush() { BackendCollect(); DmCollect(); }
    // Backend::PauseRequest / Resume (src/backend.cpp:296-343): keyframes inserted while the backend is
    // paused are not optimised
    void SetBackendEnabled(bool on) { backend_enabled_ = on; }
    bool BackendEnabled() const { return backend_enabled_; }
    // Backend::UpdateMap called from outside the frontend (include/StereoVisionSLAM/backend.h:30): one local
    // BA over every stream's active window, now.  Needs the host-side feature lists (resident_track = 0).
    void OptimizeNow()
    {
        if (device_map()) { OptimizeNowOnDevice(); return; }
        if (resident()) throw std::runtime_error("OptimizeNow: the feature lists live on the device (resident_track)");
        BackendCollect();
        std::vector<int> MS;
        for (int s = 0; s < nstreams(); ++s) if (!streams_[s]->map.active_keyframes_.empty()) MS.push_back(s);
        if (MS.empty()) return;
        BackendSubmit(MS);
        BackendCollect();
    }
    // ... with the map in the provider's memory: one optimise-only job per stream (svslam_dmap_job::is_init == 2), the
    // window's poses come back like after a keyframe
    void OptimizeNowOnDevice()
    {
        if (!backend_enabled_) return;
        DmCollect();                      // a deferred local BA (backend_on 2) lands first, like BackendCollect() in the host-map form
        std::vector<int> MS;
        for (int s = 0; s < nstreams(); ++s) if (!streams_[s]->map.active_keyframes_.empty()) MS.push_back(s);
        const int n = (int)MS.size();
        if (n == 0) return;
        jobs_dm_.assign((size_t)n, svslam_dmap_job());
        dm_left_.assign((size_t)n, nullptr); dm_right_.assign((size_t)n, nullptr); strides_.assign((size_t)n, cfg_.width);
        for (int i = 0; i < n; ++i) {
            svslam_dmap_job &j = jobs_dm_[i];
            std::memset(&j, 0, sizeof(j));
            j.stream = MS[i]; j.is_init = 2; j.npts = streams_[MS[i]]->dev_feat; j.kf_slot = -1; j.remove_slot = -1;
        }
        svslam_dmap_params prm{};
        prm.num_features = cfg_.num_features; prm.num_features_init = cfg_.num_features_init;
        prm.num_active_keyframes = cfg_.num_active_keyframes; prm.ba_iters = 10;
        prm.max_triangulation_depth = cfg_.max_triangulation_depth; prm.chi2_th = cfg_.chi2_th;
        for (int c0 = 0; c0 < n; c0 += dm_chunk_) {
            const int m = std::min(dm_chunk_, n - c0);
            KTimer kt_(cnt_);
            check(k_.dmap_keyframe(m, jobs_dm_.data() + c0, dm_left_.data() + c0, dm_right_.data() + c0, strides_.data() + c0, 1,
                                   cam_l_, cfg_.cam_l.pose.v, cam_r_, cfg_.cam_r.pose.v, &prm), "dmap_keyframe (optimise only)");
        }
        for (int i = 0; i < n; ++i) {
            Stream &st = *streams_[MS[i]];
            const svslam_dmap_job &j = jobs_dm_[i];
            if (j.flags & 4) { cnt_.ba_skipped++; continue; }
            ApplyDeviceBa(st, j);
        }
    }
    // the hooks the reference fires at the end of InsertKeyframe / StereoInit (src/frontend.cpp:618-640,
    // 236-246): backend_->UpdateMap() is the pipeline's own BA; loop closure and viewer are callbacks
    std::function<void(int stream, const Frame &)> on_keyframe;
private:
    bool backend_enabled_ = true;
    int dump_seq_ = 0;
    std::vector<int> ba_ms_;
    bool ba_inflight_ = false;
    int ba_age_ = 0;
    bool dm_inflight_ = false;                       // device map, backend_on 2: a deferred local BA is running
    std::vector<svslam_dmap_job> dm_pending_;
    std::vector<int> dm_pending_streams_;
    int ba_ko_ = 0, ba_lo_ = 0, ba_oo_ = 0;
    long long st_[12] = { 0 };   // 0 begin 1 track-prep 2 track-finish 3 detect 4 right 5 tri 6 ba-gather 7 ba-scatter 8 end
    Config cfg_;
    K &k_;
    ThreadPool pool_;
    std::vector<std::unique_ptr<Stream>> streams_;
    Counters cnt_;
    double cam_l_[4], cam_r_[4];
    // staging vectors (reused across frames: no per-frame allocation in steady state)
    std::vector<svslam_track_job> jobs_track_;
    std::vector<svslam_rtrack_job> jobs_rt_;
    std::vector<int> rt_mp_, up_stream_, up_ofs_, up_cnt_, up_mp_;
    std::vector<float> up_xy_;
    std::vector<double> up_xyz_;
    std::vector<svslam_lk_job> jobs_lk_;
    std::vector<svslam_gftt_job> jobs_gftt_;
    int detector_ = 0;                              // SetDetector: 0 GFTT, 1 ORB
    std::vector<svslam_orb_job> jobs_orb_;
    std::vector<svslam_orb_kp> kps_orb_;
    std::vector<svslam_tri_job> jobs_tri_;
    std::vector<svslam_ba_job> jobs_ba_;
    std::vector<svslam_dmap_job> jobs_dm_;
    std::vector<const void *> dm_left_, dm_right_;
    int dm_chunk_ = 512;              // SVSLAM_DMAP_CHUNK of the provider
    std::vector<const void *> imgs_;
    std::vector<int> strides_;
    std::vector<float> prev_xy_, next_xy_, rects_, corners_, uv_l_, uv_r_, err_, ba_uv_;
    std::vector<uint8_t> has_mp_, status_, outlier_, tri_ok_, ba_right_;
    std::vector<double> xyz_, tri_xyz_, ba_poses_, ba_pts_, ba_chi2_;
    std::vector<int> ncorners_, ba_okf_, ba_olm_;
};

} // namespace svs
