// local_fusion_host.cpp — the host glue of LocalFusion (slam_host.h: Map::RemoveLandmark / Revive, Pipeline::LocalFusion, the
// local_fusion flag of DetectLoops) on small scripted maps, with a CPU kernel provider whose local-fusion and pose-graph calls are
// csrc/k_local_fusion.h and csrc/k_pose_graph.h compiled for the host.  Every scenario writes the map before and after its call to
// <dir>/<scenario>.before / .after; tests/test_host_local_fusion.py loads the first into tests/ref_glue.py's object graph, runs
// tests/ref_local_fusion.py on it and compares with the second.  Built and run by that test (a second time with
// -fsanitize=address,undefined); no GPU.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "lf_host_emu/emu.cpp"
#include "pg_host_emu/emu.cpp"
#include "../../stereovision-slam_amd/host/slam_host.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// what Pipeline<K> needs of a provider on the paths this program takes.  The loop calls of DetectLoops answer from a script.
struct CpuKernels {
    int lf_calls = 0, lf_jobs = 0, uploads = 0;
    std::string err;
    // the scripted loop: every query finds `cand`, verification accepts it with these matches (descriptor rows) and this T_corr
    int cand = 0, need_correction = 1;
    std::vector<int> mc, mq;
    svs::SE3 T_corr;
    const char *last_error() { return err.c_str(); }
    int local_ba_collect(int, svslam_ba_job *, int, double *, int, double *, int, double *) { return -1; }
    int dmap_ba_collect(int, svslam_dmap_job *, int *) { return -1; }
    int dmap_read(int, long long *, int *, double *, int *, int *, double *, int *, uint8_t *) { return -1; }
    int rtrack_upload(int, const int *, const int *, const int *, const float *, const int *, const double *) { ++uploads; return 0; }
    int local_fusion(int n, svslam_lf_job *j, int total_kf, double *P, int total_pts, double *X, const int *op, int total_obs, const int *ok, int *pk)
    {
        ++lf_calls; lf_jobs += n;
        static_assert(sizeof(EmuLfJob) == sizeof(svslam_lf_job), "job layout");
        const int rc = emu_local_fusion(n, reinterpret_cast<EmuLfJob *>(j), total_kf, P, total_pts, X, op, total_obs, ok, pk);
        if (rc) err = emu_lf_error();
        return rc;
    }
    int pose_graph(int n, svslam_pg_job *j, int total_kf, double *P, const uint8_t *F, int total_edges, const int *a, const int *b,
                   const double *M, int total_pts, const int *an, double *X, int iters)
    {
        static_assert(sizeof(EmuJob) == sizeof(svslam_pg_job), "job layout");
        const int rc = emu_pose_graph(n, reinterpret_cast<EmuJob *>(j), total_kf, P, F, total_edges, a, b, M, total_pts, an, X, iters, nullptr);
        if (rc) err = emu_pg_error();
        return rc;
    }
    int gdesc_describe(int, const int *, float *) { return -1; }
    int loopdb_configure(int, int, int) { return 0; }
    int loopdb_count(int, int *count) { *count = 0; return 0; }
    int loopdb_append(int, const int *, const int *, const float *) { return 0; }
    int loop_candidates(int n, svslam_lc_job *jobs, const svslam_lc_params *, const float *)
    {
        for (int i = 0; i < n; ++i) { jobs[i].status = SVSLAM_LC_FOUND; jobs[i].cand_kf = cand; }
        return 0;
    }
    int loop_verify(int n, svslam_loop_job *jobs, const svslam_loop_params *, int, const uint8_t *, const double *, const uint8_t *, int,
                    const uint8_t *, const float *, int *m_c, int *m_q, int *m_d, uint8_t *m_i)
    {
        for (int i = 0; i < n; ++i) {
            svslam_loop_job &J = jobs[i];
            J.status = SVSLAM_LOOP_ACCEPTED; J.need_correction = need_correction; J.n_matches = J.n_points = J.n_inliers = (int)mc.size();
            std::memcpy(J.T_corr, T_corr.v, 56);
            const svs::SE3 I; std::memcpy(J.T_rel, I.v, 56);
            for (size_t r = 0; r < mc.size(); ++r) { m_c[J.c_ofs + (int)r] = mc[r]; m_q[J.c_ofs + (int)r] = mq[r]; m_d[J.c_ofs + (int)r] = 0; m_i[J.c_ofs + (int)r] = 1; }
        }
        return 0;
    }
};
typedef svs::Pipeline<CpuKernels> Pipe;

static svs::SE3 expy(double ang, double tx, double tz)            // rotation about y, translation
{
    svs::SE3 T; T.v[1] = std::sin(0.5 * ang); T.v[3] = std::cos(0.5 * ang); T.v[4] = tx; T.v[6] = tz;
    return T;
}

// A drive of N keyframes with a window of three.  Keyframe k creates four landmarks at its features 0 .. 3 (left and right
// observations) and sees the first two landmarks of keyframe k - 1 again at its features 4 and 5; keyframe 0 also creates `ndummy`
// landmarks at further features, seen by nothing else: they die with it, and 1024 of them make the map's id window slide.  After
// the last keyframe comes a tracked frame that carries the newest keyframe's landmarks.
static const int N = 8;
static void script(Pipe &pipe, int ndummy, bool resident_last_is_kf = false)
{
    svs::Stream &st = pipe.stream(0);
    svs::SE3 E;
    std::vector<long> prev;
    for (int k = 0; k < N; ++k) {
        if (k > 0) E = (expy(0.03, 0.01, -0.02) * expy(0.02, 0.05, -1.0)) * E;
        st.kf_store.emplace_back(new svs::Frame());
        svs::Frame *f = st.kf_store.back().get();
        const size_t nf = 6 + (k == 0 ? (size_t)ndummy : 0);
        f->id = 3 * k; f->keyframe_id = k; f->is_keyframe = true; f->pose = E;
        f->left.resize(nf); f->right.resize(nf); f->right_ok.assign(nf, 1);
        for (size_t i = 0; i < nf; ++i) { f->left[i].x = 10.f * (float)i + (float)k; f->left[i].y = 5.f; f->right[i].x = f->left[i].x - 3.f; f->right[i].y = 5.f; }
        if (k > 0) { f->prev_keyframe = st.kf_store[(size_t)k - 1].get(); f->relative_pose_pkf = f->pose * f->prev_keyframe->pose.inverse(); }
        st.map.InsertKeyFrame(f);
        std::vector<long> mine;
        for (size_t i = 0; i < nf; ++i) {
            if (i == 4 || i == 5) {
                if (k == 0) { f->right_ok[i] = 0; continue; }
                svs::MapPoint *m = st.map.point(prev[i - 4]);
                f->left[i].mp = m->id; st.map.AddObservation(m, svs::ObsRef{ f, (int)i, true });
                f->right_ok[i] = 0;
                continue;
            }
            svs::MapPoint *m = st.map.CreateNewMappoint();
            m->pos[0] = 0.5 * (double)(i % 7) - 1.0 + 1.0 / 3.0; m->pos[1] = 0.1 * k; m->pos[2] = 6.0 + k + 0.01 * (double)(i % 11);
            f->left[i].mp = m->id; st.map.AddObservation(m, svs::ObsRef{ f, (int)i, true });
            if (i < 4) { f->right[i].mp = m->id; st.map.AddObservation(m, svs::ObsRef{ f, (int)i, false }); } else f->right_ok[i] = 0;
            st.map.InsertMapPoint(m);
            if (i < 4) mine.push_back(m->id);
        }
        prev = mine;
        st.map.ReleaseRetired(&f->left, k);
        st.frontend_prev_kf = st.frontend_current_kf; st.frontend_current_kf = f;
    }
    svs::Frame *newest = st.kf_store.back().get();
    if (resident_last_is_kf) { st.current = st.last = newest; return; }
    st.cur_owned.reset(new svs::Frame());
    svs::Frame *t = st.cur_owned.get();
    t->id = 3 * N; t->pose = expy(0.01, 0.0, -0.3) * newest->pose;
    t->left.assign(newest->left.begin(), newest->left.begin() + 5);
    st.current = st.last = t;
    st.last_owned = std::move(st.cur_owned);
    st.relative_motion = expy(0.01, 0.0, -0.3);
}

// ---- the dump: everything LocalFusion may change, bit-exact (hex floats) -----------------------------------------------------------
static void put7(std::ostream &o, const double *v, int n = 7) { char b[64]; for (int i = 0; i < n; ++i) { std::snprintf(b, sizeof(b), " %a", v[i]); o << b; } }
static std::string dump(Pipe &pipe)
{
    svs::Stream &st = pipe.stream(0);
    svs::Map &m = st.map;
    std::ostringstream o;
    Pipe::ArchiveCache cache;
    auto named = [&](long id) { double p[3]; return pipe.LandmarkPosition(0, id, cache, p) ? id : -1L; };       // -1: the pointer has expired
    auto frame = [&](const svs::Frame *f, const char *tag) {
        bool act = false;
        for (const svs::Frame *a : m.active_keyframes_) act = act || a == f;
        o << tag << " " << f->id << " " << (f->is_keyframe ? f->keyframe_id : -1) << " " << (act ? 1 : 0) << " " << f->left.size();
        put7(o, f->pose.v); put7(o, f->relative_pose_pkf.v); o << "\n";
        for (size_t i = 0; i < f->left.size(); ++i) {
            o << "f " << i << " " << named(f->left[i].mp) << " " << (f->left[i].outlier ? 1 : 0);
            if (i < f->right_ok.size() && f->right_ok[i]) o << " " << named(f->right[i].mp) << " " << (f->right[i].outlier ? 1 : 0); else o << " x x";
            o << "\n";
        }
    };
    for (const svs::Frame *f : m.keyframes_) frame(f, "kf");
    if (st.last && !st.last->is_keyframe) frame(st.last, "last"); else o << "lastkf " << (st.last ? st.last->keyframe_id : -1) << "\n";
    o << "motion"; put7(o, st.relative_motion.v); o << "\n";
    for (const svs::LandmarkRecord &r : m.AllLandmarks()) {
        const svs::MapPoint *mp = m.point(r.id);
        o << "lm " << r.id << " " << (r.active ? 1 : 0) << " " << r.observed_times << " " << r.anchor_kf << " " << (mp ? (int)mp->observations.size() : 0);
        put7(o, r.pos, 3); o << "\n";
        if (mp) for (const svs::ObsRef &b : mp->observations) o << "o " << b.frame->keyframe_id << " " << b.idx << " " << (b.is_left ? 1 : 0) << "\n";
    }
    return o.str();
}
static void save(const std::string &dir, const std::string &name, const std::string &what) { std::ofstream f(dir + "/" + name); f << what; }

static Pipe::FusionJob job(long kf, long cand, const svs::SE3 &T_corr, std::vector<std::pair<int, int>> pairs)
{
    Pipe::FusionJob F; F.stream = 0; F.kf_id = kf; F.cand_kf_id = cand; F.T_corr = T_corr; F.pairs = std::move(pairs);
    return F;
}
static void save_job(const std::string &dir, const std::string &name, const Pipe::FusionJob &F, const Pipe::FusionStats &S)
{
    std::ostringstream o;
    o << "job " << F.kf_id << " " << F.cand_kf_id; put7(o, F.T_corr.v); o << "\n";
    for (auto &p : F.pairs) o << "pair " << p.first << " " << p.second << "\n";
    o << "stats " << S.nkf << " " << S.npt << " " << S.n_unanchored << " " << S.pairs << " " << S.merged << " " << S.revived << " " << S.repointed << " " << S.same_deleted << "\n";
    save(dir, name + ".job", o.str());
}

static bool ids_once(Pipe &pipe)
{
    std::set<long> seen;
    for (const svs::LandmarkRecord &r : pipe.stream(0).map.AllLandmarks()) if (!seen.insert(r.id).second) return false;
    std::vector<double> pts; std::vector<int> an;
    pipe.stream(0).map.CollectAnchored(pts, an);
    return an.size() == seen.size();
}

struct Run {
    svs::Config cfg; CpuKernels k; std::unique_ptr<Pipe> pipe;
    explicit Run(int ndummy, bool keep_archive = true, int resident = 0, bool last_is_kf = false)
    {
        cfg.num_active_keyframes = 3; cfg.resident_track = resident;
        pipe.reset(new Pipe(cfg, k, 2));
        pipe->stream(0).map.set_keep_archive(keep_archive);
        pipe->SetKeepKeyframeFeatures(true);
        script(*pipe, ndummy, last_is_kf);
    }
    svs::SE3 corr(long kf) { return expy(0.04, 0.3, -0.2) * pipe->stream(0).kf_store[(size_t)kf]->pose; }
    // one fusion, dumped around: returns the statistics
    Pipe::FusionStats fuse(const std::string &dir, const std::string &name, const Pipe::FusionJob &F)
    {
        save(dir, name + ".before", dump(*pipe));
        std::vector<Pipe::FusionStats> st;
        const int calls = k.lf_calls;
        CHECK(pipe->LocalFusion({ F }, &st));
        CHECK(k.lf_calls == calls + 1 && st.size() == 1);
        save(dir, name + ".after", dump(*pipe));
        save_job(dir, name, F, st.empty() ? Pipe::FusionStats() : st[0]);
        CHECK(ids_once(*pipe));
        return st.empty() ? Pipe::FusionStats() : st[0];
    }
};

static void scenarios(const std::string &dir)
{
    {   // the candidate's landmark is live and distinct: keyframe 5 is still in the window
        Run r(0);
        svs::Map &m = r.pipe->stream(0).map;
        svs::Frame *k5 = m.keyframes_[5], *k7 = m.keyframes_[7];
        const long loop_id = k5->left[0].mp, cur_id = k7->left[0].mp;
        svs::MapPoint *loop = m.point(loop_id);
        const int n0 = (int)loop->observations.size(), t0 = loop->observed_times;
        const size_t nact = m.active_landmarks_.size(), nall = m.AllLandmarks().size();
        const svs::SE3 T = r.corr(7);
        const Pipe::FusionStats S = r.fuse(dir, "merge_live", job(7, 5, T, { { 0, 0 } }));
        CHECK(S.nkf == 3 && S.pairs == 1 && S.merged == 1 && S.revived == 0 && S.repointed == 2 && S.same_deleted == 0 && S.n_unanchored == 0);
        CHECK((int)loop->observations.size() == n0 + 2 && loop->observed_times == t0 + 2);
        CHECK(loop->observations[(size_t)n0] == (svs::ObsRef{ k7, 0, true }) && loop->observations[(size_t)n0 + 1] == (svs::ObsRef{ k7, 0, false }));   // in list order
        CHECK(loop->anchor_kf() == 5);                                       // set once: the merge does not move it
        CHECK(k7->left[0].mp == loop_id && k7->right[0].mp == loop_id && m.point(cur_id) == nullptr);
        CHECK(m.active_landmarks_.size() == nact - 1 && m.AllLandmarks().size() == nall - 1);
        for (const svs::LandmarkRecord &a : m.AllLandmarks()) CHECK(a.id != cur_id);
        CHECK(r.pipe->stream(0).last->left[0].mp == cur_id);                 // the tracked frame keeps the stale id: an expired pointer
        CHECK(std::memcmp(k7->pose.v, T.v, 56) == 0);                // corrected[cur] is T_corr itself
    }
    for (int slid = 0; slid < 2; ++slid) {   // the candidate's landmarks are archived; with 1100 dead ids in front the id window has slid past them
        Run r(slid ? 1100 : 0);
        svs::Map &m = r.pipe->stream(0).map;
        svs::Frame *k0 = m.keyframes_[0], *k7 = m.keyframes_[7];
        const long id0 = k0->left[0].mp, id1 = k0->left[1].mp, cur0 = k7->left[0].mp;
        CHECK(m.point(id0) == nullptr && m.point(id1) == nullptr);
        const size_t arch = m.num_archived(), nall = m.AllLandmarks().size();
        float apos[3] = { 0, 0, 0 };
        for (const svs::LandmarkRecord &a : m.AllLandmarks()) if (a.id == id0) for (int c = 0; c < 3; ++c) apos[c] = (float)a.pos[c];
        const Pipe::FusionStats S = r.fuse(dir, slid ? "revive_slid" : "revive", job(7, 0, r.corr(7), { { 1, 1 }, { 0, 0 } }));
        CHECK(S.pairs == 2 && S.merged == 2 && S.revived == 2 && S.repointed == 4);
        CHECK(m.num_revived_below_base() == (slid ? 2u : 0u));
        svs::MapPoint *L0 = m.point(id0);
        CHECK(L0 && L0->id == id0 && !L0->active && L0->observed_times == 2 && L0->anchor_kf() == 0);
        if (L0) for (int c = 0; c < 3; ++c) CHECK(L0->pos[c] == (double)apos[c]);          // the archived float, widened: it is not an active landmark, step 2 does not move it
        CHECK(m.num_archived() == arch - 2 && m.AllLandmarks().size() == nall - 2 && m.point(cur0) == nullptr);
        for (svs::MapPoint *a : m.active_landmarks_) CHECK(a->id != id0 && a->id != id1);
        {   // SaveOutputs on the fused map: landmarks.pcd has one point per id the map still has - no removed landmark, every
            // revived one once - and the revived landmark's position is among them
            CHECK(r.pipe->SaveOutputs(0, dir, "d", 0));
            std::ifstream pcd(dir + "/landmarks.pcd");
            std::string line; size_t header = 0, rows = 0, hit = 0; bool data = false;
            char want[96]; std::snprintf(want, sizeof(want), "%.8g %.8g %.8g", (double)apos[0], (double)apos[1], (double)apos[2]);
            while (std::getline(pcd, line)) {
                if (!data) { if (line.rfind("POINTS ", 0) == 0) header = (size_t)std::atol(line.c_str() + 7); data = line == "DATA ascii"; continue; }
                ++rows; if (line == want) ++hit;
            }
            size_t same = 0;                                                 // (the dummies of the slid map repeat positions)
            for (const svs::LandmarkRecord &a : m.AllLandmarks()) same += ((float)a.pos[0] == apos[0] && (float)a.pos[1] == apos[1] && (float)a.pos[2] == apos[2]) ? 1 : 0;
            CHECK(header == nall - 2 && rows == nall - 2 && hit == same && same >= 1 && (slid || same == 1));
        }
        // its observations leave again: limbo, then the archive, by the existing rules
        m.RemoveObservation(L0, svs::ObsRef{ k7, 0, true }); m.RemoveObservation(L0, svs::ObsRef{ k7, 0, false });
        std::vector<svs::Feature> carried(1);
        m.ReleaseRetired(&carried, 1000);
        CHECK(m.point(id0) == nullptr && m.num_archived() == arch - 1 && ids_once(*r.pipe));
        int listed = 0;
        for (const svs::LandmarkRecord &a : m.AllLandmarks()) if (a.id == id0) { ++listed; CHECK(a.anchor_kf == 0 && a.observed_times == 0); }
        CHECK(listed == 1);
        // the fused map carries on: a pose-graph run sees every id once, and a ninth keyframe goes through the window
        std::vector<Pipe::PoseGraphStats> ps;
        CHECK(r.pipe->AddLoopEdge(0, 7, 0, svs::SE3()));
        CHECK(r.pipe->PoseGraphOptimization({ 0 }, 5, &ps));
        CHECK(ps.size() == 1 && (size_t)ps[0].npt == m.AllLandmarks().size() && ps[0].nkf == N);
        svs::Stream &st = r.pipe->stream(0);
        st.kf_store.emplace_back(new svs::Frame());
        svs::Frame *f = st.kf_store.back().get();
        f->id = 99; f->keyframe_id = N; f->is_keyframe = true; f->pose = expy(0.02, 0.05, -1.0) * k7->pose;
        f->left.resize(2); f->right.resize(2); f->right_ok.assign(2, 0);
        f->left[0].mp = id1; f->left[1].mp = k7->left[2].mp;
        f->prev_keyframe = k7; f->relative_pose_pkf = f->pose * k7->pose.inverse();
        st.map.InsertKeyFrame(f);                                            // keyframe 5 leaves (RemoveOldKeyframe)
        for (int i = 0; i < 2; ++i) st.map.AddObservation(st.map.point(f->left[(size_t)i].mp), svs::ObsRef{ f, i, true });
        st.map.ReleaseRetired(&f->left, 2000);
        CHECK(m.active_keyframes_.size() == 3 && m.point(id1) && m.point(id1)->observed_times == 3 && ids_once(*r.pipe));
    }
    {   // the same landmark on both sides: keyframe 7's feature 4 sees keyframe 6's landmark 0 again
        Run r(0);
        svs::Map &m = r.pipe->stream(0).map;
        const long id = m.keyframes_[6]->left[0].mp;
        CHECK(m.keyframes_[7]->left[4].mp == id);
        const size_t nall = m.AllLandmarks().size();
        const Pipe::FusionStats S = r.fuse(dir, "same_landmark", job(7, 6, r.corr(7), { { 0, 4 } }));
        CHECK(S.same_deleted == 1 && S.merged == 0 && S.repointed == 3);
        CHECK(m.point(id) == nullptr && m.AllLandmarks().size() == nall - 1);
        CHECK(m.keyframes_[6]->left[0].mp == id);                             // the stale id stays: expired everywhere
    }
    {   // mp_curr expired: the feature is pointed at the revived landmark, which gets no observation
        Run r(0);
        svs::Map &m = r.pipe->stream(0).map;
        svs::Frame *k7 = m.keyframes_[7];
        k7->left[2].outlier = true;
        m.RemoveObservation(m.point(k7->left[2].mp), svs::ObsRef{ k7, 2, true });      // as the backend drops an outlier: mp = -1
        CHECK(k7->left[2].mp == -1);
        const long id2 = m.keyframes_[0]->left[2].mp;
        const Pipe::FusionStats S = r.fuse(dir, "curr_expired", job(7, 0, r.corr(7), { { 2, 2 } }));
        CHECK(S.revived == 1 && S.merged == 0 && S.repointed == 1);
        CHECK(k7->left[2].mp == id2 && m.point(id2) && m.point(id2)->observed_times == 0 && m.point(id2)->observations.size() == 0);
    }
    {   // mp_loop expired: without the archive a dead landmark is gone for good and the pair does nothing
        Run r(0, false);
        svs::Map &m = r.pipe->stream(0).map;
        const long cur0 = m.keyframes_[7]->left[0].mp;
        const Pipe::FusionStats S = r.fuse(dir, "loop_expired", job(7, 0, r.corr(7), { { 0, 0 } }));
        CHECK(S.pairs == 1 && S.revived == 0 && S.merged == 0 && S.repointed == 0 && m.keyframes_[7]->left[0].mp == cur0 && m.point(cur0));
    }
    {   // two pairs on one current feature, in the set's order: (0, 0) merges into landmark A, (1, 0) then finds A there and merges it into B
        Run r(0);
        svs::Map &m = r.pipe->stream(0).map;
        const long a = m.keyframes_[0]->left[0].mp, b = m.keyframes_[0]->left[1].mp;
        const Pipe::FusionStats S = r.fuse(dir, "two_pairs_one_feature", job(7, 0, r.corr(7), { { 1, 0 }, { 0, 0 } }));
        CHECK(S.merged == 2 && S.revived == 2 && S.repointed == 4 && m.point(a) == nullptr && m.point(b) && m.keyframes_[7]->left[0].mp == b);
        CHECK(m.point(b)->observed_times == 2);
    }
    {   // cur has left the window (keyframe 4) and the last frame is the newest keyframe
        Run r(0, true, 0, true);
        const Pipe::FusionStats S = r.fuse(dir, "cur_inactive", job(4, 0, r.corr(4), { { 0, 0 } }));
        CHECK(S.nkf == 3 && S.n_unanchored == 0);
    }
    std::printf("scenarios ok\n");
}

static void refusals()
{
    Run r(0);
    Pipe &p = *r.pipe;
    const std::string before = dump(p);
    const svs::SE3 T = r.corr(7);
    auto refused = [&](const std::vector<Pipe::FusionJob> &jobs, const char *word) {
        std::vector<Pipe::FusionStats> st;
        const bool ok = p.LocalFusion(jobs, &st);
        if (ok || p.last_error().find(word) == std::string::npos || dump(p) != before || r.k.lf_calls != 0)
            { std::fprintf(stderr, "FAIL refusal '%s': ok %d, error '%s'\n", word, (int)ok, p.last_error().c_str()); ++g_fail; }
    };
    Pipe::FusionJob good = job(7, 0, T, { { 0, 0 } }), F;
    F = good; F.stream = 2; refused({ F }, "no such stream");
    F = good; F.stream = -1; refused({ F }, "no such stream");
    F = good; F.stream = 1; refused({ F }, "not a keyframe id");            // stream 1 has no keyframes
    F = good; F.kf_id = 8; refused({ F }, "not a keyframe id");
    F = good; F.cand_kf_id = -1; refused({ F }, "not a keyframe id");
    F = good; F.cand_kf_id = 7; refused({ F }, "older");
    F = good; F.pairs = { { 6, 0 } }; refused({ F }, "not a feature");
    F = good; F.pairs = { { 0, -1 } }; refused({ F }, "not a feature");
    F = good; F.pairs = { { 0, 0 }, { 1, 1 }, { 0, 0 } }; refused({ F }, "repeated");
    F = good; F.T_corr.v[3] *= 1.01; refused({ F }, "unit length");
    refused({ good, job(6, 1, T, {}) }, "two jobs on one stream");
    F = good; F.stream = 1; refused({ good, F }, "not a keyframe id");       // a bad job after a good one: nothing of the good one is done
    {   // a keyframe whose feature list was released
        svs::Config cfg; cfg.num_active_keyframes = 3; cfg.resident_track = 0;
        CpuKernels k; Pipe q(cfg, k, 1);
        script(q, 0);
        std::vector<svs::Feature>().swap(q.stream(0).map.keyframes_[0]->left);
        const std::string b = dump(q);
        CHECK(!q.LocalFusion({ good }, nullptr) && q.last_error().find("released") != std::string::npos && k.lf_calls == 0);
        CHECK(dump(q) == b);
    }
    {   // device map
        svs::Config dc; dc.device_map = 1; dc.resident_track = 1;
        CpuKernels dk; Pipe dp(dc, dk, 1);
        script(dp, 0);                                                      // (the host containers, filled by hand: something a fusion could change)
        const std::string b = dump(dp);
        CHECK(!dp.LocalFusion({ good }, nullptr) && dp.last_error().find("device_map") != std::string::npos && dk.lf_calls == 0);
        CHECK(dump(dp) == b && b.size() > 1000);
    }
    {   // resident tracking: refused when the last frame is not the keyframe, with a message that says why; fine when it is,
        // and the stream's feature list is uploaded again
        Run a(0, true, 1, false);
        const std::string b = dump(*a.pipe);
        CHECK(!a.pipe->LocalFusion({ good }, nullptr) && a.pipe->last_error().find("held only by the kernel provider") != std::string::npos);
        CHECK(dump(*a.pipe) == b && a.k.lf_calls == 0 && a.k.uploads == 0);
        Run c(0, true, 1, true);
        CHECK(c.pipe->LocalFusion({ good }, nullptr) && c.k.lf_calls == 1 && c.k.uploads == 1);
    }
    CHECK(p.LocalFusion({}, nullptr) && r.k.lf_calls == 1 && r.k.lf_jobs == 0 && dump(p) == before);     // no job: the provider's empty call
    std::printf("refusals ok\n");
}

// DetectLoops with a scripted loop: the flag off makes no local_fusion call and changes nothing; on, the accepted pair is fused
static void detect_loops_flag(const std::string &dir)
{
    for (int on = 0; on < 3; ++on) {                                        // 0: off, 1: on, 2: on but need_correction is not set
        Run r(0, true, 0, true);
        Pipe &p = *r.pipe;
        svs::Map &m = p.stream(0).map;
        for (svs::Frame *f : m.keyframes_) {                                // descriptor rows in reverse feature order: row r describes feature nf - 1 - r
            const int nf = (int)f->left.size();
            f->desc.assign(32 * (size_t)nf, 0); f->desc_feat_indx.resize((size_t)nf); f->described = true; f->loop_checked = f != m.keyframes_[7];
            for (int i = 0; i < nf; ++i) f->desc_feat_indx[(size_t)i] = nf - 1 - i;
        }
        r.k.cand = 0; r.k.T_corr = r.corr(7); r.k.need_correction = on == 2 ? 0 : 1;
        r.k.mc = { 5, 4, 1 }; r.k.mq = { 5, 4, 0 };                        // features (0, 0), (1, 1) and (4, 5): keyframe 0's feature 4 has no landmark
        CHECK(p.ConfigureLoopStore(16, 4));
        std::vector<float> vecs(8, 1.0f);
        Pipe::LoopDetectParams prm{};
        prm.keyframes_to_ignore_after_loop = 0; prm.local_fusion = on != 0;
        const std::string before = dump(p);
        std::vector<Pipe::LoopDetection> out;
        CHECK(p.DetectLoops(vecs.data(), prm, &out));
        CHECK(out.size() == 2 && out[0].verified && out[0].loop.status == SVSLAM_LOOP_ACCEPTED && !out[1].is_keyframe);
        if (on == 1) {
            CHECK(r.k.lf_calls == 1 && out[0].fused && out[0].fusion.pairs == 2 && out[0].fusion.merged == 2 && out[0].fusion.revived == 2);
            CHECK(p.LastDetections()[0].fused);
            save(dir, "detect_loops.before", before); save(dir, "detect_loops.after", dump(p));
            save_job(dir, "detect_loops", job(7, 0, r.k.T_corr, { { 0, 0 }, { 1, 1 } }), out[0].fusion);
        } else {
            // the loop edge is recorded either way (VerifyLoops); nothing else moves
            CHECK(r.k.lf_calls == 0 && !out[0].fused && out[0].fusion.pairs == 0 && dump(p) == before);
        }
    }
    std::printf("detect_loops_flag ok\n");
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    scenarios(dir);
    refusals();
    detect_loops_flag(dir);
    if (g_fail) { std::fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    std::printf("all local-fusion host tests passed\n");
    return 0;
}
