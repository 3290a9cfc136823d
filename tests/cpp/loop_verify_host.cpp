// loop_verify_host.cpp — the host glue of the loop verification (slam_host.h: Pipeline::VerifyLoops, KeyframeFeatures,
// Map::ArchiveIndex / set_keep_features) on a small scripted map, with a CPU kernel provider whose loop-verify call is
// csrc/k_loop_verify.h compiled for the host (tests/cpp/lv_host_emu) and whose pose-graph call is csrc/k_pose_graph.h likewise.
// Built and run by tests/test_host_loop_verify.py; no GPU.
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "lv_host_emu/emu.cpp"
#include "pg_host_emu/emu.cpp"
#include "../../stereovision-slam_amd/host/slam_host.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

// what Pipeline<K> needs of a provider on the paths this program takes; the loop-verify call records what it was handed
struct CpuKernels {
    int lv_calls = 0, pg_calls = 0;
    std::vector<svslam_loop_job> jobs;
    svslam_loop_params prm;
    std::vector<double> xyz;
    std::vector<uint8_t> has;
    std::vector<float> uv;
    std::string err;
    const char *last_error() { return err.c_str(); }
    int local_ba_collect(int, svslam_ba_job *, int, double *, int, double *, int, double *) { return -1; }
    int dmap_ba_collect(int, svslam_dmap_job *, int *) { return -1; }
    int dmap_read(int, long long *, int *, double *, int *, int *, double *, int *, uint8_t *) { return -1; }
    int pose_graph(int n, svslam_pg_job *j, int total_kf, double *P, const uint8_t *F, int total_edges, const int *a, const int *b,
                   const double *M, int total_pts, const int *an, double *X, int iters)
    {
        ++pg_calls;
        static_assert(sizeof(EmuJob) == sizeof(svslam_pg_job), "job layout");
        const int rc = emu_pose_graph(n, reinterpret_cast<EmuJob *>(j), total_kf, P, F, total_edges, a, b, M, total_pts, an, X, iters, nullptr);
        if (rc) err = emu_pg_error();
        return rc;
    }
    int loop_verify(int n, svslam_loop_job *j, const svslam_loop_params *p, int total_c, const uint8_t *dc, const double *X, const uint8_t *H,
                    int total_q, const uint8_t *dq, const float *U, int *mc, int *mq, int *md, uint8_t *mi)
    {
        ++lv_calls;
        jobs.assign(j, j + n); prm = *p; xyz.assign(X, X + 3 * (size_t)total_c); has.assign(H, H + total_c); uv.assign(U, U + 2 * (size_t)total_q);
        static_assert(sizeof(EmuLoopJob) == sizeof(svslam_loop_job) && sizeof(EmuLoopParams) == sizeof(svslam_loop_params), "layouts");
        const int rc = emu_loop_verify(n, reinterpret_cast<EmuLoopJob *>(j), reinterpret_cast<const EmuLoopParams *>(p), total_c, dc, X, H, total_q, dq, U,
                                       mc, mq, md, mi);
        if (rc) err = emu_lv_error();
        return rc;
    }
};
typedef svs::Pipeline<CpuKernels> Pipe;

static svs::SE3 expy(double ang, double tx, double tz)            // rotation about y, translation
{
    svs::SE3 T; T.v[1] = std::sin(0.5 * ang); T.v[3] = std::cos(0.5 * ang); T.v[4] = tx; T.v[6] = tz;
    return T;
}

static const int NL = 40, NKF = 5;
static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static void landmark(int i, double *p)
{
    uint32_t s = 77u + 13u * (uint32_t)i;
    p[0] = -6.0 + 12.0 * (lcg(s) % 1000) / 1000.0; p[1] = -1.5 + 3.0 * (lcg(s) % 1000) / 1000.0; p[2] = 8.0 + 25.0 * (lcg(s) % 1000) / 1000.0;
    for (int k = 0; k < 3; ++k) p[k] = (double)(float)p[k];              // exactly representable: archived (float) and live positions agree
}
static void descriptor(uint32_t key, uint8_t *d)
{
    uint32_t s = key * 2654435761u + 12345u;
    for (int k = 0; k < 32; ++k) d[k] = (uint8_t)(lcg(s) & 0xff);
}

static svs::Config config()
{
    svs::Config cfg;
    cfg.cam_l.fx = 718.0; cfg.cam_l.fy = 705.0; cfg.cam_l.cx = 607.0; cfg.cam_l.cy = 185.0;
    cfg.cam_l.pose = expy(0.02, 0.03, -0.01);
    cfg.cam_r = cfg.cam_l;
    return cfg;
}

// NKF keyframes on a gentle curve, every one seeing the NL landmarks: feature i of every keyframe is landmark i.  In the candidate
// keyframe (1): features 0-2 have no landmark (mp == -1), landmarks 3-8 are DEAD (archived) by the time of the call, the rest live.
static void script(Pipe &pipe, const svs::Config &cfg, int s, std::vector<long> &ids)
{
    svs::Stream &st = pipe.stream(s);
    ids.assign(NL, -1);
    std::vector<svs::MapPoint *> mps(NL, nullptr);
    for (int i = 0; i < NL; ++i) {
        svs::MapPoint *m = st.map.CreateNewMappoint();
        landmark(i, m->pos);
        mps[(size_t)i] = m; ids[(size_t)i] = m->id;
        if (i >= 9) st.map.InsertMapPoint(m);                        // 3-8 never become active: they die once unobserved
    }
    svs::SE3 T;
    for (int k = 0; k < NKF; ++k) {
        if (k > 0) T = expy(0.03, 0.1, -0.8) * T;
        st.kf_store.emplace_back(new svs::Frame());
        svs::Frame *f = st.kf_store.back().get();
        f->id = 3 * k; f->keyframe_id = k; f->is_keyframe = true; f->pose = T;
        f->left.resize(NL); f->right.resize(NL); f->right_ok.assign(NL, 0);
        if (k > 0) { f->prev_keyframe = st.kf_store[(size_t)k - 1].get(); f->relative_pose_pkf = f->pose * f->prev_keyframe->pose.inverse(); }
        const svs::SE3 Tc = cfg.cam_l.pose * T;
        for (int i = 0; i < NL; ++i) {
            double uv[2];
            cfg.cam_l.project(Tc, mps[(size_t)i]->pos, uv);
            f->left[(size_t)i].x = (float)uv[0]; f->left[(size_t)i].y = (float)uv[1];
            f->left[(size_t)i].mp = (k == 1 && i < 3) ? -1 : ids[(size_t)i];
        }
        st.map.InsertKeyFrame(f);
        if (k == 1)
            for (int i = 3; i < 9; ++i) {                            // observed, then unobserved and outside the active set: limbo
                st.map.AddObservation(mps[(size_t)i], svs::ObsRef{ f, i, true });
                st.map.RemoveObservation(mps[(size_t)i], svs::ObsRef{ f, i, true });
            }
        std::vector<svs::Feature> carried(f->left.begin() + 9, f->left.end());      // tracking carries 9.. forward: 3-8 are dead at k == 1
        st.map.ReleaseRetired(&carried, k + 1);
    }
}

struct Desc { std::vector<uint8_t> d; std::vector<int> idx; };
// descriptors of a keyframe's features, rows in DESCENDING feature order (desc_feat_indx is not the identity); salt != 0: unrelated
static Desc describe(int n, uint32_t salt)
{
    Desc D; D.d.resize(32 * (size_t)n); D.idx.resize((size_t)n);
    for (int r = 0; r < n; ++r) { const int feat = n - 1 - r; D.idx[(size_t)r] = feat; descriptor((uint32_t)feat + salt, &D.d[32 * (size_t)r]); }
    return D;
}
static Pipe::LoopQuery query(int s, long kf, long cand, const Desc &q, const Desc &c)
{
    return Pipe::LoopQuery{ s, kf, cand, (int)q.idx.size(), q.d.data(), (int)q.idx.size(), q.idx.data(), (int)c.idx.size(), c.d.data(), (int)c.idx.size(), c.idx.data() };
}
static svslam_loop_params params()
{
    svslam_loop_params p;
    std::memset(&p, 0, sizeof(p));
    p.min_matches = 20; p.ransac_iters = 100; p.reproj_px = 5.991; p.max_pose_distance = 20.0; p.min_pose_difference = 1.0; p.max_pose_difference = 50.0;
    return p;
}
static bool untouched(Pipe &pipe, int nstreams)
{
    for (int s = 0; s < nstreams; ++s)
        for (auto &f : pipe.stream(s).kf_store) if (f->loop_keyframe) return false;
    return true;
}

static void gather_accept_and_pose_graph()
{
    const svs::Config cfg = config();
    CpuKernels k; Pipe pipe(cfg, k, 2);
    std::vector<long> ids0, ids1;
    script(pipe, cfg, 0, ids0); script(pipe, cfg, 1, ids1);
    CHECK(pipe.stream(0).map.num_archived() == 6);
    const Desc q = describe(NL, 0), c = describe(NL, 0), other = describe(NL, 1000);
    std::vector<Pipe::LoopResult> res;
    // stream 0: keyframe 4 against keyframe 1, the same landmarks: a loop.  stream 1: unrelated descriptors, no loop.
    CHECK(pipe.VerifyLoops({ query(0, 4, 1, q, c), query(1, 3, 1, q, other) }, params(), &res));
    CHECK(k.lv_calls == 1 && k.jobs.size() == 2 && res.size() == 2);                  // one provider call for both streams
    const double cam4[4] = { 718.0, 705.0, 607.0, 185.0 };
    CHECK(std::memcmp(k.prm.cam, cam4, 32) == 0 && std::memcmp(k.prm.ext_l, cfg.cam_l.pose.v, 56) == 0);
    // what was gathered for stream 0: row r is feature NL - 1 - r
    const svs::Frame *kf4 = pipe.stream(0).kf_store[4].get(), *kf1 = pipe.stream(0).kf_store[1].get();
    CHECK(std::memcmp(k.jobs[0].T_cur, kf4->pose.v, 56) == 0 && std::memcmp(k.jobs[0].T_cand, kf1->pose.v, 56) == 0);
    int n_has = 0;
    for (int r = 0; r < NL; ++r) {
        const int feat = NL - 1 - r;
        double want[3]; landmark(feat, want);
        CHECK(k.uv[2 * (size_t)r] == kf4->left[(size_t)feat].x && k.uv[2 * (size_t)r + 1] == kf4->left[(size_t)feat].y);
        CHECK(k.has[(size_t)r] == (feat < 3 ? 0 : 1));                                  // mp == -1 dropped; archived (3-8) and live gathered
        if (feat >= 3) { ++n_has; for (int a = 0; a < 3; ++a) CHECK(k.xyz[3 * (size_t)r + (size_t)a] == want[a]); }
        if (feat >= 3 && feat < 9) CHECK(pipe.stream(0).map.point(ids0[(size_t)feat]) == nullptr);      // really from the archive
    }
    CHECK(n_has == NL - 3);
    CHECK(res[0].status == SVSLAM_LOOP_ACCEPTED && res[0].n_matches == NL && res[0].n_points == NL - 3 && res[0].n_inliers == NL - 3 && !res[0].need_correction);
    CHECK((int)res[0].match_c.size() == NL && res[0].match_c[0] == 0 && res[0].match_q[0] == 0 && res[0].match_dist[0] == 0);
    int ninl = 0; for (uint8_t b : res[0].match_inlier) ninl += b;
    CHECK(ninl == NL - 3);
    CHECK((res[0].T_corr * kf4->pose.inverse()).log_norm() < 1e-4 && res[0].d < 1e-4);
    CHECK((res[0].T_rel * (kf4->pose * kf1->pose.inverse()).inverse()).log_norm() < 1e-4);
    // unrelated descriptors are all "matched" (d_min is large, so is 2 d_min): the geometry rejects them
    CHECK(res[1].status == SVSLAM_LOOP_FEW_INLIERS && res[1].n_matches == NL && res[1].match_c.size() == (size_t)NL);
    // the accepted pair is a loop edge, the rejected one is not
    CHECK(kf4->loop_keyframe == kf1 && std::memcmp(kf4->loop_relative_pose.v, res[0].T_rel.v, 56) == 0);
    for (auto &f : pipe.stream(1).kf_store) CHECK(f->loop_keyframe == nullptr);
    std::vector<Pipe::PoseGraphStats> stats;
    CHECK(pipe.PoseGraphOptimization({ 0, 1 }, 22, &stats));
    CHECK(stats.size() == 2 && stats[0].nedge == NKF && stats[1].nedge == NKF - 1);       // exactly one more edge
    // KeyframeFeatures: the same gather, read-only
    std::vector<double> f8; double pose[7];
    CHECK(pipe.KeyframeFeatures(0, 1, &f8, pose) && f8.size() == 8 * (size_t)NL && std::memcmp(pose, kf1->pose.v, 56) == 0);
    CHECK(f8[2] == -1.0 && f8[4] == 0.0 && f8[8 * 5 + 4] == 1.0 && f8[8 * 5 + 2] == (double)ids0[5] && f8[8 * 20 + 4] == 1.0 && f8[8 * 20 + 0] == (double)kf1->left[20].x);
    CHECK(!pipe.KeyframeFeatures(0, NKF, &f8, pose) && !pipe.KeyframeFeatures(2, 0, &f8, pose));
    std::printf("gather_accept_and_pose_graph ok (n_inliers %d, d %.3g)\n", res[0].n_inliers, res[0].d);
}

static void refusals()
{
    const svs::Config cfg = config();
    CpuKernels k; Pipe pipe(cfg, k, 2);
    std::vector<long> ids;
    script(pipe, cfg, 0, ids);
    const Desc q = describe(NL, 0), c = describe(NL, 0);
    std::vector<Pipe::LoopResult> res;
    auto refused = [&](const Pipe::LoopQuery &Q, const char *word) {
        CHECK(!pipe.VerifyLoops({ query(0, 4, 1, q, c), Q }, params(), &res));
        CHECK(pipe.last_error().find(word) != std::string::npos);
        CHECK(k.lv_calls == 0 && untouched(pipe, 2));
    };
    refused(query(2, 4, 1, q, c), "no such stream");
    refused(query(-1, 4, 1, q, c), "no such stream");
    refused(query(1, 4, 1, q, c), "not a keyframe");                       // stream 1 has no keyframes
    refused(query(0, NKF, 1, q, c), "not a keyframe");
    refused(query(0, 4, -1, q, c), "not a keyframe");
    refused(query(0, 3, 3, q, c), "older");
    refused(query(0, 2, 4, q, c), "older");
    Desc bad = c; bad.idx[5] = NL;
    refused(query(0, 4, 1, q, bad), "not a feature");
    bad = c; bad.idx[5] = -1;
    refused(query(0, 4, 1, q, bad), "not a feature");
    bad = q; bad.idx[7] = bad.idx[8];
    refused(query(0, 4, 1, bad, c), "repeated");
    Pipe::LoopQuery mism = query(0, 4, 1, q, c); mism.nfc = NL - 1;
    refused(mism, "count");
    mism = query(0, 4, 1, q, c); mism.nfq = NL + 1;
    refused(mism, "count");
    // the provider's refusal (a parameter outside its range) comes back as a refusal too, and records no edge
    svslam_loop_params p = params(); p.ransac_iters = 0;
    CHECK(!pipe.VerifyLoops({ query(0, 4, 1, q, c) }, p, &res) && k.lv_calls == 1 && untouched(pipe, 2));
    CHECK(pipe.last_error().find("ransac_iters") != std::string::npos);
    // device_map = 1
    svs::Config dc = config(); dc.device_map = 1; dc.resident_track = 1;
    CpuKernels dk; Pipe dpipe(dc, dk, 1);
    CHECK(!dpipe.VerifyLoops({ query(0, 4, 1, q, c) }, params(), &res) && dk.lv_calls == 0);
    CHECK(dpipe.last_error().find("device") != std::string::npos);
    std::printf("refusals ok\n");
}

// keep_archive off: a dead landmark is found in neither place (has_xyz = 0); released feature lists: refused unless kept
static void archive_off_and_released_lists()
{
    svs::Config cfg = config();
    {
        CpuKernels k; Pipe pipe(cfg, k, 1);
        pipe.stream(0).map.set_keep_archive(false);
        std::vector<long> ids;
        script(pipe, cfg, 0, ids);
        const Desc q = describe(NL, 0), c = describe(NL, 0);
        std::vector<Pipe::LoopResult> res;
        CHECK(pipe.VerifyLoops({ query(0, 4, 1, q, c) }, params(), &res));
        int n_has = 0; for (uint8_t h : k.has) n_has += h;
        CHECK(n_has == NL - 9 && res[0].n_points == NL - 9 && res[0].status == SVSLAM_LOOP_ACCEPTED);
    }
    for (int keep = 0; keep < 2; ++keep) {
        cfg.num_active_keyframes = 3;                                       // keyframe 1 leaves the window
        CpuKernels k; Pipe pipe(cfg, k, 1);
        pipe.SetKeepKeyframeFeatures(keep != 0);
        std::vector<long> ids;
        script(pipe, cfg, 0, ids);
        const Desc q = describe(NL, 0), c = describe(NL, 0);
        std::vector<Pipe::LoopResult> res;
        const bool ok = pipe.VerifyLoops({ query(0, 4, 1, q, c) }, params(), &res);
        if (keep) CHECK(ok && res[0].status == SVSLAM_LOOP_ACCEPTED && pipe.stream(0).kf_store[1]->left.size() == (size_t)NL);
        else CHECK(!ok && pipe.last_error().find("released") != std::string::npos && k.lv_calls == 0);
    }
    std::printf("archive_off_and_released_lists ok\n");
}

int main()
{
    gather_accept_and_pose_graph();
    refusals();
    archive_off_and_released_lists();
    if (g_fail) { std::fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
    std::printf("all loop-verify host tests passed\n");
    return 0;
}
