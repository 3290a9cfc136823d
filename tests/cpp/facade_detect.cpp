// facade_detect.cpp — the facade's loop detection on the HIP kernels (tests/test_gpu_facade_detect.py): VisualOdometry::step() over a
// KITTI-layout sequence, and after every step VisualOdometry::DetectLoop with a planted global descriptor: keyframe k >= 2 gets a noisy
// copy of keyframe k - 2's.  The configuration sets loop_min_keyframe_gap: 2 and keyframes_to_ignore_after_loop: 1 so that a short run
// reaches the branches.  The program keeps its own books (which ids are stored, which keyframe last closed a loop) and every result
// must agree with them; <expect: 1>.  With `loop_descriptors` absent DetectLoop is refused; <expect: 0>.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "../../stereovision-slam_amd/host/slam_facade_hip.h"

using namespace svs::facade;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const int DIM = 64;

static std::vector<float> planted(std::vector<std::vector<float>> &all, size_t k)
{
    std::mt19937 g((unsigned)(77 + k));
    std::normal_distribution<float> n(0.0f, 1.0f);
    std::vector<float> v((size_t)DIM);
    for (float &x : v) x = n(g);
    if (k >= 2) for (int e = 0; e < DIM; ++e) v[(size_t)e] = all[k - 2][(size_t)e] + 0.01f * v[(size_t)e];
    all.push_back(v);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: facade_detect <config.yaml> <expect detection: 0|1>\n"); return 2; }
    typedef svs::Pipeline<svs::HipKernels> Pipe;
    VisualOdometryT<svs::HipKernels> vo(argv[1]);
    CHECK(vo.initialize());
    const bool expect = std::atoi(argv[2]) != 0;
    std::vector<std::vector<float>> vecs;
    std::vector<long> stored;
    long last_closed = -1;
    size_t nkf = 0, n_accepted = 0, n_skipped = 0, n_found = 0;
    while (vo.step()) {
        Pipe *pipe = vo.frontend()->pipeline();
        CHECK(pipe && !pipe->MapOnDevice());
        const size_t now = pipe->stream(0).kf_store.size();
        CHECK(now == nkf || now == nkf + 1);
        Pipe::LoopDetection D;
        if (!expect) {
            if (now == nkf) continue;
            bool refused = false;
            try { vo.DetectLoop(std::vector<float>((size_t)DIM, 1.0f).data(), &D); } catch (const SLAMException &e) { refused = std::strstr(e.what(), "loop_descriptors") != nullptr; }
            CHECK(refused);
            std::printf("facade detect ok: refused without loop_descriptors\n");
            return 0;
        }
        if (now == nkf) {                                   // no new keyframe: nothing to do, and nothing done
            const std::vector<float> any((size_t)DIM, 1.0f);
            CHECK(vo.DetectLoop(any.data(), &D) && !D.is_keyframe && !D.searched && !D.stored);
            continue;
        }
        const long k = (long)nkf;
        nkf = now;
        const std::vector<float> v = planted(vecs, (size_t)k);
        CHECK(vo.DetectLoop(v.data(), &D));
        CHECK(D.is_keyframe && D.kf_id == k);
        if (last_closed >= 0 && k - last_closed <= 1) {
            CHECK(D.skipped && !D.searched && !D.verified && !D.stored);
            ++n_skipped;
        } else {
            CHECK(!D.skipped && D.searched);
            const int compared = (int)std::count_if(stored.begin(), stored.end(), [k](long id) { return k - id >= 2; });
            CHECK(D.cand.n_compared == compared && D.cand.status != SVSLAM_LC_BAD_VECTOR);
            CHECK(D.verified == (D.cand.status == SVSLAM_LC_FOUND));
            if (D.verified) {
                ++n_found;
                CHECK(std::find(stored.begin(), stored.end(), (long)D.cand.cand_kf) != stored.end() && k - D.cand.cand_kf >= 2);
                CHECK(D.cand.best_sim > 0.95f && D.cand.best_kf == D.cand.cand_kf);
                Pipe::LoopResult again;                     // the verification is VerifyLoop's on the stored descriptors
                const svs::Frame *edge = pipe->stream(0).kf_store[(size_t)k]->loop_keyframe;           // an accepted pair is a loop edge already
                CHECK((edge != nullptr) == (D.loop.status == SVSLAM_LOOP_ACCEPTED));
                if (edge) CHECK(edge->keyframe_id == D.cand.cand_kf);
                CHECK(vo.VerifyLoop((unsigned long)k, (unsigned long)D.cand.cand_kf, &again));
                CHECK(again.status == D.loop.status && again.n_matches == D.loop.n_matches && again.n_inliers == D.loop.n_inliers);
                CHECK(std::memcmp(again.T_corr.v, D.loop.T_corr.v, 56) == 0 && again.match_c == D.loop.match_c);
            } else {
                CHECK(D.cand.cand_kf == -1);
            }
            const bool closed = D.verified && D.loop.status == SVSLAM_LOOP_ACCEPTED;
            CHECK(D.stored == !closed);
            if (closed) { last_closed = k; ++n_accepted; } else stored.push_back(k);
        }
        int n = -1;
        CHECK(vo.frontend()->kernels()->loopdb_count(0, &n) == 0 && n == (int)stored.size());
        CHECK(pipe->LastClosedKeyframe(0) == last_closed);
        Pipe::LoopDetection twice;
        CHECK(vo.DetectLoop(v.data(), &twice) && !twice.is_keyframe);     // a keyframe is handled once
    }
    CHECK(nkf >= 4 && n_found >= 1);
    std::vector<int> ids(stored.size());
    std::vector<float> rows(stored.size() * (size_t)DIM);
    CHECK(vo.frontend()->kernels()->loopdb_read(0, (int)stored.size(), ids.data(), rows.data()) == 0);
    for (size_t i = 0; i < stored.size(); ++i) CHECK(ids[i] == (int)stored[i]);
    std::printf("facade detect ok: %zu keyframes, %zu stored, %zu verified, %zu accepted, %zu skipped\n", nkf, stored.size(), n_found, n_accepted, n_skipped);
    return 0;
}
