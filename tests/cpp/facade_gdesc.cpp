// facade_gdesc.cpp — the facade closing the loop-detection path from the frames alone (tests/test_gpu_facade_global_desc.py):
// VisualOdometry::step() over a KITTI-layout sequence with `loop_global_descriptor: <file written by gdesc.save>` in the configuration,
// and after every step VisualOdometry::DetectLoop(&D) WITHOUT a vector.  The program keeps its own books (which ids are stored, which
// keyframe last closed a loop) and every result must agree with them; the vector the network computes for a new keyframe is read
// through Pipeline::DescribeGlobalNewKeyframes and must be the one DetectLoop(vec, ...) would be given: a second facade over the
// same sequence is fed exactly those vectors and must return the same results; <expect: 1>.  With the key absent the overload
// throws; <expect: 0>.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../stereovision-slam_amd/host/slam_facade_hip.h"

using namespace svs::facade;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: facade_gdesc <config.yaml> <config of the twin fed the vectors> <expect detection: 0|1>\n"); return 2; }
    typedef svs::Pipeline<svs::HipKernels> Pipe;
    VisualOdometryT<svs::HipKernels> vo(argv[1]), twin(argv[2]);
    CHECK(vo.initialize() && twin.initialize());
    const bool expect = std::atoi(argv[3]) != 0;
    std::vector<long> stored;
    long last_closed = -1;
    size_t nkf = 0, n_searched = 0, n_skipped = 0, n_accepted = 0;
    while (vo.step()) {
        CHECK(twin.step());
        Pipe *pipe = vo.frontend()->pipeline();
        CHECK(pipe && !pipe->MapOnDevice());
        const size_t now = pipe->stream(0).kf_store.size();
        CHECK(now == nkf || now == nkf + 1);
        Pipe::LoopDetection D, T;
        if (!expect) {
            if (now == nkf) continue;
            bool refused = false;
            try { vo.DetectLoop(&D); } catch (const SLAMException &e) { refused = std::strstr(e.what(), "loop_global_descriptor") != nullptr; }
            CHECK(refused && pipe->GlobalDescriptorDim() == 0);
            std::printf("facade gdesc ok: refused without loop_global_descriptor\n");
            return 0;
        }
        const int dim = pipe->GlobalDescriptorDim();
        CHECK(dim >= 1);
        if (now == nkf) {                                   // no new keyframe: nothing to do, and nothing done
            CHECK(vo.DetectLoop(&D) && !D.is_keyframe && !D.searched && !D.stored);
            continue;
        }
        const long k = (long)nkf;
        nkf = now;
        std::vector<float> v;
        int n = 0;
        CHECK(pipe->DescribeGlobalNewKeyframes(&v, &n) && n == 1 && (int)v.size() == dim);
        bool any = false;
        for (float x : v) { CHECK(x == x); any = any || x != 0.f; }
        CHECK(any);
        CHECK(vo.DetectLoop(&D));
        CHECK(twin.DetectLoop(v.data(), &T));               // the twin has no network: it is given the vector
        CHECK(D.is_keyframe && D.kf_id == k && T.is_keyframe && T.kf_id == k);
        CHECK(D.skipped == T.skipped && D.searched == T.searched && D.verified == T.verified && D.stored == T.stored);
        CHECK(std::memcmp(&D.cand, &T.cand, sizeof(D.cand)) == 0);
        if (D.verified) {
            CHECK(D.loop.status == T.loop.status && D.loop.n_matches == T.loop.n_matches && D.loop.n_inliers == T.loop.n_inliers);
            CHECK(std::memcmp(D.loop.T_corr.v, T.loop.T_corr.v, 56) == 0 && D.loop.match_c == T.loop.match_c);
        }
        if (last_closed >= 0 && k - last_closed <= 1) {
            CHECK(D.skipped && !D.searched && !D.verified && !D.stored);
            ++n_skipped;
        } else {
            CHECK(!D.skipped && D.searched);
            ++n_searched;
            const int compared = (int)std::count_if(stored.begin(), stored.end(), [k](long id) { return k - id >= 2; });
            CHECK(D.cand.n_compared == compared && D.cand.status != SVSLAM_LC_BAD_VECTOR);
            CHECK(D.verified == (D.cand.status == SVSLAM_LC_FOUND));
            const bool closed = D.verified && D.loop.status == SVSLAM_LOOP_ACCEPTED;
            CHECK(D.stored == !closed);
            if (closed) { last_closed = k; ++n_accepted; } else stored.push_back(k);
        }
        int cnt = -1;
        CHECK(vo.frontend()->kernels()->loopdb_count(0, &cnt) == 0 && cnt == (int)stored.size());
        CHECK(pipe->LastClosedKeyframe(0) == last_closed);
        Pipe::LoopDetection twice;
        CHECK(vo.DetectLoop(&twice) && !twice.is_keyframe);               // a keyframe is handled once
    }
    CHECK(nkf >= 4 && n_searched >= 3);
    std::printf("facade gdesc ok: %zu keyframes, %zu stored, %zu searched, %zu accepted, %zu skipped\n", nkf, stored.size(), n_searched, n_accepted, n_skipped);
    return 0;
}
