// facade_loop.cpp — the facade's loop-closure path on the HIP kernels (tests/test_gpu_facade_loop.py), driven the way a user of
// the reference drives it: VisualOdometry::run() over a KITTI-layout sequence.  The SetLoopClosure hook plays the caller's place
// recognition: with <loop> = 1 every new keyframe from the fourth on is "matched" with keyframe 1 and the measured relative pose
// is the ground truth (gt file: 7 doubles per frame, T_cw).  run() then does what the reference does at shutdown: Stop() — the
// pose-graph optimisation when global_pose_graph_optimization >= 1 — and the outputs under the config's output_dir.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include "../../stereovision-slam_amd/host/slam_facade_hip.h"

using namespace svs::facade;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
#define CHECK_VOID(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: facade_loop <config.yaml> <gt.txt> <loop: 0|1>\n"); return 2; }
    VisualOdometryT<svs::HipKernels> vo(argv[1]);
    CHECK(vo.initialize());
    std::vector<svs::SE3> gt;
    {
        std::ifstream f(argv[2]);
        double v[7];
        while (f >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6]) gt.push_back(svs::SE3(v));
    }
    const bool loop = std::atoi(argv[3]) != 0;
    unsigned long frame_of_kf1 = 0;
    int n_edges = 0;
    vo.frontend()->SetLoopClosure([&](const Frame::Ptr &f) {
        const unsigned long k = f->keyframe_id_;
        if (k == 1) frame_of_kf1 = f->id_;
        if (k == 3) {        // refusals of the facade call: ids that are no keyframes, a loop keyframe that is not older
            CHECK_VOID(!vo.AddLoopEdge(k + 1, 1, svs::SE3()) && !vo.AddLoopEdge(1, 1, svs::SE3()) && !vo.AddLoopEdge(1, k, svs::SE3()));
        }
        if (loop && k >= 3) {
            CHECK_VOID(f->id_ < gt.size());
            CHECK_VOID(vo.AddLoopEdge(k, 1, gt[f->id_] * gt[frame_of_kf1].inverse()));
            ++n_edges;
        }
    });
    vo.run();
    std::printf("map: %s\n", vo.frontend()->pipeline()->MapOnDevice() ? "device" : "host");
    const auto kfs = vo.map()->GetAllKeyFrames();
    CHECK(kfs.size() >= 4 && (!loop || n_edges == (int)kfs.size() - 3));
    for (const auto &k : kfs)
        std::printf("kf %lu frame %lu pose %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k.keyframe_id, k.id, k.pose.v[0], k.pose.v[1], k.pose.v[2],
                    k.pose.v[3], k.pose.v[4], k.pose.v[5], k.pose.v[6]);
    std::printf("facade loop ok\n");
    return 0;
}
