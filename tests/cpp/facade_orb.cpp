// facade_orb.cpp — the drop-in facade (host/slam_facade.h) with `keypoint_feature_detector` in the configuration file: runs the
// sequence the Python side wrote through VisualOdometry like tests/cpp/facade_kitti.cpp, prints one line per frame and writes the
// outputs; what the facade throws is printed as "threw: <message>" (exit status 3) for the tests of the refusals.
// -DFACADE_ORACLE: the oracle's kernel provider, which has no ORB detector (CPU test); otherwise the HIP kernels (GPU test).
#include <cstdio>
#include <cstdlib>
#ifdef FACADE_ORACLE
#include "../../oracle/kernels_oracle.h"
#include "../../stereovision-slam_amd/host/slam_facade.h"
typedef svs::OracleKernels Provider;
#else
#include "../../stereovision-slam_amd/host/slam_facade_hip.h"
typedef svs::HipKernels Provider;
#endif

using namespace svs::facade;

static int run(const char *config, const char *out_dir)
{
    VisualOdometryT<Provider> vo(config);
    if (!vo.initialize()) { std::printf("initialize failed\n"); return 1; }
    int n = 0, nkf = 0;
    bool said = false;
    while (vo.step()) {
        if (!said) {
            std::printf("map: %s detector: %d\n", vo.frontend()->pipeline()->MapOnDevice() ? "device" : "host", vo.frontend()->pipeline()->detector());
            said = true;
        }
        Frame::Ptr f = vo.frontend()->GetLastFrame();
        if (!f) { std::printf("no frame\n"); return 1; }
        nkf += f->is_keyframe_ ? 1 : 0;
        std::printf("frame %lu status %d kf %d feat %d inl %d\n", f->id_, (int)vo.GetFrontendStatus(), (int)f->is_keyframe_, f->n_features_, f->n_inliers_);
        ++n;
    }
    if (!vo.saveSLAMOutputInFile(out_dir)) { std::printf("no outputs\n"); return 1; }
    std::printf("frames %d keyframes %d landmarks %zu\nfacade orb ok\n", n, nkf, vo.map()->GetAllMapPoints().size());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: facade_orb <config.yaml> <out_dir>\n"); return 2; }
    try {
        return run(argv[1], argv[2]);
    } catch (const std::exception &e) {
        std::printf("threw: %s\n", e.what());
        return 3;
    }
}
