// pipeline_capi.cpp — product build of the host pipeline: the reference-shaped
// Frontend/Backend/Map host logic bound to the HIP kernels through the C ABI.
#include "kernels_hip.h"
#define SVS_PIPE_KERNELS svs::HipKernels
#define SVS_PIPE_MAKE_KERNELS(lim) new svs::HipKernels(lim)
#define SVS_PIPE_IMAGES_ARE_DEVICE 1
#include "pipeline_capi_impl.h"

extern "C" void *svs_pipe_kernel_ctx(void *p) { return static_cast<PipeHandle *>(p)->kernels->ctx(); }

// Loop edges and the global pose-graph optimisation (product build only: the CPU twins' kernel providers have no pose-graph call)
extern "C" int svs_pipe_add_loop_edge(void *p, int stream, long long kf_id, long long loop_kf_id, const double *T_rel7)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (!T_rel7) { g_err = "svs_pipe_add_loop_edge: null pose"; return -1; }
    if (h->pipe->AddLoopEdge(stream, (long)kf_id, (long)loop_kf_id, svs::SE3(T_rel7))) return 0;
    g_err = h->pipe->last_error();
    return -1;
}
extern "C" int svs_pipe_pose_graph_optimization(void *p, int nstreams, const int *streams, int iters, double *stats7_or_null)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        std::vector<int> ss;
        if (streams) ss.assign(streams, streams + nstreams);
        else for (int s = 0; s < h->pipe->nstreams(); ++s) ss.push_back(s);
        std::vector<svs::Pipeline<SVS_PIPE_KERNELS>::PoseGraphStats> st;
        if (!h->pipe->PoseGraphOptimization(ss, iters, &st)) { g_err = h->pipe->last_error(); return -1; }
        if (stats7_or_null)
            for (size_t i = 0; i < st.size(); ++i) {
                double *o = stats7_or_null + 7 * i;
                o[0] = st[i].nkf; o[1] = st[i].nedge; o[2] = st[i].npt; o[3] = st[i].iters; o[4] = st[i].trials; o[5] = st[i].chi2_before; o[6] = st[i].chi2_after;
            }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" void *svs_pipe_backend_ctx(void *p) { return static_cast<PipeHandle *>(p)->kernels->backend_ctx(); }
