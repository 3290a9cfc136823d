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
// Loop verification (product build only, like the pose graph)
extern "C" int svs_pipe_verify_loops(void *p, int nqueries, const svs_loop_query *queries, const void *params, svs_loop_result *results, int *match4_or_null)
{
    typedef svs::Pipeline<SVS_PIPE_KERNELS> Pipe;
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (nqueries < 0 || (nqueries > 0 && (!queries || !results)) || !params) { g_err = "svs_pipe_verify_loops: null argument"; return -1; }
    try {
        std::vector<Pipe::LoopQuery> qs((size_t)nqueries);
        for (int i = 0; i < nqueries; ++i) {
            const svs_loop_query &q = queries[i];
            qs[(size_t)i] = Pipe::LoopQuery{ q.stream, (long)q.kf_id, (long)q.cand_kf_id, q.n_desc_q, q.desc_q, q.n_idx_q, q.feat_q, q.n_desc_c, q.desc_c, q.n_idx_c, q.feat_c };
        }
        std::vector<Pipe::LoopResult> rs;
        if (!h->pipe->VerifyLoops(qs, *static_cast<const svslam_loop_params *>(params), &rs)) { g_err = h->pipe->last_error(); return -1; }
        size_t row = 0;
        for (int i = 0; i < nqueries; ++i) {
            const Pipe::LoopResult &R = rs[(size_t)i];
            svs_loop_result &o = results[i];
            o.status = R.status; o.n_matches = R.n_matches; o.n_points = R.n_points; o.n_inliers = R.n_inliers; o.need_correction = R.need_correction ? 1 : 0; o.reserved = 0;
            std::memcpy(o.T_corr, R.T_corr.v, 56); std::memcpy(o.T_rel, R.T_rel.v, 56); o.d = R.d;
            if (match4_or_null) {
                int *m = match4_or_null + 4 * row;
                std::memset(m, 0, sizeof(int) * 4 * (size_t)queries[i].n_desc_c);
                for (int k = 0; k < R.n_matches; ++k) { m[4 * k] = R.match_c[(size_t)k]; m[4 * k + 1] = R.match_q[(size_t)k]; m[4 * k + 2] = R.match_dist[(size_t)k]; m[4 * k + 3] = R.match_inlier[(size_t)k]; }
            }
            row += (size_t)queries[i].n_desc_c;
        }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" int svs_pipe_keep_keyframe_features(void *p, int on)
{
    static_cast<PipeHandle *>(p)->pipe->SetKeepKeyframeFeatures(on != 0);
    return 0;
}
extern "C" long long svs_pipe_keyframe_features(void *p, int stream, long long kf_id, double *out8, long long cap, double *pose7_or_null)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        std::vector<double> f;
        double pose[7];
        if (!h->pipe->KeyframeFeatures(stream, (long)kf_id, &f, pose)) { g_err = h->pipe->last_error(); return -1; }
        const long long n = (long long)(f.size() / 8);
        if (out8 && cap >= n) {
            if (n) std::memcpy(out8, f.data(), sizeof(double) * f.size());
            if (pose7_or_null) std::memcpy(pose7_or_null, pose, sizeof(pose));
        }
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
// Loop-closure descriptors (product build only: the CPU twins' providers have no brief_describe)
extern "C" int svs_pipe_describe_new_keyframes(void *p, const void *brief_params_or_null)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        int n = 0;
        if (!h->pipe->DescribeNewKeyframes(static_cast<const svslam_brief_params *>(brief_params_or_null), &n)) { g_err = h->pipe->last_error(); return -1; }
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" int svs_pipe_describe_new_keyframes_oriented(void *p, const void *orb_desc_params_or_null)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        int n = 0;
        if (!h->pipe->DescribeNewKeyframesOriented(static_cast<const svslam_orb_desc_params *>(orb_desc_params_or_null), &n)) { g_err = h->pipe->last_error(); return -1; }
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" long long svs_pipe_keyframe_keypoints(void *p, int stream, long long kf_id, float *rows4, long long cap)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        const long n = h->pipe->KeyframeKeypoints(stream, (long)kf_id, rows4, (long)cap);
        if (n < 0) g_err = h->pipe->last_error();
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" long long svs_pipe_keyframe_descriptors(void *p, int stream, long long kf_id, uint8_t *desc32, int *feat, long long cap)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        const std::vector<uint8_t> *d = nullptr;
        const std::vector<int> *f = nullptr;
        if (!h->pipe->KeyframeDescriptors(stream, (long)kf_id, &d, &f)) { g_err = h->pipe->last_error(); return -1; }
        const long long n = (long long)f->size();
        if (desc32 && feat && cap >= n && n) { std::memcpy(desc32, d->data(), 32 * (size_t)n); std::memcpy(feat, f->data(), sizeof(int) * (size_t)n); }
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" int svs_pipe_verify_loops_stored(void *p, int npairs, const svs_loop_pair *pairs, const void *params, svs_loop_result *results, int *match4_or_null,
                                            long long match_rows)
{
    typedef svs::Pipeline<SVS_PIPE_KERNELS> Pipe;
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (npairs < 0 || (npairs > 0 && (!pairs || !results)) || !params) { g_err = "svs_pipe_verify_loops_stored: null argument"; return -1; }
    try {
        std::vector<Pipe::LoopPair> ps((size_t)npairs);
        long long rows = 0;
        for (int i = 0; i < npairs; ++i) {
            ps[(size_t)i] = Pipe::LoopPair{ pairs[i].stream, (long)pairs[i].kf_id, (long)pairs[i].cand_kf_id };
            const std::vector<int> *f = nullptr;
            if (!h->pipe->KeyframeDescriptors(pairs[i].stream, (long)pairs[i].cand_kf_id, nullptr, &f)) { g_err = h->pipe->last_error(); return -1; }
            rows += (long long)f->size();
        }
        if (match4_or_null && match_rows < rows) { g_err = "svs_pipe_verify_loops_stored: the match array is shorter than the candidates' descriptor rows"; return -1; }
        std::vector<Pipe::LoopResult> rs;
        if (!h->pipe->VerifyLoopsStored(ps, *static_cast<const svslam_loop_params *>(params), &rs)) { g_err = h->pipe->last_error(); return -1; }
        size_t row = 0;
        for (int i = 0; i < npairs; ++i) {
            const Pipe::LoopResult &R = rs[(size_t)i];
            svs_loop_result &o = results[i];
            o.status = R.status; o.n_matches = R.n_matches; o.n_points = R.n_points; o.n_inliers = R.n_inliers; o.need_correction = R.need_correction ? 1 : 0; o.reserved = 0;
            std::memcpy(o.T_corr, R.T_corr.v, 56); std::memcpy(o.T_rel, R.T_rel.v, 56); o.d = R.d;
            const std::vector<int> *f = nullptr;
            (void)h->pipe->KeyframeDescriptors(pairs[i].stream, (long)pairs[i].cand_kf_id, nullptr, &f);
            if (match4_or_null) {
                int *m = match4_or_null + 4 * row;
                std::memset(m, 0, sizeof(int) * 4 * f->size());
                for (int k = 0; k < R.n_matches; ++k) { m[4 * k] = R.match_c[(size_t)k]; m[4 * k + 1] = R.match_q[(size_t)k]; m[4 * k + 2] = R.match_dist[(size_t)k]; m[4 * k + 3] = R.match_inlier[(size_t)k]; }
            }
            row += f->size();
        }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
// Loop detection (product build only: the CPU twins' providers have no loop_candidates)
extern "C" int svs_pipe_loopdb_configure(void *p, int capacity, int dim)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        if (!h->pipe->ConfigureLoopStore(capacity, dim)) { g_err = h->pipe->last_error(); return -1; }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" int svs_pipe_detect_loops(void *p, const float *vecs, const svs_loop_detect_params *dp, const void *loop_params, svs_loop_detection *results)
{
    return svs_pipe_detect_loops_fused(p, vecs, dp, loop_params, 0, results, nullptr);
}
static void put_stats(svs_fusion_stats &o, bool fused, const svs::Pipeline<SVS_PIPE_KERNELS>::FusionStats &S)
{
    o.fused = fused ? 1 : 0; o.nkf = S.nkf; o.npt = S.npt; o.n_unanchored = S.n_unanchored; o.pairs = S.pairs; o.merged = S.merged;
    o.revived = S.revived; o.repointed = S.repointed; o.same_deleted = S.same_deleted; o.reserved = 0;
}
extern "C" int svs_pipe_detect_loops_fused(void *p, const float *vecs, const svs_loop_detect_params *dp, const void *loop_params, int local_fusion,
                                           svs_loop_detection *results, svs_fusion_stats *fusion_or_null)
{
    typedef svs::Pipeline<SVS_PIPE_KERNELS> Pipe;
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (!dp || !loop_params || !results) { g_err = "svs_pipe_detect_loops: null argument"; return -1; }     // vecs == NULL: the configured network
    try {
        Pipe::LoopDetectParams P;
        P.cand.weak = dp->weak; P.cand.strong = dp->strong; P.cand.max_num_weak = dp->max_num_weak; P.cand.min_gap = dp->min_gap;
        P.verify = *static_cast<const svslam_loop_params *>(loop_params);
        P.keyframes_to_ignore_after_loop = dp->keyframes_to_ignore_after_loop;
        P.local_fusion = local_fusion != 0;
        std::vector<Pipe::LoopDetection> ds;
        // a refusal of the fusion comes after the detection has taken effect: ds is filled then, and so are the results
        const bool ok = h->pipe->DetectLoops(vecs, P, &ds);
        if (!ok) { g_err = h->pipe->last_error(); if (ds.empty()) return -1; }
        for (size_t s = 0; s < ds.size(); ++s) {
            const Pipe::LoopDetection &D = ds[s];
            svs_loop_detection &o = results[s];
            std::memset(&o, 0, sizeof(o));
            o.is_keyframe = D.is_keyframe; o.skipped = D.skipped; o.searched = D.searched; o.verified = D.verified; o.stored = D.stored;
            o.kf_id = D.kf_id;
            o.cand_status = D.searched ? D.cand.status : -1; o.cand_kf = D.searched ? D.cand.cand_kf : -1; o.best_kf = D.searched ? D.cand.best_kf : -1;
            o.n_weak = D.cand.n_weak; o.n_compared = D.cand.n_compared; o.best_sim = D.cand.best_sim;
            const Pipe::LoopResult &R = D.loop;
            o.loop.status = D.verified ? R.status : -1; o.loop.n_matches = R.n_matches; o.loop.n_points = R.n_points; o.loop.n_inliers = R.n_inliers;
            o.loop.need_correction = R.need_correction ? 1 : 0;
            std::memcpy(o.loop.T_corr, R.T_corr.v, 56); std::memcpy(o.loop.T_rel, R.T_rel.v, 56); o.loop.d = R.d;
            if (fusion_or_null) put_stats(fusion_or_null[s], D.fused, D.fusion);
        }
        return ok ? 0 : -1;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
// Global image descriptor (product build only: the CPU twins' providers have no gdesc_describe)
extern "C" int svs_pipe_gdesc_configure(void *p, int nlayers, const void *layers, const float *params, long long nparams, const void *prep_or_null)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    try {
        if (!h->pipe->ConfigureGlobalDescriptor(nlayers, static_cast<const svslam_gd_layer *>(layers), params, nparams,
                                                static_cast<const svslam_gd_prep *>(prep_or_null))) { g_err = h->pipe->last_error(); return -1; }
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" int svs_pipe_gdesc_dim(void *p) { return static_cast<PipeHandle *>(p)->pipe->GlobalDescriptorDim(); }
extern "C" int svs_pipe_describe_global_new_keyframes(void *p, float *vecs)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (!vecs) { g_err = "svs_pipe_describe_global_new_keyframes: null argument"; return -1; }
    try {
        std::vector<float> v;
        int n = 0;
        if (!h->pipe->DescribeGlobalNewKeyframes(&v, &n)) { g_err = h->pipe->last_error(); return -1; }
        if (!v.empty()) std::memcpy(vecs, v.data(), sizeof(float) * v.size());
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" long long svs_pipe_loop_matches(void *p, int stream, int *match4, long long cap)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    const auto &ds = h->pipe->LastDetections();
    if (stream < 0 || (size_t)stream >= ds.size() || !ds[(size_t)stream].verified) { g_err = "svs_pipe_loop_matches: the last svs_pipe_detect_loops verified nothing on this stream"; return -1; }
    const auto &R = ds[(size_t)stream].loop;
    const long long n = R.n_matches;
    if (match4 && cap >= n)
        for (long long k = 0; k < n; ++k) { match4[4 * k] = R.match_c[(size_t)k]; match4[4 * k + 1] = R.match_q[(size_t)k]; match4[4 * k + 2] = R.match_dist[(size_t)k]; match4[4 * k + 3] = R.match_inlier[(size_t)k]; }
    return n;
}
extern "C" long long svs_pipe_loopdb_ids(void *p, int stream, int *ids, long long cap)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    int n = 0;
    if (h->kernels->loopdb_count(stream, &n) != 0) { g_err = h->kernels->last_error(); return -1; }
    if (ids && cap >= n && n) {
        std::vector<float> rows((size_t)n * 4096);
        if (h->kernels->loopdb_read(stream, n, ids, rows.data()) != 0) { g_err = h->kernels->last_error(); return -1; }
    }
    return n;
}
extern "C" long long svs_pipe_last_closed_keyframe(void *p, int stream) { return static_cast<PipeHandle *>(p)->pipe->LastClosedKeyframe(stream); }
extern "C" void *svs_pipe_backend_ctx(void *p) { return static_cast<PipeHandle *>(p)->kernels->backend_ctx(); }
// LocalFusion (product build only: the CPU twins' providers have no local_fusion)
extern "C" int svs_pipe_local_fusion(void *p, int njobs, const svs_fusion_job *jobs, const int *pairs2, svs_fusion_stats *stats_or_null)
{
    typedef svs::Pipeline<SVS_PIPE_KERNELS> Pipe;
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (njobs < 0 || (njobs > 0 && !jobs)) { g_err = "svs_pipe_local_fusion: null argument"; return -1; }
    try {
        std::vector<Pipe::FusionJob> js((size_t)njobs);
        for (int i = 0; i < njobs; ++i) {
            const svs_fusion_job &j = jobs[i];
            if (j.npairs < 0 || j.pair_ofs < 0 || (j.npairs > 0 && !pairs2)) { g_err = "svs_pipe_local_fusion: a job's pairs are null or negative"; return -1; }
            js[(size_t)i].stream = j.stream; js[(size_t)i].kf_id = (long)j.kf_id; js[(size_t)i].cand_kf_id = (long)j.cand_kf_id; js[(size_t)i].T_corr = svs::SE3(j.T_corr);
            for (int k = 0; k < j.npairs; ++k) js[(size_t)i].pairs.emplace_back(pairs2[2 * (j.pair_ofs + k)], pairs2[2 * (j.pair_ofs + k) + 1]);
        }
        std::vector<Pipe::FusionStats> st;
        if (!h->pipe->LocalFusion(js, &st)) { g_err = h->pipe->last_error(); return -1; }
        if (stats_or_null) for (size_t i = 0; i < st.size(); ++i) put_stats(stats_or_null[i], true, st[i]);
        return 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" long long svs_pipe_all_landmarks(void *p, int stream, double *out7, long long cap)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (stream < 0 || stream >= h->pipe->nstreams()) { g_err = "svs_pipe_all_landmarks: no such stream"; return -1; }
    try {
        h->pipe->Flush();
        const std::vector<svs::LandmarkRecord> all = h->pipe->AllLandmarks(stream);
        const long long n = (long long)all.size();
        if (out7 && cap >= n)
            for (long long i = 0; i < n; ++i) {
                const svs::LandmarkRecord &r = all[(size_t)i];
                double *o = out7 + 7 * i;
                o[0] = (double)r.id; o[1] = r.pos[0]; o[2] = r.pos[1]; o[3] = r.pos[2]; o[4] = r.observed_times; o[5] = r.active ? 1.0 : 0.0; o[6] = (double)r.anchor_kf;
            }
        return n;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -1;
    }
}
extern "C" long long svs_pipe_last_frame(void *p, int stream, double *pose7)
{
    PipeHandle *h = static_cast<PipeHandle *>(p);
    if (stream < 0 || stream >= h->pipe->nstreams() || !h->pipe->stream(stream).last) { g_err = "svs_pipe_last_frame: no such stream, or it has seen no frame"; return -2; }
    const svs::Frame *f = h->pipe->stream(stream).last;
    if (pose7) std::memcpy(pose7, f->pose.v, 56);
    return f->is_keyframe ? (long long)f->keyframe_id : -1;
}
