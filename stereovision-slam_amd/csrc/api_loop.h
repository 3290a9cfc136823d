// api_loop.h — included by svslam_hip.hip.  Entry points: svslam_pose_graph_batch, svslam_loop_verify_batch, svslam_local_fusion_batch,
// svslam_brief_*, svslam_loopdb_*, svslam_loop_candidates_batch, svslam_gdesc_*.  Owns of svslam_ctx: pg, lv, lf, br, lc, gd.

extern "C" {

// ------------------------------------------------------------------ global pose-graph optimisation
int svslam_pose_graph_batch(svslam_ctx *c, int njobs, svslam_pg_job *jobs, int total_kf, double *poses, const uint8_t *fixed,
                            int total_edges, const int *edge_a, const int *edge_b, const double *edge_meas,
                            int total_pts, const int *pt_anchor, double *pts, int iters)
{
    if (!c) return -1;
    if (njobs < 0 || total_kf < 0 || total_edges < 0 || total_pts < 0) return fail(c, "pose_graph: negative count");
    if (iters < 0) return fail(c, "pose_graph: iters %d < 0", iters);
    if (njobs == 0) return 0;
    if (!jobs) return fail(c, "pose_graph: null jobs");
    if ((total_kf && (!poses || !fixed)) || (total_edges && (!edge_a || !edge_b || !edge_meas)) || (total_pts && (!pt_anchor || !pts)))
        return fail(c, "pose_graph: null array");
    if (arena_busy(c)) return -1;
    std::vector<PgIn> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) {
        const svslam_pg_job &s = jobs[j];
        in[(size_t)j] = PgIn{ s.kf_ofs, s.nkf, s.edge_ofs, s.nedge, s.pt_ofs, s.npt };
    }
    for (int e = 0; e < total_edges; ++e) {
        const double *q = edge_meas + 7 * (size_t)e;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(fabs(n2 - 1.0) <= 2e-6)) return fail(c, "pose_graph: the quaternion of measurement %d is not of unit length (1e-6)", e);
    }
    static_assert(LM_TRACE_REC == 6 && LM_TRACE_CAP == 408 && LM_TRACE_STRIDE == 8 + 6 * 408,
                  "k_pose_graph.h (host emulation) and tests/pose_graph_cases.py restate the trace layout of dev_common.h");
    PgPlan &P = c->pg.plan;
    const char *why = pg_plan(njobs, in.data(), total_kf, poses, fixed, total_edges, edge_a, edge_b, total_pts, pt_anchor, iters,
                              c->d_lm_trace ? c->lim.max_jobs : 0, P);
    if (why) return fail(c, "pose_graph: %s", why);
    (void)pg_layout(P, njobs, total_kf, total_edges, total_pts, nullptr);         // sizes
    if (c->pg.reserve(c, "pose_graph", P.bytes, P.bytes / 4, P.front_bytes)) return -1;
    const PgBuf Hb = pg_layout(P, njobs, total_kf, total_edges, total_pts, c->pg.h.data());
    const PgBuf Db = pg_layout(P, njobs, total_kf, total_edges, total_pts, c->pg.d);
    pg_fill_front(P, Hb, njobs, total_kf, poses, total_edges, edge_a, edge_b, edge_meas, total_pts, pt_anchor, pts);
    HIPCHK(c, hipMemcpyAsync(c->pg.d, c->pg.h.data(), P.front_bytes, hipMemcpyHostToDevice, c->stream));
    if (c->d_lm_trace) HIPCHK(c, hipMemsetAsync(c->d_lm_trace, 0, sizeof(double) * LM_TRACE_STRIDE * (size_t)std::min(njobs, c->lim.max_jobs), c->stream));
    tm_begin(c, FAM_PG, njobs);
    hipLaunchKernelGGL(k_pose_graph, dim3(njobs), dim3(PG_THREADS), 0, c->stream, Db, c->d_lm_trace);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->pg.h.data(), c->pg.d, P.result_bytes, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    for (int j = 0; j < njobs; ++j) {
        const PgJob &J = Hb.jobs[j];
        jobs[j].iters_done = J.iters_done; jobs[j].n_trials = J.n_trials; jobs[j].chi2_before = J.chi2_before; jobs[j].chi2_after = J.chi2_after;
    }
    if (total_kf) memcpy(poses, Hb.poses, 56 * (size_t)total_kf);
    if (total_pts) memcpy(pts, Hb.pts, 24 * (size_t)total_pts);
    return 0;
}

// ------------------------------------------------------------------ loop verification
int svslam_loop_verify_batch(svslam_ctx *c, int njobs, svslam_loop_job *jobs, const svslam_loop_params *prm, int total_c, const uint8_t *desc_c,
                             const double *xyz_c, const uint8_t *has_xyz, int total_q, const uint8_t *desc_q, const float *uv_q,
                             int *match_c, int *match_q, int *match_dist, uint8_t *match_inlier)
{
    if (!c) return -1;
    if (njobs < 0 || total_c < 0 || total_q < 0) return fail(c, "loop_verify: negative count");
    if (!prm) return fail(c, "loop_verify: null params");
    if (njobs == 0) return 0;
    if (!jobs) return fail(c, "loop_verify: null jobs");
    if ((total_c && (!desc_c || !xyz_c || !has_xyz || !match_c || !match_q || !match_dist || !match_inlier)) || (total_q && (!desc_q || !uv_q)))
        return fail(c, "loop_verify: null array");
    if (arena_busy(c)) return -1;
    std::vector<LvIn> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = LvIn{ jobs[j].c_ofs, jobs[j].nc, jobs[j].q_ofs, jobs[j].nq, jobs[j].T_cur, jobs[j].T_cand };
    const char *why = lv_check(njobs, in.data(), total_c, total_q, prm->ext_l, prm->ransac_iters, prm->min_matches, prm->reproj_px);
    if (why) return fail(c, "loop_verify: %s", why);
    LvParams P;
    memset(&P, 0, sizeof(P));
    memcpy(P.cam, prm->cam, sizeof(P.cam)); memcpy(P.ext_l, prm->ext_l, sizeof(P.ext_l));
    P.reproj2 = prm->reproj_px * prm->reproj_px; P.max_pose_distance = prm->max_pose_distance;
    P.min_pose_difference = prm->min_pose_difference; P.max_pose_difference = prm->max_pose_difference;
    P.min_matches = prm->min_matches; P.ransac_iters = prm->ransac_iters; P.seed = prm->seed;
    LvSizes Z;
    (void)lv_layout(Z, njobs, total_c, total_q, nullptr);                       // sizes
    if (c->lv.reserve(c, "loop_verify", Z.bytes, Z.bytes / 4, Z.bytes)) return -1;
    const LvBuf Hb = lv_layout(Z, njobs, total_c, total_q, c->lv.h.data());
    const LvBuf Db = lv_layout(Z, njobs, total_c, total_q, c->lv.d);
    lv_fill(Z, Hb, njobs, in.data(), total_c, desc_c, xyz_c, has_xyz, total_q, desc_q, uv_q);
    HIPCHK(c, hipMemcpyAsync(c->lv.d, c->lv.h.data(), Z.bytes, hipMemcpyHostToDevice, c->stream));
    tm_begin(c, FAM_LV, njobs);
    hipLaunchKernelGGL(k_loop_verify, dim3(njobs), dim3(LV_THREADS), 0, c->stream, Db, P);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->lv.h.data(), c->lv.d, Z.result_bytes, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    for (int j = 0; j < njobs; ++j) {
        const LvJob &J = Hb.jobs[j];
        jobs[j].status = J.status; jobs[j].n_matches = J.n_matches; jobs[j].n_points = J.n_points; jobs[j].n_inliers = J.n_inliers;
        jobs[j].need_correction = J.need_correction;
        memcpy(jobs[j].T_corr, J.T_corr, 56); memcpy(jobs[j].T_rel, J.T_rel, 56); jobs[j].d = J.d;
    }
    if (total_c) {
        memcpy(match_c, Hb.m_c, 4 * (size_t)total_c); memcpy(match_q, Hb.m_q, 4 * (size_t)total_c); memcpy(match_dist, Hb.m_d, 4 * (size_t)total_c);
        memcpy(match_inlier, Hb.m_inl, (size_t)total_c);
    }
    return 0;
}

// ------------------------------------------------------------------ local fusion after a closed loop
int svslam_local_fusion_batch(svslam_ctx *c, int njobs, svslam_lf_job *jobs, int total_kf, double *poses, int total_pts, double *pts,
                              const int *obs_ptr, int total_obs, const int *obs_kf, int *pt_kf)
{
    if (!c) return -1;
    std::vector<LfIn> in((size_t)(njobs > 0 && jobs ? njobs : 0));
    for (size_t j = 0; j < in.size(); ++j) {
        svslam_lf_job &s = jobs[j];
        in[j] = LfIn{ s.kf_ofs, s.nkf, s.pt_ofs, s.npt, s.cur, s.last, s.T_cur, s.T_corr, s.T_last };
    }
    const char *why = lf_plan(njobs, jobs ? in.data() : nullptr, total_kf, poses, total_pts, pts, obs_ptr, total_obs, obs_kf, pt_kf);
    if (why) return fail(c, "local_fusion: %s", why);
    if (njobs == 0) return 0;
    if (arena_busy(c)) return -1;
    LfSizes Z;
    (void)lf_layout(Z, njobs, total_kf, total_pts, total_obs, nullptr);          // sizes
    if (c->lf.reserve(c, "local_fusion", Z.bytes, Z.bytes / 4, Z.bytes)) return -1;
    const LfBuf Hb = lf_layout(Z, njobs, total_kf, total_pts, total_obs, c->lf.h.data());
    const LfBuf Db = lf_layout(Z, njobs, total_kf, total_pts, total_obs, c->lf.d);
    lf_fill(Z, Hb, njobs, in.data(), total_kf, poses, total_pts, pts, obs_ptr, total_obs, obs_kf);
    HIPCHK(c, hipMemcpyAsync(c->lf.d, c->lf.h.data(), Z.bytes, hipMemcpyHostToDevice, c->stream));
    tm_begin(c, FAM_LF, njobs);
    hipLaunchKernelGGL(k_local_fusion, dim3(njobs), dim3(LF_THREADS), 0, c->stream, Db);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->lf.h.data(), c->lf.d, Z.result_bytes, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    for (int j = 0; j < njobs; ++j) lf_copy_out(Hb, j, poses, pts, pt_kf, jobs[j].T_last, &jobs[j].n_unanchored);
    return 0;
}

// ------------------------------------------------------------------ BRIEF descriptors
int svslam_brief_default_pattern(int8_t *out)
{
    if (!out) return -1;
    memcpy(out, BR_DEFAULT_PATTERN, sizeof(BR_DEFAULT_PATTERN));
    return 0;
}

int svslam_brief_describe_batch(svslam_ctx *c, int njobs, svslam_brief_job *jobs, const svslam_brief_params *prm, int total_pts,
                                const float *xy, uint8_t *desc, int *desc_pt)
{
    if (!c) return -1;
    if (njobs < 0 || total_pts < 0) return fail(c, "brief: negative count");
    if (!prm) return fail(c, "brief: null params");
    if (njobs && !jobs) return fail(c, "brief: null jobs");
    if (total_pts && (!xy || !desc || !desc_pt)) return fail(c, "brief: null array");
    if (arena_busy(c)) return -1;
    std::vector<BrJob> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = BrJob{ jobs[j].slot, jobs[j].pt_ofs, jobs[j].npts, 0 };
    int off[1024], reach = 0;
    const char *why = br_check(njobs, in.data(), total_pts, c->lim.max_slots, prm->pattern ? prm->pattern : BR_DEFAULT_PATTERN,
                               prm->angle_deg, prm->edge, off, &reach);
    if (why) return fail(c, "brief: %s", why);
    if (njobs == 0) return 0;
    const BrPlan L = br_plan(reach);
    BrSizes Z;
    (void)br_layout(Z, njobs, total_pts, nullptr);                              // sizes
    if (c->br.reserve(c, "brief", Z.bytes, Z.bytes / 4, Z.bytes)) return -1;
    const BrBuf Hb = br_layout(Z, njobs, total_pts, c->br.h.data());
    const BrBuf Db = br_layout(Z, njobs, total_pts, c->br.d);
    br_fill(Hb, L, njobs, in.data(), total_pts, xy, off);
    const BrImg I = level0_view<BrImg>(c);
    HIPCHK(c, hipMemcpyAsync(c->br.d, c->br.h.data(), Z.upload_bytes, hipMemcpyHostToDevice, c->stream));
    tm_begin(c, FAM_BRIEF, total_pts);
    hipLaunchKernelGGL(k_brief_filter, dim3(njobs), dim3(BR_THREADS), 0, c->stream, Db, I, prm->edge, L.R);
    if (total_pts)
        hipLaunchKernelGGL(k_brief_describe, dim3((total_pts + BR_ROWS_PER_WG - 1) / BR_ROWS_PER_WG), dim3(BR_THREADS),
                           (size_t)L.wave_bytes * BR_ROWS_PER_WG, c->stream, Db, I, L, total_pts);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->br.h.data() + Z.result_ofs, c->br.d + Z.result_ofs, Z.bytes - Z.result_ofs, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    br_copy_out(Hb, njobs, in.data(), desc, desc_pt);
    for (int j = 0; j < njobs; ++j) jobs[j].n_desc = in[(size_t)j].n_desc;
    return 0;
}


// ------------------------------------------------------------------ loop candidates: resident store and search
namespace {
// a call's staging: a struct array of head bytes, then n vectors of dim floats; grown on demand and kept
int lc_stage(svslam_ctx *c, size_t bytes, const char *what) { return c->lc.reserve(c, what, bytes, bytes / 4, bytes); }
inline size_t lc_head(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
}

int svslam_loopdb_configure(svslam_ctx *c, int nstreams, int capacity, int dim)
{
    if (!c) return -1;
    const char *why = lc_check_configure(nstreams, capacity, dim);
    if (why) return fail(c, "loopdb_configure: %s", why);
    if (arena_busy(c)) return -1;
    const size_t nrows = (size_t)nstreams * (size_t)capacity, dp = (size_t)lc_padded(dim);
    if (nrows > ((size_t)1 << 31) - 1 || nrows * dp > ((size_t)1 << 40) / sizeof(float)) return fail(c, "loopdb_configure: the store would pass 2^31 rows or 1 TiB");
    float *rows = nullptr; int *ids = nullptr;
    if (hipMalloc(&rows, nrows * dp * sizeof(float)) != hipSuccess || hipMalloc(&ids, nrows * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(rows);
        return fail(c, "loopdb_configure: no device memory for %zu rows of %zu floats (the store is as it was)", nrows, dp);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->lc.S.rows); (void)hipFree(c->lc.S.ids);
    c->lc.S = LcStore{ rows, ids, nstreams, capacity, dim, (int)dp };
    lc_host_configure(c->lc.H, nstreams, capacity, dim);
    return 0;
}

int svslam_loopdb_append_batch(svslam_ctx *c, int n, const int *streams, const int *kf_ids, const float *vecs)
{
    if (!c) return -1;
    if (n < 0) return fail(c, "loopdb_append: negative count");
    if (n && (!streams || !kf_ids || !vecs)) return fail(c, "loopdb_append: null array");
    if (arena_busy(c)) return -1;
    std::vector<LcApp> apps((size_t)n);
    const char *why = lc_check_append(c->lc.H, n, streams, kf_ids, apps.data());
    if (why) return fail(c, "loopdb_append: %s", why);
    if (n == 0) return 0;
    const size_t head = lc_head(sizeof(LcApp) * (size_t)n), vbytes = sizeof(float) * (size_t)n * c->lc.S.dim;
    if (lc_stage(c, head + vbytes, "loopdb_append")) return -1;
    memcpy(c->lc.h.data(), apps.data(), sizeof(LcApp) * (size_t)n);
    memcpy(c->lc.h.data() + head, vecs, vbytes);
    LcApp *d_apps = reinterpret_cast<LcApp *>(c->lc.d);
    const float *d_vecs = reinterpret_cast<const float *>(c->lc.d + head);
    HIPCHK(c, hipMemcpyAsync(c->lc.d, c->lc.h.data(), head + vbytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_lc_append, dim3(n), dim3(64), 0, c->stream, c->lc.S, d_apps, d_vecs, 0);        // which vectors can be normalised
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->lc.h.data(), c->lc.d, sizeof(LcApp) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const LcApp *back = reinterpret_cast<const LcApp *>(c->lc.h.data());
    for (int i = 0; i < n; ++i)
        if (back[i].status) return fail(c, "loopdb_append: a vector cannot be normalised (BAD_VECTOR): row %d", i);
    hipLaunchKernelGGL(k_lc_append, dim3(n), dim3(64), 0, c->stream, c->lc.S, d_apps, d_vecs, 1);        // all can: write the rows
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lc_host_appended(c->lc.H, n, apps.data());
    return 0;
}

int svslam_loop_candidates_batch(svslam_ctx *c, int njobs, svslam_lc_job *jobs, const svslam_lc_params *prm, const float *vecs)
{
    if (!c) return -1;
    if (njobs < 0) return fail(c, "loop_candidates: negative count");
    if (!prm) return fail(c, "loop_candidates: null params");
    if (njobs && (!jobs || !vecs)) return fail(c, "loop_candidates: null array");
    if (arena_busy(c)) return -1;
    const LcParams P = { prm->weak, prm->strong, prm->max_num_weak, prm->min_gap };
    std::vector<int> streams((size_t)njobs), kfs((size_t)njobs);
    for (int j = 0; j < njobs; ++j) { streams[(size_t)j] = jobs[j].stream; kfs[(size_t)j] = jobs[j].kf_id; }
    std::vector<LcJob> J((size_t)njobs);
    const char *why = lc_check_jobs(c->lc.H, njobs, streams.data(), kfs.data(), P, J.data());
    if (why) return fail(c, "loop_candidates: %s", why);
    if (njobs == 0) return 0;
    const size_t head = lc_head(sizeof(LcJob) * (size_t)njobs), vbytes = sizeof(float) * (size_t)njobs * c->lc.S.dim;
    if (lc_stage(c, head + vbytes, "loop_candidates")) return -1;
    memcpy(c->lc.h.data(), J.data(), sizeof(LcJob) * (size_t)njobs);
    memcpy(c->lc.h.data() + head, vecs, vbytes);
    HIPCHK(c, hipMemcpyAsync(c->lc.d, c->lc.h.data(), head + vbytes, hipMemcpyHostToDevice, c->stream));
    tm_begin(c, FAM_LC, 0);                                     // the units are known once the jobs are back
    hipLaunchKernelGGL(k_lc_candidates, dim3(njobs), dim3(LC_THREADS), 0, c->stream, c->lc.S, P, reinterpret_cast<LcJob *>(c->lc.d),
                       reinterpret_cast<const float *>(c->lc.d + head));
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->lc.h.data(), c->lc.d, sizeof(LcJob) * (size_t)njobs, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    const LcJob *R = reinterpret_cast<const LcJob *>(c->lc.h.data());
    long long compared = 0;
    for (int j = 0; j < njobs; ++j) {
        jobs[j].status = R[j].status; jobs[j].cand_kf = R[j].cand_kf; jobs[j].best_kf = R[j].best_kf; jobs[j].n_weak = R[j].n_weak;
        jobs[j].n_compared = R[j].n_compared; jobs[j].best_sim = R[j].best_sim;
        compared += R[j].n_compared;
    }
    if (c->timing) c->tm.units[FAM_LC] += compared;
    return 0;
}

int svslam_loopdb_count(svslam_ctx *c, int stream, int *count)
{
    if (!c) return -1;
    if (!count) return fail(c, "loopdb_count: null output");
    if (c->lc.H.nstreams == 0) return fail(c, "loopdb_count: the store is not configured");
    if (stream < 0 || stream >= c->lc.H.nstreams) return fail(c, "loopdb_count: unknown stream");
    *count = c->lc.H.count[(size_t)stream];
    return 0;
}

int svslam_loopdb_read(svslam_ctx *c, int stream, int max_rows, int *kf_ids, float *vecs)
{
    if (!c) return -1;
    if (c->lc.H.nstreams == 0) return fail(c, "loopdb_read: the store is not configured");
    if (stream < 0 || stream >= c->lc.H.nstreams) return fail(c, "loopdb_read: unknown stream");
    if (max_rows < 0) return fail(c, "loopdb_read: negative count");
    const int n = c->lc.H.count[(size_t)stream] < max_rows ? c->lc.H.count[(size_t)stream] : max_rows;
    if (n == 0) return 0;
    if (!kf_ids || !vecs) return fail(c, "loopdb_read: null array");
    const LcStore &S = c->lc.S;
    std::vector<float> rows;
    try { rows.resize((size_t)n * S.dp); }
    catch (const std::bad_alloc &) { return fail(c, "loopdb_read: no host memory"); }
    const size_t at = (size_t)stream * S.capacity;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(rows.data(), S.rows + at * S.dp, sizeof(float) * (size_t)n * S.dp, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(kf_ids, S.ids + at, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    for (int r = 0; r < n; ++r) lc_unpermute(rows.data() + (size_t)r * S.dp, S.dim, S.dp, vecs + (size_t)r * S.dim);
    return 0;
}

// ------------------------------------------------------------------ global image descriptor
int svslam_gdesc_mobilenet_v2(svslam_gd_layer *out, int cap)
{
    static_assert(sizeof(svslam_gd_layer) == sizeof(GdLayer), "svslam_gd_layer is GdLayer");
    if (cap < 0 || (cap && !out)) return -1;
    return gd_mobilenet_v2(reinterpret_cast<GdLayer *>(out), cap);
}

int svslam_gdesc_dim(svslam_ctx *c) { return c ? c->gd.N.dim : 0; }

int svslam_gdesc_configure(svslam_ctx *c, int nlayers, const svslam_gd_layer *layers, const float *params, long long nparams,
                           const svslam_gd_prep *prep)
{
    if (!c) return -1;
    static_assert(sizeof(svslam_gd_prep) == sizeof(GdPrep), "svslam_gd_prep is GdPrep");
    if (arena_busy(c)) return -1;
    GdNet M;
    const char *why = nullptr;
    try { why = gd_configure(M, c->geom.w[0], c->geom.h[0], nlayers, reinterpret_cast<const GdLayer *>(layers), params, nparams,
                             reinterpret_cast<const GdPrep *>(prep)); }
    catch (const std::bad_alloc &) { return fail(c, "gdesc_configure: no host memory"); }
    if (why) return fail(c, "gdesc_configure: %s", why);
    float *d_prm = nullptr; int *d_tab = nullptr;
    const size_t pb = sizeof(float) * std::max(M.packed.size(), (size_t)32), tb = sizeof(int) * M.tab.size();
    if (hipMalloc(&d_prm, pb) != hipSuccess || hipMalloc(&d_tab, tb) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d_prm);
        return fail(c, "gdesc_configure: no device memory for %zu bytes of parameters (the old network is kept)", pb + tb);
    }
    if ((M.packed.size() && hipMemcpy(d_prm, M.packed.data(), sizeof(float) * M.packed.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(d_tab, M.tab.data(), tb, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d_prm); (void)hipFree(d_tab);
        return fail(c, "gdesc_configure: the upload of the parameters failed (the old network is kept)");
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->gd.d_prm); (void)hipFree(c->gd.d_tab); c->gd.ws.release();
    c->gd.d_prm = d_prm; c->gd.d_tab = d_tab;
    c->gd.N = std::move(M);
    return 0;
}

int svslam_gdesc_describe_batch(svslam_ctx *c, int njobs, const int *slots, float *vecs)
{
    if (!c) return -1;
    if (njobs < 0) return fail(c, "gdesc_describe: negative count");
    if (njobs && (!slots || !vecs)) return fail(c, "gdesc_describe: null array");
    if (arena_busy(c)) return -1;
    const GdNet &N = c->gd.N;
    const char *why = gd_check_describe(N, njobs, slots, c->lim.max_slots);
    if (why) return fail(c, "gdesc_describe: %s", why);
    if (njobs == 0) return 0;
    static const bool valu = []{ const char *e = std::getenv("SVSLAM_GD_VALU"); return e && atoi(e) != 0; }();   // A/B: PW on the VALU
    const int chunk = gd_chunk(N, njobs);
    const size_t ws_bytes = sizeof(float) * (size_t)chunk * (size_t)N.job_floats;
    if (c->gd.ws.reserve(c, "gdesc_describe", ws_bytes, 0)) return -1;
    const size_t sb = (sizeof(int) * (size_t)njobs + 255) & ~(size_t)255, vb = sizeof(float) * (size_t)njobs * N.dim;
    if (c->gd.io.reserve(c, "gdesc_describe", sb + vb, (sb + vb) / 4, vb)) return -1;
    float *const d_ws = reinterpret_cast<float *>(c->gd.ws.d);
    int *d_slots = reinterpret_cast<int *>(c->gd.io.d);
    float *d_vecs = reinterpret_cast<float *>(c->gd.io.d + sb);
    HIPCHK(c, hipMemcpyAsync(d_slots, slots, sizeof(int) * (size_t)njobs, hipMemcpyHostToDevice, c->stream));
    GdPrepArgs PA;
    PA.I = level0_view<GdImg>(c);
    PA.tab = c->gd.d_tab; PA.ws = d_ws; PA.u8 = nullptr; PA.job_floats = N.job_floats; PA.out_w = N.prep.out_w; PA.out_h = N.prep.out_h;
    for (int k = 0; k < 3; ++k) PA.mean[k] = N.prep.mean[k];
    PA.scale = N.prep.scale;
    tm_begin(c, FAM_GD, njobs);
    for (int j0 = 0; j0 < njobs; j0 += chunk) {
        const int nj = std::min(chunk, njobs - j0);
        PA.slots = d_slots + j0; PA.njobs = nj;
        hipLaunchKernelGGL(k_gd_prep, dim3(cdiv(PA.out_w * PA.out_h, GD_THREADS), nj), dim3(GD_THREADS), 0, c->stream, PA);
        for (const GdL &L : N.L) {
            GdArgs A;
            A.L = L; A.prm = c->gd.d_prm; A.ws = d_ws; A.vecs = d_vecs + (size_t)j0 * N.dim; A.job_floats = N.job_floats; A.njobs = nj;
            const long long hw = (long long)L.hout * L.wout, elems = hw * L.cout;
            if (L.op == GD_CONV3)
                hipLaunchKernelGGL(k_gd_conv3, dim3((unsigned)((hw + GD_THREADS - 1) / GD_THREADS), L.cout, nj), dim3(GD_THREADS), 0, c->stream, A);
            else if (L.op == GD_DW3)
                hipLaunchKernelGGL(k_gd_dw3, dim3((unsigned)((elems + GD_THREADS - 1) / GD_THREADS), nj), dim3(GD_THREADS), 0, c->stream, A);
            else if (L.op == GD_PW && valu)
                hipLaunchKernelGGL(k_gd_pw, dim3((unsigned)((elems + GD_THREADS - 1) / GD_THREADS), nj), dim3(GD_THREADS), 0, c->stream, A);
            else if (L.op == GD_PW) {
                const long long ptiles = (hw * nj + 31) / 32;
                const int NT = gd_pw_tiles(hw, nj, L.coutp);
                const dim3 grid((unsigned)((ptiles + 3) / 4), cdiv(L.coutp / 32, NT));
                if (NT == 4) hipLaunchKernelGGL(k_gd_pw_mfma<4>, grid, dim3(GD_THREADS), 0, c->stream, A);
                else if (NT == 2) hipLaunchKernelGGL(k_gd_pw_mfma<2>, grid, dim3(GD_THREADS), 0, c->stream, A);
                else hipLaunchKernelGGL(k_gd_pw_mfma<1>, grid, dim3(GD_THREADS), 0, c->stream, A);
            }
            else
                hipLaunchKernelGGL(k_gd_pool, dim3(cdiv(L.cout, GD_THREADS), nj), dim3(GD_THREADS), 0, c->stream, A);
        }
    }
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->gd.io.h.data(), d_vecs, vb, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    memcpy(vecs, c->gd.io.h.data(), vb);
    return 0;
}

} // extern "C"
