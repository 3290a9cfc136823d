// api_dense.h — included by svslam_hip.hip.  Entry points: svslam_stereo_bm_*, svslam_dense_cloud_batch, svslam_cloud_sor_batch,
// svslam_cloud_voxel_grid, svslam_debug_cloud_sor_climbs, svslam_colour_reserve, svslam_pyramid_bgr_batch, svslam_colour_read,
// svslam_dense_cloud_bgr_batch.  Owns of svslam_ctx: bm, cf, col.

extern "C" {

// ------------------------------------------------------------------ dense stereo (run_dense_reconstruction)
static int bm_check_params(svslam_ctx *c, const svslam_bm_params *p, BmParams &P)
{
    if (!p) return fail(c, "stereo_bm: null parameters");
    if (p->num_disparities <= 0 || (p->num_disparities & 15) || p->num_disparities > 256)
        return fail(c, "stereo_bm: num_disparities %d must be a positive multiple of 16, <= 256", p->num_disparities);
    if (!(p->block_size & 1) || p->block_size < 5 || p->block_size > 21) return fail(c, "stereo_bm: block_size %d must be odd and in [5, 21]", p->block_size);
    if (p->pre_filter_cap < 1 || p->pre_filter_cap > 63) return fail(c, "stereo_bm: pre_filter_cap %d out of [1, 63]", p->pre_filter_cap);
    if (p->texture_threshold < 0 || p->uniqueness_ratio < 0) return fail(c, "stereo_bm: texture_threshold %d / uniqueness_ratio %d must not be negative", p->texture_threshold, p->uniqueness_ratio);
    // (uniqueness_ratio stays an int product: minsad <= 21 * 21 * 126)
    if (p->uniqueness_ratio > 10000) return fail(c, "stereo_bm: uniqueness_ratio %d > 10000", p->uniqueness_ratio);
    P.nd = p->num_disparities; P.bs = p->block_size; P.cap = p->pre_filter_cap; P.tex_thr = p->texture_threshold; P.uniq = p->uniqueness_ratio;
    return 0;
}

int svslam_stereo_bm_strip_rows(svslam_ctx *c, int njobs, const svslam_bm_params *p)
{
    if (!c) return -1;
    BmParams P;
    if (bm_check_params(c, p, P)) return -1;
    if (njobs <= 0 || njobs > c->lim.max_jobs) return fail(c, "stereo_bm: %d jobs out of [1, max_jobs]", njobs);
    return bm_plan(c->geom.w[0], c->geom.h[0], njobs, P).th;
}

// enqueue the matcher for njobs jobs (device array djobs) into c->bm.disp; no-op arithmetic when OpenCV's early-out applies
static int launch_stereo_bm(svslam_ctx *c, int njobs, const BmJob *djobs, const BmParams &P)
{
    const int w = c->geom.w[0], h = c->geom.h[0];
    if (c->bm.disp.reserve(c, "stereo_bm", sizeof(int16_t) * (size_t)w * h * c->lim.max_jobs, 0)) return -1;
    int16_t *disp = (int16_t *)c->bm.disp.d;
    const BmPlan pl = bm_plan(w, h, njobs, P);
    const size_t n = (size_t)w * h * njobs;
    hipLaunchKernelGGL(k_bm_fill, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->stream, disp, w, h, njobs, pl.x0, pl.x1, pl.y0, pl.y1);
    if (pl.th) {
        const dim3 grid(pl.tiles, pl.strips, njobs);
        switch ((P.bs + 3) / 4) {
        case 2: hipLaunchKernelGGL(k_stereo_bm<2>, grid, dim3(BM_THREADS), pl.lds, c->stream, djobs, c->d_pyr, c->geom, P, pl.th, disp); break;
        case 3: hipLaunchKernelGGL(k_stereo_bm<3>, grid, dim3(BM_THREADS), pl.lds, c->stream, djobs, c->d_pyr, c->geom, P, pl.th, disp); break;
        case 4: hipLaunchKernelGGL(k_stereo_bm<4>, grid, dim3(BM_THREADS), pl.lds, c->stream, djobs, c->d_pyr, c->geom, P, pl.th, disp); break;
        case 5: hipLaunchKernelGGL(k_stereo_bm<5>, grid, dim3(BM_THREADS), pl.lds, c->stream, djobs, c->d_pyr, c->geom, P, pl.th, disp); break;
        default: hipLaunchKernelGGL(k_stereo_bm<6>, grid, dim3(BM_THREADS), pl.lds, c->stream, djobs, c->d_pyr, c->geom, P, pl.th, disp); break;
        }
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int svslam_stereo_bm_batch(svslam_ctx *c, int njobs, const svslam_bm_job *jobs, const svslam_bm_params *p, int16_t *out_disp)
{
    if (!c) return -1;
    BmParams P;
    if (bm_check_params(c, p, P)) return -1;
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "stereo_bm: %d jobs > max_jobs", njobs);
    if (!jobs || !out_disp) return fail(c, "stereo_bm: null jobs / output");
    for (int i = 0; i < njobs; ++i) if (check_slot(c, jobs[i].slot_left) || check_slot(c, jobs[i].slot_right)) return -1;
    if (arena_busy(c)) return -1;
    c->ar.reset();
    static_assert(sizeof(BmJob) == sizeof(svslam_bm_job), "job layout");
    const size_t ojobs = c->ar.take(sizeof(BmJob) * njobs);
    memcpy(hp<void>(c, ojobs), jobs, sizeof(BmJob) * njobs);
    if (h2d(c, 0, c->ar.off)) return -1;
    tm_begin(c, FAM_BM, njobs);
    const int rc = launch_stereo_bm(c, njobs, dp<BmJob>(c, ojobs), P);
    tm_end(c);
    if (rc) return -1;
    HIPCHK(c, hipMemcpyAsync(out_disp, c->bm.disp.d, sizeof(int16_t) * (size_t)c->geom.w[0] * c->geom.h[0] * njobs, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    return 0;
}

// svslam_dense_cloud_batch, and with planes / out_bgr svslam_dense_cloud_bgr_batch: the same launches, then the colour gather
static int dense_cloud_common(svslam_ctx *c, int njobs, svslam_dense_job *jobs, const double cam_l[4], const double ext_l[7], double baseline,
                              const svslam_bm_params *p, double min_depth, int max_pts_per_job, float *out_xyz, int *out_pix,
                              int16_t *out_disp_or_null, bool colour, const int *planes, uint8_t *out_bgr)
{
    if (!c) return -1;
    BmParams P;
    if (bm_check_params(c, p, P)) return -1;
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "dense_cloud: %d jobs > max_jobs", njobs);
    if (!jobs || !cam_l || !ext_l || !out_xyz || !out_pix) return fail(c, "dense_cloud: null argument");
    if (max_pts_per_job < 1) return fail(c, "dense_cloud: max_pts_per_job %d < 1", max_pts_per_job);
    if (!(cam_l[0] > 0) || !(cam_l[1] > 0) || !(baseline > 0) || !(min_depth > 0)) return fail(c, "dense_cloud: fx, fy, baseline and min_depth must be positive");
    for (int i = 0; i < njobs; ++i) {
        if (check_slot(c, jobs[i].slot_left) || check_slot(c, jobs[i].slot_right)) return -1;
        if (jobs[i].pt_ofs < 0) return fail(c, "dense_cloud: job %d: negative pt_ofs", i);
    }
    if (colour) {
        if (!planes || !out_bgr) return fail(c, "colour: null planes / out_bgr");
        if (c->col.nplanes <= 0) return fail(c, "colour: no planes reserved (svslam_colour_reserve)");
        for (int i = 0; i < njobs; ++i) {
            if (planes[i] < 0 || planes[i] >= c->col.nplanes) return fail(c, "colour: job %d: plane %d out of range [0,%d)", i, planes[i], c->col.nplanes);
            if (!c->col.written[(size_t)planes[i]]) return fail(c, "colour: job %d: plane %d has not been written since it was reserved", i, planes[i]);
        }
    }
    if (arena_busy(c)) return -1;
    const int w = c->geom.w[0], h = c->geom.h[0];
    const size_t N = (size_t)w * h;
    const int cap = (int)std::min<size_t>((size_t)max_pts_per_job, N);     // a job has at most w h survivors
    const size_t bgr_per = col_bgr_per(cap);
    if (colour && c->col.bgr.reserve(c, "colour", bgr_per * (size_t)c->lim.max_jobs, 0)) return -1;
    if (c->bm.xyz.reserve(c, "dense_cloud", sizeof(float) * 3 * N * c->lim.max_jobs, 0) || c->bm.pix.reserve(c, "dense_cloud", sizeof(int) * N * c->lim.max_jobs, 0)) return -1;
    float *const d_xyz = (float *)c->bm.xyz.d;
    int *const d_pix = (int *)c->bm.pix.d;
    c->ar.reset();
    static_assert(sizeof(DenseJob) == sizeof(svslam_dense_job), "job layout");
    const size_t obm = c->ar.take(sizeof(BmJob) * njobs);
    const size_t oj = c->ar.take(sizeof(DenseJob) * njobs);
    for (int i = 0; i < njobs; ++i) { hp<BmJob>(c, obm)[i].slot_left = jobs[i].slot_left; hp<BmJob>(c, obm)[i].slot_right = jobs[i].slot_right; }
    memcpy(hp<void>(c, oj), jobs, sizeof(DenseJob) * njobs);
    const size_t opl = c->ar.take(sizeof(int) * njobs);
    if (colour) memcpy(hp<void>(c, opl), planes, sizeof(int) * njobs);
    if (h2d(c, 0, c->ar.off)) return -1;
    DenseCam cam;
    cam.fx = cam_l[0]; cam.fy = cam_l[1]; cam.cx = cam_l[2]; cam.cy = cam_l[3];
    memcpy(cam.ext, ext_l, 56);
    cam.min_depth = min_depth;
    cam.fxb = (float)cam_l[0] * (float)baseline;       // focal_length * baseline, both float (src/dense_reconstruction.cpp:120-124, 135)
    tm_begin(c, FAM_BM, njobs);
    const int rc = launch_stereo_bm(c, njobs, dp<BmJob>(c, obm), P);
    if (!rc) hipLaunchKernelGGL(k_dense_cloud, dim3(njobs), dim3(DC_THREADS), 0, c->stream, dp<DenseJob>(c, oj), (const int16_t *)c->bm.disp.d, w, h, cam, cap, d_xyz, d_pix);
    static_assert(sizeof(DenseJob) % sizeof(int) == 0 && offsetof(DenseJob, n_points) == 3 * sizeof(int), "n_points as k_colour_gather reads it");
    if (!rc && colour)
        hipLaunchKernelGGL(k_colour_gather, dim3(col_gather_blocks(cap), njobs), dim3(COL_THREADS), 0, c->stream, dp<int>(c, oj) + 3,
                           (int)(sizeof(DenseJob) / sizeof(int)), dp<int>(c, opl), (const int *)d_pix, cap, (const uint8_t *)c->col.planes.d, 3 * N,
                           (uint8_t *)c->col.bgr.d, bgr_per);
    tm_end(c);
    if (rc) return -1;
    HIPCHK(c, hipGetLastError());
    if (d2h_sync(c, oj, oj + sizeof(DenseJob) * njobs)) return -1;
    for (int i = 0; i < njobs; ++i) {
        jobs[i].n_points = hp<DenseJob>(c, oj)[i].n_points;
        if (jobs[i].n_points > max_pts_per_job) return fail(c, "dense_cloud: job %d has %d points > max_pts_per_job %d", i, jobs[i].n_points, max_pts_per_job);
    }
    for (int i = 0; i < njobs; ++i) {
        const size_t n = (size_t)jobs[i].n_points;
        if (!n) continue;
        HIPCHK(c, hipMemcpy(out_xyz + 3 * (size_t)jobs[i].pt_ofs, d_xyz + 3 * (size_t)i * cap, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out_pix + (size_t)jobs[i].pt_ofs, d_pix + (size_t)i * cap, sizeof(int) * n, hipMemcpyDeviceToHost));
        if (colour) HIPCHK(c, hipMemcpy(out_bgr + 3 * (size_t)jobs[i].pt_ofs, c->col.bgr.d + (size_t)i * bgr_per, 3 * n, hipMemcpyDeviceToHost));
    }
    if (out_disp_or_null) HIPCHK(c, hipMemcpy(out_disp_or_null, c->bm.disp.d, sizeof(int16_t) * N * njobs, hipMemcpyDeviceToHost));
    return 0;
}

int svslam_dense_cloud_batch(svslam_ctx *c, int njobs, svslam_dense_job *jobs, const double cam_l[4], const double ext_l[7], double baseline,
                             const svslam_bm_params *p, double min_depth, int max_pts_per_job, float *out_xyz, int *out_pix,
                             int16_t *out_disp_or_null)
{
    return dense_cloud_common(c, njobs, jobs, cam_l, ext_l, baseline, p, min_depth, max_pts_per_job, out_xyz, out_pix, out_disp_or_null, false, nullptr, nullptr);
}

// ------------------------------------------------------------------ colour input (src/dense_reconstruction.cpp:104-171)
int svslam_dense_cloud_bgr_batch(svslam_ctx *c, int njobs, svslam_dense_job *jobs, const double cam_l[4], const double ext_l[7], double baseline,
                                 const svslam_bm_params *p, double min_depth, int max_pts_per_job, const int *planes, float *out_xyz,
                                 int *out_pix, uint8_t *out_bgr, int16_t *out_disp_or_null)
{
    return dense_cloud_common(c, njobs, jobs, cam_l, ext_l, baseline, p, min_depth, max_pts_per_job, out_xyz, out_pix, out_disp_or_null, true, planes, out_bgr);
}

int svslam_colour_reserve(svslam_ctx *c, int nplanes)
{
    if (!c) return -1;
    if (nplanes < 0 || nplanes > 1 << 16) return fail(c, "colour: %d planes out of [0, 65536]", nplanes);
    if (nplanes == c->col.nplanes) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->col.planes.release();
    c->col.nplanes = 0;
    c->col.written.clear();
    if (nplanes == 0) return 0;
    if (c->col.planes.reserve(c, "colour", (size_t)3 * c->geom.w[0] * c->geom.h[0] * (size_t)nplanes, 0)) return -1;
    c->col.nplanes = nplanes;
    c->col.written.assign((size_t)nplanes, 0);
    return 0;
}

int svslam_pyramid_bgr_batch(svslam_ctx *c, int n, const int *slots, const int *planes, const void *const *imgs, const int *strides,
                             int src_w, int src_h, int src_is_device)
{
    if (!c) return -1;
    if (n <= 0) return 0;
    if (!slots || !planes || !imgs || !strides) return fail(c, "colour: null argument");
    if (n > c->lim.max_jobs) return fail(c, "colour: %d images > max_jobs %d", n, c->lim.max_jobs);
    const int w = c->geom.w[0], h = c->geom.h[0];
    bool decimate = false;
    if (src_w != w || src_h != h) {
        // svslam_pyramid_decimate_batch's rule, cvRound(src * 0.5): round half to even
        const int dw = src_w > 0 ? (int)std::nearbyint(src_w * 0.5) : -1, dh = src_h > 0 ? (int)std::nearbyint(src_h * 0.5) : -1;
        if (dw != w || dh != h) return fail(c, "colour: source %dx%d is not the context's %dx%d and does not halve to it", src_w, src_h, w, h);
        decimate = true;
    }
    if ((long long)3 * src_w > INT32_MAX / 2) return fail(c, "colour: source width %d too large", src_w);
    for (int i = 0; i < n; ++i) {
        if (!imgs[i]) return fail(c, "colour: image %d is null", i);
        if (check_slot(c, slots[i])) return -1;
        if (strides[i] > INT32_MAX / 2) return fail(c, "colour: image %d: stride %d too large", i, strides[i]);
        if (strides[i] < 3 * src_w) return fail(c, "colour: image %d: stride %d < 3 * %d", i, strides[i], src_w);
        if (planes[i] < -1 || planes[i] >= std::max(c->col.nplanes, 0)) {
            if (planes[i] >= 0 && c->col.nplanes <= 0) return fail(c, "colour: no planes reserved (svslam_colour_reserve)");
            return fail(c, "colour: image %d: plane %d out of range [-1,%d)", i, planes[i], c->col.nplanes);
        }
        for (int k = 0; k < i; ++k) if (planes[i] >= 0 && planes[k] == planes[i]) return fail(c, "colour: plane %d named twice (images %d and %d)", planes[i], k, i);
    }
    if (arena_busy(c)) return -1;
    const size_t grey_per = ((size_t)w * h + 255) & ~(size_t)255;
    if (c->col.grey.reserve(c, "colour", grey_per * (size_t)c->lim.max_jobs + 256, 0)) return -1;
    c->ar.reset();
    const size_t ob = c->ar.take(sizeof(BgrJob) * n), opj = c->ar.take(sizeof(PyrJob) * n);
    BgrJob *bj = hp<BgrJob>(c, ob);
    PyrJob *pj = hp<PyrJob>(c, opj);
    if (!src_is_device) {
        // only the rows the kernel reads are staged: every row, or the even ones
        const int rows = decimate ? h : src_h, step = decimate ? 2 : 1;
        const size_t rb = (size_t)3 * src_w, per = (rb * (size_t)rows + 255) & ~(size_t)255;
        if (c->img.reserve(c, "colour", per * (size_t)n, 0, 0, true)) return -1;
        for (int i = 0; i < n; ++i) {
            const uint8_t *s = static_cast<const uint8_t *>(imgs[i]);
            uint8_t *d = c->img.pin + per * i;
            for (int y = 0; y < rows; ++y) memcpy(d + (size_t)y * rb, s + (size_t)(y * step) * (size_t)strides[i], rb);
            bj[i].src = c->img.d + per * i;
            bj[i].stride = (int)rb;
        }
        HIPCHK(c, hipMemcpyAsync(c->img.d, c->img.pin, per * (size_t)n, hipMemcpyHostToDevice, c->stream));
    } else {
        for (int i = 0; i < n; ++i) { bj[i].src = static_cast<const uint8_t *>(imgs[i]); bj[i].stride = col_row_stride(strides[i], decimate); }
    }
    for (int i = 0; i < n; ++i) {
        bj[i].plane = planes[i];
        pj[i].src = c->col.grey.d + grey_per * i; pj[i].src_stride = w; pj[i].slot = slots[i];
    }
    if (h2d(c, 0, c->ar.off)) return -1;
    const int chunks = col_chunks(w);
    const dim3 grid(col_prepare_blocks(w, h), n);
    tm_begin(c, FAM_COL, n);
    if (decimate) hipLaunchKernelGGL(k_bgr_prepare<true>, grid, dim3(COL_THREADS), 0, c->stream, dp<BgrJob>(c, ob), w, h, src_w, chunks, (uint8_t *)c->col.grey.d, grey_per, (uint8_t *)c->col.planes.d);
    else hipLaunchKernelGGL(k_bgr_prepare<false>, grid, dim3(COL_THREADS), 0, c->stream, dp<BgrJob>(c, ob), w, h, src_w, chunks, (uint8_t *)c->col.grey.d, grey_per, (uint8_t *)c->col.planes.d);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    if (launch_pyramid(c, dp<PyrJob>(c, opj), n, false, w, h)) return -1;
    if (d2h_sync(c, 0, 0)) return -1;
    for (int i = 0; i < n; ++i) if (planes[i] >= 0) c->col.written[(size_t)planes[i]] = 1;
    return 0;
}

int svslam_colour_read(svslam_ctx *c, int plane, uint8_t *out)
{
    if (!c) return -1;
    if (!out) return fail(c, "colour: null output");
    if (c->col.nplanes <= 0) return fail(c, "colour: no planes reserved (svslam_colour_reserve)");
    if (plane < 0 || plane >= c->col.nplanes) return fail(c, "colour: plane %d out of range [0,%d)", plane, c->col.nplanes);
    const size_t bytes = (size_t)3 * c->geom.w[0] * c->geom.h[0];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->col.planes.d + bytes * (size_t)plane, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ cloud filters (src/dense_reconstruction.cpp:175-209)
// a cloud-filter buffer of at least `bytes`; a regrow takes a quarter of headroom plus 256 bytes
static int cf_reserve(svslam_ctx *c, DevBuf &b, size_t bytes) { return b.reserve(c, "cloud_filter", bytes, bytes / 4 + 256); }
static inline dim3 cf_grid(long long n) { return dim3((unsigned)((n + CF_THREADS - 1) / CF_THREADS)); }

int svslam_cloud_sor_batch(svslam_ctx *c, int nseg, const int64_t *seg_ofs, const float *xyz, int mean_k, double stddev_mul, uint8_t *out_keep,
                           float *out_mean_dist_or_null, double *out_threshold)
{
    if (!c) return -1;
    if (mean_k < 1 || mean_k > CF_KMAX) return fail(c, "cloud_filter: mean_k %d out of [1, %d]", mean_k, CF_KMAX);
    if (nseg < 0) return fail(c, "cloud_filter: %d segments", nseg);
    if (nseg == 0) return 0;
    if (!seg_ofs || !out_threshold) return fail(c, "cloud_filter: null seg_ofs / out_threshold");
    for (int s = 0; s < nseg; ++s) if (seg_ofs[s + 1] < seg_ofs[s] || seg_ofs[s] < 0) return fail(c, "cloud_filter: seg_ofs must be non-negative and ascending (segment %d)", s);
    const int64_t first = seg_ofs[0], total64 = seg_ofs[nseg] - first;
    if (total64 > (int64_t)1 << 30) return fail(c, "cloud_filter: %lld points in one call > 2^30", (long long)total64);
    if (nseg > 1 << 20) return fail(c, "cloud_filter: %d segments > 2^20", nseg);
    const int total = (int)total64;
    if (total && (!xyz || !out_keep)) return fail(c, "cloud_filter: null xyz / out_keep");
    std::vector<CfSeg> segs((size_t)nseg);
    bool any = false;
    char msg[CF_MSG];
    if (const char *e = cf_segments(nseg, seg_ofs, xyz, mean_k, segs.data(), &any, msg)) return fail(c, "%s", e);
    std::vector<float> md_own;
    if (!out_mean_dist_or_null) md_own.resize((size_t)std::max(total, 1));
    float *mdv = out_mean_dist_or_null ? out_mean_dist_or_null + first : md_own.data();       // mean distance of point seg_ofs[0] + i
    if (!any) std::fill(mdv, mdv + total, 0.f);
    else {
        const size_t N = (size_t)total;
        auto &f = c->cf;
        if (cf_reserve(c, f.xyz, 12 * N) || cf_reserve(c, f.segs, sizeof(CfSeg) * (size_t)nseg) || cf_reserve(c, f.keys, 8 * N) || cf_reserve(c, f.keys2, 8 * N) ||
            cf_reserve(c, f.vals, 4 * N) || cf_reserve(c, f.vals2, 4 * N) || cf_reserve(c, f.soa, 12 * N) || cf_reserve(c, f.out, 4 * N) || f.climbs.reserve(c, "cloud_filter", sizeof(unsigned), 0)) return -1;
        unsigned *const climbs = (unsigned *)f.climbs.d;
        int seg_bits = 1;
        while ((1 << seg_bits) < nseg) ++seg_bits;
        size_t tmp_bytes = 0;
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, (unsigned long long *)f.keys.d, (unsigned long long *)f.keys2.d, (unsigned *)f.vals.d,
                                            (unsigned *)f.vals2.d, N, 0u, (unsigned)(30 + seg_bits), c->stream));
        if (cf_reserve(c, f.tmp, tmp_bytes)) return -1;
        HIPCHK(c, hipMemcpy(f.xyz.d, xyz + 3 * (size_t)first, 12 * N, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(f.segs.d, segs.data(), sizeof(CfSeg) * (size_t)nseg, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemsetAsync(climbs, 0, sizeof(unsigned), c->stream));
        float *sx = (float *)f.soa.d, *sy = sx + N, *sz = sy + N;
        tm_begin(c, FAM_CF, total);
        hipLaunchKernelGGL(k_cf_keys, cf_grid(total), dim3(CF_THREADS), 0, c->stream, (const float *)f.xyz.d, total, (const CfSeg *)f.segs.d, nseg,
                           (unsigned long long *)f.keys.d, (unsigned *)f.vals.d);
        HIPCHK(c, rocprim::radix_sort_pairs(f.tmp.d, tmp_bytes, (unsigned long long *)f.keys.d, (unsigned long long *)f.keys2.d, (unsigned *)f.vals.d,
                                            (unsigned *)f.vals2.d, N, 0u, (unsigned)(30 + seg_bits), c->stream));
        hipLaunchKernelGGL(k_cf_gather, cf_grid(total), dim3(CF_THREADS), 0, c->stream, (const float *)f.xyz.d, (const unsigned *)f.vals2.d, total, sx, sy, sz);
        // 51 register slots hold the reference's k = 50; a larger k takes the 65-slot instance
        if (mean_k <= 50)
            hipLaunchKernelGGL(k_cf_knn<51>, cf_grid(total), dim3(CF_THREADS), 0, c->stream, (const unsigned long long *)f.keys2.d, (const unsigned *)f.vals2.d,
                               (const float *)sx, (const float *)sy, (const float *)sz, total, (const CfSeg *)f.segs.d, mean_k, (float *)f.out.d, climbs);
        else
            hipLaunchKernelGGL(k_cf_knn<CF_KMAX + 1>, cf_grid(total), dim3(CF_THREADS), 0, c->stream, (const unsigned long long *)f.keys2.d, (const unsigned *)f.vals2.d,
                               (const float *)sx, (const float *)sy, (const float *)sz, total, (const CfSeg *)f.segs.d, mean_k, (float *)f.out.d, climbs);
        tm_end(c);
        HIPCHK(c, hipGetLastError());
        if (d2h_sync(c, 0, 0)) return -1;
        HIPCHK(c, hipMemcpy(mdv, f.out.d, 4 * N, hipMemcpyDeviceToHost));
        unsigned climbed = 0;
        HIPCHK(c, hipMemcpy(&climbed, climbs, sizeof(unsigned), hipMemcpyDeviceToHost));
        for (const CfSeg &g : segs) if (g.n >= mean_k + 1) f.queries += g.n;
        f.climbed += climbed;
    }
    for (int s = 0; s < nseg; ++s) out_threshold[s] = cf_sor_decide(segs[(size_t)s].n, mdv + segs[(size_t)s].ofs, mean_k, stddev_mul, out_keep + seg_ofs[s]);
    return 0;
}

int svslam_debug_cloud_sor_climbs(svslam_ctx *c, long long *out_queries, long long *out_climbed)
{
    if (!c) return -1;
    if (out_queries) *out_queries = c->cf.queries;
    if (out_climbed) *out_climbed = c->cf.climbed;
    c->cf.queries = c->cf.climbed = 0;
    return 0;
}

int svslam_cloud_voxel_grid(svslam_ctx *c, int64_t n, const float *xyz, const uint8_t *rgb, double leaf, float *out_xyz, uint8_t *out_rgb,
                            int64_t *out_n, int *out_overflowed)
{
    if (!c) return -1;
    if (!(leaf > 0) || !std::isfinite(leaf)) return fail(c, "cloud_filter: leaf %g must be positive", leaf);
    if (n < 0 || n > (int64_t)1 << 30) return fail(c, "cloud_filter: %lld points out of [0, 2^30]", (long long)n);
    if (!out_n || !out_overflowed) return fail(c, "cloud_filter: null out_n / out_overflowed");
    *out_n = 0; *out_overflowed = 0;
    if (n == 0) return 0;
    if (!xyz || !rgb || !out_xyz || !out_rgb) return fail(c, "cloud_filter: null cloud / output");
    const size_t N = (size_t)n;
    VgParams P;
    bool over = false;
    char msg[CF_MSG];
    if (const char *e = vg_plan(N, xyz, leaf, P, &over, msg)) return fail(c, "%s", e);
    if (over) {
        memcpy(out_xyz, xyz, 12 * N); memcpy(out_rgb, rgb, 3 * N);
        *out_n = n; *out_overflowed = 1;
        return 0;
    }
    auto &f = c->cf;
    if (cf_reserve(c, f.xyz, 12 * N) || cf_reserve(c, f.rgb, 3 * N) || cf_reserve(c, f.keys, 8 * N) || cf_reserve(c, f.keys2, 8 * N) || cf_reserve(c, f.flag, 4 * N) ||
        cf_reserve(c, f.pos, 4 * N) || cf_reserve(c, f.start, 4 * N) || cf_reserve(c, f.oxyz, 12 * N) || cf_reserve(c, f.orgb, 3 * N)) return -1;
    size_t sort_bytes = 0, scan_bytes = 0;
    HIPCHK(c, rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)f.keys.d, (unsigned long long *)f.keys2.d, N, 0u, 64u, c->stream));
    HIPCHK(c, rocprim::inclusive_scan(nullptr, scan_bytes, (unsigned *)f.flag.d, (unsigned *)f.pos.d, N, rocprim::plus<unsigned>(), c->stream));
    if (cf_reserve(c, f.tmp, std::max(sort_bytes, scan_bytes))) return -1;
    HIPCHK(c, hipMemcpy(f.xyz.d, xyz, 12 * N, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(f.rgb.d, rgb, 3 * N, hipMemcpyHostToDevice));
    const int ni = (int)n;
    tm_begin(c, FAM_CF, n);
    hipLaunchKernelGGL(k_vg_keys, cf_grid(n), dim3(CF_THREADS), 0, c->stream, (const float *)f.xyz.d, ni, P, (unsigned long long *)f.keys.d);
    HIPCHK(c, rocprim::radix_sort_keys(f.tmp.d, sort_bytes, (unsigned long long *)f.keys.d, (unsigned long long *)f.keys2.d, N, 0u, 64u, c->stream));
    hipLaunchKernelGGL(k_vg_heads, cf_grid(n), dim3(CF_THREADS), 0, c->stream, (const unsigned long long *)f.keys2.d, ni, (unsigned *)f.flag.d);
    HIPCHK(c, rocprim::inclusive_scan(f.tmp.d, scan_bytes, (unsigned *)f.flag.d, (unsigned *)f.pos.d, N, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(k_vg_starts, cf_grid(n), dim3(CF_THREADS), 0, c->stream, (const unsigned *)f.flag.d, (const unsigned *)f.pos.d, ni, (int *)f.start.d);
    HIPCHK(c, hipGetLastError());
    // the number of voxels decides the last launch: one small read-back in the middle of the call
    unsigned m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, (unsigned *)f.pos.d + (N - 1), sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m < 1 || (size_t)m > N) return fail(c, "cloud_filter: voxel count %u out of [1, %zu]", m, N);
    hipLaunchKernelGGL(k_vg_reduce, cf_grid(m), dim3(CF_THREADS), 0, c->stream, (const unsigned long long *)f.keys2.d, (const int *)f.start.d, (int)m, ni,
                       (const float *)f.xyz.d, (const uint8_t *)f.rgb.d, (float *)f.oxyz.d, (uint8_t *)f.orgb.d);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    if (d2h_sync(c, 0, 0)) return -1;
    HIPCHK(c, hipMemcpy(out_xyz, f.oxyz.d, 12 * (size_t)m, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_rgb, f.orgb.d, 3 * (size_t)m, hipMemcpyDeviceToHost));
    *out_n = (int64_t)m;
    return 0;
}

} // extern "C"
