// api_frontend.h — included by svslam_hip.hip.  Entry points: svslam_pyramid_*, svslam_set_source_size, svslam_lk_batch, svslam_gftt_*,
// svslam_triangulate_batch, svslam_pose_only_batch, svslam_{get,set}_pose_only_xtol, svslam_track_batch, svslam_rtrack_*.
// Owns of svslam_ctx: geom, pyr_plan, pyr_fused, d_pyr, img, gw, src_w / src_h, po_xtol, rt, rt_which, rt_count.

namespace {

// more (optional): called once the pyramid's own jobs are staged and before its launch; stages the caller's further inputs behind
// them (the arena is not reset again) and may fill *ga to let the resident-tracking gather ride on the pyramid launch
struct PyrMore { std::function<int(RtGatherArgs *)> stage; bool gathered = false; };
int pyramid_common(svslam_ctx *c, int n, const int *slots, const void *const *imgs, const int *strides,
                   int src_is_device, bool decimate, int src_w, int src_h, bool sync, PyrMore *more = nullptr)
{
    if (n <= 0) return 0;
    if (n > c->lim.max_jobs) return fail(c, "pyramid: %d jobs > max_jobs %d", n, c->lim.max_jobs);
    for (int i = 0; i < n; ++i) if (check_slot(c, slots[i])) return -1;
    const int iw = decimate ? src_w : c->geom.w[0], ih = decimate ? src_h : c->geom.h[0];
    if (arena_busy(c)) return -1;
    c->ar.reset();
    size_t ojobs = c->ar.take(sizeof(PyrJob) * n);
    PyrJob *hj = hp<PyrJob>(c, ojobs);
    if (!src_is_device) {
        size_t per = ((size_t)iw * ih + 255) & ~(size_t)255;
        size_t need = per * n;
        if (c->img.reserve(c, "pyramid", need, 0, 0, true)) return -1;
        for (int i = 0; i < n; ++i) {
            const uint8_t *s = static_cast<const uint8_t *>(imgs[i]);
            uint8_t *d = c->img.pin + per * i;
            for (int y = 0; y < ih; ++y) memcpy(d + (size_t)y * iw, s + (size_t)y * strides[i], iw);
            hj[i].src = c->img.d + per * i;
            hj[i].src_stride = iw;
            hj[i].slot = slots[i];
        }
        HIPCHK(c, hipMemcpyAsync(c->img.d, c->img.pin, need, hipMemcpyHostToDevice, c->stream));
    } else {
        for (int i = 0; i < n; ++i) {
            hj[i].src = static_cast<const uint8_t *>(imgs[i]);
            hj[i].src_stride = strides[i];
            hj[i].slot = slots[i];
        }
    }
    if (!c->zero_copy && h2d(c, ojobs, c->ar.off)) return -1;
    RtGatherArgs ga = {};
    if (more && more->stage(&ga)) return -1;
    if (launch_pyramid(c, dpz<PyrJob>(c, ojobs), n, decimate, src_w, src_h, more ? &ga : nullptr, more ? &more->gathered : nullptr)) return -1;
    if (sync) return d2h_sync(c, 0, 0);
    return 0;
}

} // namespace

extern "C" {

// ------------------------------------------------------------------ pyramids
int svslam_pyramid_batch(svslam_ctx *c, int n, const int *slots, const void *const *imgs,
                         const int *strides, int src_is_device)
{
    const bool dec = c->src_w > 0;
    return pyramid_common(c, n, slots, imgs, strides, src_is_device, dec, dec ? c->src_w : c->geom.w[0],
                          dec ? c->src_h : c->geom.h[0], true);
}

double svslam_get_pose_only_xtol(const svslam_ctx *c) { return c ? c->po_xtol : -1.0; }

int svslam_set_pose_only_xtol(svslam_ctx *c, double xtol)
{
    if (!(xtol >= 0) || xtol > 1e-6) return fail(c, "svslam_set_pose_only_xtol: 0 <= xtol <= 1e-6 (got %g)", xtol);
    c->po_xtol = xtol;
    return 0;
}

int svslam_set_source_size(svslam_ctx *c, int src_w, int src_h)
{
    if (src_w <= 0 || src_h <= 0) { c->src_w = c->src_h = 0; return 0; }
    const int dw = (int)std::nearbyint(src_w * 0.5), dh = (int)std::nearbyint(src_h * 0.5);   // cvRound
    if (dw != c->geom.w[0] || dh != c->geom.h[0])
        return fail(c, "source %dx%d halves to %dx%d, context is %dx%d", src_w, src_h, dw, dh, c->geom.w[0], c->geom.h[0]);
    c->src_w = src_w; c->src_h = src_h;
    return 0;
}

int svslam_pyramid_decimate_batch(svslam_ctx *c, int n, const int *slots, const void *const *imgs,
                                  const int *strides, int src_w, int src_h, int src_is_device)
{
    // cvRound(src*0.5): round half to even
    int dw = (int)std::nearbyint(src_w * 0.5), dh = (int)std::nearbyint(src_h * 0.5);
    if (dw != c->geom.w[0] || dh != c->geom.h[0])
        return fail(c, "decimate: source %dx%d halves to %dx%d, context is %dx%d", src_w, src_h, dw, dh,
                    c->geom.w[0], c->geom.h[0]);
    return pyramid_common(c, n, slots, imgs, strides, src_is_device, true, src_w, src_h, true);
}

int svslam_pyramid_read(svslam_ctx *c, int slot, int level, uint8_t *out, int *w, int *h)
{
    if (check_slot(c, slot)) return -1;
    if (level < 0 || level >= c->geom.nlevels) return fail(c, "level %d out of range", level);
    const PyrGeom &g = c->geom;
    if (w) *w = g.w[level];
    if (h) *h = g.h[level];
    if (!out) return 0;
    const uint8_t *src = c->d_pyr + (size_t)slot * g.slot_bytes + g.ofs[level] + (size_t)SVS_BORDER * g.pitch[level] + SVS_BORDER;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(out, g.w[level], src, g.pitch[level], g.w[level], g.h[level], hipMemcpyDeviceToHost));
    return 0;
}

// test hook: one level WITH its stored 16-px REFLECT_101 border, tight rows of (w + 32) bytes
int svslam_pyramid_read_padded(svslam_ctx *c, int slot, int level, uint8_t *out)
{
    if (check_slot(c, slot)) return -1;
    if (level < 0 || level >= c->geom.nlevels) return fail(c, "level %d out of range", level);
    const PyrGeom &g = c->geom;
    const int pw = g.w[level] + 2 * SVS_BORDER, ph = g.h[level] + 2 * SVS_BORDER;
    const uint8_t *src = c->d_pyr + (size_t)slot * g.slot_bytes + g.ofs[level];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(out, pw, src, g.pitch[level], pw, ph, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ LK
static LkParams make_lk_params(const svslam_lk_params *p)
{
    LkParams k;
    k.max_level = p ? p->max_level : 3;
    int mc = p ? p->max_iter : 30;
    k.max_count = std::min(std::max(mc, 0), 100);
    double eps = p ? p->epsilon : 0.01;
    eps = std::min(std::max(eps, 0.), 10.);
    k.eps2 = eps * eps;
    k.min_eig_thr = p ? p->min_eig_thr : 1e-4;
    k.use_initial_flow = p ? p->use_initial_flow : 1;
    // k_lk tests the min eigenvalue as numerator < x* instead of (double)(numerator / 242.f) < thr: x* is the
    // smallest float whose quotient reaches the threshold (float division is monotone), found by stepping
    const float den = (float)(2 * LK_WIN * LK_WIN);
    float x = (float)(k.min_eig_thr * (double)den);
    int steps = 0;
    bool ok = std::isfinite(x) && k.min_eig_thr > 1e-30;
    while (ok && (double)(x / den) >= k.min_eig_thr) { x = std::nextafterf(x, -INFINITY); if (++steps > 64) ok = false; }
    while (ok && (double)(x / den) < k.min_eig_thr) { x = std::nextafterf(x, INFINITY); if (++steps > 128) ok = false; }
    k.eig_num_thr = x;
    k.eig_use_div = ok ? 0 : 1;
    k.njobs = 0; k.blocks_per_job = 1;
    return k;
}

static void launch_lk(svslam_ctx *c, int njobs, int maxn, const LkJob *jobs, const float2 *prev, float2 *next, uint8_t *stat,
                      float *err, const svslam_lk_params *p)
{
    LkParams k = make_lk_params(p);
    k.njobs = njobs; k.blocks_per_job = cdiv(maxn, LK_WAVES_PER_BLOCK);
    hipLaunchKernelGGL(k_lk, dim3(8 * k.blocks_per_job * cdiv(njobs, 8)), dim3(64 * LK_WAVES_PER_BLOCK), 0, c->stream, jobs,
                       c->d_pyr, c->geom, prev, next, stat, err, k);
}

int svslam_lk_batch(svslam_ctx *c, int njobs, const svslam_lk_job *jobs, int total_pts,
                    const float *prev_xy, float *next_xy, uint8_t *status, float *err,
                    const svslam_lk_params *p)
{
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "lk: %d jobs > max_jobs", njobs);
    if (total_pts > c->lim.max_jobs * c->lim.max_pts) return fail(c, "lk: too many points");
    int maxn = 0;
    for (int i = 0; i < njobs; ++i) {
        if (check_slot(c, jobs[i].prev_slot) || check_slot(c, jobs[i].next_slot)) return -1;
        if (jobs[i].npts < 0 || jobs[i].pt_ofs < 0 || jobs[i].pt_ofs + jobs[i].npts > total_pts)
            return fail(c, "lk: job %d point range out of bounds", i);
        maxn = std::max(maxn, jobs[i].npts);
    }
    if (arena_busy(c)) return -1;
    c->ar.reset();
    size_t ojobs = c->ar.take(sizeof(LkJob) * njobs);
    size_t oprev = c->ar.take(sizeof(float) * 2 * total_pts);
    size_t onext = c->ar.take(sizeof(float) * 2 * total_pts);
    size_t in_end = c->ar.off;
    size_t ostat = c->ar.take(total_pts);
    size_t oerr = c->ar.take(sizeof(float) * total_pts);
    static_assert(sizeof(LkJob) == sizeof(svslam_lk_job), "job layout");
    memcpy(hp<void>(c, ojobs), jobs, sizeof(LkJob) * njobs);
    memcpy(hp<void>(c, oprev), prev_xy, sizeof(float) * 2 * total_pts);
    memcpy(hp<void>(c, onext), next_xy, sizeof(float) * 2 * total_pts);
    if (h2d(c, 0, in_end)) return -1;
    if (maxn > 0) {
        tm_begin(c, FAM_LK, total_pts);
        launch_lk(c, njobs, maxn, dp<LkJob>(c, ojobs), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, ostat),
                  dp<float>(c, oerr), p);
        tm_end(c);
        HIPCHK(c, hipGetLastError());
    }
    if (d2h_sync(c, onext, c->ar.off)) return -1;
    memcpy(next_xy, hp<void>(c, onext), sizeof(float) * 2 * total_pts);
    memcpy(status, hp<void>(c, ostat), total_pts);
    if (err) memcpy(err, hp<void>(c, oerr), sizeof(float) * total_pts);
    return 0;
}

// ------------------------------------------------------------------ GFTT
static int launch_gftt(svslam_ctx *c, int njobs, const GfttJob *djobs, const float2 *drects,
                       int max_corners, double quality, double min_dist, float2 *dout, int *dn)
{
    const int w = c->geom.w[0], h = c->geom.h[0];
    tm_begin(c, c->timing_split ? FAM_DBG0 : FAM_GFTT, njobs);
    // one-dimensional grid, jobs dealt over the XCDs (see LkParams): the strips of an image share their halo
    // columns, rows and the 64-byte lines they straddle through one L2
    hipLaunchKernelGGL(k_gftt_eig3<false>, dim3(8 * cdiv(w, GE_COLS) * cdiv(h, GE_ROWS) * cdiv(njobs, 8)), dim3(64), 0, c->stream, djobs,
                       njobs, c->d_pyr, c->geom, c->gw, drects, quality, (float *)nullptr);
    if (c->timing_split) { tm_end(c); tm_begin(c, FAM_DBG1, njobs); }
    hipLaunchKernelGGL(k_gftt_select2, dim3(njobs), dim3(GS_THREADS), 0, c->stream, c->gw, w, h, max_corners, quality,
                       min_dist, dout, dn, max_corners);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int svslam_gftt_batch(svslam_ctx *c, int njobs, const svslam_gftt_job *jobs, int total_rects,
                      const float *rect_xy, int max_corners, double quality, double min_dist,
                      float *out_xy, int *out_n)
{
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "gftt: %d jobs > max_jobs", njobs);
    if (max_corners < 1 || max_corners > c->lim.max_corners) return fail(c, "gftt: max_corners %d out of [1,%d]", max_corners, c->lim.max_corners);
    if (total_rects > c->lim.max_jobs * c->lim.max_pts) return fail(c, "gftt: too many mask rects");
    for (int i = 0; i < njobs; ++i) {
        if (check_slot(c, jobs[i].slot)) return -1;
        if (jobs[i].nrect < 0 || jobs[i].rect_ofs < 0 || jobs[i].rect_ofs + jobs[i].nrect > total_rects)
            return fail(c, "gftt: job %d rect range out of bounds", i);
    }
    if (arena_busy(c)) return -1;
    c->ar.reset();
    size_t ojobs = c->ar.take(sizeof(GfttJob) * njobs);
    size_t orect = c->ar.take(sizeof(float) * 2 * std::max(total_rects, 1));
    size_t in_end = c->ar.off;
    size_t oout = c->ar.take(sizeof(float) * 2 * (size_t)max_corners * njobs);
    size_t on = c->ar.take(sizeof(int) * njobs);
    static_assert(sizeof(GfttJob) == sizeof(svslam_gftt_job), "job layout");
    memcpy(hp<void>(c, ojobs), jobs, sizeof(GfttJob) * njobs);
    if (total_rects > 0) memcpy(hp<void>(c, orect), rect_xy, sizeof(float) * 2 * total_rects);
    if (h2d(c, 0, in_end)) return -1;
    if (launch_gftt(c, njobs, dp<GfttJob>(c, ojobs), dp<float2>(c, orect), max_corners, quality,
                    min_dist, dp<float2>(c, oout), dp<int>(c, on))) return -1;
    if (d2h_sync(c, oout, c->ar.off)) return -1;
    memcpy(out_n, hp<void>(c, on), sizeof(int) * njobs);
    memcpy(out_xy, hp<void>(c, oout), sizeof(float) * 2 * (size_t)max_corners * njobs);
    return 0;
}

int svslam_gftt_eigmap(svslam_ctx *c, int slot, float *out)
{
    if (check_slot(c, slot)) return -1;
    if (arena_busy(c)) return -1;
    c->ar.reset();
    size_t ojobs = c->ar.take(sizeof(GfttJob));
    GfttJob *j = hp<GfttJob>(c, ojobs);
    j->slot = slot; j->rect_ofs = 0; j->nrect = 0;
    if (h2d(c, 0, c->ar.off)) return -1;
    const int w = c->geom.w[0], h = c->geom.h[0];
    float *d_eig = nullptr;
    HIPCHK(c, hipMalloc(&d_eig, sizeof(float) * (size_t)w * h));
    // the production kernel with its eigenvalue store compiled in (the product instantiation differs by
    // exactly that store), so the eig-map parity tests check what ships
    hipLaunchKernelGGL(k_gftt_eig3<true>, dim3(8 * cdiv(w, GE_COLS) * cdiv(h, GE_ROWS)), dim3(64), 0, c->stream,
                       dp<GfttJob>(c, ojobs), 1, c->d_pyr, c->geom, c->gw, (const float2 *)nullptr, 0.01, d_eig);
    hipError_t e1 = hipGetLastError();
    hipError_t e2 = hipMemsetAsync(c->gw.counters, 0, sizeof(unsigned int) * GF_CNT_STRIDE, c->stream);   // job 0's counters back to zero
    hipError_t e3 = hipStreamSynchronize(c->stream);
    hipError_t e4 = hipMemcpy(out, d_eig, sizeof(float) * (size_t)w * h, hipMemcpyDeviceToHost);
    (void)hipFree(d_eig);
    HIPCHK(c, e1); HIPCHK(c, e2); HIPCHK(c, e3); HIPCHK(c, e4);
    return 0;
}

// ------------------------------------------------------------------ triangulation
int svslam_triangulate_batch(svslam_ctx *c, int njobs, const svslam_tri_job *jobs, int total_pts,
                             const double cam_l[4], const double ext_l[7], const double cam_r[4],
                             const double ext_r[7], const float *uv_l, const float *uv_r,
                             double *out_xyz, uint8_t *out_ok)
{
    if (njobs <= 0 || total_pts <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "triangulate: %d jobs > max_jobs", njobs);
    if (total_pts > c->lim.max_jobs * c->lim.max_pts) return fail(c, "triangulate: too many points");
    int maxn = 0;
    for (int i = 0; i < njobs; ++i) {
        if (jobs[i].npts < 0 || jobs[i].pt_ofs < 0 || jobs[i].pt_ofs + jobs[i].npts > total_pts)
            return fail(c, "triangulate: job %d point range out of bounds", i);
        maxn = std::max(maxn, jobs[i].npts);
    }
    if (arena_busy(c)) return -1;
    c->ar.reset();
    static_assert(sizeof(TriJob) == sizeof(svslam_tri_job), "job layout");
    size_t ojobs = c->ar.take(sizeof(TriJob) * njobs);
    size_t ol = c->ar.take(sizeof(float) * 2 * total_pts);
    size_t orr = c->ar.take(sizeof(float) * 2 * total_pts);
    size_t in_end = c->ar.off;
    size_t oxyz = c->ar.take(sizeof(double) * 3 * total_pts);
    size_t ook = c->ar.take(total_pts);
    memcpy(hp<void>(c, ojobs), jobs, sizeof(TriJob) * njobs);
    memcpy(hp<void>(c, ol), uv_l, sizeof(float) * 2 * total_pts);
    memcpy(hp<void>(c, orr), uv_r, sizeof(float) * 2 * total_pts);
    TriCams cams;
    memcpy(cams.cam_l, cam_l, 32); memcpy(cams.ext_l, ext_l, 56);
    memcpy(cams.cam_r, cam_r, 32); memcpy(cams.ext_r, ext_r, 56);
    if (h2d(c, 0, in_end)) return -1;
    if (maxn > 0) {
        tm_begin(c, FAM_TRI, total_pts);
        hipLaunchKernelGGL(k_triangulate, dim3(njobs, cdiv(maxn, 64)), dim3(64), 0, c->stream, dp<TriJob>(c, ojobs),       // (job-major grid: k_geom.h)
                           cams, dp<float2>(c, ol), dp<float2>(c, orr), dp<double>(c, oxyz), dp<uint8_t>(c, ook));
        tm_end(c);
        HIPCHK(c, hipGetLastError());
    }
    if (d2h_sync(c, oxyz, c->ar.off)) return -1;
    memcpy(out_xyz, hp<void>(c, oxyz), sizeof(double) * 3 * total_pts);
    memcpy(out_ok, hp<void>(c, ook), total_pts);
    return 0;
}

// ------------------------------------------------------------------ pose-only
int svslam_pose_only_batch(svslam_ctx *c, int njobs, svslam_pose_job *jobs, int total_pts,
                           const double cam[4], const double *xyz, const float *uv,
                           uint8_t *outlier, double chi2_th, int rounds, int iters)
{
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "pose_only: %d jobs > max_jobs", njobs);
    if (total_pts > c->lim.max_jobs * c->lim.max_pts) return fail(c, "pose_only: too many points");
    for (int i = 0; i < njobs; ++i) {
        if (jobs[i].npts < 0 || jobs[i].npts > c->lim.max_pts || jobs[i].pt_ofs < 0 ||
            jobs[i].pt_ofs + jobs[i].npts > total_pts)
            return fail(c, "pose_only: job %d point range out of bounds", i);
    }
    if (arena_busy(c)) return -1;
    c->ar.reset();
    static_assert(sizeof(PoseJob) == sizeof(svslam_pose_job), "job layout");
    size_t ocam = c->ar.take(32);
    size_t oxyz = c->ar.take(sizeof(double) * 3 * std::max(total_pts, 1));
    size_t ouv = c->ar.take(sizeof(float) * 2 * std::max(total_pts, 1));
    size_t ojobs = c->ar.take(sizeof(PoseJob) * njobs);
    size_t in_end = c->ar.off;
    size_t oout = c->ar.take(std::max(total_pts, 1));
    memcpy(hp<void>(c, ocam), cam, 32);
    if (total_pts > 0) {
        memcpy(hp<void>(c, oxyz), xyz, sizeof(double) * 3 * total_pts);
        memcpy(hp<void>(c, ouv), uv, sizeof(float) * 2 * total_pts);
    }
    memcpy(hp<void>(c, ojobs), jobs, sizeof(PoseJob) * njobs);
    if (h2d(c, 0, in_end)) return -1;
    tm_begin(c, FAM_POSE, njobs);
    launch_pose_only(c, njobs, dp<PoseJob>(c, ojobs), dp<double>(c, ocam), dp<double>(c, oxyz), dp<float2>(c, ouv),
                     nullptr, dp<uint8_t>(c, oout), chi2_th, rounds, iters);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    if (d2h_sync(c, ojobs, c->ar.off)) return -1;
    memcpy(jobs, hp<void>(c, ojobs), sizeof(PoseJob) * njobs);
    if (total_pts > 0) memcpy(outlier, hp<void>(c, oout), total_pts);
    return 0;
}

// ------------------------------------------------------------------ fused tracking
int svslam_track_batch(svslam_ctx *c, int njobs, svslam_track_job *jobs, const void *const *next_imgs,
                       const int *strides, int src_is_device, int total_pts, const double cam[4],
                       const float *prev_xy, float *next_xy, const uint8_t *has_mp, const double *xyz,
                       uint8_t *status, uint8_t *outlier, const svslam_lk_params *p, double chi2_th)
{
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "track: %d jobs > max_jobs", njobs);
    if (total_pts > c->lim.max_jobs * c->lim.max_pts) return fail(c, "track: too many points");
    std::vector<int> slots(njobs);
    for (int i = 0; i < njobs; ++i) {
        if (check_slot(c, jobs[i].prev_slot) || check_slot(c, jobs[i].next_slot)) return -1;
        if (jobs[i].npts < 0 || jobs[i].npts > c->lim.max_pts || jobs[i].pt_ofs < 0 ||
            jobs[i].pt_ofs + jobs[i].npts > total_pts)
            return fail(c, "track: job %d point range out of bounds", i);
        slots[i] = jobs[i].next_slot;
    }
    // 1. pyramids of the new left images (enqueue only)
    {
        const bool dec = c->src_w > 0;
        if (pyramid_common(c, njobs, slots.data(), next_imgs, strides, src_is_device, dec, dec ? c->src_w : c->geom.w[0],
                           dec ? c->src_h : c->geom.h[0], false)) return -1;
    }
    // 2. LK + pose-only back to back, single readback.  The arena region used by the
    //    pyramid job array stays live until the stream drains, so continue after it.
    int maxn = 0;
    for (int i = 0; i < njobs; ++i) maxn = std::max(maxn, jobs[i].npts);
    size_t base = c->ar.off;
    size_t olk = c->ar.take(sizeof(LkJob) * njobs);
    size_t ocam = c->ar.take(32);
    size_t oprev = c->ar.take(sizeof(float) * 2 * std::max(total_pts, 1));
    size_t omp = c->ar.take(std::max(total_pts, 1));
    size_t oxyz = c->ar.take(sizeof(double) * 3 * std::max(total_pts, 1));
    size_t opj = c->ar.take(sizeof(PoseJob) * njobs);
    size_t onext = c->ar.take(sizeof(float) * 2 * std::max(total_pts, 1));
    size_t in_end = c->ar.off;
    size_t ostat = c->ar.take(std::max(total_pts, 1));
    size_t oerr = c->ar.take(sizeof(float) * std::max(total_pts, 1));
    size_t oval = c->ar.take(std::max(total_pts, 1));
    size_t oout = c->ar.take(std::max(total_pts, 1));
    size_t ontr = c->ar.take(sizeof(int) * njobs);
    LkJob *lj = hp<LkJob>(c, olk);
    PoseJob *pj = hp<PoseJob>(c, opj);
    for (int i = 0; i < njobs; ++i) {
        lj[i].prev_slot = jobs[i].prev_slot; lj[i].next_slot = jobs[i].next_slot;
        lj[i].pt_ofs = jobs[i].pt_ofs; lj[i].npts = jobs[i].npts;
        pj[i].pt_ofs = jobs[i].pt_ofs; pj[i].npts = jobs[i].npts;
        memcpy(pj[i].pose, jobs[i].pose, 56);
        pj[i].n_inlier = 0; pj[i].pad = 0;
    }
    memcpy(hp<void>(c, ocam), cam, 32);
    if (total_pts > 0) {
        memcpy(hp<void>(c, oprev), prev_xy, sizeof(float) * 2 * total_pts);
        memcpy(hp<void>(c, onext), next_xy, sizeof(float) * 2 * total_pts);
        memcpy(hp<void>(c, omp), has_mp, total_pts);
        memcpy(hp<void>(c, oxyz), xyz, sizeof(double) * 3 * total_pts);
    }
    if (h2d(c, base, in_end)) return -1;
    if (maxn > 0) {
        tm_begin(c, FAM_LK, total_pts);
        launch_lk(c, njobs, maxn, dp<LkJob>(c, olk), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, ostat),
                  dp<float>(c, oerr), p);
        tm_end(c);
        // status && in image && has map point -> pose-only edge (src/frontend.cpp:361-371, 443-444)
        hipLaunchKernelGGL(k_track_filter, dim3(njobs), dim3(256), 0, c->stream,
                           reinterpret_cast<const LkJobView *>(dp<LkJob>(c, olk)), dp<float2>(c, onext),
                           dp<uint8_t>(c, ostat), dp<uint8_t>(c, omp), dp<uint8_t>(c, oval), dp<int>(c, ontr),
                           c->geom.w[0], c->geom.h[0]);
    }
    tm_begin(c, FAM_POSE, njobs);
    launch_pose_only(c, njobs, dp<PoseJob>(c, opj), dp<double>(c, ocam), dp<double>(c, oxyz), dp<float2>(c, onext),
                     dp<uint8_t>(c, oval), dp<uint8_t>(c, oout), chi2_th, 4, 10);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    // readback: pose jobs .. n_tracked (next_xy sits between; one contiguous copy)
    if (d2h_sync(c, opj, c->ar.off)) return -1;
    const int *ntr = hp<int>(c, ontr);
    for (int i = 0; i < njobs; ++i) {
        memcpy(jobs[i].pose, pj[i].pose, 56);
        jobs[i].n_inlier = pj[i].n_inlier;
        jobs[i].n_tracked = maxn > 0 ? ntr[i] : 0;
    }
    if (total_pts > 0) {
        memcpy(next_xy, hp<void>(c, onext), sizeof(float) * 2 * total_pts);
        memcpy(status, hp<void>(c, ostat), total_pts);
        memcpy(outlier, hp<void>(c, oout), total_pts);
    }
    return 0;
}

int svslam_rtrack_batch(svslam_ctx *c, int njobs, svslam_rtrack_job *jobs, const void *const *next_imgs,
                        const int *strides, int src_is_device, int total_pts, const double cam[4],
                        float *out_xy, int *out_mp, const svslam_lk_params *p, double chi2_th)
{
    if (njobs <= 0) return 0;
    if (c->rt.max_pts <= 0) return fail(c, "rtrack: context created with max_streams = 0");
    if (njobs > c->lim.max_jobs) return fail(c, "rtrack: %d jobs > max_jobs", njobs);
    if (total_pts > c->lim.max_jobs * c->lim.max_pts) return fail(c, "rtrack: too many points");
    std::vector<int> slots(njobs);
    for (int i = 0; i < njobs; ++i) {
        const svslam_rtrack_job &j = jobs[i];
        if (check_slot(c, j.prev_slot) || check_slot(c, j.next_slot)) return -1;
        if (j.stream < 0 || j.stream >= c->lim.max_streams) return fail(c, "rtrack: job %d stream %d out of range", i, j.stream);
        if (j.npts != c->rt_count[(size_t)j.stream])
            return fail(c, "rtrack: job %d says %d features, stream %d holds %d", i, j.npts, j.stream, c->rt_count[(size_t)j.stream]);
        if (j.pt_ofs < 0 || j.pt_ofs + j.npts > total_pts) return fail(c, "rtrack: job %d point range out of bounds", i);
        slots[i] = j.next_slot;
    }
    int maxn = 0;
    for (int i = 0; i < njobs; ++i) maxn = std::max(maxn, jobs[i].npts);
    const size_t T = (size_t)std::max(total_pts, 1);
    size_t olk = 0, ocam = 0, opj = 0, ort = 0, in_end = 0, oxy = 0, ompo = 0, out_end = 0, oprev = 0, onext = 0, omp = 0, oxyz = 0, ostat = 0,
           oerr = 0, oout = 0;
    LkJob *lj = nullptr;
    PoseJob *pj = nullptr;
    RtJob *rj = nullptr;
    // this call's inputs are staged behind the pyramid's jobs and before its launch, so that the gather can ride on it
    PyrMore more;
    more.stage = [&](RtGatherArgs *ga) -> int {
        const size_t base = c->ar.off;
        olk = c->ar.take(sizeof(LkJob) * njobs);
        ocam = c->ar.take(32);
        opj = c->ar.take(sizeof(PoseJob) * njobs);
        ort = c->ar.take(sizeof(RtJob) * njobs);
        in_end = c->ar.off;
        oxy = c->ar.take(sizeof(float) * 2 * T);        // compacted survivors for the host
        ompo = c->ar.take(sizeof(int) * T);
        out_end = c->ar.off;
        // device-only scratch of this call
        oprev = c->ar.take(sizeof(float) * 2 * T);
        onext = c->ar.take(sizeof(float) * 2 * T);
        omp = c->ar.take(T);
        oxyz = c->ar.take(sizeof(double) * 3 * T);
        ostat = c->ar.take(T);
        oerr = c->ar.take(sizeof(float) * T);
        oout = c->ar.take(T);
        if (c->ar.off > c->ar.cap) return fail(c, "rtrack: staging arena too small (%zu > %zu bytes)", c->ar.off, c->ar.cap);
        lj = hp<LkJob>(c, olk);
        pj = hp<PoseJob>(c, opj);
        rj = hp<RtJob>(c, ort);
        for (int i = 0; i < njobs; ++i) {
            const svslam_rtrack_job &j = jobs[i];
            lj[i].prev_slot = j.prev_slot; lj[i].next_slot = j.next_slot; lj[i].pt_ofs = j.pt_ofs; lj[i].npts = j.npts;
            pj[i].pt_ofs = j.pt_ofs; pj[i].npts = j.npts;
            memcpy(pj[i].pose, j.pose, 56);
            pj[i].n_inlier = 0; pj[i].pad = 0;
            rj[i].stream = j.stream; rj[i].pt_ofs = j.pt_ofs; rj[i].npts = j.npts; rj[i].src_buf = c->rt_which[(size_t)j.stream];
            memcpy(rj[i].T_cam_w, j.T_cam_w, 56);
            rj[i].n_tracked = rj[i].n_edges = rj[i].n_outlier = 0; rj[i].pad = 0;
        }
        memcpy(hp<void>(c, ocam), cam, 32);
        if (!c->zero_copy && h2d(c, base, in_end)) return -1;
        if (maxn > 0)
            *ga = RtGatherArgs{ dpz<RtJob>(c, ort), c->rt, dpz<double>(c, ocam), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, omp),
                                dp<double>(c, oxyz), njobs, cdiv(maxn, PF_THREADS) };
        return 0;
    };
    {
        const bool dec = c->src_w > 0;
        if (pyramid_common(c, njobs, slots.data(), next_imgs, strides, src_is_device, dec, dec ? c->src_w : c->geom.w[0],
                           dec ? c->src_h : c->geom.h[0], false, &more)) return -1;
    }
    if (maxn > 0) {
        if (!more.gathered)
            hipLaunchKernelGGL(k_rt_gather, dim3(cdiv(maxn, 256), njobs), dim3(256), 0, c->stream, dpz<RtJob>(c, ort), c->rt,
                               dpz<double>(c, ocam), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, omp), dp<double>(c, oxyz));
        tm_begin(c, FAM_LK, total_pts);
        launch_lk(c, njobs, maxn, dpz<LkJob>(c, olk), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, ostat),
                  dp<float>(c, oerr), p);
        tm_end(c);
    }
    // survivor filter, pose-only LM and the hand-over of the survivors in one launch (k_geom.h: k_pose_only<.., true>)
    const PoFuse fz = { dp<uint8_t>(c, ostat), dp<uint8_t>(c, omp), c->geom.w[0], c->geom.h[0], dpz<RtJob>(c, ort), c->rt,
                        dpz<float2>(c, oxy), dpz<int>(c, ompo) };
    tm_begin(c, FAM_POSE, njobs);
    launch_pose_only(c, njobs, dpz<PoseJob>(c, opj), dpz<double>(c, ocam), dp<double>(c, oxyz), dp<float2>(c, onext),
                     nullptr, dp<uint8_t>(c, oout), chi2_th, 4, 10, &fz);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    // pose jobs, rt jobs (+ the compacted survivors unless the caller keeps its map on the device and passes no buffers);
    // zero_copy: the kernels wrote them where the host reads them, only the completion is awaited
    if (c->zero_copy ? d2h_sync(c, 0, 0) : d2h_sync(c, opj, (out_xy || out_mp) ? out_end : in_end)) return -1;
    for (int i = 0; i < njobs; ++i) {
        svslam_rtrack_job &j = jobs[i];
        memcpy(j.pose, pj[i].pose, 56);
        j.n_tracked = rj[i].n_tracked; j.n_edges = rj[i].n_edges; j.n_outlier = rj[i].n_outlier;
        c->rt_which[(size_t)j.stream] ^= 1;
        c->rt_count[(size_t)j.stream] = j.n_tracked;
    }
    if (total_pts > 0) {
        if (out_xy) memcpy(out_xy, hp<void>(c, oxy), sizeof(float) * 2 * total_pts);
        if (out_mp) memcpy(out_mp, hp<void>(c, ompo), sizeof(int) * total_pts);
    }
    return 0;
}

int svslam_rtrack_upload(svslam_ctx *c, int n, const int *streams, const int *ofs, const int *counts,
                         const float *xy, const int *mp, const double *xyz)
{
    if (n <= 0) return 0;
    if (c->rt.max_pts <= 0) return fail(c, "rtrack_upload: context created with max_streams = 0");
    if (n > c->lim.max_jobs) return fail(c, "rtrack_upload: %d streams > max_jobs", n);
    int total = 0, maxc = 0;
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= c->lim.max_streams) return fail(c, "rtrack_upload: stream %d out of range", streams[i]);
        if (counts[i] < 0 || counts[i] > c->lim.max_pts) return fail(c, "rtrack_upload: %d features > max_pts %d", counts[i], c->lim.max_pts);
        total = std::max(total, ofs[i] + counts[i]); maxc = std::max(maxc, counts[i]);
    }
    if (arena_busy(c)) return -1;
    c->ar.reset();
    const size_t T = (size_t)std::max(total, 1);
    size_t oj = c->ar.take(sizeof(RtUpJob) * n);
    size_t oxy = c->ar.take(sizeof(float) * 2 * T);
    size_t omp = c->ar.take(sizeof(int) * T);
    size_t oxyz = c->ar.take(sizeof(double) * 3 * T);
    if (c->ar.off > c->ar.cap) return fail(c, "rtrack_upload: staging arena too small");
    RtUpJob *uj = hp<RtUpJob>(c, oj);
    for (int i = 0; i < n; ++i) {
        uj[i].stream = streams[i]; uj[i].ofs = ofs[i]; uj[i].count = counts[i]; uj[i].dst_buf = c->rt_which[(size_t)streams[i]];
        c->rt_count[(size_t)streams[i]] = counts[i];
    }
    if (total > 0) {
        memcpy(hp<void>(c, oxy), xy, sizeof(float) * 2 * total);
        memcpy(hp<void>(c, omp), mp, sizeof(int) * total);
        memcpy(hp<void>(c, oxyz), xyz, sizeof(double) * 3 * total);
    }
    if (h2d(c, 0, c->ar.off)) return -1;
    if (maxc > 0)
        hipLaunchKernelGGL(k_rt_store, dim3(cdiv(maxc, 256), n), dim3(256), 0, c->stream, dp<RtUpJob>(c, oj), c->rt,
                           dp<float2>(c, oxy), dp<int>(c, omp), dp<double>(c, oxyz));
    HIPCHK(c, hipGetLastError());
    return d2h_sync(c, 0, 0);       // the staging memory is reused by the next call
}

} // extern "C"
