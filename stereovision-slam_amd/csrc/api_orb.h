// api_orb.h — the ORB detector's entry points of the C ABI (part of svslam_hip.hip's translation unit):
// svslam_orb_detect_batch, svslam_orb_read_level.  Owns of svslam_ctx: orb.  Every host rule is orb_plan's (k_orb.h); this file
// reserves the buffer, uploads, enqueues the kernels of a chunk in the order tests/cpp/orb_host_emu restates, and copies out.
static_assert(sizeof(OrbKp) == sizeof(svslam_orb_kp) && sizeof(OrbParams) == sizeof(svslam_orb_params), "k_orb.h mirrors the ABI's structs");

extern "C" {

int svslam_orb_detect_batch(svslam_ctx *c, int njobs, svslam_orb_job *jobs, const svslam_orb_params *prm, int total_rects,
                            const float *rect_xy, int max_out, svslam_orb_kp *out)
{
    if (!c) return -1;
    if (njobs < 0 || total_rects < 0) return fail(c, "orb: negative count");
    if (!prm) return fail(c, "orb: null params");
    if (njobs && (!jobs || !out)) return fail(c, "orb: null array");
    if (total_rects && !rect_xy) return fail(c, "orb: null rects");
    if (arena_busy(c)) return -1;
    std::vector<OrbJob> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = OrbJob{ jobs[j].slot, jobs[j].rect_ofs, jobs[j].nrect };
    size_t budget = ORB_BUDGET_DEFAULT;
    if (const char *e = std::getenv("SVSLAM_ORB_BUDGET_MB")) { const long v = atol(e); if (v >= 1 && v <= (1L << 20)) budget = (size_t)v << 20; }     // development and tests: the chunking
    OrbPlan &P = c->orb.plan;
    c->orb.have = false;
    const OrbParams pp{ prm->nfeatures, prm->nlevels, prm->fast_threshold, prm->edge };
    const char *why = orb_plan(P, c->geom.w[0], c->geom.h[0], c->lim.max_slots, njobs, in.data(), &pp, total_rects, max_out, budget);
    if (why) return fail(c, "orb: %s", why);
    if (njobs == 0) return 0;
    const OrbGeom &G = P.G;
    const OrbImg I = level0_view<OrbImg>(c);
    size_t most = 0;
    for (OrbChunk &C : P.chunks) { (void)orb_layout(P, C, nullptr); most = std::max(most, C.bytes); }
    if (c->orb.reserve(c, "orb", most, 0, 0)) return -1;
    std::vector<int> n_out((size_t)njobs), n_found((size_t)njobs);
    for (OrbChunk &C : P.chunks) {
        try { if (c->orb.h.size() < C.hist_ofs) c->orb.h.resize(C.hist_ofs); }
        catch (const std::bad_alloc &) { return fail(c, "orb: no host memory for %zu bytes", C.hist_ofs); }
        // the host mirror holds the uploaded part and the results; the pointers behind them are never followed on the host
        const OrbBuf Hb = orb_layout(P, C, c->orb.h.data());
        const OrbBuf Db = orb_layout(P, C, c->orb.d);
        const int nr = orb_fill(P, C, Hb, in.data(), rect_xy);
        HIPCHK(c, hipMemcpyAsync(c->orb.d, c->orb.h.data(), C.upload_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->orb.d + C.hist_ofs, 0, C.hist_bytes, c->stream));
        tm_begin(c, FAM_ORB, C.n);
        const unsigned n16 = (unsigned)(orb_up16((size_t)G.L[0].w * G.L[0].h) / 16);
        hipLaunchKernelGGL(k_orb_fill, dim3((n16 + ORB_THREADS - 1) / ORB_THREADS, C.n), dim3(ORB_THREADS), 0, c->stream, Db);
        if (nr) hipLaunchKernelGGL(k_orb_rects, dim3(nr), dim3(ORB_THREADS), 0, c->stream, Db);
        for (int l = 1; l < G.nlevels; ++l) {
            const unsigned nt = (unsigned)((G.L[l].w * G.L[l].h + 3) / 4);
            hipLaunchKernelGGL(k_orb_resize, dim3((nt + ORB_THREADS - 1) / ORB_THREADS, C.n, 2), dim3(ORB_THREADS), 0, c->stream, I, Db, l);
        }
        for (int l = 0; l < G.nlevels; ++l)
            if (G.L[l].active)
                hipLaunchKernelGGL(k_orb_fast, dim3(G.L[l].tiles_x * G.L[l].tiles_y, C.n), dim3(ORB_THREADS), 0, c->stream, I, Db, l);
        hipLaunchKernelGGL(k_orb_select, dim3(G.nlevels, C.n), dim3(ORB_THREADS), 0, c->stream, I, Db);
        hipLaunchKernelGGL(k_orb_emit, dim3(G.nlevels, C.n), dim3(ORB_THREADS), 0, c->stream, I, Db);
        tm_end(c);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->orb.h.data() + C.result_ofs, c->orb.d + C.result_ofs, C.result_bytes, hipMemcpyDeviceToHost, c->stream));
        if (d2h_sync(c, 0, 0)) return -1;
        orb_copy_out(P, C, Hb, n_out.data(), n_found.data(), reinterpret_cast<OrbKp *>(out));
    }
    for (int j = 0; j < njobs; ++j) { jobs[j].n_out = n_out[(size_t)j]; jobs[j].n_found = n_found[(size_t)j]; }
    c->orb.have = true;
    return 0;
}

int svslam_orb_read_level(svslam_ctx *c, int job, int level, uint8_t *img, uint8_t *mask, int *w, int *h)
{
    if (!c) return -1;
    if (!c->orb.have || c->orb.plan.chunks.empty()) return fail(c, "orb_read_level: no call has left its levels");
    if (!w || !h) return fail(c, "orb_read_level: null size");
    OrbPlan &P = c->orb.plan;
    OrbChunk C = P.chunks.back();
    const OrbGeom &G = P.G;
    if (level < 0 || level >= G.nlevels) return fail(c, "orb_read_level: level %d out of range [0,%d)", level, G.nlevels);
    if (job < C.j0 || job >= C.j0 + C.n) return fail(c, "orb_read_level: job %d is not in the last chunk [%d,%d) of the last call", job, C.j0, C.j0 + C.n);
    const OrbBuf Db = orb_layout(P, C, c->orb.d);
    const OrbLevel &L = G.L[level];
    *w = L.w; *h = L.h;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned char *blk = Db.blocks + (size_t)(job - C.j0) * G.job_bytes;
    if (img) {
        if (level == 0) {
            std::vector<OrbDevJob> dj((size_t)C.n);
            HIPCHK(c, hipMemcpy(dj.data(), Db.jobs, sizeof(OrbDevJob) * (size_t)C.n, hipMemcpyDeviceToHost));
            const OrbImg I = level0_view<OrbImg>(c);
            HIPCHK(c, hipMemcpy2D(img, (size_t)L.w, I.base + (size_t)dj[(size_t)(job - C.j0)].slot * I.slot_bytes + I.origin, (size_t)I.pitch,
                                  (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
        } else HIPCHK(c, hipMemcpy(img, blk + L.img, (size_t)L.w * L.h, hipMemcpyDeviceToHost));
    }
    if (mask) HIPCHK(c, hipMemcpy(mask, blk + L.mask, (size_t)L.w * L.h, hipMemcpyDeviceToHost));
    return 0;
}

} // extern "C"
