// api_orb_desc.h — the ORB descriptors' entry point of the C ABI (part of svslam_hip.hip's translation unit):
// svslam_orb_describe_batch.  Owns of svslam_ctx: orbd.  Every host rule is od_plan's (k_orb_desc.h); this file reserves the buffer,
// uploads, enqueues the kernels of a chunk in the order tests/cpp/orb_desc_host_emu restates, and copies out.
static_assert(sizeof(OdParams) == sizeof(svslam_orb_desc_params), "k_orb_desc.h mirrors the ABI's structs");

extern "C" {

int svslam_orb_describe_batch(svslam_ctx *c, int njobs, svslam_orb_desc_job *jobs, const svslam_orb_desc_params *prm, int total_pts,
                              const svslam_orb_kp *kps, uint8_t *desc, int *desc_pt)
{
    if (!c) return -1;
    if (njobs < 0 || total_pts < 0) return fail(c, "orb_desc: negative count");
    if (!prm) return fail(c, "orb_desc: null params");
    if (njobs && !jobs) return fail(c, "orb_desc: null jobs");
    if (total_pts && (!kps || !desc || !desc_pt)) return fail(c, "orb_desc: null array");
    if (arena_busy(c)) return -1;
    std::vector<OdJob> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = OdJob{ jobs[j].slot, jobs[j].pt_ofs, jobs[j].npts, 0 };
    size_t budget = ORB_BUDGET_DEFAULT;
    if (const char *e = std::getenv("SVSLAM_ORB_BUDGET_MB")) { const long v = atol(e); if (v >= 1 && v <= (1L << 20)) budget = (size_t)v << 20; }     // development and tests: the chunking
    OdPlan &P = c->orbd.plan;
    const OdParams pp{ prm->pattern, prm->edge, prm->nlevels, 0 };
    const char *why = od_plan(P, c->geom.w[0], c->geom.h[0], c->lim.max_slots, njobs, in.data(), &pp, total_pts,
                              reinterpret_cast<const OrbKp *>(kps), budget);
    if (why) return fail(c, "orb_desc: %s", why);
    if (njobs == 0) return 0;
    const OdGeom &G = P.G;
    const OrbImg I = level0_view<OrbImg>(c);
    size_t most = 0, most_host = 0;
    for (OdChunk &C : P.chunks) {
        (void)od_layout(P, C, nullptr);
        most = std::max(most, C.bytes);
        most_host = std::max(most_host, C.result_ofs + C.result_bytes);
    }
    if (c->orbd.reserve(c, "orb_desc", most, 0, most_host)) return -1;
    for (OdChunk &C : P.chunks) {
        // the host mirror holds the uploaded part and the results; the pointers behind them are never followed on the host
        const OdBuf Hb = od_layout(P, C, c->orbd.h.data());
        const OdBuf Db = od_layout(P, C, c->orbd.d);
        od_fill(P, C, Hb, in.data(), reinterpret_cast<const OrbKp *>(kps));
        HIPCHK(c, hipMemcpyAsync(c->orbd.d, c->orbd.h.data(), C.upload_bytes, hipMemcpyHostToDevice, c->stream));
        long long units = 0;
        for (int j = C.j0; j < C.j0 + C.n; ++j) units += in[(size_t)j].npts;
        tm_begin(c, FAM_ORBD, units);
        for (int l = 1; l <= G.lmax; ++l) {
            const unsigned nt = (unsigned)((G.L[l].w * G.L[l].h + 3) / 4);
            hipLaunchKernelGGL(k_orbd_resize, dim3((nt + BR_THREADS - 1) / BR_THREADS, C.n), dim3(BR_THREADS), 0, c->stream, I, Db, l);
        }
        hipLaunchKernelGGL(k_orbd_filter, dim3(C.n), dim3(BR_THREADS), 0, c->stream, Db);
        if (C.npts)
            hipLaunchKernelGGL(k_orbd_describe, dim3((C.npts + BR_ROWS_PER_WG - 1) / BR_ROWS_PER_WG), dim3(BR_THREADS),
                               (size_t)P.lds.wave_bytes * BR_ROWS_PER_WG, c->stream, I, Db, P.lds);
        tm_end(c);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->orbd.h.data() + C.result_ofs, c->orbd.d + C.result_ofs, C.result_bytes, hipMemcpyDeviceToHost, c->stream));
        if (d2h_sync(c, 0, 0)) return -1;
        od_copy_out(C, Hb, in.data(), desc, desc_pt);
    }
    for (int j = 0; j < njobs; ++j) jobs[j].n_desc = in[(size_t)j].n_desc;
    return 0;
}

} // extern "C"
