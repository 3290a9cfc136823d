// api_ba.h — included by svslam_hip.hip.  Entry points: svslam_set_low_latency, svslam_local_ba_*, svslam_lm_trace, svslam_ba_profile,
// svslam_debug_ll_*, svslam_debug_ba_struct; the solver launchers (launch_ba_solver) are shared with the device map.
// Owns of svslam_ctx: bw, bw_jobs, ba_eid, ll, ba_pending, ba_last*, ba_host_in_order, d_ba_prof, d_lm_trace, low_latency, zero_copy.

extern "C" {

// co-resident workgroups of kernel `f` the device can hold: occupancy per CU x CUs
static int ll_resident_blocks(const void *f, size_t lds, int cus)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, BA_THREADS, lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return nb * cus;
}
static void ll_release(svslam_ctx *c)
{
    if (c->ll.shards) (void)hipFree(c->ll.shards);
    if (c->ll.xch) (void)hipFree(c->ll.xch);
    if (c->ll.cnt) (void)hipFree(c->ll.cnt);
    ba_work_free(c->ll.bw);
    c->ll.shards = nullptr; c->ll.xch = nullptr; c->ll.cnt = nullptr; c->ll.w = 0; c->ll.max_problems = 0;
}

int svslam_set_low_latency(svslam_ctx *c, int on)
{
    c->low_latency = on != 0;
    // a caller that waits for one camera's frame wants the result, not its core back: block in the
    // runtime instead of sleep-polling the event (SVSLAM_WAIT=poll|spin still overrides)
    if (!std::getenv("SVSLAM_WAIT")) c->wait_poll = !c->low_latency;
    { const char *z = std::getenv("SVSLAM_ZERO_COPY"); c->zero_copy = c->low_latency && !(z && atoi(z) == 0); }
    // one local-BA problem over several workgroups (k_ba_ll / k_local_ba_t<2>): shard descriptors, exchange area, arrival
    // counters and the per-shard solver scratch, once.  SVSLAM_LL_SHARDS = 4 | 8 | 16 (default); 0 keeps one workgroup per problem.
    if (c->low_latency && c->ll.w == 0 && c->lim.max_kf > 0 && !c->ba_host_build && ba_tile_cap_ll(c->lim.max_kf) >= std::max(c->lim.max_kf, 64)) {
        const char *e = std::getenv("SVSLAM_LL_SHARDS");
        int w = e ? atoi(e) : 16;
        if (w != 0 && w != 4 && w != 8 && w != 16) return fail(c, "SVSLAM_LL_SHARDS=%d (4, 8, 16 or 0)", w);
        if (w > 0) {
            // the resident kernel (SVSLAM_LL_RESIDENT=0: every problem through the streaming kernel, A/B and its tests)
            const char *er = std::getenv("SVSLAM_LL_RESIDENT");
            const LlCaps caps = (er && atoi(er) == 0) ? LlCaps{ 0, 0, 0 } : ba_ll_caps(c->lim.max_kf);
            HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_split), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)ba_split_lds_bytes(c->lim.max_lm, LL_MAX_W)));
            if (caps.B > 0)
                for (const void *f : { reinterpret_cast<const void *>(k_ba_ll<4, false>), reinterpret_cast<const void *>(k_ba_ll<8, false>),
                                       reinterpret_cast<const void *>(k_ba_ll<16, false>), reinterpret_cast<const void *>(k_ba_ll<4, true>),
                                       reinterpret_cast<const void *>(k_ba_ll<8, true>), reinterpret_cast<const void *>(k_ba_ll<16, true>) })
                    HIPCHK(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ba_ll_lds_bytes(c->lim.max_kf, caps)));
            // Guard of the in-launch barriers: every shard of every problem of a launch must be resident at
            // the same time.  CUs of the device (SVSLAM_LL_CUS overrides: a CU-masked process, a partitioned device whose
            // property still reports the whole chip) x the occupancy of the two solver kernels at their LDS sizes; if not even
            // one problem fits at w shards the shard count is halved, and without a fit the batch solver keeps the problems.
            int cus = 0;
            HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
            if (const char *ec = std::getenv("SVSLAM_LL_CUS")) { const int v = atoi(ec); if (v > 0) cus = std::min(cus, v); }
            int maxp = 0, per_cu = 0;
            for (; w >= 4; w /= 2) {
                // every kernel a launch at this shard count may use: both extrinsic instantiations of the resident solver have their
                // own register count (the reference's rig launches <W, true>), the streaming solver has one
                const void *fr = w == 4 ? reinterpret_cast<const void *>(k_ba_ll<4, false>) : w == 8 ? reinterpret_cast<const void *>(k_ba_ll<8, false>) : reinterpret_cast<const void *>(k_ba_ll<16, false>);
                const void *fe = w == 4 ? reinterpret_cast<const void *>(k_ba_ll<4, true>) : w == 8 ? reinterpret_cast<const void *>(k_ba_ll<8, true>) : reinterpret_cast<const void *>(k_ba_ll<16, true>);
                const void *fs = w == 4 ? reinterpret_cast<const void *>(k_local_ba_t<2, 4>) : w == 8 ? reinterpret_cast<const void *>(k_local_ba_t<2, 8>) : reinterpret_cast<const void *>(k_local_ba_t<2, 16>);
                int blocks = ll_resident_blocks(fs, ba_lds_bytes_ll(c->lim.max_kf), cus);
                if (caps.B > 0)
                    for (const void *f : { fr, fe }) blocks = std::min(blocks, ll_resident_blocks(f, ba_ll_lds_bytes(c->lim.max_kf, caps), cus));
                per_cu = cus > 0 ? blocks / cus : 0;
                maxp = std::min(SVSLAM_LL_MAX_PROBLEMS, blocks / w);
                if (maxp >= 1) break;
            }
            c->ll.cus = cus; c->ll.blocks_per_cu = per_cu;
            if (maxp < 1) return 0;               // no shard count fits: one workgroup per problem (the batch solver)
            const size_t nsh = (size_t)SVSLAM_LL_MAX_PROBLEMS * w;
            c->ll.xch_stride = ll_xch_doubles(6 * c->lim.max_kf, w);
            hipError_t er_ = hipMalloc(&c->ll.shards, sizeof(BaDev) * nsh);
            if (er_ == hipSuccess) er_ = hipMalloc(&c->ll.xch, sizeof(double) * c->ll.xch_stride * SVSLAM_LL_MAX_PROBLEMS);
            if (er_ == hipSuccess) er_ = hipMalloc(&c->ll.cnt, sizeof(unsigned int) * LL_CNT_WORDS * SVSLAM_LL_MAX_PROBLEMS);
            if (er_ == hipSuccess) er_ = hipMemset(c->ll.xch, 0, sizeof(double) * c->ll.xch_stride * SVSLAM_LL_MAX_PROBLEMS);
            if (er_ == hipSuccess) er_ = hipMemset(c->ll.cnt, 0, sizeof(unsigned int) * LL_CNT_WORDS * SVSLAM_LL_MAX_PROBLEMS);
            if (er_ == hipSuccess) er_ = ba_work_alloc(c->ll.bw, (int)nsh, c->lim.max_kf, c->lim.max_lm, c->lim.max_obs);
            if (er_ != hipSuccess) {              // nothing half-built stays behind: a later call starts over
                ll_release(c);
                return fail(c, "low-latency BA workspace allocation failed: %s", hipGetErrorString(er_));
            }
            c->ll.caps = caps;
            c->ll.w = w;
            c->ll.max_problems = maxp;
            if (const char *et = std::getenv("SVSLAM_LL_TEST_DROP_SHARD")) c->ll.test_drop = atoi(et);   // test hook, see launch_ba_solver
            if (const char *eu = std::getenv("SVSLAM_LL_TIMEOUT_US")) { const long long us = atoll(eu); if (us >= 50 && us <= 5000000) c->ll.timeout_ticks = us * 100; }
            if (const char *ecp = std::getenv("SVSLAM_LL_COOP")) c->ll.coop = atoi(ecp) != 0;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ local BA
int svslam_local_ba_submit(svslam_ctx *c, int njobs, const svslam_ba_job *jobs, const double cam_l[4],
                           const double ext_l[7], const double cam_r[4], const double ext_r[7],
                           int total_kf, const double *poses, int total_lm, const double *pts, int total_obs,
                           const int *obs_kf, const int *obs_lm, const uint8_t *obs_is_right,
                           const float *obs_uv, double huber_delta, int iters)
{
    if (njobs <= 0) return 0;
    if (njobs > c->lim.max_jobs) return fail(c, "local_ba: %d jobs > max_jobs", njobs);
    if (njobs > c->bw_jobs) return fail(c, "local_ba: %d problems in one call, this context's solver scratch holds %d (a context with the map on the device takes 64 per host-side call)", njobs, c->bw_jobs);
    // the solver scratch (c->bw, the low-latency exchange area, the LM trace) is one per context: a deferred local BA of the
    // device map that is still running on the context's second stream owns it
    if (c->dmba.inflight) return fail(c, "local_ba: a deferred local BA of the device map is in flight on this context: call svslam_dmap_ba_collect first");
    for (int i = 0; i < njobs; ++i) {
        const svslam_ba_job &j = jobs[i];
        if (j.nkf < 0 || j.nkf > c->lim.max_kf || j.nlm < 0 || j.nlm > c->lim.max_lm || j.nobs < 0 ||
            j.nobs > c->lim.max_obs || j.kf_ofs < 0 || j.kf_ofs + j.nkf > total_kf || j.lm_ofs < 0 ||
            j.lm_ofs + j.nlm > total_lm || j.obs_ofs < 0 || j.obs_ofs + j.nobs > total_obs)
            return fail(c, "local_ba: job %d exceeds limits (kf %d/%d lm %d/%d obs %d/%d)", i, j.nkf,
                        c->lim.max_kf, j.nlm, c->lim.max_lm, j.nobs, c->lim.max_obs);
    }
    const long long t_prep0 = now_ns();
    if (arena_busy(c)) return -1;
    c->ar.reset();
    c->ba_eid = ba_ext_identity(ext_l, ext_r);
    static_assert(sizeof(BaJob) == sizeof(svslam_ba_job), "job layout");
    const size_t TO = (size_t)std::max(total_obs, 1);
    const bool use_ll = !c->ba_host_build && ba_ll_usable(c, njobs);
    const int tile_cap = use_ll ? ba_ll_tile_cap(c) : ba_tile_cap(c->lim.max_kf);     // (reservations: the smaller tiles need more room)
    // arena: cams | jobs | poses | points | [raw edges + order (device build)] | chi2 + flag (out) |
    //        records | aux  (records and aux are device-only when the device builds the structure)
    size_t ocams = c->ar.take(sizeof(BaCams));
    size_t opk_o = 0, ouv_o = 0, osrt_o = 0;
    if (!c->ba_host_build) {
        opk_o = c->ar.take(sizeof(unsigned int) * TO); osrt_o = c->ar.take(sizeof(int) * TO);
        ouv_o = c->ar.take(sizeof(float) * 2 * TO);
    }
    size_t ojobs = c->ar.take(sizeof(BaDev) * njobs);          // read back from here ...
    size_t oposes = c->ar.take(sizeof(double) * 7 * std::max(total_kf, 1));
    size_t opts = c->ar.take(sizeof(double) * 3 * std::max(total_lm, 1));
    size_t in_end = c->ar.off;
    size_t ochi = c->ar.take(sizeof(double) * TO);
    size_t oflag = c->ar.take(sizeof(int) * 4);
    size_t out_end = c->ar.off;
    size_t orecs = c->ar.take(sizeof(BaRec) * 2 * TO);   // landmark-major + pose-major edge records
    size_t oaux = c->ar.take(0);
    if (oaux > c->ar.cap) return fail(c, "local_ba: staging arena too small (%zu > %zu bytes)", oaux, c->ar.cap);
    BaCams *cams = hp<BaCams>(c, ocams);
    memcpy(cams->cam[0], cam_l, 32); memcpy(cams->cam[1], cam_r, 32);
    memcpy(cams->ext[0], ext_l, 56); memcpy(cams->ext[1], ext_r, 56);
    BaDev *dj = hp<BaDev>(c, ojobs);
    hp<int>(c, oflag)[0] = 0;
    size_t aux_total = 0;
    int max_nlm = 1, max_nobs = 1;
    bool all_sorted = true;
    if (c->ba_host_build) {
        c->ba_host_in_order.assign((size_t)njobs, 0);
        // Host-side structure of every problem (edge records, blocks, pose-pair lists), built by the
        // pool with one scratch structure per thread (stays cache-hot) and written straight into the
        // arena; the aux space of a problem comes from a bump allocator, so its position depends on
        // thread timing but nothing else does (every problem carries its own offsets).
        std::vector<int> bad((size_t)njobs, 0);
        std::atomic<size_t> bump{ 0 };
        const size_t aux_cap_ints = (c->ar.cap - oaux) / sizeof(int);
        int *aux = hp<int>(c, oaux);
        BaRec *recs = hp<BaRec>(c, orecs);
        auto build_one = [&](int i) {
            static thread_local BaHostStruct hs;
            BaJob bj;
            memcpy(&bj, &jobs[i], sizeof(bj));
            if (!hs.build(bj, obs_kf, obs_lm, obs_is_right, obs_uv, tile_cap)) { bad[(size_t)i] = 1; return; }   // index out of range
            const size_t need = hs.aux_ints(bj);
            const size_t at = bump.fetch_add(need);
            if (at + need > aux_cap_ints) { bad[(size_t)i] = 2; return; }
            hs.write(bj, aux + at, recs + 2 * (size_t)bj.obs_ofs, dj[i]);
            dj[i].aux_ofs = (int)at;
            dj[i].rec_ofs = 2 * bj.obs_ofs;
            c->ba_host_in_order[(size_t)i] = hs.in_order ? 1 : 0;
        };
        if (c->pool && njobs > 1) c->pool->parallel_for(njobs, build_one);
        else for (int i = 0; i < njobs; ++i) build_one(i);
        for (int i = 0; i < njobs; ++i) {
            if (bad[(size_t)i] == 1) return fail(c, "local_ba: job %d has an edge index out of range", i);
            if (bad[(size_t)i] == 2) return fail(c, "local_ba: staging arena too small for the problem structure");
        }
        aux_total = bump.load();
        (void)c->ar.take(sizeof(int) * aux_total);
    } else {
        // The device builds the structure (k_ba_build).  One pass of the pool over the problems validates the
        // edge indices, packs them (landmark | keyframe << 16 | camera << 24: 4 bytes per edge instead of 9),
        // notes whether they arrive in (landmark, keyframe) order — the order the backend gathers them in
        // (src/backend.cpp:83-160); a stable sort otherwise — and copies the problem's measurements, poses and
        // positions into the staging arena: every input byte is touched once, by the thread that has it in cache.
        std::vector<int> bad((size_t)njobs, 0);
        int *srt = hp<int>(c, osrt_o);
        unsigned int *pk = hp<unsigned int>(c, opk_o);
        float *auv = hp<float>(c, ouv_o);
        double *aposes = hp<double>(c, oposes), *apts = hp<double>(c, opts);
        auto check_one = [&](int i) {
            const svslam_ba_job &j = jobs[i];
            const int *kf = obs_kf + j.obs_ofs, *lm = obs_lm + j.obs_ofs;
            const uint8_t *rt = obs_is_right + j.obs_ofs;
            unsigned int *pj = pk + j.obs_ofs;
            bool sorted = true;
            for (int e = 0; e < j.nobs; ++e) {
                const int k = kf[e], l = lm[e];
                if (k < 0 || k >= j.nkf || l < 0 || l >= j.nlm) { bad[(size_t)i] = 1; return; }
                if (e && !((lm[e - 1] < l) || (lm[e - 1] == l && kf[e - 1] <= k))) sorted = false;
                pj[e] = (unsigned int)l | ((unsigned int)k << 16) | ((rt[e] ? 1u : 0u) << 24);
            }
            if (!sorted) {
                int *sr = srt + j.obs_ofs;
                for (int e = 0; e < j.nobs; ++e) sr[e] = e;
                std::stable_sort(sr, sr + j.nobs, [&](int a, int b) { return lm[a] != lm[b] ? lm[a] < lm[b] : kf[a] < kf[b]; });
            }
            if (j.nobs) memcpy(auv + 2 * (size_t)j.obs_ofs, obs_uv + 2 * (size_t)j.obs_ofs, sizeof(float) * 2 * j.nobs);
            if (j.nkf) memcpy(aposes + 7 * (size_t)j.kf_ofs, poses + 7 * (size_t)j.kf_ofs, sizeof(double) * 7 * j.nkf);
            if (j.nlm) memcpy(apts + 3 * (size_t)j.lm_ofs, pts + 3 * (size_t)j.lm_ofs, sizeof(double) * 3 * j.nlm);
            dj[i].reserved = sorted ? 1 : 0;
        };
        if (c->pool && njobs > 1) c->pool->parallel_for(njobs, check_one);
        else for (int i = 0; i < njobs; ++i) check_one(i);
        size_t at = 0;
        for (int i = 0; i < njobs; ++i) {
            if (bad[(size_t)i]) return fail(c, "local_ba: job %d has an edge index out of range", i);
            const svslam_ba_job &j = jobs[i];
            BaDev &d = dj[i];
            d.kf_ofs = j.kf_ofs; d.nkf = j.nkf; d.lm_ofs = j.lm_ofs; d.nlm = j.nlm; d.obs_ofs = j.obs_ofs; d.nobs = j.nobs;
            d.nblk = d.na = d.ncontrib = d.ntile = 0; d.iters_done = 0; d.nmv = 0;
            d.rec_ofs = 2 * j.obs_ofs;
            d.lay_nblk = j.nobs; d.lay_na = j.nkf; d.lay_ntile = ba_tile_bound(j.nlm, j.nobs, j.nkf, tile_cap);
            d.aux_ofs = (int)at; d.lm_base = 0; d.shmask = 0; d.ntrial = 0;
            at += ba_aux_layout(j.nkf, j.nlm, j.nobs, d.lay_nblk, d.lay_na, 0, d.lay_ntile).total + ba_pitem_bound(j.nobs, j.nkf);
            if (use_ll) at += ba_split_aux_extra(j.nkf, c->ll.w);
            if (!d.reserved) all_sorted = false;
            max_nlm = std::max(max_nlm, j.nlm); max_nobs = std::max(max_nobs, j.nobs);
        }
        aux_total = at;
        (void)c->ar.take(sizeof(int) * aux_total);
        if (c->ar.off > c->ar.cap) return fail(c, "local_ba: staging arena too small for the problem structure (%zu > %zu bytes)", c->ar.off, c->ar.cap);
    }
    if (c->ba_host_build) {
        if (total_kf > 0) memcpy(hp<void>(c, oposes), poses, sizeof(double) * 7 * total_kf);
        if (total_lm > 0) memcpy(hp<void>(c, opts), pts, sizeof(double) * 3 * total_lm);
    }
    c->host_ns[4] += now_ns() - t_prep0;
    if (h2d(c, 0, in_end)) return -1;
    if (h2d(c, oflag, oflag + sizeof(int) * 4)) return -1;
    if (c->ba_host_build) { if (h2d(c, orecs, c->ar.off)) return -1; }
    if (c->d_lm_trace) HIPCHK(c, hipMemsetAsync(c->d_lm_trace, 0, sizeof(double) * LM_TRACE_STRIDE * (size_t)njobs, c->stream));
    tm_begin(c, c->timing_split ? FAM_DBG2 : FAM_BA, njobs);
    if (!c->ba_host_build)
        launch_ba_solver(c, njobs, use_ll && all_sorted, dp<BaDev>(c, ojobs), dp<BaCams>(c, ocams), dp<double>(c, oposes), dp<double>(c, opts),
                         dp<unsigned int>(c, opk_o), dp<float2>(c, ouv_o), dp<int>(c, osrt_o), dp<BaRec>(c, orecs), dp<int>(c, oaux),
                         dp<double>(c, ochi), dp<int>(c, oflag), max_nlm, max_nobs, huber_delta, iters, c->timing_split);
    else
        hipLaunchKernelGGL((k_local_ba_t<0, 1, false>), dim3(njobs), dim3(BA_THREADS), ba_lds_bytes(c->lim.max_kf), c->stream,
                           dp<BaDev>(c, ojobs), dp<BaCams>(c, ocams), dp<double>(c, oposes), dp<double>(c, opts),
                           dp<BaRec>(c, orecs), dp<int>(c, oaux), c->bw, huber_delta, iters, dp<double>(c, ochi), c->d_ba_prof,
                           tile_cap, SbaArgs{ 0, 0, 0.0, nullptr, c->d_lm_trace, 0, nullptr, nullptr, nullptr, 0, 0 });
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    c->ba_pending.oflag = oflag;
    if (d2h_enqueue(c, ojobs, out_end)) return -1;
    c->ba_pending.active = true; c->ba_pending.njobs = njobs;
    c->ba_pending.total_kf = total_kf; c->ba_pending.total_lm = total_lm; c->ba_pending.total_obs = total_obs;
    c->ba_pending.ojobs = ojobs; c->ba_pending.oposes = oposes; c->ba_pending.opts = opts; c->ba_pending.ochi = ochi;
    c->ba_pending.ll_used = !c->ba_host_build && use_ll && all_sorted;
    if (c->ba_pending.ll_used) {
        c->ba_pending.ocams = ocams; c->ba_pending.opk = opk_o; c->ba_pending.ouv = ouv_o; c->ba_pending.osrt = osrt_o; c->ba_pending.orecs = orecs;
        c->ba_pending.oaux = oaux; c->ba_pending.out_end = out_end; c->ba_pending.max_nlm = max_nlm; c->ba_pending.max_nobs = max_nobs;
        c->ba_pending.iters = iters; c->ba_pending.delta = huber_delta;
        // the descriptors as uploaded, re-tiled for the batch solver (larger tiles: the aux room reserved for the smaller ones holds them)
        c->ll.saved.assign(dj, dj + njobs);        // (dj: the host arena; the read-back below overwrites it)
        for (int i = 0; i < njobs; ++i) c->ll.saved[(size_t)i].lay_ntile = ba_tile_bound(jobs[i].nlm, jobs[i].nobs, jobs[i].nkf, ba_tile_cap(c->lim.max_kf));
    }
    return 0;
}

int svslam_local_ba_collect(svslam_ctx *c, int njobs, svslam_ba_job *jobs, int total_kf, double *poses,
                            int total_lm, double *pts, int total_obs, double *edge_chi2)
{
    if (!c->ba_pending.active) return njobs <= 0 ? 0 : fail(c, "local_ba_collect: nothing submitted");
    if (njobs != c->ba_pending.njobs || total_kf != c->ba_pending.total_kf || total_lm != c->ba_pending.total_lm ||
        total_obs != c->ba_pending.total_obs)
        return fail(c, "local_ba_collect: sizes differ from the submitted batch");
    c->ba_pending.active = false;
    if (finish(c)) return -1;
    if (const int fl = hp<int>(c, c->ba_pending.oflag)[0])
        return fail(c, "local_ba: the device structure build overflowed a capacity (code %d)", fl);
    const BaDev *dj = hp<BaDev>(c, c->ba_pending.ojobs);
    std::vector<int> bad;
    for (int i = 0; i < njobs; ++i) if (dj[i].iters_done < 0) bad.push_back(i);
    std::vector<BaDev> &res = c->ba_last;          // descriptors as the first solve returned them (kept for svslam_debug_ba_struct)
    res.assign(dj, dj + njobs);
    if (!bad.empty()) {
        // a shard of the low-latency solver never became resident.  A problem that gives up writes nothing back, so ITS inputs are
        // untouched in the device arena; the problems that finished have their results there already (poses and positions are
        // updated in place) and must not be solved a second time (20 LM iterations instead of the reference's 10).
        // Only the problems that gave up go to the batch solver — one workgroup per problem, no barrier — as a compacted list:
        // every descriptor carries its own offsets into the arena.
        if (!c->ba_pending.ll_used || (int)c->ll.saved.size() != njobs) return fail(c, "local_ba: a problem reports iters_done < 0 outside the low-latency solver");
        const auto &bp = c->ba_pending;
        const int nb = (int)bad.size();
        BaDev *hj = hp<BaDev>(c, bp.ojobs);
        int max_nlm = 1, max_nobs = 1;
        for (int k = 0; k < nb; ++k) {
            hj[k] = c->ll.saved[(size_t)bad[(size_t)k]];
            max_nlm = std::max(max_nlm, hj[k].nlm); max_nobs = std::max(max_nobs, hj[k].nobs);
        }
        hp<int>(c, bp.oflag)[0] = 0;
        if (h2d(c, bp.ojobs, bp.ojobs + sizeof(BaDev) * (size_t)nb)) return -1;
        if (h2d(c, bp.oflag, bp.oflag + sizeof(int) * 4)) return -1;
        launch_ba_solver(c, nb, false, dp<BaDev>(c, bp.ojobs), dp<BaCams>(c, bp.ocams), dp<double>(c, bp.oposes), dp<double>(c, bp.opts),
                         dp<unsigned int>(c, bp.opk), dp<float2>(c, bp.ouv), dp<int>(c, bp.osrt), dp<BaRec>(c, bp.orecs), dp<int>(c, bp.oaux),
                         dp<double>(c, bp.ochi), dp<int>(c, bp.oflag), max_nlm, max_nobs, bp.delta, bp.iters, false);
        HIPCHK(c, hipGetLastError());
        if (d2h_sync(c, bp.ojobs, bp.out_end)) return -1;
        if (const int fl = hp<int>(c, bp.oflag)[0]) return fail(c, "local_ba: the device structure build overflowed a capacity (code %d)", fl);
        for (int k = 0; k < nb; ++k) res[(size_t)bad[(size_t)k]] = dj[k];
        c->ll.fallbacks += nb;
    }
    for (int i = 0; i < njobs; ++i) {
        const BaDev &d = res[(size_t)i];
        if (d.iters_done < 0) return fail(c, "local_ba: job %d reports iters_done < 0 from the batch solver", i);
        jobs[i].iters_done = d.iters_done;
        jobs[i].reserved = (int)(((unsigned)std::min(d.ntrial, 255) << 24) | ((unsigned)d.ncontrib & 0x00ffffffu));   // accounting (svslam.h)
    }
    if (total_kf > 0) memcpy(poses, hp<void>(c, c->ba_pending.oposes), sizeof(double) * 7 * total_kf);
    if (total_lm > 0) memcpy(pts, hp<void>(c, c->ba_pending.opts), sizeof(double) * 3 * total_lm);
    if (total_obs > 0) memcpy(edge_chi2, hp<void>(c, c->ba_pending.ochi), sizeof(double) * total_obs);
    return 0;
}

int svslam_local_ba_batch(svslam_ctx *c, int njobs, svslam_ba_job *jobs, const double cam_l[4],
                          const double ext_l[7], const double cam_r[4], const double ext_r[7],
                          int total_kf, double *poses, int total_lm, double *pts, int total_obs,
                          const int *obs_kf, const int *obs_lm, const uint8_t *obs_is_right,
                          const float *obs_uv, double huber_delta, int iters, double *edge_chi2)
{
    if (njobs <= 0) return 0;
    if (int rc = svslam_local_ba_submit(c, njobs, jobs, cam_l, ext_l, cam_r, ext_r, total_kf, poses, total_lm, pts,
                                        total_obs, obs_kf, obs_lm, obs_is_right, obs_uv, huber_delta, iters))
        return rc;
    return svslam_local_ba_collect(c, njobs, jobs, total_kf, poses, total_lm, pts, total_obs, edge_chi2);
}

// test hook: the shard descriptors of the last low-latency local-BA call (k_ba_split / k_ba_build): 8 ints per shard —
// landmarks, edges, blocks, tiles, solver (2: resident kernel k_ba_ll, 1: streaming k_local_ba_t<2>), active poses, mask of shards with edges, iterations
int svslam_debug_ll_limits(svslam_ctx *c, int *out4)
{
    out4[0] = c->ll.w; out4[1] = c->ll.max_problems; out4[2] = c->ll.cus; out4[3] = c->ll.blocks_per_cu;
    return 0;
}
int svslam_debug_ll_shards(svslam_ctx *c, int nproblems, int *out8, int *shards_per_problem)
{
    if (shards_per_problem) *shards_per_problem = c->ll.w;
    if (!c->ll.shards || nproblems < 1 || nproblems > SVSLAM_LL_MAX_PROBLEMS) return fail(c, "debug_ll_shards: no low-latency solver / bad count");
    std::vector<BaDev> h((size_t)nproblems * c->ll.w);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h.data(), c->ll.shards, sizeof(BaDev) * h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) {
        int *o = out8 + 8 * i;
        o[0] = h[i].nlm; o[1] = h[i].nobs; o[2] = h[i].nblk; o[3] = h[i].ntile; o[4] = h[i].reserved; o[5] = h[i].na; o[6] = h[i].shmask; o[7] = h[i].iters_done;
    }
    return 0;
}

// test hook: the problem descriptors of the last svslam_local_ba_batch / _collect as the batch solver returned them, 8 ints per
// problem — blocks, active poses, block pairs, tiles, landmarks in the tiles (nmv), iterations, LM trials, flags (bit 0: the edges
// arrived landmark-major with keyframes ascending; bit 1: the edge_cache argument of the last k_ba_build launch; bit 2: structure
// built on the host).  After a call the low-latency solver took, the counts are those of the parents' descriptors, which carry
// none but iterations, trials and block pairs: use svslam_debug_ll_shards there.
int svslam_debug_ba_struct(svslam_ctx *c, int njobs, int *out8)
{
    if (njobs < 1 || (size_t)njobs != c->ba_last.size()) return fail(c, "debug_ba_struct: the last local-BA call had %zu problems, not %d", c->ba_last.size(), njobs);
    for (int i = 0; i < njobs; ++i) {
        const BaDev &d = c->ba_last[(size_t)i];
        int *o = out8 + 8 * (size_t)i;
        o[0] = d.nblk; o[1] = d.na; o[2] = d.ncontrib; o[3] = d.ntile; o[4] = d.nmv; o[5] = d.iters_done; o[6] = d.ntrial;
        if (c->ba_host_build) o[7] = 4 | ((size_t)i < c->ba_host_in_order.size() && c->ba_host_in_order[(size_t)i] ? 1 : 0);
        else o[7] = (d.reserved ? 1 : 0) | (c->ba_last_ec ? 2 : 0);      // (reserved: the host's in-order mark, which the batch kernels leave alone)
    }
    return 0;
}

// test hook: per-phase cycle counters of BA job 0 (wall_clock64 ticks, 100 MHz)
int svslam_ba_profile(svslam_ctx *c, int enable, long long *out12)
{
    if (enable && !c->d_ba_prof) {
        HIPCHK(c, hipMalloc(&c->d_ba_prof, sizeof(long long) * (BA_PROF_N + 4)));
        HIPCHK(c, hipMemset(c->d_ba_prof, 0, sizeof(long long) * (BA_PROF_N + 4)));
    }
    if (out12 && c->d_ba_prof) {
        long long all[BA_PROF_N + 4];
        HIPCHK(c, hipMemcpy(all, c->d_ba_prof, sizeof(all), hipMemcpyDeviceToHost));
        memcpy(out12, all, sizeof(long long) * BA_PROF_N);
        // development (-DBA_CHOL_PROF builds): wave 0's clocks inside the factorisation — wait at the top of a block column,
        // its share of the trailing update, factor + panel of the next column, wait at the column's barrier
        if (std::getenv("SVSLAM_BA_PROF_EXTRA"))
            fprintf(stderr, "[chol wave 0, us] top %.1f  trail %.1f  factor+panel %.1f  barrier %.1f\n", all[12] / 100.0, all[13] / 100.0, all[14] / 100.0, all[15] / 100.0);
        HIPCHK(c, hipMemset(c->d_ba_prof, 0, sizeof(long long) * (BA_PROF_N + 4)));
    }
    if (!enable && c->d_ba_prof) { (void)hipFree(c->d_ba_prof); c->d_ba_prof = nullptr; }
    return 0;
}

// test hook: the LM trajectory of the last pose-only / local-BA call (every trial, rejected ones included), job by job.
// enable = 1 allocates the buffer (the kernels then record), 0 frees it; out != NULL copies job `job`'s records
// (6 doubles each: iteration [pose-only: 16 round + iteration], lambda, chi2 before, chi2 of the trial, rho, accepted).
int svslam_lm_trace(svslam_ctx *c, int enable, int job, double *out, int cap_records, int *n_records)
{
    if (enable && !c->d_lm_trace) {
        HIPCHK(c, hipMalloc(&c->d_lm_trace, sizeof(double) * LM_TRACE_STRIDE * (size_t)c->lim.max_jobs));
        HIPCHK(c, hipMemset(c->d_lm_trace, 0, sizeof(double) * LM_TRACE_STRIDE * (size_t)c->lim.max_jobs));
    }
    if (out && c->d_lm_trace) {
        if (job < 0 || job >= c->lim.max_jobs) return fail(c, "lm_trace: job %d out of range", job);
        std::vector<double> t(LM_TRACE_STRIDE);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(t.data(), c->d_lm_trace + (size_t)job * LM_TRACE_STRIDE, sizeof(double) * LM_TRACE_STRIDE, hipMemcpyDeviceToHost));
        const int n = std::min((int)t[0], cap_records);
        if (n_records) *n_records = n;
        if (n > 0) memcpy(out, t.data() + 8, sizeof(double) * LM_TRACE_REC * (size_t)n);
    } else if (n_records) *n_records = 0;
    if (!enable && c->d_lm_trace) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->d_lm_trace); c->d_lm_trace = nullptr; }
    return 0;
}

} // extern "C"
