// api_dmap.h — included by svslam_hip.hip.  Entry points: svslam_dmap_*, svslam_debug_dmap_* (with DbgBufs), svslam_debug_rtrack_read.
// Owns of svslam_ctx: dm, dm_all, dm_stamp, dm_seen, dm_seen_gen, evicted, dmba.

extern "C" {

// ------------------------------------------------------------------ the launches of the device map's kernels
// One function per kernel: dmap_keyframe_impl, svslam_dmap_ba_collect and the stage hook of the tests (svslam_debug_dmap_stage)
// launch through these, so a kernel that a test runs alone has the launch shape and the LDS size of the keyframe path.
static void dm_launch_begin(svslam_ctx *c, int njobs, DmJob *dj, DmEvicted *ev, int *ev_cursor, int ev_quota)
{
    hipLaunchKernelGGL(k_dmap_begin, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, c->rt, ev, ev_cursor, ev_quota);
}
static void dm_launch_stereo_prep(svslam_ctx *c, int njobs, DmJob *dj, const DmParams &prm, const float2 *corners, const int *ncorners, int max_corners,
                                  LkJob *lkjobs, float2 *prev_xy, float2 *next_xy)
{
    hipLaunchKernelGGL(k_dmap_stereo_prep, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, prm, corners, ncorners, max_corners, lkjobs, prev_xy, next_xy);
}
static void dm_launch_stereo_finish(svslam_ctx *c, int njobs, DmJob *dj, const DmParams &prm, const float2 *next_xy, const uint8_t *status,
                                    TriJob *trijobs, float2 *uv_l, float2 *uv_r, int *tri_idx)
{
    hipLaunchKernelGGL(k_dmap_stereo_finish, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, prm, next_xy, status, trijobs, uv_l, uv_r, tri_idx);
}
static void dm_launch_commit(svslam_ctx *c, int njobs, DmJob *dj, const double *tri_xyz, const uint8_t *tri_ok, const int *tri_idx, int *slot_tmp)
{
    hipLaunchKernelGGL(k_dmap_commit, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, tri_xyz, tri_ok, tri_idx, slot_tmp);
}
// wide: 1024 threads per problem (a call of a few problems), else 512 (a batch)
static void dm_launch_ba_gather(svslam_ctx *c, int njobs, bool wide, DmJob *dj, const DmParams &prm, BaDev *bd, double *poses, double *pts,
                                unsigned int *packed, float2 *uv, int *edge_ref, int *lm_slot_of, int max_kf, int tile_cap, size_t aux_stride)
{
    const int NL = c->dm.NL;
    if (wide)
        hipLaunchKernelGGL(k_dmap_ba_gather<1024>, dim3(njobs), dim3(1024), dmg_lds_bytes_t<1024>(NL), c->stream, dj, c->dm, prm, bd, poses, pts,
                           packed, uv, edge_ref, lm_slot_of, max_kf, tile_cap, aux_stride);
    else
        hipLaunchKernelGGL(k_dmap_ba_gather<512>, dim3(njobs), dim3(512), dmg_lds_bytes_t<512>(NL), c->stream, dj, c->dm, prm, bd, poses, pts,
                           packed, uv, edge_ref, lm_slot_of, max_kf, tile_cap, aux_stride);
}
static void dm_launch_ba_scatter(svslam_ctx *c, int njobs, DmJob *dj, const DmParams &prm, const BaDev *bd, const double *poses, const double *pts,
                                 const double *chi2, const int *edge_ref, const int *lm_slot_of, int max_kf)
{
    hipLaunchKernelGGL(k_dmap_ba_scatter, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, prm, bd, poses, pts, chi2, edge_ref, lm_slot_of, max_kf);
}
static void dm_launch_refresh(svslam_ctx *c, int njobs, DmJob *dj)
{
    hipLaunchKernelGGL(k_dmap_refresh, dim3(njobs), dim3(DM_THREADS), 0, c->stream, dj, c->dm, c->rt);
}
static void dm_launch_refresh_xyz(svslam_ctx *c, int njobs, const int *list3)
{
    hipLaunchKernelGGL(k_dmap_refresh_xyz, dim3(njobs), dim3(DM_THREADS), 0, c->stream, list3, c->dm, c->rt);
}

// ------------------------------------------------------------------ the keyframe path on the device-resident map
// fb_mode: 0 the call as the caller made it; 1 / 2: the batch-solver repeat of local BAs the low-latency solver gave up on
// (dmap_ll_fallback) — optimise-only jobs; 1 also rebuilds the resident feature list of the job's keyframe (k_dmap_refresh ran
// before the outlier observations were removed), 2 refreshes positions only (a deferred BA that landed frames later)
static int dmap_keyframe_impl(svslam_ctx *c, int njobs, svslam_dmap_job *jobs, const void *const *left_imgs,
                              const void *const *right_imgs, const int *strides, int src_is_device,
                              const double cam_l[4], const double ext_l[7], const double cam_r[4], const double ext_r[7],
                              const svslam_dmap_params *p, int fb_mode)
{
    if (njobs <= 0) return 0;
    if (!c->dm_all) return fail(c, "dmap: context created without device_map");
    if (c->dmba.inflight) return fail(c, "dmap: a deferred local BA is in flight: call svslam_dmap_ba_collect first");
    static_assert(sizeof(DmJob) == sizeof(svslam_dmap_job), "job layout");
    static_assert(sizeof(DmEvicted) == sizeof(svslam_dmap_evicted_rec), "evicted record layout");
    c->evicted.clear();
    const DMap &m = c->dm;
    if (2 * njobs > c->lim.max_jobs) return fail(c, "dmap: %d jobs need max_jobs >= %d", njobs, 2 * njobs);
    if (njobs > SVSLAM_DMAP_CHUNK) return fail(c, "dmap: at most %d jobs per call", SVSLAM_DMAP_CHUNK);
    if (p->num_features < 1 || p->num_features > c->lim.max_corners) return fail(c, "dmap: num_features %d out of [1,%d]", p->num_features, c->lim.max_corners);
    if (p->num_active_keyframes + 1 > m.KW) return fail(c, "dmap: window of %d keyframes needs max_kf >= %d", p->num_active_keyframes, p->num_active_keyframes + 1);
    std::vector<int> slots; std::vector<const void *> imgs; std::vector<int> strd;
    // is_init == 2: no keyframe — ONE local BA over the stream's window as it is (Backend::UpdateMap from outside the
    // frontend, include/StereoVisionSLAM/backend.h:30).  A call holds keyframe jobs or such jobs, not both.
    int n_opt = 0;
    for (int i = 0; i < njobs; ++i) n_opt += jobs[i].is_init == 2 ? 1 : 0;
    if (n_opt != 0 && n_opt != njobs) return fail(c, "dmap: optimise-only jobs (is_init 2) cannot share a call with keyframe jobs");
    const bool opt_only = n_opt == njobs;
    for (int i = 0; i < njobs; ++i) {
        svslam_dmap_job &j = jobs[i];
        if (j.stream < 0 || j.stream >= c->lim.max_streams) return fail(c, "dmap: job %d stream %d out of range", i, j.stream);
        // two jobs of one call on the same stream would work on the same map arenas at once
        if (c->dm_seen.size() != (size_t)c->lim.max_streams) c->dm_seen.assign((size_t)c->lim.max_streams, 0u);
        if (i == 0 && ++c->dm_seen_gen == 0u) { std::fill(c->dm_seen.begin(), c->dm_seen.end(), 0u); c->dm_seen_gen = 1u; }
        if (c->dm_seen[(size_t)j.stream] == c->dm_seen_gen) return fail(c, "dmap: stream %d appears twice in one call (job %d)", j.stream, i);
        c->dm_seen[(size_t)j.stream] = c->dm_seen_gen;
        if (opt_only) {
            if (j.npts != c->rt_count[(size_t)j.stream]) return fail(c, "dmap: job %d says %d features, stream %d holds %d", i, j.npts, j.stream, c->rt_count[(size_t)j.stream]);
            continue;
        }
        if (check_slot(c, j.slot_cur) || check_slot(c, j.slot_right)) return -1;
        if (j.kf_slot < 0 || j.kf_slot >= m.KW || j.remove_slot >= m.KW) return fail(c, "dmap: job %d keyframe slot out of range", i);
        if (j.is_init ? j.npts != 0 : j.npts != c->rt_count[(size_t)j.stream])
            return fail(c, "dmap: job %d says %d features, stream %d holds %d", i, j.npts, j.stream, c->rt_count[(size_t)j.stream]);
        if (j.is_init) { slots.push_back(j.slot_cur); imgs.push_back(left_imgs[i]); strd.push_back(strides[i]); }
    }
    for (int i = 0; i < njobs && !opt_only; ++i) { slots.push_back(jobs[i].slot_right); imgs.push_back(right_imgs[i]); strd.push_back(strides[i]); }
    if (opt_only) {
        if (arena_busy(c)) return -1;
        c->ar.reset();
    } else {
        const bool dec = c->src_w > 0;
        if (pyramid_common(c, (int)slots.size(), slots.data(), imgs.data(), strd.data(), src_is_device, dec, dec ? c->src_w : c->geom.w[0],
                           dec ? c->src_h : c->geom.h[0], false)) return -1;
    }
    const int NF = m.NF, NL = m.NL, MO = c->lim.max_obs, MK = c->lim.max_kf, MC = p->num_features;
    c->ba_eid = ba_ext_identity(ext_l, ext_r);
    const bool use_ll = ba_ll_usable(c, njobs);
    const int tile_cap = use_ll ? ba_ll_tile_cap(c) : ba_tile_cap(MK);
    const size_t aux_stride = ba_aux_layout(MK, NL, MO, MO, MK, 0, ba_tile_bound(NL, MO, MK, tile_cap)).total + ba_pitem_bound(MO, MK) +
                              (use_ll ? ba_split_aux_extra(MK, c->ll.w) : 0);
    const size_t n = njobs, P = n * NF, E = n * MO;
    const size_t base = c->ar.off;
    size_t ojobs = c->ar.take(sizeof(DmJob) * n);
    size_t ogj = c->ar.take(sizeof(GfttJob) * n);
    size_t ocams = c->ar.take(sizeof(BaCams));
    size_t in_end = c->ar.off;
    // device-only scratch of this call
    size_t ocor = c->ar.take(sizeof(float2) * n * MC), oncor = c->ar.take(sizeof(int) * n);
    size_t olk = c->ar.take(sizeof(LkJob) * n), oprev = c->ar.take(sizeof(float2) * P), onext = c->ar.take(sizeof(float2) * P);
    size_t ostat = c->ar.take(P), oerr = c->ar.take(sizeof(float) * P);
    size_t otj = c->ar.take(sizeof(TriJob) * n), oul = c->ar.take(sizeof(float2) * P), our_ = c->ar.take(sizeof(float2) * P);
    size_t otidx = c->ar.take(sizeof(int) * P), oxyz = c->ar.take(sizeof(double) * 3 * P), ook = c->ar.take(P), oslot = c->ar.take(sizeof(int) * P);
    // the local-BA problem and the solver's scratch: in the arena, or — deferred — in the buffer that outlives this call
    const bool defer = p->ba_defer != 0 && p->ba_iters > 0 && !opt_only;
    Arena bar;                                    // offsets only (take()): base pointer chosen below
    bar.cap = ~(size_t)0;
    Arena &A = defer ? bar : c->ar;
    size_t obd = A.take(sizeof(BaDev) * n), oposes = A.take(sizeof(double) * 7 * MK * n), opts = A.take(sizeof(double) * 3 * NL * n);
    size_t opk = A.take(sizeof(unsigned int) * E), ouv = A.take(sizeof(float2) * E), oref = A.take(sizeof(int) * E);
    size_t olms = A.take(sizeof(int) * NL * n), ochi = A.take(sizeof(double) * E), oflag = A.take(sizeof(int) * 4);
    size_t orecs = A.take(sizeof(BaRec) * 2 * E), oaux = A.take(sizeof(int) * aux_stride * n);
    size_t obcams = 0, objobs = 0;
    if (defer) {
        obcams = A.take(sizeof(BaCams)); objobs = A.take(sizeof(DmJob) * n);
        if (!c->dmba.stream) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->dmba.stream, hipStreamNonBlocking));
            for (hipEvent_t *e : { &c->dmba.gathered, &c->dmba.solved }) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
            for (hipEvent_t *e : { &c->dmba.t0, &c->dmba.t1 }) HIPCHK(c, hipEventCreate(e));
        }
        if (A.off > c->dmba.cap) {
            if (c->dmba.buf) { HIPCHK(c, hipStreamSynchronize(c->dmba.stream)); (void)hipFree(c->dmba.buf); c->dmba.buf = nullptr; c->dmba.cap = 0; }
            const size_t want = A.off + A.off / 4;
            HIPCHK(c, hipMalloc(&c->dmba.buf, want));
            c->dmba.cap = want;
        }
    }
    unsigned char *bab = defer ? c->dmba.buf : c->ar.d;          // base of the BA buffers
    auto bp_ = [&](size_t off) { return bab + off; };
    // (test hook SVSLAM_DMAP_EVICT_CAP: a smaller list for the whole call, to exercise the "waits for the next keyframe" path)
    static const int ev_cap_env = []{ const char *e = std::getenv("SVSLAM_DMAP_EVICT_CAP"); return e ? atoi(e) : 0; }();
    const int ev_cap = ev_cap_env > 0 ? std::max(njobs, std::min(ev_cap_env, njobs * SVSLAM_DMAP_EVICT_PER_JOB)) : njobs * SVSLAM_DMAP_EVICT_PER_JOB;
    size_t oev = c->ar.take(sizeof(DmEvicted) * (size_t)ev_cap);
    if (c->ar.off > c->ar.cap) return fail(c, "dmap: staging arena too small (%zu > %zu bytes); fewer jobs per call", c->ar.off, c->ar.cap);
    DmJob *hj = hp<DmJob>(c, ojobs);
    GfttJob *gj = hp<GfttJob>(c, ogj);
    memcpy(hj, jobs, sizeof(DmJob) * n);
    c->dm_stamp++;
    for (int i = 0; i < njobs; ++i) {
        hj[i].src_buf = c->rt_which[(size_t)hj[i].stream];
        hj[i].dst_buf = c->rt_which[(size_t)hj[i].stream];      // the survivors have been copied into the keyframe by then
        hj[i].stamp = c->dm_stamp;
        if (opt_only) {          // what k_dmap_begin would have initialised
            hj[i].ok = 1; hj[i].dead = 0; hj[i].flags = 0; hj[i].n_features = hj[i].npts; hj[i].n_corners = hj[i].n_right_ok = hj[i].n_tri_in = hj[i].n_tri_ok = 0;
            hj[i].ba_nkf = hj[i].ba_nlm = hj[i].ba_nobs = hj[i].ba_iters = hj[i].ba_npair = hj[i].ba_ntrial = 0; hj[i].ev_ofs = hj[i].ev_n = 0;
            if (fb_mode != 1) hj[i].kf_slot = -1;
            hj[i].remove_slot = -1; hj[i].pad0 = 0;
        }
        gj[i].slot = hj[i].slot_cur; gj[i].nrect = hj[i].npts;
        gj[i].rect_ofs = (int)(((size_t)hj[i].stream * m.KW + hj[i].kf_slot) * NF);
    }
    BaCams *cams = hp<BaCams>(c, ocams);
    memcpy(cams->cam[0], cam_l, 32); memcpy(cams->cam[1], cam_r, 32);
    memcpy(cams->ext[0], ext_l, 56); memcpy(cams->ext[1], ext_r, 56);
    DmParams prm;
    prm.num_features = p->num_features; prm.num_features_init = p->num_features_init; prm.num_active = p->num_active_keyframes;
    prm.zmax = p->max_triangulation_depth; prm.chi2_th = p->chi2_th;
    memcpy(prm.cam_l, cam_l, 32); memcpy(prm.cam_r, cam_r, 32);
    prm.max_obs = MO; prm.max_lm = NL; prm.w = c->geom.w[0]; prm.h = c->geom.h[0];
    TriCams tc;
    memcpy(tc.cam_l, cam_l, 32); memcpy(tc.ext_l, ext_l, 56); memcpy(tc.cam_r, cam_r, 32); memcpy(tc.ext_r, ext_r, 56);
    if (h2d(c, base, in_end)) return -1;
    // flag words: [0] BA structure build overflow, [1] evicted-list cursor.  Deferred: the build's word lives with the problem,
    // the cursor of this call's evicted list stays in the arena
    size_t oevc = oflag;
    if (defer) { oevc = c->ar.take(sizeof(int) * 4); if (c->ar.off > c->ar.cap) return fail(c, "dmap: staging arena too small"); }
    HIPCHK(c, hipMemsetAsync(bp_(oflag), 0, sizeof(int) * 4, c->stream));
    if (defer) HIPCHK(c, hipMemsetAsync(dp<void>(c, oevc), 0, sizeof(int) * 4, c->stream));
    int *d_evcur = defer ? dp<int>(c, oevc) + 1 : reinterpret_cast<int *>(bp_(oflag)) + 1;
    DmJob *dj = dp<DmJob>(c, ojobs);
    if (!opt_only) {
    // every job may hand over ev_cap / njobs landmarks per call: what a job evicts does not depend on the other jobs' timing
    dm_launch_begin(c, njobs, dj, dp<DmEvicted>(c, oev), d_evcur, std::max(1, ev_cap / njobs));
    if (launch_gftt(c, njobs, dp<GfttJob>(c, ogj), m.f_xy, MC, 0.01, 20.0, dp<float2>(c, ocor), dp<int>(c, oncor))) return -1;   // src/frontend.cpp:24
    dm_launch_stereo_prep(c, njobs, dj, prm, dp<float2>(c, ocor), dp<int>(c, oncor), MC, dp<LkJob>(c, olk), dp<float2>(c, oprev), dp<float2>(c, onext));
    {
        svslam_lk_params lp = { 3, 30, 0.01, 1e-4, 1 };                     // src/frontend.cpp:105-109
        tm_begin(c, FAM_LK, 0);
        launch_lk(c, njobs, NF, dp<LkJob>(c, olk), dp<float2>(c, oprev), dp<float2>(c, onext), dp<uint8_t>(c, ostat), dp<float>(c, oerr), &lp);
        tm_end(c);
    }
    dm_launch_stereo_finish(c, njobs, dj, prm, dp<float2>(c, onext), dp<uint8_t>(c, ostat), dp<TriJob>(c, otj), dp<float2>(c, oul), dp<float2>(c, our_),
                            dp<int>(c, otidx));
    tm_begin(c, FAM_TRI, 0);
    hipLaunchKernelGGL(k_triangulate, dim3(njobs, cdiv(NF, 64)), dim3(64), 0, c->stream, dp<TriJob>(c, otj), tc, dp<float2>(c, oul), dp<float2>(c, our_),
                       dp<double>(c, oxyz), dp<uint8_t>(c, ook));
    tm_end(c);
    dm_launch_commit(c, njobs, dj, dp<double>(c, oxyz), dp<uint8_t>(c, ook), dp<int>(c, otidx), dp<int>(c, oslot));
    }
    // Backend::UpdateMap (src/backend.cpp:14-18) only runs with a backend: a paused / absent one (ba_iters <= 0) means no
    // Optimize, so no outlier classification and no observation removed either — like the host-map path
    if (p->ba_iters > 0) {
        BaDev *b_bd = reinterpret_cast<BaDev *>(bp_(obd));
        double *b_poses = reinterpret_cast<double *>(bp_(oposes)), *b_pts = reinterpret_cast<double *>(bp_(opts)), *b_chi = reinterpret_cast<double *>(bp_(ochi));
        int *b_ref = reinterpret_cast<int *>(bp_(oref)), *b_lms = reinterpret_cast<int *>(bp_(olms));
        const BaCams *b_cams = defer ? reinterpret_cast<const BaCams *>(bp_(obcams)) : dp<BaCams>(c, ocams);
        hipStream_t main_stream = c->stream;
        if (!defer) tm_begin(c, FAM_BA, njobs);
        dm_launch_ba_gather(c, njobs, njobs <= SVSLAM_LL_MAX_PROBLEMS, dj, prm, b_bd, b_poses, b_pts, reinterpret_cast<unsigned int *>(bp_(opk)),
                            reinterpret_cast<float2 *>(bp_(ouv)), b_ref, b_lms, MK, tile_cap, aux_stride);
        if (defer) {
            // the solve leaves this call's stream: a copy of the jobs (the scatter needs streams, window slots) and of the
            // cameras goes with the problem; the second stream picks up behind the gather
            HIPCHK(c, hipMemcpyAsync(bp_(objobs), dj, sizeof(DmJob) * n, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(bp_(obcams), dp<void>(c, ocams), sizeof(BaCams), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipEventRecord(c->dmba.gathered, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->dmba.stream, c->dmba.gathered, 0));
            c->stream = c->dmba.stream;                       // (launch_ba_solver enqueues on the context's stream)
            (void)hipEventRecord(c->dmba.t0, c->stream);
        }
        launch_ba_solver(c, njobs, use_ll, b_bd, b_cams, b_poses, b_pts, reinterpret_cast<unsigned int *>(bp_(opk)),
                         reinterpret_cast<float2 *>(bp_(ouv)), b_ref /* order: identity, not read */, reinterpret_cast<BaRec *>(bp_(orecs)),
                         reinterpret_cast<int *>(bp_(oaux)), b_chi, reinterpret_cast<int *>(bp_(oflag)), NL, MO, p->chi2_th, p->ba_iters, false, !defer);
        if (defer) {
            (void)hipEventRecord(c->dmba.t1, c->stream);
            const hipError_t rec_rc = hipEventRecord(c->dmba.solved, c->stream);
            c->stream = main_stream;
            HIPCHK(c, rec_rc);
            c->dmba.inflight = true; c->dmba.njobs = njobs; c->dmba.ojobs = objobs; c->dmba.obd = obd; c->dmba.oposes = oposes; c->dmba.opts = opts;
            c->dmba.ochi = ochi; c->dmba.oref = oref; c->dmba.olms = olms; c->dmba.oflag = oflag; c->dmba.prm = prm; c->dmba.MK = MK;
            c->dmba.cams = *cams; c->dmba.ba_iters = p->ba_iters;
        } else {
            dm_launch_ba_scatter(c, njobs, dj, prm, b_bd, b_poses, b_pts, b_chi, b_ref, b_lms, MK);
            tm_end(c);
        }
    }
    if (opt_only && fb_mode == 1) dm_launch_refresh(c, njobs, dj);
    else if (opt_only) {
        size_t ol3 = c->ar.take(sizeof(int) * 3 * n);
        if (c->ar.off > c->ar.cap) return fail(c, "dmap: staging arena too small");
        int *l3 = hp<int>(c, ol3);
        for (int i = 0; i < njobs; ++i) { l3[3 * i] = hj[i].stream; l3[3 * i + 1] = hj[i].src_buf; l3[3 * i + 2] = hj[i].npts; }
        if (h2d(c, ol3, ol3 + sizeof(int) * 3 * n)) return -1;
        dm_launch_refresh_xyz(c, njobs, dp<int>(c, ol3));
    } else dm_launch_refresh(c, njobs, dj);
    HIPCHK(c, hipGetLastError());
    // ONE wait for everything the host reads (round 4: three copies each behind its own wait cost a lone camera ~50 us per
    // keyframe): the jobs, the flag words and the head of the evicted list ride one completion; only a list longer than the
    // head is fetched with a second copy
    // (deferred: the build's overflow word is read by svslam_dmap_ba_collect; word 0 of the arena copy stays 0)
    const size_t ofw = defer ? oevc : oflag;
    const int ev_head = std::min(ev_cap, 256);
    HIPCHK(c, hipMemcpyAsync(hp<void>(c, ojobs), dp<void>(c, ojobs), sizeof(DmJob) * n, hipMemcpyDeviceToHost, c->stream));
    if (defer) HIPCHK(c, hipMemcpyAsync(hp<void>(c, ofw), dp<void>(c, ofw), sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
    else HIPCHK(c, hipMemcpyAsync(hp<void>(c, ofw), bp_(ofw), sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
    if (!opt_only && ev_head > 0) HIPCHK(c, hipMemcpyAsync(hp<void>(c, oev), dp<void>(c, oev), sizeof(DmEvicted) * (size_t)ev_head, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    const int *fw = hp<int>(c, ofw);
    if (const int fl = fw[0]) return fail(c, "dmap: the BA structure build overflowed a capacity (code %d)", fl);
    if (const int nev = fw[1]) {                // the landmarks this call freed (svslam_dmap_evicted)
        if (nev < 0 || nev > ev_cap) return fail(c, "dmap: evicted-list cursor %d out of [0,%d]", nev, ev_cap);
        if (nev > ev_head && d2h_sync(c, oev + sizeof(DmEvicted) * (size_t)ev_head, oev + sizeof(DmEvicted) * (size_t)nev)) return -1;
        c->evicted.assign(hp<DmEvicted>(c, oev), hp<DmEvicted>(c, oev) + nev);
    }
    memcpy(jobs, hj, sizeof(DmJob) * n);
    for (int i = 0; i < njobs && !opt_only; ++i) c->rt_count[(size_t)jobs[i].stream] = jobs[i].n_features;
    for (int i = 0; i < njobs; ++i)
        if (jobs[i].ba_iters < 0 && fb_mode != 0) return fail(c, "dmap: job %d: the batch solver reported a low-latency failure", i);
    return 0;
}

// Local BAs of `jobs` whose low-latency solve gave up (ba_iters < 0: a shard of the problem never became resident — the CUs were
// taken by something else; nothing was written back) are solved again with the batch solver, one workgroup per problem, which
// has no inter-workgroup barrier: optimise-only jobs over the same windows, their BA outputs copied into the caller's jobs.
static int dmap_ll_fallback(svslam_ctx *c, int njobs, svslam_dmap_job *jobs, const double cam_l[4], const double ext_l[7],
                            const double cam_r[4], const double ext_r[7], const svslam_dmap_params *p, int fb_mode)
{
    std::vector<int> bad;
    for (int i = 0; i < njobs; ++i) if (jobs[i].ba_iters < 0) bad.push_back(i);
    if (bad.empty()) return 0;
    const int nb = (int)bad.size();
    std::vector<svslam_dmap_job> oj((size_t)nb);
    for (int k = 0; k < nb; ++k) {
        oj[(size_t)k] = jobs[bad[(size_t)k]];
        oj[(size_t)k].is_init = 2;
        oj[(size_t)k].npts = c->rt_count[(size_t)oj[(size_t)k].stream];
    }
    std::vector<DmEvicted> keep;
    keep.swap(c->evicted);                         // (the repeat frees nothing; the caller still reads this call's list)
    svslam_dmap_params q = *p;
    q.ba_defer = 0;
    if (q.ba_iters <= 0) q.ba_iters = 10;
    std::vector<const void *> nul((size_t)nb, nullptr);
    std::vector<int> st((size_t)nb, 0);
    c->ll.force_batch = true;
    const int rc = dmap_keyframe_impl(c, nb, oj.data(), nul.data(), nul.data(), st.data(), 1, cam_l, ext_l, cam_r, ext_r, &q, fb_mode);
    c->ll.force_batch = false;
    c->evicted.swap(keep);
    if (rc) return rc;
    for (int k = 0; k < nb; ++k) {
        svslam_dmap_job &d = jobs[bad[(size_t)k]];
        const svslam_dmap_job &o = oj[(size_t)k];
        d.ba_nkf = o.ba_nkf; d.ba_nlm = o.ba_nlm; d.ba_nobs = o.ba_nobs; d.ba_iters = o.ba_iters; d.ba_npair = o.ba_npair; d.ba_ntrial = o.ba_ntrial;
        d.flags |= o.flags & 4;
        memcpy(d.win_pose, o.win_pose, sizeof(d.win_pose)); memcpy(d.win_slot, o.win_slot, sizeof(d.win_slot));
        if (fb_mode == 1) memcpy(d.pose, o.pose, sizeof(d.pose));
    }
    c->ll.fallbacks += nb;
    return 0;
}

int svslam_dmap_keyframe_batch(svslam_ctx *c, int njobs, svslam_dmap_job *jobs, const void *const *left_imgs,
                               const void *const *right_imgs, const int *strides, int src_is_device,
                               const double cam_l[4], const double ext_l[7], const double cam_r[4], const double ext_r[7],
                               const svslam_dmap_params *p)
{
    if (njobs <= 0) return 0;
    const bool was_inflight = c->dmba.inflight;
    const int rc = dmap_keyframe_impl(c, njobs, jobs, left_imgs, right_imgs, strides, src_is_device, cam_l, ext_l, cam_r, ext_r, p, 0);
    if (rc != 0) {
        // a failure behind the point where the deferred solve was armed must not leave it armed: the caller never learns
        // that it has to collect, and every later keyframe call would be refused
        if (!was_inflight && c->dmba.inflight) {
            const std::string keep_err = c->err;
            if (c->dmba.stream) (void)hipStreamSynchronize(c->dmba.stream);
            c->dmba.inflight = false;
            c->err = keep_err;
        }
        return rc;
    }
    return dmap_ll_fallback(c, njobs, jobs, cam_l, ext_l, cam_r, ext_r, p, 1);
}

int svslam_dmap_ba_collect(svslam_ctx *c, int njobs, svslam_dmap_job *jobs_out, int *njobs_inflight)
{
    if (njobs_inflight) *njobs_inflight = c->dmba.inflight ? c->dmba.njobs : 0;
    if (!c->dmba.inflight) return 0;
    if (njobs != c->dmba.njobs || !jobs_out) return fail(c, "dmap_ba_collect: %d jobs are in flight, the caller passed %d", c->dmba.njobs, njobs);
    if (arena_busy(c)) return -1;
    c->dmba.inflight = false;
    const DMap &m = c->dm;
    unsigned char *b = c->dmba.buf;
    const size_t n = (size_t)njobs;
    c->ar.reset();
    size_t ojobs = c->ar.take(sizeof(DmJob) * n), oflag = c->ar.take(sizeof(int) * 4), ol3 = c->ar.take(sizeof(int) * 3 * n);
    if (c->ar.off > c->ar.cap) return fail(c, "dmap_ba_collect: staging arena too small");
    // the solve is done when its event is: this stream goes on behind it
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->dmba.solved, 0));
    DmJob *dj = reinterpret_cast<DmJob *>(b + c->dmba.ojobs);
    tm_begin(c, FAM_BA, 0);
    dm_launch_ba_scatter(c, njobs, dj, c->dmba.prm, reinterpret_cast<const BaDev *>(b + c->dmba.obd),
                         reinterpret_cast<const double *>(b + c->dmba.oposes), reinterpret_cast<const double *>(b + c->dmba.opts),
                         reinterpret_cast<const double *>(b + c->dmba.ochi), reinterpret_cast<const int *>(b + c->dmba.oref),
                         reinterpret_cast<const int *>(b + c->dmba.olms), c->dmba.MK);
    tm_end(c);
    // the jobs come back first: the streams whose resident lists are refreshed are named by them
    HIPCHK(c, hipMemcpyAsync(hp<void>(c, ojobs), dj, sizeof(DmJob) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hp<void>(c, oflag), b + c->dmba.oflag, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
    if (d2h_sync(c, 0, 0)) return -1;
    {   // the solver's time, measured on its own stream
        float ms = 0.f;
        if (c->timing && hipEventElapsedTime(&ms, c->dmba.t0, c->dmba.t1) == hipSuccess) { c->tm.ms[FAM_BA] += ms; c->tm.launches[FAM_BA] += 1; c->tm.units[FAM_BA] += njobs; }
    }
    if (const int fl = hp<int>(c, oflag)[0]) return fail(c, "dmap: the BA structure build overflowed a capacity (code %d)", fl);
    const DmJob *hj = hp<DmJob>(c, ojobs);
    int *l3 = hp<int>(c, ol3);
    for (int i = 0; i < njobs; ++i) {
        const int s_ = hj[i].stream;
        l3[3 * i] = s_; l3[3 * i + 1] = c->rt_which[(size_t)s_]; l3[3 * i + 2] = c->rt_count[(size_t)s_];
    }
    if (h2d(c, ol3, ol3 + sizeof(int) * 3 * n)) return -1;
    dm_launch_refresh_xyz(c, njobs, dp<int>(c, ol3));
    HIPCHK(c, hipGetLastError());
    if (d2h_sync(c, 0, 0)) return -1;
    memcpy(jobs_out, hj, sizeof(DmJob) * n);
    {   // problems the low-latency solver gave up on: once more with the batch solver (the map has not moved since the gather:
        // the host collects before the next keyframe)
        svslam_dmap_params q{};
        q.num_features = c->dmba.prm.num_features; q.num_features_init = c->dmba.prm.num_features_init; q.num_active_keyframes = c->dmba.prm.num_active;
        q.ba_iters = c->dmba.ba_iters; q.max_triangulation_depth = c->dmba.prm.zmax; q.chi2_th = c->dmba.prm.chi2_th;
        return dmap_ll_fallback(c, njobs, jobs_out, c->dmba.prm.cam_l, c->dmba.cams.ext[0], c->dmba.prm.cam_r, c->dmba.cams.ext[1], &q, 2);
    }
}

int svslam_dmap_evicted(svslam_ctx *c, const svslam_dmap_evicted_rec **recs, int *n)
{
    if (!c->dm_all) return fail(c, "dmap_evicted: context created without device_map");
    *recs = reinterpret_cast<const svslam_dmap_evicted_rec *>(c->evicted.data());
    *n = (int)c->evicted.size();
    return 0;
}

int svslam_dmap_read(svslam_ctx *c, int stream, long long *kf_frame, int *kf_id, double *kf_pose, int *kf_n, int *lm_id,
                     double *lm_pos, int *lm_obs, uint8_t *lm_state)
{
    if (!c->dm_all) return fail(c, "dmap_read: context created without device_map");
    if (stream < 0 || stream >= c->lim.max_streams) return fail(c, "dmap_read: stream %d out of range", stream);
    const DMap &m = c->dm;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t K = (size_t)stream * m.KW, L = (size_t)stream * m.NL;
    if (kf_frame) HIPCHK(c, hipMemcpy(kf_frame, m.kf_frame + K, sizeof(long long) * m.KW, hipMemcpyDeviceToHost));
    if (kf_id) HIPCHK(c, hipMemcpy(kf_id, m.kf_id + K, sizeof(int) * m.KW, hipMemcpyDeviceToHost));
    if (kf_pose) HIPCHK(c, hipMemcpy(kf_pose, m.kf_pose + K * 7, sizeof(double) * 7 * m.KW, hipMemcpyDeviceToHost));
    if (kf_n) HIPCHK(c, hipMemcpy(kf_n, m.kf_n + K, sizeof(int) * m.KW, hipMemcpyDeviceToHost));
    if (lm_id) HIPCHK(c, hipMemcpy(lm_id, m.lm_id + L, sizeof(int) * m.NL, hipMemcpyDeviceToHost));
    if (lm_pos) HIPCHK(c, hipMemcpy(lm_pos, m.lm_pos + L * 3, sizeof(double) * 3 * m.NL, hipMemcpyDeviceToHost));
    if (lm_obs) HIPCHK(c, hipMemcpy(lm_obs, m.lm_obs + L, sizeof(int) * m.NL, hipMemcpyDeviceToHost));
    if (lm_state) HIPCHK(c, hipMemcpy(lm_state, m.lm_st + L, m.NL, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------ test hooks of the device map (tests/test_gpu_dmap_kernels.py)
// every array of one stream's map, to the device (write) or back
static int dmap_state_io(svslam_ctx *c, int stream, const svslam_dmap_state *a, bool write, const char *what)
{
    if (!c->dm_all) return fail(c, "%s: context created without device_map", what);
    if (stream < 0 || stream >= c->lim.max_streams) return fail(c, "%s: stream %d out of range", what, stream);
    if (!a) return fail(c, "%s: no arrays", what);
    const DMap &m = c->dm;
    const size_t KW = m.KW, NF = m.NF, NL = m.NL, K = (size_t)stream * KW, F = K * NF, L = (size_t)stream * NL;
    if (write) {        // what the kernels index with must stay inside the stream's arenas
        if (a->kf_n) for (size_t k = 0; k < KW; ++k) if (a->kf_n[k] < 0 || a->kf_n[k] > (int)NF) return fail(c, "%s: kf_n[%zu] = %d out of [0,%zu]", what, k, a->kf_n[k], NF);
        for (const int *lk : { a->f_lm, a->f_lmr })
            if (lk) for (size_t i = 0; i < KW * NF; ++i) if (lk[i] < -1 || lk[i] >= (int)NL) return fail(c, "%s: landmark slot %d of feature %zu out of [-1,%zu)", what, lk[i], i, NL);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    auto io = [&](void *dev, const void *host, size_t bytes) -> hipError_t {
        if (!host) return hipSuccess;
        return write ? hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) : hipMemcpy(const_cast<void *>(host), dev, bytes, hipMemcpyDeviceToHost);
    };
    HIPCHK(c, io(m.kf_frame + K, a->kf_frame, 8 * KW));
    HIPCHK(c, io(m.kf_id + K, a->kf_id, 4 * KW));
    HIPCHK(c, io(m.kf_pose + K * 7, a->kf_pose, 56 * KW));
    HIPCHK(c, io(m.kf_n + K, a->kf_n, 4 * KW));
    HIPCHK(c, io(m.f_xy + F, a->f_xy, 8 * KW * NF));
    HIPCHK(c, io(m.f_xyr + F, a->f_xyr, 8 * KW * NF));
    HIPCHK(c, io(m.f_lm + F, a->f_lm, 4 * KW * NF));
    HIPCHK(c, io(m.f_lmr + F, a->f_lmr, 4 * KW * NF));
    HIPCHK(c, io(m.f_fl + F, a->f_fl, KW * NF));
    HIPCHK(c, io(m.lm_pos + L * 3, a->lm_pos, 24 * NL));
    HIPCHK(c, io(m.lm_id + L, a->lm_id, 4 * NL));
    HIPCHK(c, io(m.lm_obs + L, a->lm_obs, 4 * NL));
    HIPCHK(c, io(m.lm_st + L, a->lm_state, NL));
    HIPCHK(c, io(m.lm_stamp + L, a->lm_stamp, 4 * NL));
    HIPCHK(c, io(m.next_lm_id + stream, a->next_lm_id, 4));
    return 0;
}

int svslam_debug_dmap_write(svslam_ctx *c, int stream, const svslam_dmap_state *a) { return dmap_state_io(c, stream, a, true, "debug_dmap_write"); }
int svslam_debug_dmap_read(svslam_ctx *c, int stream, svslam_dmap_state *a) { return dmap_state_io(c, stream, a, false, "debug_dmap_read"); }

// the resident feature list of one stream (the buffer the next call reads): max_pts entries each
int svslam_debug_rtrack_read(svslam_ctx *c, int stream, float *xy, int *mp, double *xyz)
{
    if (c->rt.max_pts <= 0) return fail(c, "debug_rtrack_read: context created with max_streams = 0");
    if (stream < 0 || stream >= c->lim.max_streams) return fail(c, "debug_rtrack_read: stream %d out of range", stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int b = c->rt_which[(size_t)stream];
    const size_t R = (size_t)stream * c->rt.max_pts, n = (size_t)c->rt.max_pts;
    if (xy) HIPCHK(c, hipMemcpy(xy, c->rt.xy[b] + R, 8 * n, hipMemcpyDeviceToHost));
    if (mp) HIPCHK(c, hipMemcpy(mp, c->rt.mp[b] + R, 4 * n, hipMemcpyDeviceToHost));
    if (xyz) HIPCHK(c, hipMemcpy(xyz, c->rt.xyz[b] + 3 * R, 24 * n, hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// device copies of the stage hook's arrays: uploaded before the launch, downloaded after it, freed with the object
struct DbgBufs {
    struct B { void *dev; void *host; size_t bytes; };
    std::vector<B> bufs;
    ~DbgBufs() { for (B &b : bufs) (void)hipFree(b.dev); }
    hipError_t add(void *host, size_t bytes, void **dev)
    {
        *dev = nullptr;
        hipError_t e = hipMalloc(dev, std::max<size_t>(bytes, 16));
        if (e != hipSuccess) return e;
        bufs.push_back({ *dev, host, bytes });
        return host ? hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice) : hipMemset(*dev, 0, std::max<size_t>(bytes, 16));
    }
    hipError_t download()
    {
        for (B &b : bufs)
            if (b.host) { hipError_t e = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
};
}

// ONE kernel of the keyframe path on maps the test seeded (svslam_debug_dmap_write), launched as dmap_keyframe_impl launches it
int svslam_debug_dmap_stage(svslam_ctx *c, int stage, int njobs, svslam_dmap_job *jobs, const svslam_dmap_stage_io *io)
{
    if (!c->dm_all) return fail(c, "debug_dmap_stage: context created without device_map");
    if (njobs <= 0 || njobs > c->lim.max_streams || !jobs || !io) return fail(c, "debug_dmap_stage: %d jobs out of [1,%d] or no arguments", njobs, c->lim.max_streams);
    static_assert(sizeof(DmJob) == sizeof(svslam_dmap_job), "job layout");
    static_assert(sizeof(BaDev) == sizeof(int) * SVSLAM_DMAP_BADEV_INTS, "BaDev layout");
    static_assert(sizeof(TriJob) == sizeof(svslam_tri_job) && sizeof(LkJob) == sizeof(svslam_lk_job), "job layouts");
    if (arena_busy(c)) return -1;
    const DMap &m = c->dm;
    const int NF = m.NF, NL = m.NL, KW = m.KW;
    const size_t n = (size_t)njobs, P = n * NF;
    const bool uses_kf = stage != SVSLAM_DMAP_STAGE_BA_GATHER && stage != SVSLAM_DMAP_STAGE_BA_SCATTER && stage != SVSLAM_DMAP_STAGE_REFRESH_XYZ;
    std::vector<char> seen((size_t)c->lim.max_streams, 0);
    for (int i = 0; i < njobs; ++i) {
        svslam_dmap_job &j = jobs[i];
        if (j.stream < 0 || j.stream >= c->lim.max_streams || seen[(size_t)j.stream]) return fail(c, "debug_dmap_stage: job %d: stream %d out of range or named twice", i, j.stream);
        seen[(size_t)j.stream] = 1;
        if (uses_kf && (j.kf_slot < 0 || j.kf_slot >= KW)) return fail(c, "debug_dmap_stage: job %d keyframe slot %d out of range", i, j.kf_slot);
        if (j.remove_slot >= KW) return fail(c, "debug_dmap_stage: job %d remove_slot %d out of range", i, j.remove_slot);
        if (j.npts < 0 || j.npts > NF || j.n_features < 0 || j.n_features > NF || j.n_tri_in < 0 || j.n_tri_in > NF)
            return fail(c, "debug_dmap_stage: job %d: npts %d / n_features %d / n_tri_in %d out of [0,%d]", i, j.npts, j.n_features, j.n_tri_in, NF);
        j.src_buf = j.dst_buf = c->rt_which[(size_t)j.stream];          // as dmap_keyframe_impl places them; the stamp is the caller's
    }
    DmParams prm{};
    prm.num_features = io->max_corners; prm.num_features_init = io->num_features_init; prm.num_active = KW - 1;
    prm.zmax = io->zmax; prm.chi2_th = io->chi2_th;
    memcpy(prm.cam_r, io->cam_r, 32);          // (no kernel of the map reads cam_l)
    prm.max_obs = io->max_obs; prm.max_lm = NL; prm.w = c->geom.w[0]; prm.h = c->geom.h[0];
    const int MK = io->max_kf, MO = io->max_obs;
    const bool ba = stage == SVSLAM_DMAP_STAGE_BA_GATHER || stage == SVSLAM_DMAP_STAGE_BA_SCATTER;
    if (ba && (MK < 1 || MK > 12 || MO < 1 || MO > (1 << 22))) return fail(c, "debug_dmap_stage: max_kf %d out of [1,12] or max_obs %d out of range", MK, MO);
    const size_t E = n * (size_t)std::max(MO, 1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the resident lists name landmark slots, which index the landmark arena
    auto rt_slots_ok = [&]() -> int {
        std::vector<int> mp((size_t)NF);
        for (int i = 0; i < njobs; ++i) {
            if (jobs[i].npts == 0) continue;
            HIPCHK(c, hipMemcpy(mp.data(), c->rt.mp[jobs[i].src_buf] + (size_t)jobs[i].stream * c->rt.max_pts, 4 * (size_t)jobs[i].npts, hipMemcpyDeviceToHost));
            for (int p = 0; p < jobs[i].npts; ++p)
                if (mp[(size_t)p] >= NL) return fail(c, "debug_dmap_stage: resident feature %d of stream %d names slot %d", p, jobs[i].stream, mp[(size_t)p]);
        }
        return 0;
    };
    DbgBufs B;
    void *dj_ = nullptr;
    HIPCHK(c, B.add(jobs, sizeof(DmJob) * n, &dj_));
    DmJob *dj = static_cast<DmJob *>(dj_);
#define DBG_NEED(p) do { if (!io->p) return fail(c, "debug_dmap_stage: stage %d needs io->" #p, stage); } while (0)
#define DBG_BUF(T, name, p, bytes) void *name##_ = nullptr; HIPCHK(c, B.add((void *)(p), (bytes), &name##_)); T *name = static_cast<T *>(name##_)
    switch (stage) {
    case SVSLAM_DMAP_STAGE_BEGIN: {
        DBG_NEED(evicted); DBG_NEED(ev_cursor);
        if (io->ev_quota < 1 || *io->ev_cursor != 0) return fail(c, "debug_dmap_stage: ev_quota %d < 1, or the cursor does not start at 0", io->ev_quota);
        if (rt_slots_ok()) return -1;
        DBG_BUF(DmEvicted, ev, io->evicted, sizeof(DmEvicted) * n * (size_t)io->ev_quota);
        DBG_BUF(int, cur, io->ev_cursor, 4);
        dm_launch_begin(c, njobs, dj, ev, cur, io->ev_quota);
        break; }
    case SVSLAM_DMAP_STAGE_STEREO_PREP: {
        DBG_NEED(corners); DBG_NEED(ncorners); DBG_NEED(lkjobs); DBG_NEED(prev_xy); DBG_NEED(next_xy);
        if (io->max_corners < 1) return fail(c, "debug_dmap_stage: max_corners %d < 1", io->max_corners);
        for (int i = 0; i < njobs; ++i) if (io->ncorners[i] < 0 || io->ncorners[i] > io->max_corners) return fail(c, "debug_dmap_stage: job %d: %d corners out of [0,%d]", i, io->ncorners[i], io->max_corners);
        DBG_BUF(float2, cor, io->corners, 8 * n * (size_t)io->max_corners);
        DBG_BUF(int, ncor, io->ncorners, 4 * n);
        DBG_BUF(LkJob, lk, io->lkjobs, sizeof(LkJob) * n);
        DBG_BUF(float2, prev, io->prev_xy, 8 * P);
        DBG_BUF(float2, next, io->next_xy, 8 * P);
        dm_launch_stereo_prep(c, njobs, dj, prm, cor, ncor, io->max_corners, lk, prev, next);
        break; }
    case SVSLAM_DMAP_STAGE_STEREO_FINISH: {
        DBG_NEED(next_xy); DBG_NEED(status); DBG_NEED(trijobs); DBG_NEED(uv_l); DBG_NEED(uv_r); DBG_NEED(tri_idx);
        DBG_BUF(float2, next, io->next_xy, 8 * P);
        DBG_BUF(uint8_t, stat, io->status, P);
        DBG_BUF(TriJob, tj, io->trijobs, sizeof(TriJob) * n);
        DBG_BUF(float2, ul, io->uv_l, 8 * P);
        DBG_BUF(float2, ur, io->uv_r, 8 * P);
        DBG_BUF(int, tidx, io->tri_idx, 4 * P);
        dm_launch_stereo_finish(c, njobs, dj, prm, next, stat, tj, ul, ur, tidx);
        break; }
    case SVSLAM_DMAP_STAGE_COMMIT: {
        DBG_NEED(tri_xyz); DBG_NEED(tri_ok); DBG_NEED(tri_idx);
        for (int i = 0; i < njobs; ++i)
            for (int q = 0; q < jobs[i].n_tri_in; ++q) {
                const int p = io->tri_idx[(size_t)i * NF + q];
                if (p < 0 || p >= NF) return fail(c, "debug_dmap_stage: job %d: tri_idx[%d] = %d out of [0,%d)", i, q, p, NF);
            }
        DBG_BUF(double, xyz, io->tri_xyz, 24 * P);
        DBG_BUF(uint8_t, ok, io->tri_ok, P);
        DBG_BUF(int, tidx, io->tri_idx, 4 * P);
        DBG_BUF(int, slot, nullptr, 4 * P);
        dm_launch_commit(c, njobs, dj, xyz, ok, tidx, slot);
        break; }
    case SVSLAM_DMAP_STAGE_BA_GATHER: {
        DBG_NEED(badev); DBG_NEED(poses); DBG_NEED(pts); DBG_NEED(packed); DBG_NEED(uv); DBG_NEED(edge_ref); DBG_NEED(lm_slot_of);
        if (io->threads != 512 && io->threads != 1024) return fail(c, "debug_dmap_stage: the gather runs with 512 or 1024 threads, not %d", io->threads);
        DBG_BUF(BaDev, bd, io->badev, sizeof(BaDev) * n);
        DBG_BUF(double, poses, io->poses, 56 * n * (size_t)MK);
        DBG_BUF(double, pts, io->pts, 24 * n * (size_t)NL);
        DBG_BUF(unsigned int, pk, io->packed, 4 * E);
        DBG_BUF(float2, uv, io->uv, 8 * E);
        DBG_BUF(int, ref, io->edge_ref, 4 * E);
        DBG_BUF(int, lms, io->lm_slot_of, 4 * n * (size_t)NL);
        const int tile_cap = ba_tile_cap(MK);
        const size_t aux_stride = ba_aux_layout(MK, NL, MO, MO, MK, 0, ba_tile_bound(NL, MO, MK, tile_cap)).total + ba_pitem_bound(MO, MK);
        dm_launch_ba_gather(c, njobs, io->threads == 1024, dj, prm, bd, poses, pts, pk, uv, ref, lms, MK, tile_cap, aux_stride);
        break; }
    case SVSLAM_DMAP_STAGE_BA_SCATTER: {
        DBG_NEED(badev); DBG_NEED(poses); DBG_NEED(pts); DBG_NEED(chi2); DBG_NEED(edge_ref); DBG_NEED(lm_slot_of);
        for (int i = 0; i < njobs; ++i) {
            const int *bd = io->badev + (size_t)i * SVSLAM_DMAP_BADEV_INTS;
            const int nkf = bd[1], nlm = bd[3], nobs = bd[5];
            if (nkf < 0 || nkf > MK || nlm < 0 || nlm > NL || nobs > MO) return fail(c, "debug_dmap_stage: job %d: problem of %d / %d / %d over the strides", i, nkf, nlm, nobs);
            for (int a = 0; a < nkf; ++a) if (jobs[i].win_slot[a] < 0 || jobs[i].win_slot[a] >= KW) return fail(c, "debug_dmap_stage: job %d: win_slot[%d] out of range", i, a);
            for (int e = 0; e < nobs; ++e) {
                const int r = io->edge_ref[(size_t)i * MO + e];
                if (r < 0 || (r >> 16) >= KW || ((r >> 1) & 0x7fff) >= NF) return fail(c, "debug_dmap_stage: job %d: edge_ref[%d] out of range", i, e);
            }
            for (int v = 0; v < nlm; ++v) {
                const int l = io->lm_slot_of[(size_t)i * NL + v];
                if (l < 0 || l >= NL) return fail(c, "debug_dmap_stage: job %d: lm_slot_of[%d] out of range", i, v);
            }
        }
        DBG_BUF(BaDev, bd, io->badev, sizeof(BaDev) * n);
        DBG_BUF(double, poses, io->poses, 56 * n * (size_t)MK);
        DBG_BUF(double, pts, io->pts, 24 * n * (size_t)NL);
        DBG_BUF(double, chi, io->chi2, 8 * E);
        DBG_BUF(int, ref, io->edge_ref, 4 * E);
        DBG_BUF(int, lms, io->lm_slot_of, 4 * n * (size_t)NL);
        dm_launch_ba_scatter(c, njobs, dj, prm, bd, poses, pts, chi, ref, lms, MK);
        break; }
    case SVSLAM_DMAP_STAGE_REFRESH:
        dm_launch_refresh(c, njobs, dj);
        break;
    case SVSLAM_DMAP_STAGE_REFRESH_XYZ: {
        if (rt_slots_ok()) return -1;
        std::vector<int> l3(3 * n);
        for (int i = 0; i < njobs; ++i) { l3[3 * (size_t)i] = jobs[i].stream; l3[3 * (size_t)i + 1] = jobs[i].src_buf; l3[3 * (size_t)i + 2] = jobs[i].npts; }
        DBG_BUF(int, d3, nullptr, 12 * n);
        HIPCHK(c, hipMemcpy(d3, l3.data(), 12 * n, hipMemcpyHostToDevice));
        dm_launch_refresh_xyz(c, njobs, d3);
        break; }
    default:
        return fail(c, "debug_dmap_stage: unknown stage %d", stage);
    }
#undef DBG_NEED
#undef DBG_BUF
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, B.download());
    return 0;
}

} // extern "C"
