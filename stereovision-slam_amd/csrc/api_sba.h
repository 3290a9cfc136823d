// api_sba.h — included by svslam_hip.hip.  Entry points: svslam_sba_* (shared-map BA, its RCCL loader RcclApi), svslam_device_count.
// Owns of svslam_ctx: sba, sbac.

extern "C" {

// ------------------------------------------------------------------ shared-map BA (BASELINE config 5)
// One problem, its landmarks sharded over the ranks of a node: this rank opens its shard (all K poses, its
// landmarks and their edges), then drives the LM trial pieces of k_local_ba_t<1>; what has to be summed over
// the ranks goes through `io` (host memory; the caller all-reduces it with RCCL).  See k_ba.h:SbaArgs.
int svslam_sba_io_doubles(int nkf) { return (int)SBA_IO_DOUBLES(6 * nkf); }

int svslam_sba_open(svslam_ctx *c, const double cam_l[4], const double ext_l[7], const double cam_r[4], const double ext_r[7],
                    int nkf, const double *poses, int nlm, const double *pts, int nobs, const int *obs_kf, const int *obs_lm,
                    const uint8_t *obs_is_right, const float *obs_uv, double huber_delta)
{
    if (c->ba_pending.active || c->sba.open) return fail(c, "sba_open: the context already holds a BA batch");
    if (nkf < 1 || nkf > c->lim.max_kf || nlm < 1 || nlm > c->lim.max_lm || nobs < 1 || nobs > c->lim.max_obs)
        return fail(c, "sba_open: shard exceeds limits or is empty (kf %d/%d lm %d/%d obs %d/%d)", nkf, c->lim.max_kf, nlm, c->lim.max_lm, nobs, c->lim.max_obs);
    c->ar.reset();
    const int tile_cap = ba_tile_cap(c->lim.max_kf);
    const size_t TO = (size_t)nobs;
    size_t ocams = c->ar.take(sizeof(BaCams));
    size_t opk_o = c->ar.take(sizeof(unsigned int) * TO), osrt_o = c->ar.take(sizeof(int) * TO);
    size_t ouv_o = c->ar.take(sizeof(float) * 2 * TO);
    size_t ojobs = c->ar.take(sizeof(BaDev));
    size_t oposes = c->ar.take(sizeof(double) * 7 * nkf);
    size_t opts = c->ar.take(sizeof(double) * 3 * nlm);
    size_t in_end = c->ar.off;
    size_t ochi = c->ar.take(sizeof(double) * TO);
    size_t oflag = c->ar.take(sizeof(int) * 4);
    size_t oio = c->ar.take(sizeof(double) * SBA_IO_DOUBLES(6 * nkf));
    size_t orecs = c->ar.take(sizeof(BaRec) * 2 * TO);
    size_t oaux = c->ar.take(0);
    BaCams *cams = hp<BaCams>(c, ocams);
    memcpy(cams->cam[0], cam_l, 32); memcpy(cams->cam[1], cam_r, 32);
    memcpy(cams->ext[0], ext_l, 56); memcpy(cams->ext[1], ext_r, 56);
    int *srt = hp<int>(c, osrt_o);
    unsigned int *pk = hp<unsigned int>(c, opk_o);
    bool sorted = true;
    for (int e = 0; e < nobs; ++e) {
        const int k = obs_kf[e], l = obs_lm[e];
        if (k < 0 || k >= nkf || l < 0 || l >= nlm) return fail(c, "sba_open: edge %d index out of range", e);
        if (e && !((obs_lm[e - 1] < l) || (obs_lm[e - 1] == l && obs_kf[e - 1] <= k))) sorted = false;
        srt[e] = e;
        pk[e] = (unsigned int)l | ((unsigned int)k << 16) | ((obs_is_right[e] ? 1u : 0u) << 24);
    }
    if (!sorted) std::stable_sort(srt, srt + nobs, [&](int a, int b) { return obs_lm[a] != obs_lm[b] ? obs_lm[a] < obs_lm[b] : obs_kf[a] < obs_kf[b]; });
    BaDev &d = *hp<BaDev>(c, ojobs);
    d.kf_ofs = 0; d.nkf = nkf; d.lm_ofs = 0; d.nlm = nlm; d.obs_ofs = 0; d.nobs = nobs;
    d.nblk = d.na = d.ncontrib = d.ntile = 0; d.iters_done = 0; d.rec_ofs = 0; d.nmv = 0; d.reserved = sorted ? 1 : 0;
    d.lay_nblk = nobs; d.lay_na = nkf; d.lay_ntile = ba_tile_bound(nlm, nobs, nkf, tile_cap);
    d.aux_ofs = 0; d.lm_base = 0; d.shmask = 0; d.ntrial = 0;
    (void)c->ar.take(sizeof(int) * (ba_aux_layout(nkf, nlm, nobs, d.lay_nblk, d.lay_na, 0, d.lay_ntile).total + ba_pitem_bound(nobs, nkf)));
    if (c->ar.off > c->ar.cap) return fail(c, "sba_open: staging arena too small");
    memcpy(hp<void>(c, ouv_o), obs_uv, sizeof(float) * 2 * TO);
    memcpy(hp<void>(c, oposes), poses, sizeof(double) * 7 * nkf);
    memcpy(hp<void>(c, opts), pts, sizeof(double) * 3 * nlm);
    hp<int>(c, oflag)[0] = 0;
    if (h2d(c, 0, in_end)) return -1;
    if (h2d(c, oflag, oflag + sizeof(int) * 4)) return -1;
    hipLaunchKernelGGL(k_ba_build, dim3(1), dim3(BB_THREADS), bb_lds_bytes(nlm, nobs), c->stream, dp<BaDev>(c, ojobs), dp<unsigned int>(c, opk_o),
                       dp<float2>(c, ouv_o), dp<int>(c, osrt_o), dp<BaRec>(c, orecs),
                       dp<int>(c, oaux), tile_cap, nlm, dp<int>(c, oflag), 1 /* every keyframe active on every rank */,
                       bb_edge_cache_fits(nlm, nobs) ? 1 : 0, 0);
    HIPCHK(c, hipGetLastError());
    if (d2h_sync(c, oflag, oflag + sizeof(int) * 4)) return -1;
    if (hp<int>(c, oflag)[0]) return fail(c, "sba_open: the structure build overflowed a capacity");
    c->sba.open = true; c->sba.nkf = nkf; c->sba.nlm = nlm; c->sba.nobs = nobs; c->sba.np = 6 * nkf;
    c->sba.ojobs = ojobs; c->sba.ocams = ocams; c->sba.oposes = oposes; c->sba.opts = opts; c->sba.orecs = orecs; c->sba.oaux = oaux;
    c->sba.ochi = ochi; c->sba.oio = oio; c->sba.delta = huber_delta; c->sba.launches = 0;
    return 0;
}

// phase: 1 diagonal (lambda_0), 2 linearise at lambda, 3 solve with the reduced system in io + update + errors,
//        4 reject (restore), 5 finalise.  io: svslam_sba_io_doubles(nkf) doubles, in for phase 3, out for 1-3.
static int sba_launch(svslam_ctx *c, int phase, double lambda, int add_lambda)
{
    SbaArgs a{ phase, c->sba.launches == 0 ? 1 : 0, lambda, dp<double>(c, c->sba.oio), nullptr, add_lambda, nullptr, nullptr, nullptr, 0 };
    tm_begin(c, FAM_BA, 1);
    hipLaunchKernelGGL((k_local_ba_t<1, 1>), dim3(1), dim3(BA_THREADS), ba_lds_bytes(c->lim.max_kf), c->stream, dp<BaDev>(c, c->sba.ojobs),
                       dp<BaCams>(c, c->sba.ocams), dp<double>(c, c->sba.oposes), dp<double>(c, c->sba.opts), dp<BaRec>(c, c->sba.orecs),
                       dp<int>(c, c->sba.oaux), c->bw, c->sba.delta, 1, dp<double>(c, c->sba.ochi), (long long *)nullptr,
                       ba_tile_cap(c->lim.max_kf), a);
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    c->sba.launches++;
    return 0;
}

int svslam_sba_phase(svslam_ctx *c, int phase, double lambda, double *io)
{
    if (!c->sba.open) return fail(c, "sba_phase: no shard is open");
    if (phase < 1 || phase > 5) return fail(c, "sba_phase: phase %d", phase);
    const size_t nio = SBA_IO_DOUBLES(c->sba.np) * sizeof(double);
    if (phase == 3) { memcpy(hp<void>(c, c->sba.oio), io, nio); if (h2d(c, c->sba.oio, c->sba.oio + nio)) return -1; }
    else HIPCHK(c, hipMemsetAsync(dp<void>(c, c->sba.oio), 0, nio, c->stream));
    if (sba_launch(c, phase, lambda, 0)) return -1;
    if (d2h_sync(c, c->sba.oio, c->sba.oio + nio)) return -1;
    if (io && phase <= 3) memcpy(io, hp<void>(c, c->sba.oio), nio);
    return 0;
}

// ---- the shared-map LM as a product path: the control flow of g2o's Levenberg-Marquardt (exactly the loop of
// k_local_ba_t<0> / shared_ba.py) in the library, the reduced camera system all-reduced IN PLACE on the device buffer
// by RCCL (ncclAllReduce on the context's stream: (6K)^2 + 3 (6K) + 1 doubles per trial, 3 781 at K = 10, plus two
// scalars), no host copy of the system, two launches and one 64-byte read-back per trial.
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi *rccl_api(std::string *why)
{
    static RcclApi api;
    static std::once_flag once;
    static std::string err;
    std::call_once(once, [] {
        // RCCL must sit on the SAME HIP runtime as this library (a hipStream_t means nothing to another runtime), and
        // PyTorch-ROCm ships its own libamdhip64.so + librccl.so: in a process that imported torch first this library
        // is bound to torch's runtime, otherwise to the ROCm installation's.  So: the librccl next to the
        // libamdhip64 this library actually resolved (dladdr), then the generic names.  SVSLAM_RCCL_LIB overrides.
        if (const char *e = std::getenv("SVSLAM_RCCL_LIB")) api.lib = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
        Dl_info di;
        if (!api.lib && dladdr(reinterpret_cast<void *>(&hipStreamCreateWithFlags), &di) && di.dli_fname) {
            std::string dir(di.dli_fname);
            const size_t sl = dir.rfind('/');
            if (sl != std::string::npos) {
                dir.resize(sl + 1);
                for (const char *n : { "librccl.so.1", "librccl.so" }) {
                    api.lib = dlopen((dir + n).c_str(), RTLD_NOW | RTLD_GLOBAL);
                    if (api.lib) break;
                }
            }
        }
        for (const char *n : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
            if (api.lib) break;
            api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!api.lib) { err = std::string("librccl.so not found: ") + dlerror(); return; }
#define SVS_RCCL_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.lib, name)); if (!api.field) err = std::string("missing RCCL symbol ") + name
        SVS_RCCL_SYM(GetUniqueId, "ncclGetUniqueId"); SVS_RCCL_SYM(CommInitRank, "ncclCommInitRank");
        SVS_RCCL_SYM(CommDestroy, "ncclCommDestroy"); SVS_RCCL_SYM(AllReduce, "ncclAllReduce");
        SVS_RCCL_SYM(GroupStart, "ncclGroupStart"); SVS_RCCL_SYM(GroupEnd, "ncclGroupEnd");
        SVS_RCCL_SYM(GetErrorString, "ncclGetErrorString"); SVS_RCCL_SYM(CommAbort, "ncclCommAbort");
#undef SVS_RCCL_SYM
    });
    if (!err.empty()) { if (why) *why = err; return nullptr; }
    return &api;
}
} // namespace

int svslam_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// 128 bytes that rank 0 creates and hands to every rank (over any channel: torch.distributed, MPI, a file)
int svslam_sba_comm_unique_id(char out128[128])
{
    std::string why;
    RcclApi *r = rccl_api(&why);
    if (!r) return -1;
    ncclUniqueId id;
    static_assert(sizeof(id) == 128, "ncclUniqueId");
    if (r->GetUniqueId(&id) != ncclSuccess) return -2;
    memcpy(out128, &id, 128);
    return 0;
}
int svslam_sba_comm_init(svslam_ctx *c, int nranks, int rank, const char id128[128])
{
    if (c->sbac.comm) return fail(c, "sba_comm_init: the context already has a communicator");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, "sba_comm_init: rank %d of %d", rank, nranks);
    std::string why;
    RcclApi *r = rccl_api(&why);
    if (!r) return fail(c, "sba_comm_init: %s", why.c_str());
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    const ncclResult_t rc = r->CommInitRank(&c->sbac.comm, nranks, id, rank);
    if (rc != ncclSuccess) { c->sbac.comm = nullptr; return fail(c, "ncclCommInitRank: %s", r->GetErrorString(rc)); }
    c->sbac.nranks = nranks; c->sbac.rank = rank;
    return 0;
}
int svslam_sba_comm_destroy(svslam_ctx *c)
{
    if (!c->sbac.comm) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    RcclApi *r = rccl_api(nullptr);
    if (r) (void)r->CommDestroy(c->sbac.comm);
    c->sbac.comm = nullptr; c->sbac.nranks = 1; c->sbac.rank = 0;
    return 0;
}

// The whole optimize(iters) of the open shard.  trace (optional): 6 doubles per LM trial as svslam_lm_trace;
// stats (optional, 4 doubles): trials, milliseconds in total, mean milliseconds per trial, all-reduced bytes per trial.
static int sba_solve_impl(svslam_ctx *c, int iters, int *iters_done, double *lambda_out, double *trace, int trace_cap,
                          int *n_trace, double *stats);
// A rank that fails inside the LM loop (launch, copy, collective) would leave its peers waiting in their next all-reduce:
// the communicator is aborted (ncclCommAbort), so the peers' collectives return with an error instead of hanging; the
// context needs a new communicator (svslam_sba_comm_init) before the next shared-map solve.
int svslam_sba_solve(svslam_ctx *c, int iters, int *iters_done, double *lambda_out, double *trace, int trace_cap,
                     int *n_trace, double *stats)
{
    const int rc = sba_solve_impl(c, iters, iters_done, lambda_out, trace, trace_cap, n_trace, stats);
    if (rc != 0 && c->sbac.comm) {
        RcclApi *r = rccl_api(nullptr);
        if (r && r->CommAbort) { (void)r->CommAbort(c->sbac.comm); c->sbac.comm = nullptr; c->err += " (shared-map communicator aborted)"; }
    }
    return rc;
}
static int sba_solve_impl(svslam_ctx *c, int iters, int *iters_done, double *lambda_out, double *trace, int trace_cap,
                          int *n_trace, double *stats)
{
    if (!c->sba.open) return fail(c, "sba_solve: no shard is open");
    RcclApi *r = c->sbac.comm ? rccl_api(nullptr) : nullptr;
    const int n = c->sba.np;
    const size_t oS = 0, ohd = (size_t)n * n + 2 * (size_t)n, osc = ohd + n;
    double *dio = dp<double>(c, c->sba.oio);
    double *hio = hp<double>(c, c->sba.oio);
    const size_t off_sc = c->sba.oio + osc * sizeof(double);
    auto allreduce = [&](double *buf, size_t cnt, ncclRedOp_t op) -> int {
        if (!r) return 0;                               // one rank, no communicator: the sums are the local values
        const ncclResult_t rc = r->AllReduce(buf, buf, cnt, ncclDouble, op, c->sbac.comm, c->stream);
        return rc == ncclSuccess ? 0 : fail(c, "ncclAllReduce: %s", r->GetErrorString(rc));
    };
    const long long t_begin = now_ns();
    HIPCHK(c, hipMemsetAsync(dio, 0, SBA_IO_DOUBLES(n) * sizeof(double), c->stream));
    double lam = 0, ni = 2, current = 0;
    bool have_current = false;
    int it_done = 0, ntr = 0, trials = 0;
    for (int it = 0; it < iters; ++it) {
        if (it == 0) {
            if (sba_launch(c, 1, 0.0, 0)) return -1;
            if (allreduce(dio + ohd, (size_t)n, ncclSum)) return -1;
            if (allreduce(dio + osc + 1, 1, ncclMax)) return -1;
            if (d2h_sync(c, c->sba.oio + ohd * sizeof(double), c->sba.oio + (osc + 8) * sizeof(double))) return -1;
            double md = hio[osc + 1];
            for (int i = 0; i < n; ++i) md = std::max(md, std::fabs(hio[ohd + i]));
            lam = 1e-5 * md; ni = 2;
            // the diagonal sits inside the range every trial all-reduces (S | bs | bp | hd | chi2) and no later phase rewrites
            // it: zeroed here, it stays zero under the sums instead of growing by the rank count per trial
            HIPCHK(c, hipMemsetAsync(dio + ohd, 0, sizeof(double) * (size_t)n, c->stream));
        }
        double rho = 0; int qmax = 0;
        for (;;) {
            if (sba_launch(c, 2, lam, 0)) return -1;
            if (allreduce(dio + oS, osc + 1, ncclSum)) return -1;               // S | bs | bp | (hd) | chi2
            if (sba_launch(c, 3, lam, 1)) return -1;                               // adds lambda I itself
            if (r) {                                                               // landmark part of the rho denominator, chi2 of the trial
                if (r->GroupStart() != ncclSuccess) return fail(c, "ncclGroupStart");
                if (allreduce(dio + osc + 3, 1, ncclSum) || allreduce(dio + osc + 5, 1, ncclSum)) return -1;
                if (r->GroupEnd() != ncclSuccess) return fail(c, "ncclGroupEnd");
            }
            if (d2h_sync(c, off_sc, off_sc + 8 * sizeof(double))) return -1;
            const double *sc = hio + osc;
            if (!have_current) { current = sc[0]; have_current = true; }
            const bool ok = sc[2] != 0.0;
            const double temp = ok ? sc[5] : 1.7976931348623157e308;
            const double scale = sc[3] + sc[4] + 1e-3;
            rho = (current - temp) / scale;
            const bool accept = rho > 0 && std::isfinite(temp);
            if (trace && ntr < trace_cap) {
                double *t = trace + 6 * (size_t)ntr++;
                t[0] = it; t[1] = lam; t[2] = current; t[3] = temp; t[4] = rho; t[5] = accept ? 1.0 : 0.0;
            }
            ++trials;
            if (accept) {
                const double t = 2 * rho - 1;
                const double alpha = std::min(1.0 - t * t * t, 2.0 / 3.0);
                lam *= std::max(1.0 / 3.0, alpha); ni = 2; current = temp;
            } else {
                lam *= ni; ni *= 2;
                if (sba_launch(c, 4, lam, 0)) return -1;
                if (!std::isfinite(lam)) break;
            }
            ++qmax;
            if (!(rho < 0 && qmax < 10)) break;
        }
        ++it_done;
        if (qmax == 10 || rho == 0 || !std::isfinite(lam)) break;
    }
    if (sba_launch(c, 5, lam, 0)) return -1;
    if (d2h_sync(c, off_sc, off_sc + 8 * sizeof(double))) return -1;
    if (iters_done) *iters_done = it_done;
    if (lambda_out) *lambda_out = lam;
    if (n_trace) *n_trace = ntr;
    if (stats) {
        const double ms = (now_ns() - t_begin) / 1e6;
        stats[0] = trials; stats[1] = ms; stats[2] = trials ? ms / trials : 0.0;
        stats[3] = (double)((osc + 1 + 2) * sizeof(double));
    }
    return 0;
}

// poses of all keyframes, the shard's landmark positions and per-edge chi2 (after phase 5); closes the shard
int svslam_sba_close(svslam_ctx *c, double *poses, double *pts, double *edge_chi2)
{
    if (!c->sba.open) return fail(c, "sba_close: no shard is open");
    c->sba.open = false;
    if (d2h_sync(c, c->sba.oposes, c->sba.ochi + sizeof(double) * (size_t)c->sba.nobs)) return -1;
    if (poses) memcpy(poses, hp<void>(c, c->sba.oposes), sizeof(double) * 7 * c->sba.nkf);
    if (pts) memcpy(pts, hp<void>(c, c->sba.opts), sizeof(double) * 3 * c->sba.nlm);
    if (edge_chi2) memcpy(edge_chi2, hp<void>(c, c->sba.ochi), sizeof(double) * c->sba.nobs);
    return 0;
}

} // extern "C"
