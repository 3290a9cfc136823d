// svslam_hip.hip — C-ABI entry points of libsvslam_hip.so (see include/svslam.h).
// Host side: context, HBM-resident pyramid slots, one pinned staging arena
// (one H2D + one D2H per batched call), launches on the context's own stream.
// No CPU fallback exists: if no HIP device is usable svslam_create fails.
// This file holds what every family shares: the context, the staging arena, DevBuf (a device buffer kept between calls), timing
// and waiting, the kernel launchers that more than one family uses, create / destroy.  The entry points of the families are in
// the api_*.h files included at its end: one translation unit, one file per family.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <ctime>
#include <sys/prctl.h>
#include <new>
#include <string>
#include <tuple>
#include <vector>
#include <rocprim/rocprim.hpp>     // header-only: the two radix sorts and the scan of the cloud filters (k_cloud_filter.h)

#include <dlfcn.h>
// RCCL is bound with dlopen when a shared-map communicator is asked for; the few types and constants of its C API used here
// are declared below (values of rccl.h, the NCCL ABI), so that building this library needs no RCCL headers
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclSum = 0, ncclMax = 2 } ncclRedOp_t;
typedef enum { ncclDouble = 8 } ncclDataType_t;
}
#include "../../include/svslam.h"
#include "../host/thread_pool.h"
#include <atomic>
#include <memory>
#include <mutex>
#include "dev_common.h"
#include "k_pyramid.h"
#include "k_lk.h"
#include "k_gftt.h"
#include "k_geom.h"
#include "k_ba.h"
#include "k_ba_build.h"
#include "k_ba_ll.h"
#include "k_dmap.h"
#include "k_stereo_bm.h"
#include "k_cloud_filter.h"
#include "k_pose_graph.h"
#include "k_loop_verify.h"
#include "k_local_fusion.h"
#include "k_brief.h"
#include "k_loop_candidates.h"
#include "k_global_desc.h"
#include "k_colour.h"
#include "k_orb.h"
#include "k_orb_desc.h"

#define SVSLAM_DMAP_CHUNK 512     /* keyframe jobs per svslam_dmap_keyframe_batch call the staging arena is sized for */
#define SVSLAM_DMAP_EVICT_PER_JOB 512   /* evicted-landmark records per job of a call (shared by the call's jobs; the surplus waits) */
#define SVSLAM_LL_MAX_PROBLEMS 8        /* local-BA problems per call that the low-latency path (one problem over several workgroups) takes */

namespace {

enum { FAM_PYR = 0, FAM_LK, FAM_GFTT, FAM_TRI, FAM_POSE, FAM_BA,
       FAM_BM,         // family 6 of svslam_timing_get: the dense-stereo kernels (k_bm_fill + k_stereo_bm [+ k_dense_cloud])
       FAM_DBG0, FAM_DBG1, FAM_DBG2, FAM_DBG3,      // development (SVSLAM_TIMING_SPLIT): 7 .. 10
       FAM_BA_SOLVE,   // 11: the local-BA solver kernel(s) alone, nested inside FAM_BA (gather + build + solve + scatter)
       FAM_CF,         // 12: "cloud_filter", the outlier-removal and voxel-grid kernels with their sorts (units = points); appended, nothing moved
       FAM_PG,         // 13: "pose_graph", svslam_pose_graph_batch (units = jobs); appended, nothing moved
       FAM_LV,         // 14: "loop_verify", svslam_loop_verify_batch (units = jobs); appended, nothing moved
       FAM_BRIEF,      // 15: "brief", svslam_brief_describe_batch (units = points); appended, nothing moved
       FAM_LC,         // 16: "loop_candidates", svslam_loop_candidates_batch (units = rows compared); appended, nothing moved
       FAM_GD,         // 17: "global_desc", svslam_gdesc_describe_batch (units = jobs); appended, nothing moved
       FAM_COL,        // 18: "colour", k_bgr_prepare of svslam_pyramid_bgr_batch (units = images); appended, nothing moved
       FAM_LF,         // 19: "local_fusion", svslam_local_fusion_batch (units = jobs); appended, nothing moved
       FAM_ORB,        // 20: "orb", svslam_orb_detect_batch (units = jobs); appended, nothing moved
       FAM_ORBD,       // 21: "orb_desc", svslam_orb_describe_batch (units = points); appended, nothing moved
       FAM_COUNT };

struct Timing {
    double ms[FAM_COUNT] = { 0 };
    long long launches[FAM_COUNT] = { 0 };
    long long units[FAM_COUNT] = { 0 };
};

struct Arena {
    unsigned char *h = nullptr; // pinned host
    unsigned char *d = nullptr; // device mirror
    size_t cap = 0, off = 0;
    void reset() { off = 0; }
    size_t take(size_t bytes)
    {
        size_t o = (off + 255) & ~(size_t)255;
        off = o + bytes;
        return o;
    }
};

// A device buffer that a family keeps between calls and grows when a call needs more.  Where the family stages through host
// memory the mirror lives here too: pageable (h), or pinned and as large as the device side (pin: the image upload area).
// The context's destructor frees it; svslam_destroy has set the device and drained the stream by then.
struct DevBuf {
    unsigned char *d = nullptr;
    size_t cap = 0;
    std::vector<unsigned char> h;
    unsigned char *pin = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { (void)hipFree(d); if (pin) (void)hipHostFree(pin); d = pin = nullptr; cap = 0; }
    // at least `bytes` on the device (a regrow allocates bytes + headroom) and `host_bytes` in h; on failure the buffer is empty
    int reserve(svslam_ctx *c, const char *family, size_t bytes, size_t headroom, size_t host_bytes = 0, bool pinned = false);
};

} // namespace

struct svslam_ctx {
    svslam_limits lim;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    PyrGeom geom;
    std::vector<unsigned> dm_seen; unsigned dm_seen_gen = 0;     // svslam_dmap_keyframe_batch: streams of the current call (duplicate check)
    PyrFusedPlan pyr_plan;        // all levels in one launch (k_pyr_fused), when the geometry allows it
    bool pyr_fused = false;
    uint8_t *d_pyr = nullptr;
    Arena ar;
    // image upload area (host-pointer sources): the device copy and its pinned mirror
    DevBuf img;
    // GFTT scratch
    GfttWork gw;
    // dense stereo scratch (svslam_stereo_bm_batch / svslam_dense_cloud_batch), allocated at first use for max_jobs images
    struct { DevBuf disp, xyz, pix; } bm;
    // cloud filters (svslam_cloud_sor_batch / svslam_cloud_voxel_grid): device buffers sized at first use, grown on demand
    struct { DevBuf xyz, rgb, segs, keys, keys2, vals, vals2, soa, out, flag, pos, start, oxyz, orgb, tmp, climbs;
             long long queries = 0, climbed = 0; } cf;
    // pose graph (svslam_pose_graph_batch): one device buffer (inputs, results, solver scratch) and its pageable host mirror of the
    // uploaded part, sized at first use, grown on demand and kept
    struct : DevBuf { PgPlan plan; } pg;
    // loop verification (svslam_loop_verify_batch): one device buffer (results, inputs) and its pageable host mirror, grown on demand and kept
    DevBuf lv;
    // descriptors (svslam_brief_describe_batch): the same arrangement
    DevBuf br;
    // local fusion (svslam_local_fusion_batch): the same arrangement
    DevBuf lf;
    // ORB detector (svslam_orb_detect_batch): one device buffer (tables, jobs, rects, results, the jobs' levels, maps and lists of a
    // chunk) and its pageable host mirror of the uploaded part and the results; the last call's plan stays for svslam_orb_read_level
    struct : DevBuf { OrbPlan plan; bool have = false; } orb;
    // ORB descriptors (svslam_orb_describe_batch): one device buffer (geometry, tables, points, rows, results, the jobs' levels of a
    // chunk) and its host mirror of the uploaded part and the results
    struct : DevBuf { OdPlan plan; } orbd;
    // loop candidates: the resident store of normalised global descriptors (S on the device, H its bookkeeping) and a call's staging
    struct : DevBuf { LcStore S = {}; LcHost H; } lc;
    // global descriptor (svslam_gdesc_*): the configured network, its parameters and resize tables on the device, the workspace of a
    // chunk of jobs (ws) and a call's slots / vectors (io, with the host mirror of the vectors), allocated inside the call on demand and kept
    struct { GdNet N; float *d_prm = nullptr; int *d_tab = nullptr; DevBuf ws, io; } gd;
    // colour input of the dense program (svslam_colour_reserve / svslam_pyramid_bgr_batch / svslam_dense_cloud_bgr_batch): the
    // working-resolution BGR planes, which of them an upload has written, the staged grey images of a call, a call's point colours
    struct { DevBuf planes, grey, bgr; int nplanes = 0; std::vector<uint8_t> written; } col;
    // BA scratch
    BaWork bw;
    int bw_jobs = 0;          // problems per call the BA scratch holds
    bool ba_eid = false;      // the current BA call's cameras have identity extrinsic rotations (the reference's rig): the solver
                              // kernels' EID instantiations leave the products with Re's zeros and ones out (k_ba.h: ba_project)
    std::unique_ptr<svs::ThreadPool> pool;   // host-side per-problem preparation
    long long *d_ba_prof = nullptr;
    // low-latency local BA (svslam_set_low_latency): a problem is dealt over ll.w workgroups (k_ba_split, k_local_ba_t<2>)
    struct { int w = 0; BaDev *shards = nullptr; double *xch = nullptr; unsigned int *cnt = nullptr; size_t xch_stride = 0; BaWork bw;
             LlCaps caps = { 0, 0, 0 };          // caps.B > 0: problems whose shards fit go to the resident kernel (k_ba_ll)
             // The shards of a problem meet at in-launch barriers, so all of them have to be resident at once: max_problems is
             // what the occupancy of both solver kernels x the device's CUs allows (svslam_set_low_latency); calls with more
             // problems take the batch solver.  A shard that still never arrives (the CUs were taken by something else) makes
             // the problem give up after ~1 s; the call then solves it again with the batch solver (fallbacks counts those).
             int max_problems = 0, cus = 0, blocks_per_cu = 0; bool force_batch = false; int test_drop = 0; long long fallbacks = 0;
             // round 6: the give-up is a wall-clock limit per exchange (SVSLAM_LL_TIMEOUT_US, default 2000 us; 100 MHz ticks here);
             // coop: the two solver kernels go through hipLaunchCooperativeKernel (SVSLAM_LL_COOP=1; DESIGN 4.3 has the A/B)
             long long timeout_ticks = 200000; bool coop = false; long long coop_refused = 0;
             std::vector<BaDev> saved; } ll;
    double *d_lm_trace = nullptr;            // svslam_lm_trace test hook: [max_jobs][LM_TRACE_STRIDE]
    // host-side wall time (ns): 0 h2d enqueue, 1 d2h enqueue, 2 stream wait, 3 launches, 4 staging memcpy/prep
    long long host_ns[8] = { 0 };
    bool wait_poll = true;
    bool wait_block = false;    // SVSLAM_WAIT=block: the completion event sleeps in the driver (hipEventBlockingSync)
    bool low_latency = false;   // svslam_set_low_latency: 4-wave pose-only blocks
    double po_xtol = 1e-12;     // svslam_set_pose_only_xtol: parameter tolerance of the pose-only LM (0 = g2o's schedule to the last trial)
    bool zero_copy = false;     // low latency: the small job / result structs of the tracking path are read and written by the
                                // kernels straight in the pinned staging memory (no copy kernel, no boundary before / after it)
    bool timing_split = false;  // SVSLAM_TIMING_SPLIT: per-kernel events of the multi-kernel families (families 6..9)
    bool ba_host_build = false; // SVSLAM_BA_HOST_BUILD: problem structure on the host (the checker of k_ba_build), A/B
    int src_w = 0, src_h = 0;     // > 0: level 0 is the 2:1 decimation of src_w x src_h inputs
    // resident feature lists (svslam_rtrack_*): two alternating buffers per stream
    RtStore rt = {};
    std::vector<int> rt_which, rt_count;
    std::vector<DmEvicted> evicted;      // landmarks the last svslam_dmap_keyframe_batch freed (svslam_dmap_evicted)
    DMap dm = {};                 // device-resident maps (limits.device_map)
    void *dm_all = nullptr;
    int dm_stamp = 0;
    // a deferred local BA of the device map (svslam_dmap_params::ba_defer): its problem, solver scratch and a copy of the jobs
    // live in a buffer of their own (the staging arena is recycled by every call), the solve runs on a second stream
    struct { unsigned char *buf = nullptr; size_t cap = 0; bool inflight = false; int njobs = 0; hipStream_t stream = nullptr;
             hipEvent_t gathered = nullptr, solved = nullptr, t0 = nullptr, t1 = nullptr;
             size_t ojobs = 0, obd = 0, oposes = 0, opts = 0, ochi = 0, oref = 0, olms = 0, oflag = 0; DmParams prm; int MK = 0;
             BaCams cams; int ba_iters = 0; } dmba;
    hipEvent_t done = nullptr;   // recorded after the last enqueue of a call; the stream may be shared
    // a submitted, not yet collected local-BA batch owns the staging arena
    struct { bool active = false; int njobs = 0, total_kf = 0, total_lm = 0, total_obs = 0;
             size_t ojobs = 0, oposes = 0, opts = 0, ochi = 0, oflag = 0;
             // what a repeat with the batch solver needs when the low-latency solver gives up (svslam_local_ba_collect)
             bool ll_used = false; size_t ocams = 0, opk = 0, ouv = 0, osrt = 0, orecs = 0, oaux = 0, out_end = 0; int max_nlm = 0, max_nobs = 0, iters = 0;
             double delta = 0; } ba_pending;
    // svslam_debug_ba_struct reads these: the descriptors the last collected batch came back with, the edge_cache argument the
    // last k_ba_build launch got, and (host build only) whether each problem's edges arrived in order
    std::vector<BaDev> ba_last;
    int ba_last_ec = 0;
    std::vector<unsigned char> ba_host_in_order;
    // an open shared-map BA problem (svslam_sba_*): this rank's shard lives in the arena like a submitted batch
    struct { bool open = false; int nkf = 0, nlm = 0, nobs = 0, np = 0; size_t ojobs = 0, ocams = 0, oposes = 0, opts = 0, orecs = 0,
             oaux = 0, ochi = 0, oio = 0; double delta = 0; int launches = 0; } sba;
    // shared-map BA over RCCL (svslam_sba_comm_* / svslam_sba_solve): communicator of this context's rank
    struct { ncclComm_t comm = nullptr; int nranks = 1, rank = 0; } sbac;
    // timing
    bool timing = false;
    Timing tm;
    hipEvent_t ev[2 * 8];
    int nev = 0;
    int ev_open[4]; int ev_depth = 0;   // event pairs begun and not yet ended (an interval may nest inside another)
    int ev_fam[8];
    long long ev_units[8];
};

static void ll_release(svslam_ctx *c);

namespace {

int fail(svslam_ctx *c, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return -1;
}

#define HIPCHK(c, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) return fail((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

void make_geom(PyrGeom &g, int w, int h)
{
    memset(&g, 0, sizeof(g));
    size_t off = 0;
    int lw = w, lh = h, n = 0;
    for (int l = 0; l < SVS_LEVELS; ++l) {
        g.w[l] = lw; g.h[l] = lh;
        g.pitch[l] = (lw + 2 * SVS_BORDER + 15) & ~15;      // 16-byte rows (round 4: 64-byte rows cost 8 % more slot bytes for nothing measurable)
        g.ofs[l] = off;
        off += (size_t)g.pitch[l] * (lh + 2 * SVS_BORDER);
        off = (off + 255) & ~(size_t)255;
        n = l + 1;
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
        // buildOpticalFlowPyramid stops when the next level is not larger than the window
        if (lw <= SVSLAM_LK_WIN || lh <= SVSLAM_LK_WIN) break;
    }
    g.nlevels = n;
    g.slot_bytes = off;
}
// level 0 of every slot without its border, as the kernels that read whole images take it (BrImg, GdImg: the same fields)
template <class Img> Img level0_view(const svslam_ctx *c)
{
    const PyrGeom &g = c->geom;
    Img I;
    I.base = c->d_pyr; I.slot_bytes = g.slot_bytes; I.origin = g.ofs[0] + (size_t)SVS_BORDER * g.pitch[0] + SVS_BORDER;
    I.pitch = g.pitch[0]; I.w = g.w[0]; I.h = g.h[0];
    return I;
}

int DevBuf::reserve(svslam_ctx *c, const char *family, size_t bytes, size_t headroom, size_t host_bytes, bool pinned)
{
    if (bytes > cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        release();
        const size_t want = bytes + headroom;
        if (hipMalloc(&d, want) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
            return fail(c, "%s: no device memory for %zu bytes", family, want);
        }
        if (pinned && hipHostMalloc(&pin, want) != hipSuccess) {
            (void)hipGetLastError();
            pin = nullptr;
            release();
            return fail(c, "%s: no host memory for %zu bytes", family, want);
        }
        cap = want;
    }
    try { if (h.size() < host_bytes) h.resize(host_bytes); }
    catch (const std::bad_alloc &) { return fail(c, "%s: no host memory for %zu bytes", family, host_bytes); }
    return 0;
}

// HIP-event intervals of a call, on the stream the kernels are launched on.  Intervals may nest (the solver kernel inside the
// local-BA family): tm_end closes the innermost open one.  At most 8 intervals per call; beyond that they are not recorded.
void tm_begin(svslam_ctx *c, int fam, long long units)
{
    if (!c->timing) return;
    if (c->nev >= 8 || c->ev_depth >= 4) { if (c->ev_depth < 4) c->ev_open[c->ev_depth] = -1; c->ev_depth++; return; }
    const int slot = c->nev++;
    c->ev_open[c->ev_depth++] = slot;
    c->ev_fam[slot] = fam;
    c->ev_units[slot] = units;
    (void)hipEventRecord(c->ev[2 * slot], c->stream);
}
void tm_end(svslam_ctx *c)
{
    if (!c->timing || c->ev_depth <= 0) return;
    const int d = --c->ev_depth;
    const int slot = d < 4 ? c->ev_open[d] : -1;
    if (slot >= 0) (void)hipEventRecord(c->ev[2 * slot + 1], c->stream);
}
// pose-only LM: one wave per job by default, four when the context is in low-latency mode
void launch_pose_only(svslam_ctx *c, int njobs, PoseJob *jobs, const double *cam, const double *xyz, const float2 *uv,
                      const uint8_t *valid, uint8_t *outlier, double chi2_th, int rounds, int iters, const PoFuse *fz = nullptr)
{
    if (c->d_lm_trace) (void)hipMemsetAsync(c->d_lm_trace, 0, sizeof(double) * LM_TRACE_STRIDE * (size_t)njobs, c->stream);
    const PoFuse none = {};
    if (c->low_latency) {
        if (fz) hipLaunchKernelGGL((k_pose_only<4, true>), dim3(njobs), dim3(256), 0, c->stream, jobs, cam, xyz, uv, valid, outlier, chi2_th, rounds, iters, c->d_lm_trace, *fz, c->po_xtol);
        else hipLaunchKernelGGL((k_pose_only<4, false>), dim3(njobs), dim3(256), 0, c->stream, jobs, cam, xyz, uv, valid, outlier, chi2_th, rounds, iters, c->d_lm_trace, none, c->po_xtol);
    } else {
        if (fz) hipLaunchKernelGGL((k_pose_only<1, true>), dim3(njobs), dim3(64), 0, c->stream, jobs, cam, xyz, uv, valid, outlier, chi2_th, rounds, iters, c->d_lm_trace, *fz, c->po_xtol);
        else hipLaunchKernelGGL((k_pose_only<1, false>), dim3(njobs), dim3(64), 0, c->stream, jobs, cam, xyz, uv, valid, outlier, chi2_th, rounds, iters, c->d_lm_trace, none, c->po_xtol);
    }
}
void tm_collect(svslam_ctx *c)
{
    // call after the stream has been synchronised
    for (int i = 0; i < c->nev; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]) == hipSuccess) {
            c->tm.ms[c->ev_fam[i]] += ms;
            c->tm.launches[c->ev_fam[i]] += 1;
            c->tm.units[c->ev_fam[i]] += c->ev_units[i];
        }
    }
    c->nev = 0; c->ev_depth = 0;
}

// both extrinsics are pure translations: quaternion exactly (0, 0, 0, 1)
static bool ba_ext_identity(const double *ext_l, const double *ext_r)
{
    static const bool off = []{ const char *e = std::getenv("SVSLAM_BA_GENERIC_EXT"); return e && atoi(e) != 0; }();   // A/B and parity tests: the general code
    for (const double *e : { ext_l, ext_r }) if (!(e[0] == 0.0 && e[1] == 0.0 && e[2] == 0.0 && e[3] == 1.0)) return false;
    return !off;
}
// The local-BA solver of a batch whose structure the device builds: the batch kernel (one workgroup per problem), or — in
// low-latency mode, for a few problems with landmark-major edges — every problem dealt over ll.w workgroups.
// A solver kernel of the low-latency path: an ordinary launch, or — ll.coop — a cooperative one: the runtime then checks that the
// whole grid can be resident at once (and refuses the launch otherwise: counted, the ordinary launch + the in-kernel give-up
// take over) and runs cooperative launches of different streams one after the other, so two half-resident problems of two
// contexts cannot wait for each other's CUs.
template <class... P, class... A> void ll_launch(svslam_ctx *c, void (*kern)(P...), int nshards, size_t lds, A... a)
{
    if (c->ll.coop) {
        std::tuple<P...> args(a...);
        void *ptrs[sizeof...(P)];
        size_t i = 0;
        std::apply([&](auto &...x) { ((ptrs[i++] = (void *)&x), ...); }, args);
        if (hipLaunchCooperativeKernel(reinterpret_cast<const void *>(kern), dim3(nshards), dim3(BA_THREADS), ptrs, (unsigned)lds, c->stream) == hipSuccess) return;
        (void)hipGetLastError();
        c->ll.coop_refused++;
    }
    hipLaunchKernelGGL(kern, dim3(nshards), dim3(BA_THREADS), lds, c->stream, a...);
}
template <int W> void launch_ba_ll_t(svslam_ctx *c, int nshards, BaDev *shards, const BaCams *cams, double *poses, double *pts, const BaRec *recs,
                                      const int *aux, double delta, int iters, double *chi, int tile_cap, BaDev *parents)
{
    ll_launch(c, k_local_ba_t<2, W>, nshards, ba_lds_bytes_ll(c->lim.max_kf), shards, cams, poses, pts, recs, aux, c->ll.bw, delta, iters, chi,
              c->d_ba_prof, tile_cap,
              SbaArgs{ 0, 0, 0.0, nullptr, c->d_lm_trace, 0, c->ll.xch, c->ll.cnt, parents, c->ll.xch_stride, c->ll.timeout_ticks });
}
template <int W> void launch_ba_ll_resident(svslam_ctx *c, int nshards, BaDev *shards, const BaCams *cams, double *poses, double *pts, const BaRec *recs,
                                            const int *aux, double delta, int iters, double *chi, BaDev *parents)
{
    const SbaArgs sa{ 0, 0, 0.0, nullptr, c->d_lm_trace, 0, c->ll.xch, c->ll.cnt, parents, c->ll.xch_stride, c->ll.timeout_ticks };
    if (c->ba_eid)
        ll_launch(c, k_ba_ll<W, true>, nshards, ba_ll_lds_bytes(c->lim.max_kf, c->ll.caps), shards, cams, poses, pts, recs, aux, delta, iters, chi,
                  c->d_ba_prof, c->ll.caps, sa);
    else
        ll_launch(c, k_ba_ll<W, false>, nshards, ba_ll_lds_bytes(c->lim.max_kf, c->ll.caps), shards, cams, poses, pts, recs, aux, delta, iters, chi,
                  c->d_ba_prof, c->ll.caps, sa);
}
// test hook (SVSLAM_LL_TEST_DROP_SHARD = n: the next n low-latency launches): shard 0 of problem 0 never runs, its peers give up at
// their first exchange and the call falls back to the batch solver — the path a GPU without room for every shard takes
__global__ void k_ll_test_drop(BaDev *shards) { shards[0].reserved = 3; }
bool ba_ll_usable(const svslam_ctx *c, int njobs) { return c->low_latency && c->ll.w > 0 && !c->ll.force_batch && njobs <= c->ll.max_problems; }
// tile capacity the shards of the low-latency solver are built with: what both of its kernels can hold
int ba_ll_tile_cap(const svslam_ctx *c)
{
    const int t = ba_tile_cap_ll(c->lim.max_kf);
    return c->ll.caps.B > 0 ? std::min(t, c->ll.caps.B) : t;
}
void launch_ba_solver(svslam_ctx *c, int njobs, bool ll, BaDev *jobs, const BaCams *cams, double *poses, double *pts, const unsigned int *packed,
                      const float2 *uv, const int *srt, BaRec *recs, int *aux, double *chi, int *flag, int max_nlm, int max_nobs,
                      double delta, int iters, bool split_timing, bool time_solver = true)
{
    // (time_solver: FAM_BA_SOLVE interval around the solver kernel(s); off where the solve runs on a stream the call does not wait for)
    const bool tms = time_solver && !split_timing;
    const int tile_cap = ll ? ba_ll_tile_cap(c) : ba_tile_cap(c->lim.max_kf);
    const int ec = bb_edge_cache_fits(max_nlm, max_nobs) ? 1 : 0;
    c->ba_last_ec = ec;                        // what k_ba_build is told below (svslam_debug_ba_struct reports it)
    if (!ll) {
        hipLaunchKernelGGL(k_ba_build, dim3(njobs), dim3(BB_THREADS), bb_lds_bytes(max_nlm, max_nobs), c->stream, jobs, packed, uv, srt, recs, aux,
                           tile_cap, max_nlm, flag, 0, ec, 0);
        if (split_timing) { tm_end(c); tm_begin(c, FAM_DBG3, njobs); }
        const SbaArgs sa{ 0, 0, 0.0, nullptr, c->d_lm_trace, 0, nullptr, nullptr, nullptr, 0, 0 };
        if (tms) tm_begin(c, FAM_BA_SOLVE, njobs);
        if (c->ba_eid)
            hipLaunchKernelGGL((k_local_ba_t<0, 1, true>), dim3(njobs), dim3(BA_THREADS), ba_lds_bytes(c->lim.max_kf), c->stream, jobs, cams, poses, pts, recs, aux,
                               c->bw, delta, iters, chi, c->d_ba_prof, tile_cap, sa);
        else
            hipLaunchKernelGGL((k_local_ba_t<0, 1, false>), dim3(njobs), dim3(BA_THREADS), ba_lds_bytes(c->lim.max_kf), c->stream, jobs, cams, poses, pts, recs, aux,
                               c->bw, delta, iters, chi, c->d_ba_prof, tile_cap, sa);
        if (tms) tm_end(c);
        return;
    }
    const int W = c->ll.w;
    c->host_ns[6] += njobs;                    // svslam_debug_host_ns slot 6: problems the low-latency solver took
    hipLaunchKernelGGL(k_ba_split, dim3(njobs), dim3(SP_THREADS), ba_split_lds_bytes(max_nlm, W), c->stream, jobs, c->ll.shards, packed, W, tile_cap,
                       max_nlm, c->ll.xch, c->ll.xch_stride, c->ll.cnt, c->ll.caps.B, c->ll.caps.L, c->ll.caps.E);
    hipLaunchKernelGGL(k_ba_build, dim3(njobs * W), dim3(BB_THREADS), bb_lds_bytes(max_nlm, max_nobs), c->stream, c->ll.shards, packed, uv, srt, recs, aux,
                       tile_cap, max_nlm, flag, 1 /* every keyframe active in every shard */, ec, 1 /* every landmark in the tile */);
    if (split_timing) { tm_end(c); tm_begin(c, FAM_DBG3, njobs); }
    if (c->ll.test_drop > 0) { --c->ll.test_drop; hipLaunchKernelGGL(k_ll_test_drop, dim3(1), dim3(1), 0, c->stream, c->ll.shards); }
    // problems whose shards all fit LDS: the resident kernel; the others: the streaming one (each kernel skips the other's)
    if (tms) tm_begin(c, FAM_BA_SOLVE, njobs);
    if (c->ll.caps.B > 0) {
        if (W == 4) launch_ba_ll_resident<4>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, jobs);
        else if (W == 8) launch_ba_ll_resident<8>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, jobs);
        else launch_ba_ll_resident<16>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, jobs);
    }
    if (W == 4) launch_ba_ll_t<4>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, tile_cap, jobs);
    else if (W == 16) launch_ba_ll_t<16>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, tile_cap, jobs);
    else if (W == 8) launch_ba_ll_t<8>(c, njobs * W, c->ll.shards, cams, poses, pts, recs, aux, delta, iters, chi, tile_cap, jobs);
    if (tms) tm_end(c);
}

inline long long now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// Wait for the context's stream.  The runtime's own wait spins; with thousands of streams
// the host bookkeeping needs every core that would burn, so the default here is a short
// spin followed by sleep-polling (SVSLAM_WAIT=spin restores hipStreamSynchronize).
hipError_t wait_stream(svslam_ctx *c)
{
    if (!c->wait_poll) return hipEventSynchronize(c->done);
    static thread_local bool slack_set = false;
    if (!slack_set) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0); slack_set = true; }
    const long long t0 = now_ns();
    for (;;) {
        const hipError_t e = hipEventQuery(c->done);
        if (e != hipErrorNotReady) return e;
        const long long dt = now_ns() - t0;
        // low-latency mode (a few cameras per GPU): the wait IS the frame time, so the thread keeps polling — a nap of 20 us
        // plus its wake-up was a tenth of a lone camera's frame; beyond a few ms (nothing of that mode takes that long) it naps
        if (dt < (c->low_latency ? 3000000LL : 10000LL)) continue;
        // back off with the age of the wait: a 100 us kernel is polled every ~20 us, a
        // multi-millisecond BA batch every ~150 us (overshoot stays below ~1/8 of the wait)
        static const long long nap_min = []{ const char *e = std::getenv("SVSLAM_POLL_MIN_US"); return e ? atoll(e) * 1000 : 20000LL; }();
        static const long long nap_max = []{ const char *e = std::getenv("SVSLAM_POLL_MAX_US"); return e ? atoll(e) * 1000 : 150000LL; }();
        long long nap = dt >> 3;
        nap = nap < nap_min ? nap_min : (nap > nap_max ? nap_max : nap);
        struct timespec ts = { 0, (long)nap };
        nanosleep(&ts, nullptr);
    }
}
// HIP streams are handed out from a small per-device pool: beyond ~16 hardware queues the
// GPU time-slices them and every stream stalls, while a host that runs many single-threaded
// pipelines wants one context each.  Contexts that share a stream stay independent: each
// waits on its own event (done), never on the stream.  Pool streams live until process exit.
hipError_t pool_stream(int device, hipStream_t *out)
{
    static std::mutex m;
    static std::vector<hipStream_t> pool[64];
    static size_t next[64] = { 0 };
    std::lock_guard<std::mutex> lk(m);
    const char *e = std::getenv("SVSLAM_MAX_STREAMS");
    const size_t cap = (size_t)std::max(1, e ? atoi(e) : 16);
    std::vector<hipStream_t> &p = pool[device & 63];
    if (p.size() < cap) {
        hipStream_t s = nullptr;
        hipError_t rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (rc != hipSuccess) return rc;
        p.push_back(s);
        *out = s;
        return hipSuccess;
    }
    *out = p[next[device & 63]++ % std::min(p.size(), cap)];
    return hipSuccess;
}
int h2d(svslam_ctx *c, size_t from, size_t to)
{
    const long long t0 = now_ns();
    if (to > from) HIPCHK(c, hipMemcpyAsync(c->ar.d + from, c->ar.h + from, to - from, hipMemcpyHostToDevice, c->stream));
    c->host_ns[0] += now_ns() - t0;
    return 0;
}
int d2h_enqueue(svslam_ctx *c, size_t from, size_t to)
{
    const long long t0 = now_ns();
    if (to > from) HIPCHK(c, hipMemcpyAsync(c->ar.h + from, c->ar.d + from, to - from, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->done, c->stream));
    c->host_ns[1] += now_ns() - t0;
    return 0;
}
int finish(svslam_ctx *c)
{
    const long long t1 = now_ns();
    HIPCHK(c, wait_stream(c));
    const long long t0 = now_ns();
    c->host_ns[2] += t0 - t1;
    tm_collect(c);
    c->host_ns[5] += now_ns() - t0;
    return 0;
}
int d2h_sync(svslam_ctx *c, size_t from, size_t to)
{
    if (d2h_enqueue(c, from, to)) return -1;
    return finish(c);
}

template <typename T> T *hp(svslam_ctx *c, size_t off) { return reinterpret_cast<T *>(c->ar.h + off); }
template <typename T> T *dp(svslam_ctx *c, size_t off) { return reinterpret_cast<T *>(c->ar.d + off); }
// a staged struct array as the kernels see it: the device mirror, or (zero_copy) the pinned host memory itself — hipHostMalloc
// memory is mapped into the device's address space at the same address, coherent, and what a kernel wrote there is visible to
// the host once the event behind the kernel has completed
template <typename T> T *dpz(svslam_ctx *c, size_t off) { return c->zero_copy ? hp<T>(c, off) : dp<T>(c, off); }

// The staging arena (and job 0 of the BA scratch) belongs to a submitted, uncollected local-BA batch or to an
// open shared-map shard: every other batched call on the context is refused until collect / close.
int arena_busy(svslam_ctx *c)
{
    if (c->ba_pending.active) return fail(c, "a submitted local-BA batch owns this context: call svslam_local_ba_collect first");
    if (c->sba.open) return fail(c, "an open shared-map BA shard owns this context: call svslam_sba_close first");
    return 0;
}

int check_slot(svslam_ctx *c, int s)
{
    if (s < 0 || s >= c->lim.max_slots) return fail(c, "slot %d out of range [0,%d)", s, c->lim.max_slots);
    return 0;
}

// enqueue pyramid construction for n jobs whose PyrJob array is at device offset djobs
// ga (optional): the feature gather of resident tracking, riding on the fused launch as extra workgroups (gathered = true
// says it did; with the per-level kernels the caller launches k_rt_gather itself)
int launch_pyramid(svslam_ctx *c, const PyrJob *djobs, int n, bool decimate, int src_w, int src_h, const RtGatherArgs *ga = nullptr,
                   bool *gathered = nullptr)
{
    const PyrGeom &g = c->geom;
    tm_begin(c, FAM_PYR, n);
    if (c->pyr_fused) {
        RtGatherArgs a = {};
        a.chunks = 1;
        if (ga && ga->njobs > 0) { a = *ga; if (gathered) *gathered = true; }
        const dim3 grd(((n + 7) / 8) * 8 * c->pyr_plan.nstrips + a.njobs * a.chunks);      // jobs in groups of 8 (one per XCD), all strips of a job on its XCD
        if (decimate) hipLaunchKernelGGL(k_pyr_fused<true>, grd, dim3(PF_THREADS), c->pyr_plan.lds_bytes, c->stream, djobs, n, c->d_pyr, g, src_w, src_h, c->pyr_plan, a);
        else hipLaunchKernelGGL(k_pyr_fused<false>, grd, dim3(PF_THREADS), c->pyr_plan.lds_bytes, c->stream, djobs, n, c->d_pyr, g, src_w, src_h, c->pyr_plan, a);
        tm_end(c);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    auto fast_ok = [](int w, int h) { return w >= 18 && h >= 18; };
    if (fast_ok(g.w[0], g.h[0])) {
        dim3 blk(16, 16);
        dim3 grd(cdiv(cdiv(g.w[0], 16), 16), cdiv(g.h[0], 16), n);
        if (decimate) hipLaunchKernelGGL(k_pyr_level0_fast<true>, grd, blk, 0, c->stream, djobs, c->d_pyr, g, src_w, src_h);
        else hipLaunchKernelGGL(k_pyr_level0_fast<false>, grd, blk, 0, c->stream, djobs, c->d_pyr, g, src_w, src_h);
    } else {
        dim3 blk(64, 4);
        dim3 grd(cdiv((g.w[0] + 2 * SVS_BORDER + 3) / 4, 64), cdiv(g.h[0] + 2 * SVS_BORDER, 4), n);
        if (decimate) hipLaunchKernelGGL(k_pyr_level0<true>, grd, blk, 0, c->stream, djobs, c->d_pyr, g, src_w, src_h);
        else hipLaunchKernelGGL(k_pyr_level0<false>, grd, blk, 0, c->stream, djobs, c->d_pyr, g, src_w, src_h);
    }
    for (int l = 1; l < g.nlevels; ++l) {
        if (fast_ok(g.w[l], g.h[l])) {
            dim3 blk(32, 8);
            dim3 grd(cdiv(cdiv(g.w[l], 4), 32), cdiv(g.h[l], 8), n);
            hipLaunchKernelGGL(k_pyr_down_fast, grd, blk, 0, c->stream, djobs, c->d_pyr, g, l);
        } else {
            dim3 blk(64, 4);
            dim3 grd(cdiv(g.w[l] + 2 * SVS_BORDER, 64), cdiv(g.h[l] + 2 * SVS_BORDER, 4), n);
            hipLaunchKernelGGL(k_pyr_down, grd, blk, 0, c->stream, djobs, c->d_pyr, g, l);
        }
    }
    tm_end(c);
    HIPCHK(c, hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

const char *svslam_build_info(void)
{
#ifndef SVS_SRC_HASH
#define SVS_SRC_HASH "unstamped"
#endif
    return "libsvslam_hip gfx950 (hipcc " __VERSION__ "), -ffp-contract=off, src " SVS_SRC_HASH;
}

const char *svslam_last_error(const svslam_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int svslam_create(const svslam_limits *lim, svslam_ctx **out)
{
    if (!lim || !out) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "svslam_create: no HIP device available (this library has no CPU path)\n");
        return -2;
    }
    if (lim->device < 0 || lim->device >= ndev) return -3;
    if (lim->width < 16 || lim->height < 16 || lim->max_slots < 1 || lim->max_jobs < 1 || lim->max_pts < 1)
        return -4;
    if (lim->max_pts > PO_MAX_EDGES) return -5;
    if (lim->max_corners < 1 || lim->max_corners > GF_MAX_CORNERS) return -6;
    svslam_ctx *c = new (std::nothrow) svslam_ctx();
    if (!c) return -7;
    c->lim = *lim;
    c->device = lim->device;
    *out = c; // returned even on failure so the caller can read the error
    HIPCHK(c, hipSetDevice(c->device));
    {
        const char *wm = std::getenv("SVSLAM_WAIT");        // spin | block | poll (default)
        c->wait_poll = !(wm && (std::strcmp(wm, "spin") == 0 || std::strcmp(wm, "block") == 0));
        c->wait_block = wm && std::strcmp(wm, "block") == 0;
        c->timing_split = std::getenv("SVSLAM_TIMING_SPLIT") != nullptr;
        if (const char *xt = std::getenv("SVSLAM_PO_XTOL")) {      // 0: g2o's schedule; a value the setter would refuse fails the create
            char *end = nullptr;
            const double v = strtod(xt, &end);
            if (end == xt || !(v >= 0) || v > 1e-6) return fail(c, "svslam_create: SVSLAM_PO_XTOL=%s is outside [0, 1e-6]", xt);
            c->po_xtol = v;
        }
        // the device build takes the edge indices packed into one word (landmark < 2^16, keyframe < 2^8)
        c->ba_host_build = std::getenv("SVSLAM_BA_HOST_BUILD") != nullptr || lim->max_lm >= 65536 || lim->max_kf >= 256;
    }
    HIPCHK(c, pool_stream(c->device, &c->stream));
    HIPCHK(c, hipEventCreateWithFlags(&c->done, hipEventDisableTiming | (c->wait_block ? hipEventBlockingSync : 0)));
    for (int i = 0; i < 16; ++i) HIPCHK(c, hipEventCreate(&c->ev[i]));
    make_geom(c->geom, lim->width, lim->height);
    int pyr_lds_kb = 64;            // two strips' workgroups per CU; development: SVSLAM_PYR_LDS_KB = 32 .. 160
    if (const char *e = std::getenv("SVSLAM_PYR_LDS_KB")) { const int v = std::atoi(e); if (v >= 32 && v <= 160) pyr_lds_kb = v; }
    c->pyr_fused = !std::getenv("SVSLAM_PYR_LEGACY") && pyr_fused_plan(c->geom, pyr_lds_kb * 1024, c->pyr_plan);
    if (c->pyr_fused && c->pyr_plan.lds_bytes > 64 * 1024) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pyr_fused<true>), hipFuncAttributeMaxDynamicSharedMemorySize, c->pyr_plan.lds_bytes));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pyr_fused<false>), hipFuncAttributeMaxDynamicSharedMemorySize, c->pyr_plan.lds_bytes));
    }
    if (c->pyr_fused && std::getenv("SVSLAM_PYR_PROF")) {
        HIPCHK(c, hipMalloc(&c->pyr_plan.prof, sizeof(long long) * 8));
        HIPCHK(c, hipMemset(c->pyr_plan.prof, 0, sizeof(long long) * 8));
    }
    HIPCHK(c, hipMalloc(&c->d_pyr, c->geom.slot_bytes * (size_t)lim->max_slots));
    HIPCHK(c, hipMemsetAsync(c->d_pyr, 0, c->geom.slot_bytes * (size_t)lim->max_slots, c->stream));

    // staging arena: the largest batched call decides
    const size_t J = lim->max_jobs, N = lim->max_pts;
    size_t per_job_pts = N * (8 + 8 + 1 + 4 + 24 + 8 + 1 + 1 + 8) + 1024;
    size_t per_job_ba = (size_t)lim->max_kf * 56 + (size_t)lim->max_lm * 24 +
                        (size_t)lim->max_obs * (21 + 8 + 32 + 16 + 2 * (size_t)(lim->max_kf + 1) + 8) + (size_t)lim->max_lm * 16 + 8192;
    // (per edge: raw <= 21 B, chi2 8 B, two records 32 B, edge + block lists 16 B, pair items <= 2 (K + 1) B)
    per_job_ba += 4 * (size_t)(ba_tile_bound(lim->max_lm, lim->max_obs, lim->max_kf, std::max(ba_tile_cap(lim->max_kf), 64)) + 2) *
                  ((size_t)lim->max_kf * (lim->max_kf + 1) / 2 + 1);          // per-tile pair ranges at their upper bound
    per_job_ba += 4 * ba_split_aux_extra(lim->max_kf, LL_MAX_W);                  // low-latency shards of a problem (k_ba_split)
    size_t per_job = std::max(per_job_pts, per_job_ba) + (size_t)lim->max_corners * 8 + 4096;
    c->ar.cap = per_job * J + (1 << 20);
    if (lim->device_map) {
        // With the map on the device the big consumer — BA staging for max_jobs host-gathered problems — is not used:
        // the keyframe path takes at most SVSLAM_DMAP_CHUNK jobs per call and keeps its scratch device-side (the arena
        // mirrors host and device, and 12 contexts x 4 GB of pinned host memory per process was the price of the old
        // sizing).  Tracking calls still get their per-point staging for every job; host-side BA calls on such a
        // context are limited to 64 problems per call.
        const size_t MO = lim->max_obs, NL = lim->max_lm, NF = lim->max_pts, MK = lim->max_kf;
        const int tc = std::max(ba_tile_cap(lim->max_kf), 64);
        const size_t aux = ba_aux_layout((int)MK, (int)NL, (int)MO, (int)MO, (int)MK, 0, ba_tile_bound((int)NL, (int)MO, (int)MK, tc)).total + ba_pitem_bound((int)MO, (int)MK);
        const size_t per_dm = sizeof(DmJob) + NF * 80 + NL * 32 + MO * 64 + (aux + ba_split_aux_extra((int)MK, LL_MAX_W)) * 4 + MK * 56 + (size_t)lim->max_corners * 8 + 8192 +
                              sizeof(DmEvicted) * SVSLAM_DMAP_EVICT_PER_JOB;
        const size_t chunk = std::min<size_t>(SVSLAM_DMAP_CHUNK, (size_t)std::max(1, lim->max_streams));
        c->ar.cap = std::max(chunk * per_dm, std::max(per_job_pts * J, std::min<size_t>(J, 64) * per_job)) + (4 << 20);
    }
    HIPCHK(c, hipHostMalloc(&c->ar.h, c->ar.cap));
    HIPCHK(c, hipMalloc(&c->ar.d, c->ar.cap));

    // GFTT scratch
    const size_t P = (size_t)lim->width * lim->height;
    int cap = 1;
    while ((size_t)cap < P) cap <<= 1;
    c->gw.cap = cap;
    HIPCHK(c, hipMalloc(&c->gw.keys, sizeof(unsigned long long) * (size_t)cap * J));
    HIPCHK(c, hipMalloc(&c->gw.counters, sizeof(unsigned int) * GF_CNT_STRIDE * J));
    HIPCHK(c, hipMemsetAsync(c->gw.counters, 0, sizeof(unsigned int) * GF_CNT_STRIDE * J, c->stream));   // kept zero by k_gftt_select2
    c->gw.prof = nullptr;
    if (std::getenv("SVSLAM_GFTT_PROF")) {
        HIPCHK(c, hipMalloc(&c->gw.prof, sizeof(long long) * 16));
        HIPCHK(c, hipMemsetAsync(c->gw.prof, 0, sizeof(long long) * 16, c->stream));
    }
    // BA scratch
    if (lim->max_kf > 0) {
        if (6 * lim->max_kf > BA_MAX_NP) return fail(c, "max_kf %d too large (<= %d)", lim->max_kf, BA_MAX_NP / 6);
        if (ba_tile_cap(lim->max_kf) < std::max(lim->max_kf, 64) || ba_lds_bytes(lim->max_kf) > 160 * 1024) return fail(c, "max_kf %d: reduced system does not fit LDS", lim->max_kf);
        // per-problem solver scratch (0.5 MB + 0.2 KB per landmark slot): one per job of the largest BA call — with the map on the
        // device that is a keyframe chunk (or the 64 problems a host-side BA call may bring), not max_jobs
        c->bw_jobs = lim->device_map ? (int)std::max<size_t>(std::min<size_t>(SVSLAM_DMAP_CHUNK, (size_t)std::max(1, lim->max_streams)), std::min<size_t>(J, 64)) : lim->max_jobs;
        if (ba_work_alloc(c->bw, c->bw_jobs, lim->max_kf, lim->max_lm, lim->max_obs) != hipSuccess)
            return fail(c, "BA workspace allocation failed");
        for (const void *f : { reinterpret_cast<const void *>(k_local_ba_t<0, 1, false>), reinterpret_cast<const void *>(k_local_ba_t<0, 1, true>),
                               reinterpret_cast<const void *>(k_local_ba_t<1, 1>) })
            HIPCHK(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ba_lds_bytes(lim->max_kf)));
        if (ba_tile_cap_ll(lim->max_kf) >= std::max(lim->max_kf, 64))
            for (const void *f : { reinterpret_cast<const void *>(k_local_ba_t<2, 4>), reinterpret_cast<const void *>(k_local_ba_t<2, 8>),
                                   reinterpret_cast<const void *>(k_local_ba_t<2, 16>) })
                HIPCHK(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ba_lds_bytes_ll(lim->max_kf)));
        if (bb_lds_bytes(lim->max_lm) > 160 * 1024 || lim->max_kf > 32)
            return fail(c, "max_lm %d / max_kf %d: problem structure does not fit LDS", lim->max_lm, lim->max_kf);
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_ba_build),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    if (lim->max_streams > 0) {
        const size_t n = (size_t)lim->max_streams * lim->max_pts;
        for (int b = 0; b < 2; ++b) {
            HIPCHK(c, hipMalloc(&c->rt.xy[b], n * sizeof(float2)));
            HIPCHK(c, hipMalloc(&c->rt.mp[b], n * sizeof(int)));
            HIPCHK(c, hipMalloc(&c->rt.xyz[b], n * 3 * sizeof(double)));
        }
        c->rt.max_pts = lim->max_pts;
        c->rt_which.assign((size_t)lim->max_streams, 0);
        c->rt_count.assign((size_t)lim->max_streams, 0);
    }
    if (lim->device_map) {
        if (lim->max_streams <= 0 || lim->max_kf <= 0) return fail(c, "device_map needs max_streams > 0 and BA limits");
        if (lim->max_lm & (lim->max_lm - 1)) return fail(c, "device_map: max_lm %d must be a power of two", lim->max_lm);
        if (lim->max_kf > 12 || lim->max_pts >= 32768 || lim->max_lm >= 65536) return fail(c, "device_map: max_kf <= 12, max_pts < 32768, max_lm < 65536");
        if (dmg_lds_bytes(lim->max_lm) > 160 * 1024) return fail(c, "device_map: max_lm %d does not fit the gather's LDS", lim->max_lm);
        DMap &m = c->dm;
        m.KW = lim->max_kf; m.NF = lim->max_pts; m.NL = lim->max_lm;
        const size_t S = lim->max_streams, KF = S * m.KW, FT = KF * m.NF, LM = S * m.NL;
        const size_t bytes = KF * (8 + 4 + 56 + 4) + FT * (8 + 8 + 4 + 4 + 1) + LM * (24 + 4 + 4 + 1 + 4) + S * 4 + 4096;
        HIPCHK(c, hipMalloc(&c->dm_all, bytes));
        HIPCHK(c, hipMemsetAsync(c->dm_all, 0, bytes, c->stream));
        unsigned char *q = static_cast<unsigned char *>(c->dm_all);
        auto take = [&](size_t n) { unsigned char *r = q; q += (n + 255) & ~(size_t)255; return r; };
        m.kf_pose = reinterpret_cast<double *>(take(KF * 56)); m.lm_pos = reinterpret_cast<double *>(take(LM * 24));
        m.kf_frame = reinterpret_cast<long long *>(take(KF * 8));
        m.f_xy = reinterpret_cast<float2 *>(take(FT * 8)); m.f_xyr = reinterpret_cast<float2 *>(take(FT * 8));
        m.kf_id = reinterpret_cast<int *>(take(KF * 4)); m.kf_n = reinterpret_cast<int *>(take(KF * 4));
        m.f_lm = reinterpret_cast<int *>(take(FT * 4)); m.f_lmr = reinterpret_cast<int *>(take(FT * 4));
        m.lm_id = reinterpret_cast<int *>(take(LM * 4)); m.lm_obs = reinterpret_cast<int *>(take(LM * 4)); m.lm_stamp = reinterpret_cast<int *>(take(LM * 4));
        m.next_lm_id = reinterpret_cast<int *>(take(S * 4));
        m.f_fl = take(FT); m.lm_st = take(LM);
        // empty window slots / free landmark slots are marked by -1
        HIPCHK(c, hipMemsetAsync(m.kf_frame, 0xff, KF * 8, c->stream));
        HIPCHK(c, hipMemsetAsync(m.lm_id, 0xff, LM * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(m.lm_stamp, 0xff, LM * 4, c->stream));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_dmap_ba_gather<1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)dmg_lds_bytes_t<1024>(lim->max_lm)));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_dmap_ba_gather<512>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)dmg_lds_bytes_t<512>(lim->max_lm)));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

void svslam_destroy(svslam_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int b = 0; b < 2; ++b) { (void)hipFree(c->rt.xy[b]); (void)hipFree(c->rt.mp[b]); (void)hipFree(c->rt.xyz[b]); }
    (void)hipFree(c->d_pyr);
    if (c->dm_all) (void)hipFree(c->dm_all);
    if (c->dmba.stream) (void)hipStreamSynchronize(c->dmba.stream);
    if (c->dmba.buf) (void)hipFree(c->dmba.buf);
    for (hipEvent_t e : { c->dmba.gathered, c->dmba.solved, c->dmba.t0, c->dmba.t1 }) if (e) (void)hipEventDestroy(e);
    if (c->dmba.stream) (void)hipStreamDestroy(c->dmba.stream);
    (void)hipFree(c->ar.d);
    if (c->ar.h) (void)hipHostFree(c->ar.h);
    if (c->pyr_fused && c->pyr_plan.prof) {
        long long p[8] = { 0 };
        (void)hipMemcpy(p, c->pyr_plan.prof, sizeof(p), hipMemcpyDeviceToHost);
        const double k = p[7] ? 0.01 / (double)p[7] : 0.0;
        fprintf(stderr, "[pyr fused, workgroup (1,0), %lld launches, %d strips, lds %d] us: fill %.1f | border+store+pyrDown per level %.1f %.1f %.1f | last level %.1f\n",
                p[7], c->pyr_plan.nstrips, c->pyr_plan.lds_bytes, k * p[0], k * p[1], k * p[2], k * p[3], k * p[5]);
        (void)hipFree(c->pyr_plan.prof);
    }
    if (c->gw.prof) {
        long long p[16] = { 0 };
        (void)hipMemcpy(p, c->gw.prof, sizeof(p), hipMemcpyDeviceToHost);
        const double k = p[7] ? 0.01 / (double)p[7] : 0.0;      // 100 MHz ticks -> us per call
        fprintf(stderr, "[gftt select2, job 0, %lld calls] us/call: clear %.1f hist %.1f scan %.1f gather %.1f sort %.1f greedy %.1f | candidates %.0f, sorted %.0f\n",
                p[7], k * p[8], k * p[0], k * p[1], k * p[2], k * p[3], k * p[4], p[7] ? (double)p[5] / p[7] : 0.0, p[7] ? (double)p[6] / p[7] : 0.0);
        (void)hipFree(c->gw.prof);
    }
    (void)hipFree(c->gw.keys); (void)hipFree(c->gw.counters);
    (void)hipFree(c->lc.S.rows); (void)hipFree(c->lc.S.ids);
    (void)hipFree(c->gd.d_prm); (void)hipFree(c->gd.d_tab);
    ba_work_free(c->bw);
    ll_release(c);
    if (c->d_ba_prof) (void)hipFree(c->d_ba_prof);
    if (c->d_lm_trace) (void)hipFree(c->d_lm_trace);
    (void)svslam_sba_comm_destroy(c);
    for (int i = 0; i < 16; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->done) (void)hipEventDestroy(c->done);   // the stream belongs to the pool
    delete c;                                       // frees every DevBuf
}

int svslam_sync(svslam_ctx *c)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tm_collect(c);
    return 0;
}

int svslam_dev_alloc(svslam_ctx *c, size_t bytes, void **out) { HIPCHK(c, hipMalloc(out, bytes)); return 0; }
int svslam_dev_free(svslam_ctx *c, void *p) { HIPCHK(c, hipFree(p)); return 0; }
int svslam_dev_upload(svslam_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int svslam_dev_download(svslam_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int svslam_timing_enable(svslam_ctx *c, int on) { c->timing = on != 0; return 0; }
int svslam_timing_reset(svslam_ctx *c) { c->tm = Timing(); return 0; }
int svslam_timing_get(svslam_ctx *c, int family, double *total_ms, long long *launches, long long *units)
{
    if (family < 0 || family >= FAM_COUNT) return fail(c, "bad timing family %d", family);
    if (total_ms) *total_ms = c->tm.ms[family];
    if (launches) *launches = c->tm.launches[family];
    if (units) *units = c->tm.units[family];
    return 0;
}

} // extern "C"

#include "api_ba.h"
#include "api_frontend.h"
#include "api_dense.h"
#include "api_sba.h"
#include "api_dmap.h"
#include "api_loop.h"
#include "api_orb.h"
#include "api_orb_desc.h"
#include "api_debug.h"
