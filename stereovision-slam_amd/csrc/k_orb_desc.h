// ORB descriptors (rBRIEF) at keypoints that carry an angle and an octave (svslam_orb_describe_batch): what cv::ORB::compute
// does with the keypoints cv::ORB::detect returned (LoopClosure::ExtractKeypointsDescriptor, src/loopclosure.cpp:131-171).  The contract
// is the doc comment in include/svslam.h, restated in tests/ref_orb_desc.py; every step is integer, a written-out f32 step, or f64 on the
// host only, so this header, its host build (tests/cpp/orb_desc_host_emu) and the reference agree bit for bit.
//   levels    orb_level_size and orb_axis_taps of k_orb.h on the host, orb_resize_px4 on the device: the detector's own functions.
//             Only levels 1 .. Lmax (the call's largest octave) are stored, per job of a chunk; a job builds up to its own largest octave
//   filter    edge <= x < w - edge, y alike (float, level 0); then cx = rint(x inv_L), cy alike (one f32 product, half to even) and
//             on levels >= 1 edge <= cx < w_L - edge, cy alike; kept points keep their order (k_brief_filter's compaction)
//   rotation  a = (float)cos((double)r), b = (float)sin((double)r), r = angle * (float)(pi / 180) in f32, on the host (od_fill); on the
//             device ix = rint(px a - py b), iy = rint(px b + py a), every product and sum rounded to f32 on its own
//   reach     the largest over the table of ceil(sqrt(px^2 + py^2)) in integers: no rotation carries a point further
//   blur, tests, packing   k_brief.h's phases on the level-`octave` image around (cx, cy)
// Three kernels of 256 threads.  k_orbd_resize: level l of the jobs of a chunk, four pixels and one dword store per thread.
// k_orbd_filter: a workgroup per job, thread t owns points 4t .. 4t + 3.  k_orbd_describe: one wavefront per row, four rows per workgroup,
// the (2 reach + 7)^2 patch, both blur passes and the 256 flags in the wave's LDS block (br_plan); a lane rotates the eight table points
// of tests lane, lane + 64, lane + 128, lane + 192 in registers.  The geometry travels in the buffer (k_orb.h's lesson: indexed by a
// level known at run time, by value it would go to scratch).  Nothing crosses lanes except through LDS between barriers, no float
// atomics, plain C++ between the HIP qualifiers: with OD_HOST_EMU a phase becomes a loop over the 256 thread numbers.
#pragma once
#ifdef OD_HOST_EMU
#ifndef ORB_HOST_EMU
#define ORB_HOST_EMU
#endif
#ifndef BR_HOST_EMU
#define BR_HOST_EMU
#endif
#endif
#include <cmath>
#include "k_brief.h"
#include "k_orb.h"

#define OD_PT_BYTES 96             // a point's share of a chunk's buffer (OdPt, OdRow, desc_pt, descriptor), for the chunking rule

struct OdJob { int slot, pt_ofs, npts, n_desc; };                           // what a caller's job says
struct OdParams { const int8_t *pattern; int edge, nlevels, reserved; };   // svslam_orb_desc_params
struct OdPt { float x, y, a, b; int octave, pad; };                         // uploaded per point: a, b = cos, sin of its angle
struct OdRow { int cx, cy, level, job; float a, b; int pad0, pad1; };       // written by the filter; cx = -1: no row here
struct OdDevJob { int slot, pt_ofs, npts, n_desc, lmax, pad0, pad1, pad2; };    // pt_ofs inside the chunk
struct OdLevel { int w, h; float inv; int xtap, ytap, pad; size_t img; };   // img: offset inside a job's block (levels >= 1)

struct OdGeom {
    int nlevels, lmax, edge, reach, R, npts, pad0, pad1;       // lmax: the call's largest octave; npts: the chunk's points
    size_t job_bytes;                                          // levels 1 .. lmax of one job; 0 when lmax == 0
    OdLevel L[ORB_MAX_LEVELS];
};

struct OdChunk { int j0, n, p0, npts; size_t upload_bytes, result_ofs, result_bytes, bytes; };

struct OdPlan {
    OdGeom G;
    BrPlan lds;
    const int8_t *pattern;
    std::vector<OrbTap> taps;
    std::vector<OdChunk> chunks;
};

struct OdBuf {
    OdGeom *geom;
    OrbTap *taps;
    const int8_t *tbl;             // [1024]: x0, y0, x1, y1 of the 256 tests
    const OdPt *pts;               // [npts]
    OdRow *rows;                   // [npts], uploaded with cx = -1
    OdDevJob *jobs;                // read back from here on
    int *desc_pt;                  // [npts]
    uint32_t *desc;                // [npts][8]
    unsigned char *blocks;         // [n][job_bytes]
};

// the smallest m with m^2 >= px^2 + py^2, the largest over the table
static inline int od_reach(const int8_t *pattern)
{
    int reach = 0;
    for (int i = 0; i < 512; ++i) {
        const int q = (int)pattern[2 * i] * pattern[2 * i] + (int)pattern[2 * i + 1] * pattern[2 * i + 1];
        int m = 0;
        while (m * m < q) ++m;
        if (m > reach) reach = m;
    }
    return reach;
}

static inline void od_rotation(float angle_deg, float *a, float *b)
{
    const float r = angle_deg * (float)(3.14159265358979323846 / 180.0);
    *a = (float)cos((double)r); *b = (float)sin((double)r);
}

// Every host rule of a call: defaults, refusals, reach, the levels up to the largest octave, the chunks.  Returns nullptr or the reason
// the call is refused (nothing has been launched or written then).  kps: the caller's keypoints (OrbKp's fields).
static inline const char *od_plan(OdPlan &P, int w, int h, int nslots, int njobs, const OdJob *jobs, const OdParams *prm, int total_pts,
                                  const OrbKp *kps, size_t budget)
{
    if (!prm) return "null params";
    if (njobs < 0 || total_pts < 0) return "negative count";
    OdGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    P.pattern = prm->pattern ? prm->pattern : BR_DEFAULT_PATTERN;
    G.edge = prm->edge ? prm->edge : 31;
    G.nlevels = prm->nlevels ? prm->nlevels : 8;
    for (int j = 0; j < njobs; ++j) {
        const OdJob &J = jobs[j];
        if (J.npts < 0 || J.pt_ofs < 0 || (long long)J.pt_ofs + J.npts > total_pts) return "a job's range leaves the arrays";
        if (J.npts > BR_MAX_PTS) return "a job has more than 1024 points";
        if (j > 0 && J.pt_ofs < jobs[j - 1].pt_ofs + jobs[j - 1].npts) return "the jobs' ranges must ascend and not overlap";
        if (J.slot < 0 || J.slot >= nslots) return "a job's slot is out of range";
    }
    for (int t = 0; t < 256; ++t)
        if (P.pattern[4 * t] == P.pattern[4 * t + 2] && P.pattern[4 * t + 1] == P.pattern[4 * t + 3]) return "the two points of a table entry coincide";
    G.reach = od_reach(P.pattern);
    G.R = G.reach + 3;
    if (G.edge < G.reach + 4) return "edge is below the table's reach + 4";
    if (G.reach > BR_MAX_REACH) return "the table's reach is above 24";
    if (G.nlevels < 1 || G.nlevels > ORB_MAX_LEVELS) return "nlevels is outside 1..8";
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return "the image is wider or taller than 32767";
    int lmax = 0;
    for (int j = 0; j < njobs; ++j)
        for (int i = jobs[j].pt_ofs; i < jobs[j].pt_ofs + jobs[j].npts; ++i) {
            if (kps[i].octave < 0 || kps[i].octave >= G.nlevels) return "a keypoint's octave is outside 0..nlevels-1";
            if (!std::isfinite(kps[i].angle)) return "a keypoint's angle is not finite";
            if (kps[i].octave > lmax) lmax = kps[i].octave;
        }
    G.lmax = lmax;
    P.lds = br_plan(G.reach);
    // the levels up to the largest octave, the detector's sizes and tables
    P.taps.clear();
    size_t o = 0;
    for (int l = 0; l <= lmax; ++l) {
        OdLevel &L = G.L[l];
        float scale;
        orb_level_size(w, h, l, &scale, &L.w, &L.h);
        L.inv = l == 0 ? 1.0f : 1.0f / scale;
        if (l > 0) {
            L.xtap = (int)P.taps.size();
            P.taps.resize(P.taps.size() + (size_t)L.w);
            orb_axis_taps(G.L[l - 1].w, L.w, P.taps.data() + L.xtap);
            L.ytap = (int)P.taps.size();
            P.taps.resize(P.taps.size() + (size_t)L.h);
            orb_axis_taps(G.L[l - 1].h, L.h, P.taps.data() + L.ytap);
            L.img = o; o += orb_up16((size_t)L.w * L.h);
        }
    }
    G.job_bytes = (o + 255) & ~(size_t)255;
    // chunks under the budget (a chunk has at least one job); a chunk's points are those from its first job's to its last job's
    P.chunks.clear();
    for (int j0 = 0; j0 < njobs;) {
        OdChunk C;
        memset(&C, 0, sizeof(C));
        C.j0 = j0; C.p0 = jobs[j0].pt_ofs;
        int j = j0 + 1;
        for (; j < njobs && j - j0 < 65535; ++j) {             // (65535: the resize's grid has a row per job)
            const size_t span = (size_t)(jobs[j].pt_ofs + jobs[j].npts - C.p0);
            if ((G.job_bytes + 64) * (size_t)(j - j0 + 1) + span * OD_PT_BYTES > budget) break;
        }
        C.n = j - j0;
        C.npts = jobs[j - 1].pt_ofs + jobs[j - 1].npts - C.p0;
        P.chunks.push_back(C);
        j0 = j;
    }
    return nullptr;
}

// one buffer: [geometry | taps | table | points | rows | jobs] (uploaded) [jobs | rows -> points | descriptors] (read back) [blocks]
static inline OdBuf od_layout(const OdPlan &P, OdChunk &C, unsigned char *base)
{
    OdBuf B;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *p = base + o; o += (bytes + 255) & ~(size_t)255; return p; };
    B.geom = (OdGeom *)take(sizeof(OdGeom));
    B.taps = (OrbTap *)take(sizeof(OrbTap) * P.taps.size());
    B.tbl = (const int8_t *)take(1024);
    B.pts = (const OdPt *)take(sizeof(OdPt) * (size_t)C.npts);
    B.rows = (OdRow *)take(sizeof(OdRow) * (size_t)C.npts);
    C.result_ofs = o;
    B.jobs = (OdDevJob *)take(sizeof(OdDevJob) * (size_t)C.n);
    C.upload_bytes = o;
    B.desc_pt = (int *)take(4 * (size_t)C.npts);
    B.desc = (uint32_t *)take(32 * (size_t)C.npts);
    C.result_bytes = o - C.result_ofs;
    B.blocks = base + o;
    o += P.G.job_bytes * (size_t)C.n;
    C.bytes = o;
    return B;
}

// the uploaded part of a chunk, written through a host view of the same layout
static inline void od_fill(const OdPlan &P, const OdChunk &C, const OdBuf &Hb, const OdJob *jobs, const OrbKp *kps)
{
    *Hb.geom = P.G;
    Hb.geom->npts = C.npts;
    if (!P.taps.empty()) memcpy(Hb.taps, P.taps.data(), sizeof(OrbTap) * P.taps.size());
    memcpy((void *)Hb.tbl, P.pattern, 1024);
    OdPt *pt = (OdPt *)Hb.pts;
    for (int i = 0; i < C.npts; ++i) {
        OdRow &r = Hb.rows[i];
        r.cx = -1; r.cy = -1; r.level = 0; r.job = 0; r.a = 0.f; r.b = 0.f; r.pad0 = r.pad1 = 0;
        memset(&pt[i], 0, sizeof(OdPt));                   // a gap between two jobs' ranges: nobody reads it
    }
    for (int j = 0; j < C.n; ++j) {
        const OdJob &J = jobs[C.j0 + j];
        OdDevJob &D = Hb.jobs[j];
        D.slot = J.slot; D.pt_ofs = J.pt_ofs - C.p0; D.npts = J.npts; D.n_desc = 0; D.lmax = 0; D.pad0 = D.pad1 = D.pad2 = 0;
        for (int i = 0; i < J.npts; ++i) {
            const OrbKp &K = kps[J.pt_ofs + i];
            OdPt &q = pt[D.pt_ofs + i];
            q.x = K.x; q.y = K.y; q.octave = K.octave; q.pad = 0;
            od_rotation(K.angle, &q.a, &q.b);
            if (K.octave > D.lmax) D.lmax = K.octave;
        }
    }
}

// the first n_desc rows of every job of a chunk, to the caller's arrays; what lies behind them there is left as it was
static inline void od_copy_out(const OdChunk &C, const OdBuf &Hb, OdJob *jobs, uint8_t *desc, int *desc_pt)
{
    for (int j = 0; j < C.n; ++j) {
        const OdDevJob &D = Hb.jobs[j];
        OdJob &J = jobs[C.j0 + j];
        J.n_desc = D.n_desc;
        if (D.n_desc > 0) {
            memcpy(desc_pt + J.pt_ofs, Hb.desc_pt + D.pt_ofs, 4 * (size_t)D.n_desc);
            memcpy(desc + 32 * (size_t)J.pt_ofs, Hb.desc + 8 * (size_t)D.pt_ofs, 32 * (size_t)D.n_desc);
        }
    }
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// level l of the image of job j of the chunk (level 0: the pyramid slot)
ORB_DEV OrbView od_image(const OdGeom &G, const OrbImg &I, const OdBuf &B, int j, int l)
{
    OrbView V;
    if (l == 0) { V.p = I.base + (size_t)B.jobs[j].slot * I.slot_bytes + I.origin; V.pitch = I.pitch; }
    else { V.p = B.blocks + (size_t)j * G.job_bytes + G.L[l].img; V.pitch = G.L[l].w; }
    return V;
}

// flat pixels [4 t, 4 t + 4) of level l of job j, for the jobs that have a point on level l or above
ORB_DEV void od_resize_task(const OdGeom &G, const OrbImg &I, const OdBuf &B, int l, int j, int t)
{
    const OdLevel &L = G.L[l];
    if (l > B.jobs[j].lmax || 4 * t >= L.w * L.h) return;
    const OrbView S = od_image(G, I, B, j, l - 1);
    orb_resize_px4(S.p, S.pitch, B.blocks + (size_t)j * G.job_bytes + L.img, B.taps + L.xtap, B.taps + L.ytap, L.w, L.w * L.h, 0, t);
}

// the contract's filter; the last conditions restate, on the centre, that every tap lies inside the level (they hold whenever
// edge >= reach + 4, and the octave is inside the levels the call built, and are here so that no input can make the describe kernel
// read outside an image)
ORB_DEV bool od_keep(const OdGeom &G, const OdPt &q, int *cx, int *cy)
{
    const int edge = G.edge;
    if (!((float)edge <= q.x && q.x < (float)(G.L[0].w - edge) && (float)edge <= q.y && q.y < (float)(G.L[0].h - edge))) return false;
    if (q.octave < 0 || q.octave > G.lmax) return false;
    const OdLevel &L = G.L[q.octave];
    const float fx = q.x * L.inv, fy = q.y * L.inv;
    const int ix = (int)rintf(fx), iy = (int)rintf(fy);
    *cx = ix; *cy = iy;
    if (q.octave > 0 && !(edge <= ix && ix < L.w - edge && edge <= iy && iy < L.h - edge)) return false;
    return ix - G.R >= 0 && ix + G.R < L.w && iy - G.R >= 0 && iy + G.R < L.h;
}

ORB_DEV void od_filter_run(const OdGeom &G, const OdBuf &B, int j, int *cnt)
{
    OdDevJob &J = B.jobs[j];
    const int n = J.npts, ofs = J.pt_ofs;
    const OdPt *pts = B.pts + ofs;
    BR_PAR {
        int k = 0, cx, cy;
        for (int i = tid * BR_PTS_PER_THREAD; i < (tid + 1) * BR_PTS_PER_THREAD && i < n; ++i)
            if (od_keep(G, pts[i], &cx, &cy)) ++k;
        cnt[tid] = k;
    } BR_SYNC
    BR_PAR {
        int o = 0, cx, cy;
        for (int t = 0; t < tid; ++t) o += cnt[t];
        for (int i = tid * BR_PTS_PER_THREAD; i < (tid + 1) * BR_PTS_PER_THREAD && i < n; ++i) {
            const OdPt q = pts[i];
            if (od_keep(G, q, &cx, &cy)) {
                OdRow r; r.cx = cx; r.cy = cy; r.level = q.octave; r.job = j; r.a = q.a; r.b = q.b; r.pad0 = r.pad1 = 0;
                B.rows[ofs + o] = r; B.desc_pt[ofs + o] = i;
                ++o;
            }
        }
        if (tid == BR_THREADS - 1) J.n_desc = o;
    } BR_SYNC
}

// the row of this thread's wave, or false
ORB_DEV bool od_row(const OdGeom &G, const OdBuf &B, int wg, int tid, int *g, OdRow *r)
{
    *g = wg * BR_ROWS_PER_WG + tid / BR_WAVE;
    if (*g >= G.npts) return false;
    *r = B.rows[*g];
    return r->cx >= 0;
}

// index, inside the (2 reach + 1)^2 blurred patch, of table point (px, py) turned by (a, b)
ORB_DEV int od_turned(int px, int py, float a, float b, int reach, int Bw)
{
    const float fx = (float)px, fy = (float)py;
    const float xa = fx * a, yb = fy * b, xb = fx * b, ya = fy * a;
    const float rx = xa - yb, ry = xb + ya;
    const int ix = (int)rintf(rx), iy = (int)rintf(ry);
    return (iy + reach) * Bw + ix + reach;
}

ORB_DEV void od_describe_run(const OdGeom &G, const OrbImg &I, const OdBuf &B, const BrPlan &L, int wg, unsigned char *smem)
{
    BR_PAR {                                           // the patch of the row's level
        int g; OdRow r;
        if (od_row(G, B, wg, tid, &g, &r)) {
            const OrbView V = od_image(G, I, B, r.job, r.level);
            br_patch_load(smem + (size_t)(tid / BR_WAVE) * L.wave_bytes, V.p + (size_t)(r.cy - L.R) * V.pitch + (size_t)(r.cx - L.R),
                          (size_t)V.pitch, L.P, tid % BR_WAVE);
        }
    } BR_SYNC
    BR_PAR {
        int g; OdRow r;
        if (od_row(G, B, wg, tid, &g, &r)) {
            unsigned char *wv = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes;
            br_blur_h(wv, (uint16_t *)(wv + L.o_h), L.P, L.Bw, tid % BR_WAVE);
        }
    } BR_SYNC
    BR_PAR {
        int g; OdRow r;
        if (od_row(G, B, wg, tid, &g, &r)) {
            unsigned char *wv = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes;
            br_blur_v((const uint16_t *)(wv + L.o_h), wv + L.o_b, L.Bw, tid % BR_WAVE);
        }
    } BR_SYNC
    BR_PAR {                                           // the tests, each at the row's own rotation
        int g; OdRow r;
        if (od_row(G, B, wg, tid, &g, &r)) {
            const int lane = tid % BR_WAVE;
            const uint8_t *bl = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_b;
            uint8_t *bits = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_bits;
            for (int t = lane; t < 256; t += BR_WAVE) {
                const int8_t *p = B.tbl + 4 * t;
                const int i0 = od_turned(p[0], p[1], r.a, r.b, L.reach, L.Bw), i1 = od_turned(p[2], p[3], r.a, r.b, L.reach, L.Bw);
                bits[t] = bl[i0] < bl[i1] ? 1 : 0;
            }
        }
    } BR_SYNC
    BR_PAR {                                           // 8 lanes, one dword of the descriptor each
        int g; OdRow r;
        if (od_row(G, B, wg, tid, &g, &r)) {
            const int lane = tid % BR_WAVE;
            if (lane < 8) B.desc[8 * (size_t)g + lane] = br_pack(smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_bits, lane);
        }
    } BR_SYNC
}

#ifndef OD_HOST_EMU
// grid (ceil(ceil(w_l h_l / 4) / 256), n)
__global__ void __launch_bounds__(BR_THREADS) k_orbd_resize(OrbImg I, OdBuf B, int l)
{
    od_resize_task(*B.geom, I, B, l, (int)blockIdx.y, (int)(blockIdx.x * BR_THREADS + threadIdx.x));
}
// grid (n)
__global__ void __launch_bounds__(BR_THREADS) k_orbd_filter(OdBuf B)
{
    __shared__ int cnt[BR_THREADS];
    od_filter_run(*B.geom, B, (int)blockIdx.x, cnt);
}
// grid (ceil(npts / 4))
__global__ void __launch_bounds__(BR_THREADS) k_orbd_describe(OrbImg I, OdBuf B, BrPlan L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char od_smem[];
    od_describe_run(*B.geom, I, B, L, (int)blockIdx.x, od_smem);
}
#endif
