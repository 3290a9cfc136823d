// ORB keypoint detector on level 0 of resident pyramid slots (svslam_orb_detect_batch): what cv::ORB::detect does for
// Frontend::DetectFeatures with keypoint_feature_detector: ORB (src/frontend.cpp:20-33, :51).  ORB's defaults: scale factor 1.2f,
// 8 levels, edge threshold 31, first level 0, HARRIS_SCORE, patch size 31, FAST threshold 20.  The contract is tests/ref_orb.py and
// the issue text restated in DESIGN 16; OpenCV is not on the machines, so parity with it is unpinned.  Every step is integer, a
// written-out f32 step, or f64 on the host only (orb_plan); this header, its host build (tests/cpp/orb_host_emu) and ref_orb.py
// agree bit for bit.
//   levels    scale_L = (float)pow((double)1.2f, L), inv_L = 1.f / scale_L, w_L = rint((float)w * inv_L) (half to even), h_L alike
//   quotas    factor = (float)(1.0 / (double)1.2f); nd = nfeatures * (1 - factor) / (1 - (float)pow(factor, nlevels)) in f32;
//             n_L = rint(nd), nd *= factor for L < nlevels - 1; n_last = max(nfeatures - sum, 0)
//   pyramid   level L from level L - 1 by the bit-exact bilinear resize: per axis s = 1.0 / ((double)dst / (double)src),
//             f = s * (d + 0.5) - 0.5, i = floor(f); i < 0: sample 0, weight 256; i >= src - 1: sample src - 1, weight 256; else
//             c1 = rint((f - i) * 256), c0 = 256 - c1 on samples i, i + 1.  t = p[i] c0 + p[i + 1] c1 along x (<= 65280),
//             v = t0 c0 + t1 c1 along y, out = (v + 32768) >> 16.  The tables are f64 host work (OrbTap), the device is integer
//   mask      level 0: 255, 0 inside [rint(pt - 10), rint(pt + 10)] of every rect centre, clipped (k_gftt_eig3's rule and input);
//             level L: the same resize of the level L - 1 mask, then <= 254 becomes 0
//   FAST      9 of 16 on the radius-3 circle, strict; score = max over the 16 arcs and both polarities of the arc's minimum signed
//             difference, minus 1, 0 for a non-corner; a corner survives iff its score is strictly above its 8 neighbours' scores
//   filters   border (edge <= x < w_L - edge, y alike), then mask (mask_L[y][x] != 0)
//   cut 1     m = 2 n_L; more than m survivors: all with score >= the m-th largest stay (ties all stay); m == 0: nothing
//   Harris    7 x 7 block, Sobel-like Ix, Iy in int32, a = sum Ix Ix, b = sum Iy Iy, c = sum Ix Iy;
//             response = ((float)a (float)b - (float)c (float)c - 0.04f ((float)a + (float)b) ((float)a + (float)b)) * s4, left to
//             right, s4 = scale^4, scale = 1.f / (4 * 7 * 255.f).  No NaN: |Ix|, |Iy| <= 1020, so a, b, |c| <= 49 * 1020^2 < 2^26
//             are exact in int32, the products stay below 2^52 in f32 and no inf - inf or 0 * inf can form; the smallest non-zero
//             result is far above the subnormals, so no -0.f either (orb_key still adds +0.f)
//   cut 2     more than n_L left: all with response >= the n_L-th largest stay (float compare, ties stay)
//   angle     intensity centroid over the circular patch of half-size 15 (ORB_UMAX), m10 = sum u I, m01 = sum v I in int32,
//             angle = orb_atan_deg((float)m01, (float)m10): OpenCV's fastAtan2 with the contract's constants
//   output    x = (float)xi * scale_L, y alike, size = 31 * scale_L, angle, response, octave = L; level ascending, row-major inside
//             a level (OpenCV's order comes out of nth_element and is unspecified); duplicates across levels stay, as there
// Kernels, all of 256 threads, a launch per level where a level is named:
//   k_orb_fill      mask level 0 := 255, 16 bytes per thread
//   k_orb_rects     a workgroup per rect zeroes its clipped square
//   k_orb_resize    level L of image and mask (grid z), four output pixels and one dword store per thread
//   k_orb_fast      32 x 8 interior pixels per workgroup: the 40 x 16 pixel tile (3 halo + 1 for the neighbours' scores) in LDS by dword
//                   loads, 34 x 10 scores in LDS, non-maximum suppression, border and mask; writes the kept score of every interior
//                   pixel (0: dropped) and counts the kept ones in the level's 256-bin histogram (integer atomics)
//   k_orb_select    a workgroup per (level, job): cut 1 from the histogram (suffix sums), the ordered list of kept pixels by a
//                   blocked scan over the interior, Harris keys (f32_ordered of k_gftt.h), cut 2 by a 4-pass radix select over
//                   LDS histograms, the level's final count
//   k_orb_emit      a workgroup per (level, job): the level's rows start behind the earlier levels' counts; ordered compaction of the
//                   list against cut 2, a wave per emitted row for the orientation (lane v + 15 sums patch row v, the 31 partial
//                   sums meet in LDS), rows at or behind max_out are counted and not written
// No list has a capacity an input could exceed: a level's list holds ceil(iw / 2) * ceil(ih / 2) entries, and two survivors of a strict
// 8-neighbour maximum are never adjacent.  No float atomics, no cross-lane operation: threads meet through LDS between barriers and
// the file is plain C++ between the HIP qualifiers; with ORB_HOST_EMU a phase becomes a loop over the 256 thread numbers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define ORB_THREADS 256
#define ORB_WAVE 64
#define ORB_MAX_LEVELS 8
#define ORB_TILE_W 32
#define ORB_TILE_H 8
#define ORB_PIX_W 40               // ORB_TILE_W + 8: four pixels each side
#define ORB_PIX_H 16               // ORB_TILE_H + 8
#define ORB_SC_W 34
#define ORB_SC_H 10
#define ORB_HALF_PATCH 15
#define ORB_BUDGET_DEFAULT ((size_t)1 << 30)      // device bytes of the jobs' levels, maps and lists in one chunk of a call

#ifdef ORB_HOST_EMU
#define ORB_DEV static inline
#define ORB_PAR for (int tid = 0; tid < ORB_THREADS; ++tid)
#define ORB_SYNC
#define ORB_COUNT(p) (++*(p))
#define ORB_FDIV(a, b) ((a) / (b))
#define ORB_TABLE static const
#else
#define ORB_DEV __device__ __forceinline__
#define ORB_PAR for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define ORB_SYNC __syncthreads();
#define ORB_COUNT(p) ((void)atomicAdd((p), 1u))
#define ORB_FDIV(a, b) __fdiv_rn((a), (b))
#define ORB_TABLE static __device__ const          // read by device code only in the library's build
#endif

// umax[v] = rint(sqrt(225 - v^2)) for v = 0 .. floor(15 sqrtf(2) / 2 + 1) = 11, the upper part mirrored so that the patch is
// symmetric (OpenCV's loop); orb_umax_rule rebuilds it and the host unit test compares
ORB_TABLE int8_t ORB_UMAX[16] = { 15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3 };

static inline void orb_umax_rule(int *umax)
{
    const int half = ORB_HALF_PATCH;
    const int vmax = (int)floor(half * sqrt(2.f) / 2 + 1), vmin = (int)ceil(half * sqrt(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = (int)rint(sqrt((double)half * half - (double)v * v));
    for (int v = half, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
}

// the radius-3 circle in the contract's order, (x, y)
ORB_TABLE int8_t ORB_CIRCLE[16][2] = { { 0, 3 }, { 1, 3 }, { 2, 2 }, { 3, 1 }, { 3, 0 }, { 3, -1 }, { 2, -2 }, { 1, -3 },
                                          { 0, -3 }, { -1, -3 }, { -2, -2 }, { -3, -1 }, { -3, 0 }, { -3, 1 }, { -2, 2 }, { -1, 3 } };

struct OrbKp { float x, y, size, angle, response; int octave; };           // svslam_orb_kp
struct OrbJob { int slot, rect_ofs, nrect; };                               // what a caller's job says
struct OrbParams { int nfeatures, nlevels, fast_threshold, edge; };         // 0: ORB's default
struct OrbTap { uint16_t i0, i1, c0, c1; };                                 // one destination index of one axis of the resize
struct OrbRect { int x0, y0, x1, y1, job, pad0, pad1, pad2; };              // clipped, inclusive; job inside the chunk
struct OrbDevJob { int slot, pad; };
struct OrbRes { int n_found, pad; };
struct OrbLvlState { int k1, k2; uint32_t thr2; int pad; };                 // after cut 1, after cut 2, the ordered response cut 2 keeps from

// level 0 of the slots as the kernels read it (BrImg's fields)
struct OrbImg { const uint8_t *base; size_t slot_bytes, origin; int pitch, w, h; };

struct OrbLevel {
    int w, h, quota, active;       // active: the level has an interior and a quota
    float scale;
    int iw, ih;                    // interior = [edge, w - edge) x [edge, h - edge); 0 when there is none
    int tiles_x, tiles_y;          // k_orb_fast's grid over the interior
    int xtap, ytap;                // first tap of the axes inside the tap array (levels >= 1)
    int list_cap;
    size_t img, mask, ks, pos, key;    // offsets inside a job's block (img: levels >= 1)
};

// a call's geometry: the plan's, uploaded with every chunk
struct OrbGeom {
    int nlevels, nfeatures, fast_t, edge, max_out, pad;
    size_t job_bytes;
    OrbLevel L[ORB_MAX_LEVELS];
};

// one chunk of a call: jobs [j0, j0 + n), their rects, the buffer's sizes
struct OrbChunk { int j0, n, nrects; size_t upload_bytes, result_ofs, result_bytes, hist_ofs, hist_bytes, bytes; };

struct OrbPlan {
    OrbGeom G;
    std::vector<OrbTap> taps;
    std::vector<OrbChunk> chunks;
};

struct OrbBuf {
    OrbGeom *geom;                 // the kernels read the geometry from here: indexed by level at run time, it stays out of scratch
    OrbTap *taps;
    OrbDevJob *jobs;
    OrbRect *rects;
    OrbRes *res;                   // read back from here on
    OrbKp *out;                    // [n][max_out]
    unsigned int *hist;            // [n][nlevels][256], zeroed before the launch
    OrbLvlState *lvl;              // [n][nlevels]
    unsigned char *blocks;         // [n][job_bytes]
};

static inline int orb_round_even(float v) { return (int)rintf(v); }        // the host's default rounding mode: to nearest, ties to even

// one axis of the bit-exact bilinear resize
static inline void orb_axis_taps(int src, int dst, OrbTap *t)
{
    const double s = 1.0 / ((double)dst / (double)src);
    for (int d = 0; d < dst; ++d) {
        const double a = s * ((double)d + 0.5);
        const double f = a - 0.5;
        const double fl = floor(f);
        OrbTap q;
        if (fl < 0.0) { q.i0 = q.i1 = 0; q.c0 = 256; q.c1 = 0; }
        else if (fl >= (double)(src - 1)) { q.i0 = q.i1 = (uint16_t)(src - 1); q.c0 = 256; q.c1 = 0; }
        else {
            const int i = (int)fl;
            const int c1 = (int)rint((f - fl) * 256.0);
            q.i0 = (uint16_t)i; q.i1 = (uint16_t)(i + 1); q.c1 = (uint16_t)c1; q.c0 = (uint16_t)(256 - c1);
        }
        t[d] = q;
    }
}

// scale and size of level l of a w x h image (svslam_orb_describe_batch builds its levels from the same rule)
static inline void orb_level_size(int w, int h, int l, float *scale, int *lw, int *lh)
{
    *scale = (float)pow((double)1.2f, (double)l);
    if (l == 0) { *lw = w; *lh = h; return; }
    const float inv = 1.0f / *scale;
    *lw = orb_round_even((float)w * inv);
    *lh = orb_round_even((float)h * inv);
    if (*lw < 1) *lw = 1;
    if (*lh < 1) *lh = 1;
}

static inline size_t orb_up16(size_t v) { return (v + 15) & ~(size_t)15; }

// Every host rule of a call: the parameters' defaults and refusals, level sizes, quotas, resize tables, a job's block, the chunks.
// Returns nullptr or the reason the call is refused (nothing has been launched or written then).
static inline const char *orb_plan(OrbPlan &P, int w, int h, int nslots, int njobs, const OrbJob *jobs, const OrbParams *prm, int total_rects,
                                   int max_out, size_t budget)
{
    if (!prm) return "null params";
    if (njobs < 0 || total_rects < 0) return "negative count";
    OrbGeom &G = P.G;
    memset(&G, 0, sizeof(G));
    G.nfeatures = prm->nfeatures ? prm->nfeatures : 500;
    G.nlevels = prm->nlevels ? prm->nlevels : 8;
    G.fast_t = prm->fast_threshold ? prm->fast_threshold : 20;
    G.edge = prm->edge ? prm->edge : 31;
    G.max_out = max_out;
    if (G.nfeatures < 1) return "nfeatures is below 1";
    if (G.nfeatures > (1 << 24)) return "nfeatures is above 2^24";
    if (G.nlevels < 1 || G.nlevels > ORB_MAX_LEVELS) return "nlevels is outside 1..8";
    if (G.fast_t < 1 || G.fast_t > 254) return "fast_threshold is outside 1..254";
    if (G.edge < 16) return "edge is below 16 (the orientation reads radius 15, Harris radius 4)";
    if (max_out < 1) return "max_out is below 1";
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return "the image is wider or taller than 32767";
    for (int j = 0; j < njobs; ++j) {
        if (jobs[j].slot < 0 || jobs[j].slot >= nslots) return "a job's slot is out of range";
        if (jobs[j].nrect < 0 || jobs[j].rect_ofs < 0 || (long long)jobs[j].rect_ofs + jobs[j].nrect > total_rects)
            return "a job's rect range leaves the array";
    }
    // quotas
    const int nl = G.nlevels;
    {
        const float factor = (float)(1.0 / (double)1.2f);
        const float num = (float)G.nfeatures * (1.f - factor);
        const float den = 1.f - (float)pow((double)factor, (double)nl);
        float nd = num / den;
        int sum = 0;
        for (int l = 0; l < nl - 1; ++l) {
            G.L[l].quota = orb_round_even(nd);
            sum += G.L[l].quota;
            nd *= factor;
        }
        G.L[nl - 1].quota = G.nfeatures - sum > 0 ? G.nfeatures - sum : 0;
    }
    // level sizes, tables, a job's block
    P.taps.clear();
    size_t o = 0;
    for (int l = 0; l < nl; ++l) {
        OrbLevel &L = G.L[l];
        orb_level_size(w, h, l, &L.scale, &L.w, &L.h);
        if (l > 0) {
            L.xtap = (int)P.taps.size();
            P.taps.resize(P.taps.size() + (size_t)L.w);
            orb_axis_taps(G.L[l - 1].w, L.w, P.taps.data() + L.xtap);
            L.ytap = (int)P.taps.size();
            P.taps.resize(P.taps.size() + (size_t)L.h);
            orb_axis_taps(G.L[l - 1].h, L.h, P.taps.data() + L.ytap);
        }
        const size_t px = orb_up16((size_t)L.w * L.h);
        L.iw = L.w > 2 * G.edge ? L.w - 2 * G.edge : 0;
        L.ih = L.h > 2 * G.edge ? L.h - 2 * G.edge : 0;
        if (!L.iw || !L.ih) L.iw = L.ih = 0;
        L.active = L.iw > 0 && L.quota > 0;
        L.tiles_x = (L.iw + ORB_TILE_W - 1) / ORB_TILE_W;
        L.tiles_y = (L.ih + ORB_TILE_H - 1) / ORB_TILE_H;
        L.list_cap = L.active ? ((L.iw + 1) / 2) * ((L.ih + 1) / 2) : 0;
        if (l > 0) { L.img = o; o += px; }
        L.mask = o; o += px;
        L.ks = o; o += L.active ? px : 0;
        L.pos = o; o += orb_up16(4 * (size_t)L.list_cap);
        L.key = o; o += orb_up16(4 * (size_t)L.list_cap);
    }
    G.job_bytes = (o + 255) & ~(size_t)255;
    // chunks under the budget (a chunk has at least one job)
    const size_t per_job = G.job_bytes + sizeof(OrbKp) * (size_t)max_out + (size_t)nl * (1024 + sizeof(OrbLvlState)) + 64;
    long long fit = (long long)(budget / per_job);
    if (fit < 1) fit = 1;
    if (fit > (1 << 20)) fit = 1 << 20;
    P.chunks.clear();
    for (int j0 = 0; j0 < njobs; j0 += (int)fit) {
        OrbChunk C;
        memset(&C, 0, sizeof(C));
        C.j0 = j0; C.n = njobs - j0 < (int)fit ? njobs - j0 : (int)fit;
        for (int j = j0; j < j0 + C.n; ++j) C.nrects += jobs[j].nrect;
        P.chunks.push_back(C);
    }
    return nullptr;
}

// one buffer: [geometry | taps | jobs | rects] (uploaded) [results | rows] (read back) [histograms] (zeroed) [level states | blocks]
static inline OrbBuf orb_layout(const OrbPlan &P, OrbChunk &C, unsigned char *base)
{
    OrbBuf B;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *p = base + o; o += (bytes + 255) & ~(size_t)255; return p; };
    B.geom = (OrbGeom *)take(sizeof(OrbGeom));
    B.taps = (OrbTap *)take(sizeof(OrbTap) * P.taps.size());
    B.jobs = (OrbDevJob *)take(sizeof(OrbDevJob) * (size_t)C.n);
    B.rects = (OrbRect *)take(sizeof(OrbRect) * (size_t)C.nrects);
    C.upload_bytes = o;
    C.result_ofs = o;
    B.res = (OrbRes *)take(sizeof(OrbRes) * (size_t)C.n);
    B.out = (OrbKp *)take(sizeof(OrbKp) * (size_t)C.n * (size_t)P.G.max_out);
    C.result_bytes = o - C.result_ofs;
    C.hist_ofs = o;
    B.hist = (unsigned int *)take(1024 * (size_t)C.n * (size_t)P.G.nlevels);
    C.hist_bytes = o - C.hist_ofs;
    B.lvl = (OrbLvlState *)take(sizeof(OrbLvlState) * (size_t)C.n * (size_t)P.G.nlevels);
    B.blocks = base + o;
    o += P.G.job_bytes * (size_t)C.n;
    C.bytes = o;
    return B;
}

// the uploaded part of a chunk, written through a host view of the same layout; returns the rects that touch the image
static inline int orb_fill(const OrbPlan &P, const OrbChunk &C, const OrbBuf &Hb, const OrbJob *jobs, const float *rect_xy)
{
    *Hb.geom = P.G;
    if (!P.taps.empty()) memcpy(Hb.taps, P.taps.data(), sizeof(OrbTap) * P.taps.size());
    const float wm = (float)(P.G.L[0].w - 1), hm = (float)(P.G.L[0].h - 1);
    int nr = 0;
    for (int j = 0; j < C.n; ++j) {
        const OrbJob &J = jobs[C.j0 + j];
        Hb.jobs[j].slot = J.slot; Hb.jobs[j].pad = 0;
        for (int r = 0; r < J.nrect; ++r) {
            const float cx = rect_xy[2 * (size_t)(J.rect_ofs + r)], cy = rect_xy[2 * (size_t)(J.rect_ofs + r) + 1];
            float x0 = rintf(cx - 10.f), y0 = rintf(cy - 10.f), x1 = rintf(cx + 10.f), y1 = rintf(cy + 10.f);
            if (x0 < 0.f) x0 = 0.f;
            if (y0 < 0.f) y0 = 0.f;
            if (x1 > wm) x1 = wm;
            if (y1 > hm) y1 = hm;
            if (!(x0 <= x1 && y0 <= y1)) continue;                 // outside the image, or not a number
            OrbRect R;
            R.x0 = (int)x0; R.y0 = (int)y0; R.x1 = (int)x1; R.y1 = (int)y1; R.job = j; R.pad0 = R.pad1 = R.pad2 = 0;
            Hb.rects[nr++] = R;
        }
    }
    return nr;
}

// the first n_out rows of every job of a chunk, to the caller's arrays; what lies behind them there is left as it was
static inline void orb_copy_out(const OrbPlan &P, const OrbChunk &C, const OrbBuf &Hb, int *n_out, int *n_found, OrbKp *out)
{
    for (int j = 0; j < C.n; ++j) {
        const int nf = Hb.res[j].n_found, no = nf < P.G.max_out ? nf : P.G.max_out;
        n_found[C.j0 + j] = nf; n_out[C.j0 + j] = no;
        if (no > 0) memcpy(out + (size_t)(C.j0 + j) * P.G.max_out, Hb.out + (size_t)j * P.G.max_out, sizeof(OrbKp) * (size_t)no);
    }
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
struct OrbView { const uint8_t *p; int pitch; };

// level l of the image of job j (level 0: the pyramid slot)
ORB_DEV OrbView orb_image(const OrbGeom &G, const OrbImg &I, const OrbBuf &B, int j, int l)
{
    OrbView V;
    if (l == 0) { V.p = I.base + (size_t)B.jobs[j].slot * I.slot_bytes + I.origin; V.pitch = I.pitch; }
    else { V.p = B.blocks + (size_t)j * G.job_bytes + G.L[l].img; V.pitch = G.L[l].w; }
    return V;
}

ORB_DEV uint32_t orb_f32_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
ORB_DEV float orb_bits_f32(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }
// f32_ordered of k_gftt.h: a key whose unsigned order is the floats' order (+0.f first: -0.f and 0.f are one key)
ORB_DEV uint32_t orb_key(float v)
{
    const uint32_t b = orb_f32_bits(v + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ORB_DEV float orb_unkey(uint32_t k) { return orb_bits_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// inclusive prefix sums of a[0 .. 255], b is scratch; eight steps, so the sums end in a.  a is written and a barrier passed before.
ORB_DEV void orb_scan(int *a, int *b)
{
    for (int d = 1; d < ORB_THREADS; d <<= 1) {
        ORB_PAR { b[tid] = a[tid] + (tid >= d ? a[tid - d] : 0); } ORB_SYNC
        int *t = a; a = b; b = t;
    }
}

// ---- mask level 0 ------------------------------------------------------------------------------------------------------------------
ORB_DEV void orb_fill_task(const OrbGeom &G, const OrbBuf &B, int j, int t)
{
    const size_t n16 = ((size_t)G.L[0].w * G.L[0].h + 15) / 16;
    if ((size_t)t >= n16) return;
    uint32_t *q = (uint32_t *)(B.blocks + (size_t)j * G.job_bytes + G.L[0].mask) + 4 * (size_t)t;
    q[0] = 0xffffffffu; q[1] = 0xffffffffu; q[2] = 0xffffffffu; q[3] = 0xffffffffu;
}

ORB_DEV void orb_rect_run(const OrbGeom &G, const OrbBuf &B, int r)
{
    const OrbRect R = B.rects[r];
    uint8_t *m = B.blocks + (size_t)R.job * G.job_bytes + G.L[0].mask;
    const int rw = R.x1 - R.x0 + 1, rh = R.y1 - R.y0 + 1, w = G.L[0].w;
    ORB_PAR {
        for (int i = tid; i < rw * rh; i += ORB_THREADS) m[(size_t)(R.y0 + i / rw) * w + R.x0 + i % rw] = 0;
    }
}

// ---- resize: flat pixels [4 t, 4 t + 4) of a w-wide level of n pixels from src by the axes' taps; which == 1: a mask -------------------------
ORB_DEV void orb_resize_px4(const uint8_t *src, int pitch, uint8_t *dst, const OrbTap *xt, const OrbTap *yt, int w, int n, int which, int t)
{
    if (4 * t >= n) return;
    uint32_t word = 0;
    int y = (4 * t) / w, x = 4 * t - y * w;
    for (int k = 0; k < 4; ++k) {
        if (4 * t + k < n) {
            const OrbTap tx = xt[x], ty = yt[y];
            const uint8_t *r0 = src + (size_t)ty.i0 * pitch, *r1 = src + (size_t)ty.i1 * pitch;
            const int t0 = (int)r0[tx.i0] * tx.c0 + (int)r0[tx.i1] * tx.c1;
            const int t1 = (int)r1[tx.i0] * tx.c0 + (int)r1[tx.i1] * tx.c1;
            uint32_t v = (uint32_t)(t0 * (int)ty.c0 + t1 * (int)ty.c1 + 32768) >> 16;
            if (which == 1 && v <= 254u) v = 0;
            word |= v << (8 * k);
        }
        if (++x == w) { x = 0; ++y; }
    }
    ((uint32_t *)dst)[t] = word;
}

// level l of job j, image (which == 0) or mask
ORB_DEV void orb_resize_task(const OrbGeom &G, const OrbImg &I, const OrbBuf &B, int l, int j, int which, int t)
{
    const OrbLevel &L = G.L[l];
    if (4 * t >= L.w * L.h) return;
    OrbView S;
    uint8_t *dst;
    if (which == 0) { S = orb_image(G, I, B, j, l - 1); dst = B.blocks + (size_t)j * G.job_bytes + L.img; }
    else { S.p = B.blocks + (size_t)j * G.job_bytes + G.L[l - 1].mask; S.pitch = G.L[l - 1].w; dst = B.blocks + (size_t)j * G.job_bytes + L.mask; }
    orb_resize_px4(S.p, S.pitch, dst, B.taps + L.xtap, B.taps + L.ytap, L.w, L.w * L.h, which, t);
}

// ---- FAST --------------------------------------------------------------------------------------------------------------------------
// the score of the pixel at p (rows `pitch` apart): the largest threshold at which it is still a corner, 0 when that is below t
ORB_DEV int orb_fast_score(const uint8_t *p, int pitch, int t)
{
    const int v = p[0];
    int d[25];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = (int)p[ORB_CIRCLE[k][1] * pitch + ORB_CIRCLE[k][0]] - v;
    // an arc of 9 holds one pixel of every opposite pair: no polarity passes unless it passes at (0, 8) and at (4, 12)
    const bool bright = (d[0] > t || d[8] > t) && (d[4] > t || d[12] > t);
    const bool dark = (d[0] < -t || d[8] < -t) && (d[4] < -t || d[12] < -t);
    if (!bright && !dark) return 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) d[16 + k] = d[k];
    int a = -256, b = 256;             // max over arcs of the arc's min, min over arcs of the arc's max
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int mn = d[k], mx = d[k];
#pragma unroll
        for (int i = 1; i < 9; ++i) { mn = d[k + i] < mn ? d[k + i] : mn; mx = d[k + i] > mx ? d[k + i] : mx; }
        a = mn > a ? mn : a;
        b = mx < b ? mx : b;
    }
    const int s = a > -b ? a : -b;
    return s > t ? s - 1 : 0;
}

#if defined(__HIPCC__) && !defined(ORB_HOST_EMU)
typedef uint32_t orb_u32_ua __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t orb_load4(const uint8_t *p) { return *(const __attribute__((address_space(1))) orb_u32_ua *)(reinterpret_cast<uintptr_t>(p)); }
#else
static inline uint32_t orb_load4(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
#endif

// tile `tile` of the interior of level l of job j.  pix: ORB_PIX_H x ORB_PIX_W bytes, sc: ORB_SC_H x ORB_SC_W bytes
ORB_DEV void orb_fast_run(const OrbGeom &G, const OrbImg &I, const OrbBuf &B, int l, int j, int tile, uint8_t *pix, uint8_t *sc)
{
    const OrbLevel &L = G.L[l];
    const int ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
    const int ox = G.edge + tx * ORB_TILE_W, oy = G.edge + ty * ORB_TILE_H;       // the tile's first interior pixel
    const OrbView V = orb_image(G, I, B, j, l);
    const bool whole = ox - 4 + ORB_PIX_W <= L.w && oy - 4 + ORB_PIX_H <= L.h;    // (ox - 4, oy - 4 >= 12)
    ORB_PAR {
        if (whole) {
            if (tid < ORB_PIX_H * (ORB_PIX_W / 4)) {
                const int r = tid / (ORB_PIX_W / 4), q = tid - r * (ORB_PIX_W / 4);
                ((uint32_t *)pix)[tid] = orb_load4(V.p + (size_t)(oy - 4 + r) * V.pitch + (ox - 4 + 4 * q));
            }
        } else {
            // a tile at the right or lower rim: pixel by pixel, coordinates held inside the image (what is held is outside the interior's reach)
            for (int i = tid; i < ORB_PIX_H * ORB_PIX_W; i += ORB_THREADS) {
                const int r = i / ORB_PIX_W, q = i - r * ORB_PIX_W;
                const int y = oy - 4 + r < L.h ? oy - 4 + r : L.h - 1, x = ox - 4 + q < L.w ? ox - 4 + q : L.w - 1;
                pix[i] = V.p[(size_t)y * V.pitch + x];
            }
        }
    } ORB_SYNC
    ORB_PAR {
        for (int i = tid; i < ORB_SC_H * ORB_SC_W; i += ORB_THREADS) {
            const int r = i / ORB_SC_W, q = i - r * ORB_SC_W;
            sc[i] = (uint8_t)orb_fast_score(pix + (r + 3) * ORB_PIX_W + (q + 3), ORB_PIX_W, G.fast_t);
        }
    } ORB_SYNC
    ORB_PAR {
        const int ly = tid / ORB_TILE_W, lx = tid - ly * ORB_TILE_W;
        const int x = ox + lx, y = oy + ly;
        if (x < L.w - G.edge && y < L.h - G.edge) {
            const uint8_t *s = sc + (ly + 1) * ORB_SC_W + (lx + 1);
            const int v = s[0];
            bool keep = v > 0 && v > s[-1] && v > s[1] && v > s[-ORB_SC_W - 1] && v > s[-ORB_SC_W] && v > s[-ORB_SC_W + 1] &&
                        v > s[ORB_SC_W - 1] && v > s[ORB_SC_W] && v > s[ORB_SC_W + 1];
            unsigned char *blk = B.blocks + (size_t)j * G.job_bytes;
            if (keep && blk[L.mask + (size_t)y * L.w + x] == 0) keep = false;
            blk[L.ks + (size_t)y * L.w + x] = keep ? (uint8_t)v : (uint8_t)0;
            if (keep) ORB_COUNT(B.hist + ((size_t)j * G.nlevels + l) * 256 + v);
        }
    } ORB_SYNC
}

// ---- Harris response ---------------------------------------------------------------------------------------------------------------
ORB_DEV float orb_harris(const uint8_t *c, int row)
{
    int a = 0, b = 0, cc = 0;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const uint8_t *p = c + dy * row + dx;
            const int Ix = ((int)p[1] - (int)p[-1]) * 2 + ((int)p[-row + 1] - (int)p[-row - 1]) + ((int)p[row + 1] - (int)p[row - 1]);
            const int Iy = ((int)p[row] - (int)p[-row]) * 2 + ((int)p[row - 1] - (int)p[-row - 1]) + ((int)p[row + 1] - (int)p[-row + 1]);
            a += Ix * Ix; b += Iy * Iy; cc += Ix * Iy;
        }
    const float scale = 1.f / (4 * 7 * 255.f);
    const float s2 = scale * scale, s3 = s2 * scale, s4 = s3 * scale;
    const float fa = (float)a, fb = (float)b, fc = (float)cc;
    const float ab = fa * fb, c2 = fc * fc;
    const float det = ab - c2;
    const float tr = fa + fb;
    const float k1 = 0.04f * tr, k2 = k1 * tr;
    const float r = det - k2;
    return r * s4;
}

// ---- OpenCV's fastAtan2 with the contract's constants: degrees in [0, 360) -----------------------------------------------------------
ORB_DEV float orb_atan_deg(float y, float x)
{
    const float k = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k, p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        const float den = ax + (float)DBL_EPSILON;
        c = ORB_FDIV(ay, den);
        c2 = c * c;
        float q = p7 * c2; q = q + p5; q = q * c2; q = q + p3; q = q * c2; q = q + p1;
        a = q * c;
    } else {
        const float den = ay + (float)DBL_EPSILON;
        c = ORB_FDIV(ax, den);
        c2 = c * c;
        float q = p7 * c2; q = q + p5; q = q * c2; q = q + p3; q = q * c2; q = q + p1;
        a = 90.f - q * c;
    }
    if (x < 0.f) a = 180.f - a;
    if (y < 0.f) a = 360.f - a;
    return a;
}

// ---- both cuts of level l of job j -----------------------------------------------------------------------------------------------------
// a, b: 256 ints each; sh: 256 counters; var: 8 ints
ORB_DEV void orb_select_run(const OrbGeom &G, const OrbImg &I, const OrbBuf &B, int l, int j, int *a, int *b, unsigned int *sh, int *var)
{
    const OrbLevel &L = G.L[l];
    OrbLvlState *st = B.lvl + (size_t)j * G.nlevels + l;
    if (!L.active) {
        ORB_PAR { if (tid == 0) { st->k1 = 0; st->k2 = 0; st->thr2 = 0; st->pad = 0; } }
        return;
    }
    unsigned char *blk = B.blocks + (size_t)j * G.job_bytes;
    const unsigned int *hist = B.hist + ((size_t)j * G.nlevels + l) * 256;
    uint32_t *pos = (uint32_t *)(blk + L.pos), *key = (uint32_t *)(blk + L.key);
    const int m = 2 * L.quota;
    // cut 1: a[i] = kept pixels with score >= 255 - i
    ORB_PAR { a[tid] = (int)hist[255 - tid]; if (tid < 8) var[tid] = 0; } ORB_SYNC
    orb_scan(a, b);
    ORB_PAR {
        if (a[255] <= m) { if (tid == 0) { var[0] = 1; var[1] = a[255]; } }
        else if (a[tid] >= m && (tid == 0 || a[tid - 1] < m)) { var[0] = 255 - tid; var[1] = a[tid]; }
    } ORB_SYNC
    const int thr1 = var[0], k1 = var[1];
    ORB_SYNC
    // the ordered list: 1024 interior pixels a step, thread t the four from 4 t on
    const int npx = L.iw * L.ih;
    int base = 0;
    for (int c0 = 0; c0 < npx; c0 += 4 * ORB_THREADS) {
        ORB_PAR {
            int k = 0;
            const int p0 = c0 + 4 * tid;
            int y = p0 / L.iw, x = p0 - y * L.iw;
            for (int i = 0; i < 4 && p0 + i < npx; ++i) {
                if ((int)blk[L.ks + (size_t)(G.edge + y) * L.w + G.edge + x] >= thr1) ++k;
                if (++x == L.iw) { x = 0; ++y; }
            }
            a[tid] = k;
        } ORB_SYNC
        orb_scan(a, b);
        ORB_PAR {
            const int p0 = c0 + 4 * tid;
            int y = p0 / L.iw, x = p0 - y * L.iw;
            int o = base + (tid ? a[tid - 1] : 0);
            for (int i = 0; i < 4 && p0 + i < npx; ++i) {
                if ((int)blk[L.ks + (size_t)(G.edge + y) * L.w + G.edge + x] >= thr1) {
                    if (o < L.list_cap) pos[o] = ((uint32_t)(G.edge + y) << 16) | (uint32_t)(G.edge + x);
                    ++o;
                }
                if (++x == L.iw) { x = 0; ++y; }
            }
        } ORB_SYNC
        base += a[255];
        ORB_SYNC
    }
    // (base == k1 <= list_cap: the histogram counted the same pixels, and no two of them are adjacent)
    const int n = k1 < L.list_cap ? k1 : L.list_cap;
    const OrbView V = orb_image(G, I, B, j, l);
    ORB_PAR {
        for (int i = tid; i < n; i += ORB_THREADS) {
            const uint32_t p = pos[i];
            key[i] = orb_key(orb_harris(V.p + (size_t)(p >> 16) * V.pitch + (p & 0xffffu), V.pitch));
        }
    } ORB_SYNC
    // cut 2: the quota-th largest key, byte by byte from the top
    uint32_t prefix = 0, mask = 0;
    if (n > L.quota) {
        int need = L.quota;
        for (int shift = 24; shift >= 0; shift -= 8) {
            ORB_PAR { sh[tid] = 0; } ORB_SYNC
            ORB_PAR {
                for (int i = tid; i < n; i += ORB_THREADS) {
                    const uint32_t k = key[i];
                    if ((k & mask) == prefix) ORB_COUNT(sh + ((k >> shift) & 255u));
                }
            } ORB_SYNC
            ORB_PAR { a[tid] = (int)sh[255 - tid]; } ORB_SYNC
            orb_scan(a, b);
            ORB_PAR {
                if (a[tid] >= need && (tid == 0 || a[tid - 1] < need)) { var[2] = 255 - tid; var[3] = tid ? a[tid - 1] : 0; }
            } ORB_SYNC
            prefix |= (uint32_t)var[2] << shift;
            mask |= 0xffu << shift;
            need -= var[3];
            ORB_SYNC
        }
    }
    // the level's count
    ORB_PAR {
        int k = 0;
        for (int i = tid; i < n; i += ORB_THREADS) if (key[i] >= prefix) ++k;
        a[tid] = k;
    } ORB_SYNC
    orb_scan(a, b);
    ORB_PAR { if (tid == 0) { st->k1 = n; st->k2 = a[255]; st->thr2 = prefix; st->pad = 0; } } ORB_SYNC
}

// ---- the rows of level l of job j -------------------------------------------------------------------------------------------------------
// a, b: 256 ints each; sel: 256 list positions; part: 4 waves x 2 x 32 partial sums
ORB_DEV void orb_emit_run(const OrbGeom &G, const OrbImg &I, const OrbBuf &B, int l, int j, int *a, int *b, uint32_t *sel, int *part)
{
    const OrbLevel &L = G.L[l];
    const OrbLvlState *sj = B.lvl + (size_t)j * G.nlevels;
    int row0 = 0, total = 0;
    for (int i = 0; i < G.nlevels; ++i) { if (i < l) row0 += sj[i].k2; total += sj[i].k2; }
    if (l == 0) { ORB_PAR { if (tid == 0) { B.res[j].n_found = total; B.res[j].pad = 0; } } }
    const int n = sj[l].k1;
    const uint32_t thr2 = sj[l].thr2;
    if (n == 0 || row0 >= G.max_out) return;
    unsigned char *blk = B.blocks + (size_t)j * G.job_bytes;
    const uint32_t *pos = (const uint32_t *)(blk + L.pos), *key = (const uint32_t *)(blk + L.key);
    OrbKp *out = B.out + (size_t)j * G.max_out;
    const OrbView V = orb_image(G, I, B, j, l);
    int base = row0;
    for (int c0 = 0; c0 < n && base < G.max_out; c0 += ORB_THREADS) {
        ORB_PAR { a[tid] = c0 + tid < n && key[c0 + tid] >= thr2 ? 1 : 0; } ORB_SYNC
        orb_scan(a, b);
        ORB_PAR {
            const int i = c0 + tid;
            if (i < n && key[i] >= thr2) {
                const int e = a[tid] - 1, row = base + e;
                sel[e] = pos[i];
                if (row < G.max_out) {
                    const uint32_t p = pos[i];
                    OrbKp K;
                    K.x = (float)(int)(p & 0xffffu) * L.scale; K.y = (float)(int)(p >> 16) * L.scale; K.size = 31.f * L.scale;
                    K.angle = 0.f; K.response = orb_unkey(key[i]); K.octave = l;
                    out[row] = K;
                }
            }
        } ORB_SYNC
        const int cnt = a[255] < G.max_out - base ? a[255] : G.max_out - base;      // rows of this step that are written
        const int step = a[255];
        ORB_SYNC
        // orientation: wave q of the workgroup takes row e0 + q, lane v + 15 the patch row v
        for (int e0 = 0; e0 < cnt; e0 += ORB_THREADS / ORB_WAVE) {
            ORB_PAR {
                const int q = tid / ORB_WAVE, lane = tid - q * ORB_WAVE, e = e0 + q;
                if (e < cnt && lane < 32) {
                    int m10 = 0, m01 = 0;
                    if (lane < 2 * ORB_HALF_PATCH + 1) {
                        const int v = lane - ORB_HALF_PATCH, um = ORB_UMAX[v < 0 ? -v : v];
                        const uint32_t p = sel[e];
                        const uint8_t *c = V.p + (size_t)((int)(p >> 16) + v) * V.pitch + (p & 0xffffu);
                        int s = 0;
                        for (int u = -um; u <= um; ++u) { const int val = c[u]; m10 += u * val; s += val; }
                        m01 = v * s;
                    }
                    part[q * 64 + lane] = m10; part[q * 64 + 32 + lane] = m01;
                }
            } ORB_SYNC
            ORB_PAR {
                const int q = tid / ORB_WAVE, lane = tid - q * ORB_WAVE, e = e0 + q;
                if (e < cnt && lane == 0) {
                    int m10 = 0, m01 = 0;
                    for (int i = 0; i < 32; ++i) { m10 += part[q * 64 + i]; m01 += part[q * 64 + 32 + i]; }
                    out[base + e].angle = orb_atan_deg((float)m01, (float)m10);
                }
            } ORB_SYNC
        }
        base += step;
    }
}

#ifndef ORB_HOST_EMU
// grid (ceil(ceil(w h / 16) / 256), n)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_fill(OrbBuf B)
{
    orb_fill_task(*B.geom, B, (int)blockIdx.y, (int)(blockIdx.x * ORB_THREADS + threadIdx.x));
}
// grid (rects)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_rects(OrbBuf B) { orb_rect_run(*B.geom, B, (int)blockIdx.x); }
// grid (ceil(ceil(w_l h_l / 4) / 256), n, 2)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_resize(OrbImg I, OrbBuf B, int l)
{
    orb_resize_task(*B.geom, I, B, l, (int)blockIdx.y, (int)blockIdx.z, (int)(blockIdx.x * ORB_THREADS + threadIdx.x));
}
// grid (tiles_x tiles_y, n)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_fast(OrbImg I, OrbBuf B, int l)
{
    __shared__ __attribute__((aligned(16))) uint8_t pix[ORB_PIX_H * ORB_PIX_W];
    __shared__ uint8_t sc[ORB_SC_H * ORB_SC_W];
    orb_fast_run(*B.geom, I, B, l, (int)blockIdx.y, (int)blockIdx.x, pix, sc);
}
// grid (nlevels, n)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_select(OrbImg I, OrbBuf B)
{
    __shared__ int a[ORB_THREADS], b[ORB_THREADS], var[8];
    __shared__ unsigned int sh[256];
    orb_select_run(*B.geom, I, B, (int)blockIdx.x, (int)blockIdx.y, a, b, sh, var);
}
// grid (nlevels, n)
__global__ void __launch_bounds__(ORB_THREADS) k_orb_emit(OrbImg I, OrbBuf B)
{
    __shared__ int a[ORB_THREADS], b[ORB_THREADS], part[4 * 64];
    __shared__ uint32_t sel[ORB_THREADS];
    orb_emit_run(*B.geom, I, B, (int)blockIdx.x, (int)blockIdx.y, a, b, sel, part);
}
#endif
