// BRIEF-256 descriptors at given points of level 0 of resident pyramid slots (svslam_brief_describe_batch): what
// cv::ORB::compute does with provided keypoints that carry KeyPoint's default angle (LoopClosure::ExtractKeypointsDescriptor,
// src/loopclosure.cpp:131-171).  The procedure, all integer or a written-out f32 step:
//   filter   a point is kept iff edge <= x < w - edge and edge <= y < h - edge (float compares); kept points keep their order, the
//            kept rows of a job are the first n_desc rows of its range, desc_pt[row] = the point's index inside the job;
//            centre = round-half-to-even of (x, y)
//   offsets  once per call on the host (br_offsets): a = cosf(angle_deg * (pi / 180)), b = sinf(..) in f32,
//            ix = rint(px a - py b), iy = rint(px b + py a) for the 512 table points
//   blur     separable 7 taps (18, 34, 49, 54, 49, 34, 18) / 256 (sigma 2): the horizontal sum is kept in full (<= 65280, u16), the
//            vertical sum over it, out = (v + 32768) >> 16.  Only pixels inside the image are read: edge >= reach + 4 is checked.
//   tests    bit t = B(c + off[2t]) < B(c + off[2t + 1]), strict; byte t / 8, bit t % 8
// Two kernels.  k_brief_filter: one workgroup of 256 threads per job, thread t owns points 4t .. 4t + 3 (1024 at the most), a
// blocked count, a prefix over the LDS counts, an order-keeping write of (row -> point, centre, slot).  k_brief_describe: one
// wavefront per row, four rows per 256-thread workgroup; the wave loads the (2 reach + 7)^2 patch around the centre into LDS, runs
// the horizontal pass into u16 and the vertical pass into u8 there, each lane evaluates tests lane, lane + 64, lane + 128,
// lane + 192, and 8 lanes pack the 256 flags into the row's 8 dwords.  The LDS of a wave is sized from the table's reach at launch.
// As in k_loop_verify.h nothing crosses lanes except through LDS between barriers and the file is plain C++ between the HIP
// qualifiers: compiled for the host with BR_HOST_EMU (tests/cpp/brief_host_emu) a phase becomes a loop over the 256 thread numbers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define BR_THREADS 256
#define BR_WAVE 64
#define BR_ROWS_PER_WG 4           // BR_THREADS / BR_WAVE
#define BR_PTS_PER_THREAD 4        // BR_MAX_PTS / BR_THREADS
#define BR_MAX_PTS 1024            // points per job (DESIGN 11's limit of rows per side)
#define BR_MAX_REACH 24            // largest |offset| after rotation: 4 waves x 10.9 KB of LDS

#ifdef BR_HOST_EMU
#define BR_DEV static inline
#define BR_PAR for (int tid = 0; tid < BR_THREADS; ++tid)
#define BR_SYNC
#else
#define BR_DEV __device__ __forceinline__
#define BR_PAR for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define BR_SYNC __syncthreads();
#endif

// The default table: x0, y0, x1, y1 of 256 tests, all |c| <= 13.  Candidate k = 0, 1, ... takes its four coordinates from
// m(4k) .. m(4k + 3), each ((uint64)m * 27 >> 32) - 13, where m(n) = mix(n * 0x9E3779B1 ^ 0x42524946) and mix is
// h ^= h >> 16, h *= 0x7feb352d, h ^= h >> 15, h *= 0x846ca68b, h ^= h >> 16 on 32 bits.  A candidate whose two points coincide, or
// which (or whose reverse) is in the table already, is dropped; the first 256 kept are the table.  tests/ref_brief.py regenerates it.
static const int8_t BR_DEFAULT_PATTERN[1024] = {
    -6,13,-9,11,10,-7,10,-8,4,6,13,-5,-1,2,-2,8,-4,-2,-11,7,0,4,9,-12,-10,4,-6,-6,-3,-5,11,6,
    6,-11,1,-3,-5,-1,13,-2,9,1,5,-13,-9,4,-2,-3,-9,12,-6,12,-11,4,10,5,11,-11,13,-9,9,8,-7,4,
    -3,-11,9,1,-7,0,3,4,8,3,-3,10,12,-4,-10,-1,0,-13,-4,4,-13,-9,-3,8,4,0,-13,-3,-12,-10,1,2,
    -1,-7,-12,-5,1,8,-4,2,10,-7,12,9,12,-1,-11,7,10,-11,-4,8,10,-2,6,10,-1,-4,-4,-3,-7,7,-9,-13,
    -4,1,0,-9,9,-1,-9,-12,5,1,10,-13,-9,-4,-7,9,0,-12,5,-10,13,-6,1,6,-12,5,2,3,8,-10,10,-6,
    -8,-13,-2,-12,11,11,-12,-9,-8,7,5,11,-2,-5,4,-10,-8,10,-3,4,-2,1,-3,-10,-13,0,9,-6,-7,-4,13,4,
    8,-12,-5,1,-2,-13,12,-10,11,13,-10,-7,-9,7,-9,-8,-1,4,-12,-10,-1,2,-4,-11,-1,12,0,-2,-8,-6,-7,12,
    11,-3,-7,1,1,-4,-2,11,-7,-2,-7,9,-4,-6,12,13,-12,-6,11,-6,-7,2,-2,13,-5,8,8,0,8,12,2,12,
    8,-6,-4,-5,-10,8,5,3,0,-12,5,-1,10,13,2,9,-12,-2,-2,10,11,-11,-9,12,10,7,-1,-13,-6,-3,9,3,
    6,10,-1,5,-6,-2,7,-12,-13,-11,-13,6,9,1,8,-7,0,3,-4,10,7,8,10,9,-7,-12,4,-3,-2,-1,-9,10,
    -12,0,11,-3,5,-2,-7,11,2,10,7,-9,-5,10,-4,-7,3,-7,13,6,4,-3,6,-10,1,-6,-4,-8,12,-3,13,9,
    -4,7,0,11,8,-2,-12,3,8,9,1,-12,9,4,-2,6,-6,2,12,8,9,-10,6,0,-9,-1,5,10,7,1,-9,6,
    1,11,-4,-5,-5,8,2,2,-1,13,-11,4,5,6,-12,-8,5,-7,4,-12,-9,2,1,11,-8,4,13,-13,11,-6,-5,-9,
    10,-9,13,-4,-6,-13,7,13,-12,-3,-11,-5,0,-6,-2,-6,-10,-13,8,8,7,-5,11,7,1,10,3,4,11,0,3,-13,
    6,6,-3,-12,-5,13,6,5,-12,3,6,13,-11,-9,6,-12,0,12,-12,10,-1,0,9,6,0,10,-2,-13,5,8,-11,9,
    1,12,11,13,-1,11,7,-5,-3,13,7,0,1,-12,7,5,11,9,-3,7,-3,-3,-10,1,-8,13,-11,8,7,9,3,4,
    -2,4,1,-7,8,-9,-13,3,8,1,-13,13,-3,-11,-3,4,3,-5,-11,-12,-12,-9,-3,-10,-8,-1,8,-12,12,0,-5,9,
    -13,8,1,-6,-4,-2,9,-1,6,-2,5,-4,5,3,3,-6,6,-11,8,-13,-3,6,-8,13,3,0,-3,8,-10,9,4,-2,
    3,5,-6,-10,-10,2,8,-5,10,1,-1,-1,-13,-3,-5,4,-1,6,-6,7,-11,1,-12,5,-1,-11,-8,0,-13,-5,-11,2,
    -9,-9,-9,0,7,-5,7,1,4,-3,9,-4,8,5,-5,-12,6,9,-12,-3,10,12,11,13,-7,-9,-1,-7,3,-3,-4,-7,
    11,9,4,-1,-8,-12,5,-12,12,-9,-6,-4,-7,-5,-6,-6,12,10,-11,-8,-1,-8,-7,-3,10,4,-9,-4,-4,0,7,12,
    9,5,6,4,10,6,9,0,-13,-5,6,9,-9,10,5,11,-11,2,1,-1,-10,8,8,-8,-9,-7,10,7,2,2,10,12,
    -2,-6,12,-9,-6,8,4,-2,6,12,-9,3,-4,-1,-6,-13,3,-3,-10,5,8,13,12,-8,0,4,-7,-13,9,2,11,-3,
    -4,-13,9,0,2,0,4,1,-3,-4,13,12,-4,1,-6,0,2,3,-9,7,-10,-12,5,-2,-1,5,-10,13,-2,2,-5,12,
    9,12,-11,-11,-12,1,4,-9,-10,-10,5,-2,11,-9,11,-6,-7,6,-2,0,3,-1,13,2,13,3,0,-11,-9,-2,6,0,
    -11,-1,5,4,2,2,11,1,-10,8,-8,8,-10,-6,1,8,3,-8,-10,-1,-1,-1,-8,5,11,4,11,-2,-6,-9,-11,-5,
    2,-9,-1,3,6,-13,12,3,-2,-8,-6,1,6,3,-6,2,11,7,5,-6,7,-1,4,-2,10,6,-11,-8,1,10,7,-8,
    1,-6,12,0,-7,-7,6,-1,-4,-8,5,1,7,12,5,1,-3,-8,-12,8,8,3,-8,-12,-7,7,-7,11,0,3,-10,-2,
    -11,12,9,0,-10,7,1,-7,1,2,0,-6,12,-11,3,4,-3,1,-7,0,9,-1,13,8,-11,-5,-8,-2,-9,-12,0,10,
    -10,5,-3,9,1,2,-11,12,-7,0,4,-4,-6,9,-3,12,-13,11,1,-11,-1,1,-6,-4,-4,1,8,7,3,1,11,11,
    6,3,10,2,-9,-6,-12,5,11,-3,6,-11,-11,10,6,-6,-8,9,2,-12,-1,3,8,5,-11,3,-4,-13,-11,10,12,3,
    -13,9,-2,-2,9,-9,12,6,5,11,-1,-1,-6,-8,-13,7,-13,13,8,-6,8,0,0,7,2,12,-7,6,-2,-5,-4,-8,
};

struct BrJob { int slot, pt_ofs, npts, n_desc; };
struct BrCtr { int cx, cy, slot, pad; };           // a row's centre and image; cx = -1: no row here

// level 0 of the slots as the kernels read it: pixel (x, y) of slot s is base[s * slot_bytes + origin + y * pitch + x]
struct BrImg { const uint8_t *base; size_t slot_bytes, origin; int pitch, w, h; };

// the LDS of one wave, from the table's reach
struct BrPlan { int reach, R, P, Bw, o_h, o_b, o_bits, wave_bytes; };

struct BrBuf {
    BrCtr *ctr;                 // [total_pts], uploaded with cx = -1, written by the filter
    const float *xy;            // [total_pts][2]
    const uint16_t *tbl;        // [512]: index of an offset inside a wave's (2 reach + 1)^2 blurred patch
    BrJob *jobs;                // read back from here on
    int *desc_pt;               // [total_pts]
    uint32_t *desc;             // [total_pts][8]
};

struct BrSizes { size_t upload_bytes = 0, result_ofs = 0, bytes = 0; };

static inline BrPlan br_plan(int reach)
{
    BrPlan L;
    L.reach = reach; L.R = reach + 3; L.P = 2 * reach + 7; L.Bw = 2 * reach + 1;
    int o = (L.P * L.P + 15) & ~15;
    L.o_h = o; o += (2 * L.P * L.Bw + 15) & ~15;
    L.o_b = o; o += (L.Bw * L.Bw + 15) & ~15;
    L.o_bits = o; o += 256;
    L.wave_bytes = o;
    return L;
}

// the rotated, rounded table: off[2 i], off[2 i + 1] = ix, iy of table point i (512 points); returns the reach
static inline int br_offsets(const int8_t *pattern, float angle_deg, int *off)
{
    const float ang = angle_deg * (float)(3.14159265358979323846 / 180.0);
    const float a = cosf(ang), b = sinf(ang);
    int reach = 0;
    for (int i = 0; i < 512; ++i) {
        const float px = (float)pattern[2 * i], py = (float)pattern[2 * i + 1];
        const float xa = px * a, yb = py * b, xb = px * b, ya = py * a;
        const float fx = xa - yb, fy = xb + ya;
        const int ix = (int)rintf(fx), iy = (int)rintf(fy);
        off[2 * i] = ix; off[2 * i + 1] = iy;
        const int m = abs(ix) > abs(iy) ? abs(ix) : abs(iy);
        if (m > reach) reach = m;
    }
    return reach;
}

// returns nullptr or the reason the call is refused (nothing has been written then); off and *reach are filled on the way
static inline const char *br_check(int njobs, const BrJob *jobs, int total_pts, int nslots, const int8_t *pattern, float angle_deg,
                                   int edge, int *off, int *reach)
{
    if (!(angle_deg == angle_deg) || fabsf(angle_deg) > 3.0e38f) return "angle_deg is not finite";
    for (int t = 0; t < 256; ++t)
        if (pattern[4 * t] == pattern[4 * t + 2] && pattern[4 * t + 1] == pattern[4 * t + 3]) return "the two points of a table entry coincide";
    *reach = br_offsets(pattern, angle_deg, off);
    if (edge < *reach + 4) return "edge is below the table's reach after rotation + 4";
    if (*reach > BR_MAX_REACH) return "the table's reach after rotation is above 24";
    for (int j = 0; j < njobs; ++j) {
        const BrJob &J = jobs[j];
        if (J.npts < 0 || J.pt_ofs < 0 || (long long)J.pt_ofs + J.npts > total_pts) return "a job's range leaves the arrays";
        if (J.npts > BR_MAX_PTS) return "a job has more than 1024 points";
        if (j > 0 && J.pt_ofs < jobs[j - 1].pt_ofs + jobs[j - 1].npts) return "the jobs' ranges must ascend and not overlap";
        if (J.slot < 0 || J.slot >= nslots) return "a job's slot is out of range";
    }
    return nullptr;
}

// one buffer: [centres | points | table | jobs] (uploaded) [jobs | rows -> points | descriptors] (read back)
static inline BrBuf br_layout(BrSizes &Z, int njobs, int total_pts, unsigned char *base)
{
    BrBuf B;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *p = base + o; o += (bytes + 15) & ~(size_t)15; return p; };
    B.ctr = (BrCtr *)take(sizeof(BrCtr) * (size_t)total_pts);
    B.xy = (const float *)take(8 * (size_t)total_pts);
    B.tbl = (const uint16_t *)take(2 * 512);
    Z.result_ofs = o;
    B.jobs = (BrJob *)take(sizeof(BrJob) * (size_t)njobs);
    Z.upload_bytes = o;
    B.desc_pt = (int *)take(4 * (size_t)total_pts);
    B.desc = (uint32_t *)take(32 * (size_t)total_pts);
    Z.bytes = o;
    return B;
}

// the uploaded part before the launch, written through a host view of the same layout
static inline void br_fill(const BrBuf &Hb, const BrPlan &L, int njobs, const BrJob *jobs, int total_pts, const float *xy, const int *off)
{
    for (int i = 0; i < total_pts; ++i) { BrCtr &c = Hb.ctr[i]; c.cx = -1; c.cy = -1; c.slot = -1; c.pad = 0; }
    if (total_pts) memcpy((void *)Hb.xy, xy, 8 * (size_t)total_pts);
    uint16_t *t = (uint16_t *)Hb.tbl;
    for (int i = 0; i < 512; ++i) t[i] = (uint16_t)((off[2 * i + 1] + L.reach) * L.Bw + off[2 * i] + L.reach);
    for (int j = 0; j < njobs; ++j) { Hb.jobs[j] = jobs[j]; Hb.jobs[j].n_desc = 0; }
}

// the first n_desc rows of every job, to the caller's arrays; what lies behind them there is left as it was
static inline void br_copy_out(const BrBuf &Hb, int njobs, BrJob *jobs, uint8_t *desc, int *desc_pt)
{
    for (int j = 0; j < njobs; ++j) {
        const BrJob &J = Hb.jobs[j];
        jobs[j].n_desc = J.n_desc;
        if (J.n_desc > 0) {
            memcpy(desc_pt + J.pt_ofs, Hb.desc_pt + J.pt_ofs, 4 * (size_t)J.n_desc);
            memcpy(desc + 32 * (size_t)J.pt_ofs, Hb.desc + 8 * (size_t)J.pt_ofs, 32 * (size_t)J.n_desc);
        }
    }
}

// ---- filter and compaction of one job ----------------------------------------------------------------------------------------------
// the contract's filter; the last four conditions restate, on the rounded centre, that every tap lies inside the image (they hold
// whenever edge >= reach + 4 and are here so that no input can make the describe kernel read outside its slot)
BR_DEV bool br_keep(float x, float y, int edge, int w, int h, int R, int *cx, int *cy)
{
    if (!((float)edge <= x && x < (float)(w - edge) && (float)edge <= y && y < (float)(h - edge))) return false;
    const int ix = (int)rintf(x), iy = (int)rintf(y);
    *cx = ix; *cy = iy;
    return ix - R >= 0 && ix + R < w && iy - R >= 0 && iy + R < h;
}

BR_DEV void br_filter_run(const BrBuf &B, const BrImg &I, int edge, int R, BrJob &J, int *cnt)
{
    const int n = J.npts, ofs = J.pt_ofs, slot = J.slot;
    const float *xy = B.xy + 2 * (size_t)ofs;
    BR_PAR {
        int k = 0, cx, cy;
        for (int i = tid * BR_PTS_PER_THREAD; i < (tid + 1) * BR_PTS_PER_THREAD && i < n; ++i)
            if (br_keep(xy[2 * i], xy[2 * i + 1], edge, I.w, I.h, R, &cx, &cy)) ++k;
        cnt[tid] = k;
    } BR_SYNC
    BR_PAR {
        int o = 0, cx, cy;
        for (int t = 0; t < tid; ++t) o += cnt[t];
        for (int i = tid * BR_PTS_PER_THREAD; i < (tid + 1) * BR_PTS_PER_THREAD && i < n; ++i)
            if (br_keep(xy[2 * i], xy[2 * i + 1], edge, I.w, I.h, R, &cx, &cy)) {
                BrCtr c; c.cx = cx; c.cy = cy; c.slot = slot; c.pad = 0;
                B.ctr[ofs + o] = c; B.desc_pt[ofs + o] = i;
                ++o;
            }
        if (tid == BR_THREADS - 1) J.n_desc = o;
    } BR_SYNC
}

// ---- four rows of the call: patch, blur, tests -----------------------------------------------------------------------------------
// the row of this thread's wave, or false
BR_DEV bool br_row(const BrBuf &B, int total_pts, int wg, int tid, int *g, BrCtr *c)
{
    *g = wg * BR_ROWS_PER_WG + tid / BR_WAVE;
    if (*g >= total_pts) return false;
    *c = B.ctr[*g];
    return c->cx >= 0;
}

// the phases of one wave on its LDS block (shared with k_orb_desc.h): the patch whose first pixel is src, rows `pitch` apart
BR_DEV void br_patch_load(uint8_t *patch, const uint8_t *src, size_t pitch, int P, int lane)
{
    const int sr = BR_WAVE / P, sx = BR_WAVE % P;
    int r = lane / P, x = lane % P;
    for (int i = lane; i < P * P; i += BR_WAVE) {
        patch[i] = src[(size_t)r * pitch + x];
        r += sr; x += sx;
        if (x >= P) { x -= P; ++r; }
    }
}

// horizontal: P rows of Bw sums
BR_DEV void br_blur_h(const uint8_t *patch, uint16_t *hs, int P, int Bw, int lane)
{
    const int sr = BR_WAVE / Bw, sx = BR_WAVE % Bw;
    int r = lane / Bw, x = lane % Bw;
    for (int i = lane; i < P * Bw; i += BR_WAVE) {
        const uint8_t *p = patch + r * P + x;
        const int v = 18 * (p[0] + p[6]) + 34 * (p[1] + p[5]) + 49 * (p[2] + p[4]) + 54 * p[3];
        hs[i] = (uint16_t)v;
        r += sr; x += sx;
        if (x >= Bw) { x -= Bw; ++r; }
    }
}

// vertical: Bw rows of Bw blurred pixels
BR_DEV void br_blur_v(const uint16_t *hs, uint8_t *bl, int Bw, int lane)
{
    for (int i = lane; i < Bw * Bw; i += BR_WAVE) {
        const uint16_t *p = hs + i;            // (r, x) -> rows r .. r + 6 of the sums, same column
        const int v = 18 * ((int)p[0] + (int)p[6 * Bw]) + 34 * ((int)p[Bw] + (int)p[5 * Bw]) + 49 * ((int)p[2 * Bw] + (int)p[4 * Bw])
                      + 54 * (int)p[3 * Bw];
        bl[i] = (uint8_t)((v + 32768) >> 16);
    }
}

// lane < 8: dword `lane` of the descriptor from the 256 flags
BR_DEV uint32_t br_pack(const uint8_t *bits, int lane)
{
    uint32_t v = 0;
    for (int k = 0; k < 32; ++k) v |= (uint32_t)bits[32 * lane + k] << k;
    return v;
}

BR_DEV void br_describe_run(const BrBuf &B, const BrImg &I, const BrPlan &L, int total_pts, int wg, unsigned char *smem)
{
    BR_PAR {                                           // the patch
        int g; BrCtr c;
        if (br_row(B, total_pts, wg, tid, &g, &c))
            br_patch_load(smem + (size_t)(tid / BR_WAVE) * L.wave_bytes,
                          I.base + (size_t)c.slot * I.slot_bytes + I.origin + (size_t)(c.cy - L.R) * I.pitch + (size_t)(c.cx - L.R),
                          (size_t)I.pitch, L.P, tid % BR_WAVE);
    } BR_SYNC
    BR_PAR {
        int g; BrCtr c;
        if (br_row(B, total_pts, wg, tid, &g, &c)) {
            unsigned char *wv = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes;
            br_blur_h(wv, (uint16_t *)(wv + L.o_h), L.P, L.Bw, tid % BR_WAVE);
        }
    } BR_SYNC
    BR_PAR {
        int g; BrCtr c;
        if (br_row(B, total_pts, wg, tid, &g, &c)) {
            unsigned char *wv = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes;
            br_blur_v((const uint16_t *)(wv + L.o_h), wv + L.o_b, L.Bw, tid % BR_WAVE);
        }
    } BR_SYNC
    BR_PAR {                                           // the tests
        int g; BrCtr c;
        if (br_row(B, total_pts, wg, tid, &g, &c)) {
            const int lane = tid % BR_WAVE;
            const uint8_t *bl = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_b;
            uint8_t *bits = smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_bits;
            for (int t = lane; t < 256; t += BR_WAVE) bits[t] = bl[B.tbl[2 * t]] < bl[B.tbl[2 * t + 1]] ? 1 : 0;
        }
    } BR_SYNC
    BR_PAR {                                           // 8 lanes, one dword of the descriptor each
        int g; BrCtr c;
        if (br_row(B, total_pts, wg, tid, &g, &c)) {
            const int lane = tid % BR_WAVE;
            if (lane < 8) B.desc[8 * (size_t)g + lane] = br_pack(smem + (size_t)(tid / BR_WAVE) * L.wave_bytes + L.o_bits, lane);
        }
    } BR_SYNC
}

#ifndef BR_HOST_EMU
__global__ void __launch_bounds__(BR_THREADS) k_brief_filter(BrBuf B, BrImg I, int edge, int R)
{
    __shared__ int cnt[BR_THREADS];
    br_filter_run(B, I, edge, R, B.jobs[blockIdx.x], cnt);
}

__global__ void __launch_bounds__(BR_THREADS) k_brief_describe(BrBuf B, BrImg I, BrPlan L, int total_pts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char br_smem[];
    br_describe_run(B, I, L, total_pts, (int)blockIdx.x, br_smem);
}
#endif
