// k_stereo_bm.h — dense stereo of the reference's second program (run_dense_reconstruction):
//   k_bm_fill      FILTERED (-16) into every pixel cv::StereoBM never computes
//   k_stereo_bm    cv::StereoBM::compute(left, right) with the settings of include/StereoVisionSLAM/dense_reconstruction.h:56-57
//                  (StereoBM::create(128, 15): PREFILTER_XSOBEL cap 31, minDisparity 0, textureThreshold 10, uniquenessRatio 15,
//                  no speckle filter, no disp12MaxDiff), CV_16S = 16 x disparity  (src/dense_reconstruction.cpp:114)
//   k_dense_cloud  disparity -> depth -> map frame, compacted in the reference's loop order (src/dense_reconstruction.cpp:116-173)
// Integer arithmetic throughout the matcher: bit for bit the numpy restatement tests/ref_stereo_bm.py.
//
// Shape of k_stereo_bm.  A workgroup of 4 waves owns BM_TW = 64 output columns x `th` output rows.  It runs the
// X-Sobel prefilter straight from the two level-0 images into an LDS strip of L' and R' bytes (th + 2r rows), so neither the
// prefiltered images nor the SAD volume ever exist in HBM.  Lane = output column, wave g = disparity chunks g, g+4, .. of 16
// disparities.  For one image row a lane holds the window's 2r+1 bytes of L' in <= 6 registers and, per chunk, the 16 + 2r
// bytes of R' it can meet; v_alignbyte_b32 slides R' under L' and one v_sad_u8 takes four absolute differences.  The
// horizontal row sums H(x, d, row) slide vertically in registers: S += H(new row) - H(old row).  Per output row the
// nd sums of every column go to LDS (u16 pairs); min / arg-min (ties to the LARGEST d), the uniqueness scan, the texture
// sum (wave 0, same machinery against the cap byte) and the sub-pixel step follow from there.
//
// BM_HOST_EMU (tests/cpp/bm_host_emu, after tests/cpp/hip_on_host.h): the matcher half of this file under g++ as it stands.  LDS is
// the emulation's heap block, the two byte instructions are its functions, the cloud half (d_quat_rot) is left out.
#pragma once
#ifdef BM_HOST_EMU
#include "pyr_geom.h"
#define BM_LDS(name) unsigned int *name = emu_lds
#define __builtin_amdgcn_alignbyte emu_alignbyte
#define __builtin_amdgcn_sad_u8 emu_sad_u8
#else
#include "dev_common.h"
#define BM_LDS(name) extern __shared__ unsigned int name[]
#endif

#define BM_TW 64
#define BM_THREADS 256
#define BM_FILTERED (-16)       // (minDisparity - 1) << 4

struct BmJob { int slot_left, slot_right; };
struct BmParams { int nd, bs, cap, tex_thr, uniq; };

// strip pitches in bytes (multiples of 4) and the LDS a workgroup needs; NWW = words that hold a window row = ceil(bs / 4)
__host__ __device__ inline int bm_pitch_l(int nww) { return BM_TW + 4 * nww; }
__host__ __device__ inline int bm_pitch_r(int nd, int nww) { return ((nd + 47) & ~3) + 4 * (nww + 5); }
__host__ __device__ inline size_t bm_lds_bytes(int nd, int bs, int th)
{
    const int nww = (bs + 3) / 4, srows = th + 2 * (bs / 2);
    return (size_t)srows * (bm_pitch_l(nww) + bm_pitch_r(nd, nww)) + (size_t)(nd / 2) * BM_TW * 4 + 4 * BM_TW * 8 + 2 * BM_TW * 4;
}

// What a call of njobs jobs on w x h images launches.  [x0, x1) x [y0, y1) is the window cv::StereoBM computes, k_bm_fill's argument:
// empty, and th 0, on stereobm.cpp's early-out (no column or no row to compute: every pixel FILTERED).  th = rows per strip of
// k_stereo_bm: 16 amortise the 2r+1 rows a strip starts with; a call of fewer than 1024 workgroups takes shorter strips (8, 4) to
// fill the device.  The grid is (tiles, strips, njobs), lds the dynamic LDS of a workgroup.
struct BmPlan { int x0, x1, y0, y1, th, tiles, strips; size_t lds; };
inline BmPlan bm_plan(int w, int h, int njobs, const BmParams &P)
{
    const int r = P.bs / 2;
    BmPlan p = { P.nd - 1 + r, w - r, r, h - r, 0, 0, 0, 0 };
    if (p.x0 >= p.x1 || h < 2 * r + 1) { p.x0 = p.x1 = p.y0 = p.y1 = 0; return p; }
    p.tiles = (p.x1 - p.x0 + BM_TW - 1) / BM_TW;
    p.th = 32;
    do { p.th >>= 1; p.strips = (p.y1 - p.y0 + p.th - 1) / p.th; } while (p.th > 4 && (long long)p.tiles * p.strips * njobs < 1024);
    p.lds = bm_lds_bytes(P.nd, P.bs, p.th);
    return p;
}

// one pixel of cv::prefilterXSobel: rows outside the image reflect without repeating the edge, columns 0 and w-1 and an
// unpaired last row are cap
__device__ __forceinline__ int bm_prefilter(const uint8_t *img, int pitch, int w, int h, int x, int y, int cap)
{
    if (x <= 0 || x >= w - 1 || ((h & 1) && y == h - 1)) return cap;
    const int ym = y > 0 ? y - 1 : (h > 1 ? 1 : 0), yp = y < h - 1 ? y + 1 : (h > 1 ? h - 2 : 0);
    const uint8_t *r0 = img + (size_t)ym * pitch + x, *r1 = img + (size_t)y * pitch + x, *r2 = img + (size_t)yp * pitch + x;
    const int v = ((int)r0[1] - (int)r0[-1]) + 2 * ((int)r1[1] - (int)r1[-1]) + ((int)r2[1] - (int)r2[-1]);
    return min(max(v, -cap), cap) + cap;
}

// element i of the njobs disparity images: FILTERED unless the matcher computes it
__device__ __forceinline__ void bm_fill_one(int16_t *out, size_t i, int w, int h, int x0, int x1, int y0, int y1)
{
    const int p = (int)(i % ((size_t)w * h)), y = p / w, x = p - y * w;
    if (!(x >= x0 && x < x1 && y >= y0 && y < y1)) out[i] = BM_FILTERED;
}
__global__ void k_bm_fill(int16_t *out, int w, int h, int njobs, int x0, int x1, int y0, int y1)
{
    const size_t n = (size_t)w * h * njobs;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) bm_fill_one(out, i, w, h, x0, x1, y0, y1);
}

template <int NWW>
__global__ __launch_bounds__(BM_THREADS) void k_stereo_bm(const BmJob *jobs, const uint8_t *pyr, PyrGeom g, BmParams P, int th, int16_t *out)
{
    BM_LDS(bm_lds);
    const int w = g.w[0], h = g.h[0], nd = P.nd, r = P.bs >> 1, cap = P.cap;
    const int tid = threadIdx.x, xi = tid & 63, wv = tid >> 6;
    const int x0 = nd - 1 + r + (int)blockIdx.x * BM_TW;         // first output column of the tile (< w - r by the grid)
    const int y0 = r + (int)blockIdx.y * th;                     // first output row of the strip (< h - r by the grid)
    const int rows = min(th, h - r - y0), srows = rows + 2 * r;  // output rows, strip rows (image rows y0 - r .. y0 + rows - 1 + r)
    const int pitchL = bm_pitch_l(NWW), pitchR = bm_pitch_r(nd, NWW);
    const int smax = th + 2 * r;
    uint8_t *Lb = reinterpret_cast<uint8_t *>(bm_lds);
    uint8_t *Rb = Lb + (size_t)smax * pitchL;
    unsigned int *sadw = reinterpret_cast<unsigned int *>(Rb + (size_t)smax * pitchR);     // [nd / 2][BM_TW]: SAD(d) | SAD(d + 1) << 16
    int *part = reinterpret_cast<int *>(sadw + (size_t)(nd / 2) * BM_TW);                  // [4][BM_TW] min, [4][BM_TW] arg-min
    int *uq = part + 8 * BM_TW;                                                            // [2][BM_TW] uniqueness failed (row parity)
    const BmJob jb = jobs[blockIdx.z];
    const uint8_t *imgL = lvl_origin(pyr + (size_t)jb.slot_left * g.slot_bytes, g, 0);
    const uint8_t *imgR = lvl_origin(pyr + (size_t)jb.slot_right * g.slot_bytes, g, 0);
    const int ipitch = g.pitch[0];
    // ---- the strip: prefiltered bytes; strip column 0 of L' is image column x0 - r, of R' image column x0 - r - (nd - 1) >= 0
    {
        const int cL = x0 - r, cR = x0 - r - (nd - 1);
        for (int i = tid; i < srows * pitchL; i += BM_THREADS) {
            const int rr = i / pitchL, b = i - rr * pitchL, x = cL + b;
            Lb[i] = x < w ? (uint8_t)bm_prefilter(imgL, ipitch, w, h, x, y0 - r + rr, cap) : (uint8_t)0;
        }
        for (int i = tid; i < srows * pitchR; i += BM_THREADS) {
            const int rr = i / pitchR, b = i - rr * pitchR, x = cR + b;
            Rb[i] = x < w ? (uint8_t)bm_prefilter(imgR, ipitch, w, h, x, y0 - r + rr, cap) : (uint8_t)0;
        }
        if (tid < 2 * BM_TW) uq[tid] = 0;
    }
    __syncthreads();

    const int nchunks = nd >> 4;
    const int lastbytes = P.bs - 4 * (NWW - 1);                  // 1 .. 4 bytes of the window in its last word
    const unsigned int lastmask = lastbytes == 4 ? 0xffffffffu : ((1u << (8 * lastbytes)) - 1u);
    const unsigned int capw = (unsigned int)cap * 0x01010101u;
    int S[4][16];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) S[k][i] = 0;
    int tex = 0;

    for (int oy = 0; oy < rows; ++oy) {
        // the window sums of output row oy: all 2r+1 strip rows for the first one, then + the row that enters, - the row that left
        const int nops = oy == 0 ? 2 * r + 1 : 2;
        for (int op = 0; op < nops; ++op) {
            const int rr = oy == 0 ? op : (op == 0 ? oy + 2 * r : oy - 1);
            const int neg = (oy != 0 && op == 1) ? -1 : 0;       // (v ^ neg) - neg = -v
            const unsigned int *Lrow = reinterpret_cast<const unsigned int *>(Lb + (size_t)rr * pitchL) + (xi >> 2);
            unsigned int Lw[NWW];
            {
                unsigned int raw[NWW + 1];
#pragma unroll
                for (int k = 0; k <= NWW; ++k) raw[k] = Lrow[k];
#pragma unroll
                for (int k = 0; k < NWW; ++k) Lw[k] = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], (unsigned int)(xi & 3));
                Lw[NWW - 1] &= lastmask;
            }
            if (wv == 0) {
                unsigned int t = 0;
#pragma unroll
                for (int k = 0; k < NWW; ++k) t = __builtin_amdgcn_sad_u8(Lw[k], k == NWW - 1 ? (capw & lastmask) : capw, t);
                tex += ((int)t ^ neg) - neg;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = wv + 4 * k;
                if (c < nchunks) {
                    // byte of R' under the window's first byte at the chunk's LARGEST disparity 16c + 15; disparity 16c + 15 - e is e bytes on
                    const int base = xi + (nd - 1) - (16 * c + 15);
                    const unsigned int *Rrow = reinterpret_cast<const unsigned int *>(Rb + (size_t)rr * pitchR) + (base >> 2);
                    unsigned int Wp[NWW + 4];
                    {
                        unsigned int raw[NWW + 5];
#pragma unroll
                        for (int q = 0; q < NWW + 5; ++q) raw[q] = Rrow[q];
#pragma unroll
                        for (int q = 0; q < NWW + 4; ++q) Wp[q] = __builtin_amdgcn_alignbyte(raw[q + 1], raw[q], (unsigned int)(base & 3));
                    }
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int sh = e & 3, q = e >> 2;
                        unsigned int acc = 0;
#pragma unroll
                        for (int j = 0; j < NWW; ++j) {
                            unsigned int rw = sh ? __builtin_amdgcn_alignbyte(Wp[q + j + 1], Wp[q + j], (unsigned int)sh) : Wp[q + j];
                            if (j == NWW - 1) rw &= lastmask;
                            acc = __builtin_amdgcn_sad_u8(Lw[j], rw, acc);
                        }
                        S[k][15 - e] += ((int)acc ^ neg) - neg;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = wv + 4 * k;
            if (c < nchunks) {
#pragma unroll
                for (int i = 0; i < 16; i += 2) sadw[(size_t)(8 * c + (i >> 1)) * BM_TW + xi] = (unsigned int)S[k][i] | ((unsigned int)S[k][i + 1] << 16);
            }
        }
        __syncthreads();
        // ---- min / arg-min over this thread's quarter of the disparities, ascending with <=: ties go to the largest d
        const int dq = nd >> 2, dlo = wv * dq;
        {
            int best = 0x7fffffff, bd = dlo;
            for (int d = dlo; d < dlo + dq; d += 2) {
                const unsigned int u = sadw[(size_t)(d >> 1) * BM_TW + xi];
                const int lo = (int)(u & 0xffffu), hi = (int)(u >> 16);
                if (lo <= best) { best = lo; bd = d; }
                if (hi <= best) { best = hi; bd = d + 1; }
            }
            part[wv * BM_TW + xi] = best; part[(4 + wv) * BM_TW + xi] = bd;
        }
        __syncthreads();
        int minsad = part[xi], mind = part[4 * BM_TW + xi];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const int v = part[q * BM_TW + xi];
            if (v <= minsad) { minsad = v; mind = part[(4 + q) * BM_TW + xi]; }
        }
        {
            // uniquenessRatio 0 switches the test off (stereobm.cpp: if( uniquenessRatio > 0 )): no SAD is <= -1.  The scan itself stays
            // as it is for every ratio
            const int thr = P.uniq > 0 ? minsad + minsad * P.uniq / 100 : -1;
            bool fail = false;
            for (int d = dlo; d < dlo + dq; d += 2) {
                const unsigned int u = sadw[(size_t)(d >> 1) * BM_TW + xi];
                const int lo = (int)(u & 0xffffu), hi = (int)(u >> 16);
                fail |= (lo <= thr) && (d < mind - 1 || d > mind + 1);
                fail |= (hi <= thr) && (d + 1 < mind - 1 || d + 1 > mind + 1);
            }
            if (fail) uq[(oy & 1) * BM_TW + xi] = 1;
        }
        int pv = 0, nv = 0;
        if (wv == 0) {
            const int dp = mind > 0 ? mind - 1 : 1, dn = mind < nd - 1 ? mind + 1 : nd - 2;      // SAD(-1) := SAD(1), SAD(nd) := SAD(nd - 2)
            pv = (int)((sadw[(size_t)(dp >> 1) * BM_TW + xi] >> (16 * (dp & 1))) & 0xffffu);
            nv = (int)((sadw[(size_t)(dn >> 1) * BM_TW + xi] >> (16 * (dn & 1))) & 0xffffu);
            uq[((oy & 1) ^ 1) * BM_TW + xi] = 0;                 // the next row's flag (read last by this same thread, one row ago)
        }
        __syncthreads();
        if (wv == 0) {
            const int x = x0 + xi, y = y0 + oy;
            if (x < w - r) {
                int val = BM_FILTERED;
                if (!(tex < P.tex_thr) && !uq[(oy & 1) * BM_TW + xi]) {
                    const int den = pv + nv - 2 * minsad + abs(pv - nv);
                    val = (mind * 256 + (den ? (pv - nv) * 256 / den : 0) + 15) >> 4;
                }
                out[((size_t)blockIdx.z * h + y) * w + x] = (int16_t)val;
            }
        }
    }
}

#ifndef BM_HOST_EMU
// ---- the cloud (src/dense_reconstruction.cpp:116-173 with its types) --------------------------------------------------
struct DenseJob { int slot_left, slot_right, pt_ofs, n_points; double T_cw[7]; };
struct DenseCam { double fx, fy, cx, cy, ext[7], min_depth; float fxb; };       // fxb = (float)fx * (float)baseline
#define DC_THREADS 1024

__device__ __forceinline__ bool dc_depth(int16_t d16, const DenseCam &cam, float &depth)
{
    const float disp = (float)d16 * (1.0f / 16.0f);
    depth = disp > 0.f ? cam.fxb / disp : 0.f;
    return !((double)depth < cam.min_depth);
}

// One workgroup per job.  The reference walks x outer, y inner; thread t owns the t-th contiguous piece of that walk, counts
// its survivors, the workgroup's exclusive prefix sum of the counts says where each piece starts in the output: the list is
// current->points element for element, whatever the scheduling.  A job with more survivors than max_pts writes its count only.
SVS_CONTRACT_FAST
__global__ __launch_bounds__(DC_THREADS) void k_dense_cloud(DenseJob *jobs, const int16_t *disp, int w, int h, DenseCam cam, int max_pts,
                                                             float *xyz, int *pix)
{
    __shared__ int sc[DC_THREADS];
    const int tid = threadIdx.x, N = w * h, per = (N + DC_THREADS - 1) / DC_THREADS;
    const int k0 = min(N, tid * per), k1 = min(N, k0 + per);
    const int16_t *dj = disp + (size_t)blockIdx.x * N;
    int cnt = 0;
    for (int k = k0; k < k1; ++k) {
        const int x = k / h, y = k - x * h;
        float depth;
        cnt += dc_depth(dj[y * w + x], cam, depth) ? 1 : 0;
    }
    sc[tid] = cnt;
    __syncthreads();
    for (int s = 1; s < DC_THREADS; s <<= 1) {
        const int v = tid >= s ? sc[tid - s] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    const int total = sc[DC_THREADS - 1];
    int o = sc[tid] - cnt;
    if (tid == 0) jobs[blockIdx.x].n_points = total;
    if (total > max_pts) return;
    const double *T = jobs[blockIdx.x].T_cw;
    const double qc[4] = { -T[0], -T[1], -T[2], T[3] }, qe[4] = { -cam.ext[0], -cam.ext[1], -cam.ext[2], cam.ext[3] };
    float *xo = xyz + (size_t)blockIdx.x * max_pts * 3;
    int *po = pix + (size_t)blockIdx.x * max_pts;
    for (int k = k0; k < k1; ++k) {
        const int x = k / h, y = k - x * h;
        float depth;
        if (!dc_depth(dj[y * w + x], cam, depth)) continue;
        const double z = (double)depth;
        // Camera::pixel2camera, then Camera::camera2world: T_c_w^-1 * pose_inv_ * p_c (src/camera.cpp:39-44, 58-72)
        const double pc[3] = { ((double)x - cam.cx) * z / cam.fx - cam.ext[4], ((double)y - cam.cy) * z / cam.fy - cam.ext[5], z - cam.ext[6] };
        double pr[3], pw[3];
        d_quat_rot(qe, pc, pr);
        pr[0] -= T[4]; pr[1] -= T[5]; pr[2] -= T[6];
        d_quat_rot(qc, pr, pw);
        xo[3 * (size_t)o] = (float)pw[0]; xo[3 * (size_t)o + 1] = (float)pw[1]; xo[3 * (size_t)o + 2] = (float)pw[2];
        po[o] = y * w + x;
        ++o;
    }
}
#pragma clang fp contract(off)
#endif
