// k_colour.h — colour input of the dense program (run_dense_reconstruction, src/dense_reconstruction.cpp:104-171).
//   k_bgr_prepare    packed 8-bit BGR images -> the grey image the matcher's pyramid is built from (cv::cvtColor COLOR_BGR2GRAY) and,
//                    where a plane is named, the working-resolution BGR image; optionally with the 1/2 INTER_NEAREST decimation of
//                    Dataset::FrameById (src/dataset.cpp:162-165): dst(x, y) = src(2x, 2y), only the even source rows are read
//   k_colour_gather  b, g, r of every point k_dense_cloud kept, from the plane of its job at out_pix
// Integer arithmetic only; the grey formula is SVSLAM_GREY_FROM_RGB of include/svslam.h, the one facade::read_png uses.
//
// Shape of k_bgr_prepare.  Bandwidth-bound, no LDS, no cross-lane operation (tests/cpp/colour_host_emu runs the per-thread function
// on the host).  A thread owns 16 output pixels of one row: 48 (96 when decimating) consecutive source bytes by 16-byte loads, all
// issued before the first use, 16 grey bytes and 48 plane bytes by 16-byte stores.  Rows start at any alignment (a pitch of 3 * 1241
// bytes, a tight grey row of 620): loads and stores are the unaligned 16-byte forms gfx950 serves in hardware, as k_pyr_fused's fill.
// No byte outside a row's 3 * src_w bytes is ever read: the last piece of a row does not run past the row, it is moved back to end
// with it — pixels [w - 16, w), overlapping the piece before (both write the same values) — and, where an odd source width leaves
// the decimating window three bytes short, the window starts one pixel earlier and the bytes are taken three further on.  A row
// shorter than one window (src_w < 32 when decimating) is read byte by byte.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/svslam.h"

struct BgrJob {
    const uint8_t *src;   // packed BGR (device)
    int stride;           // bytes from one row that is read to the next: the pitch, twice the pitch of a source decimated in place
    int plane;            // colour plane the working-resolution BGR image goes to, -1: none
};

#define COL_THREADS 256
#define COL_PX 16         // output pixels per thread

// the sizes a caller and the kernels agree on (host): pieces of a row, grid.x of the two kernels, BgrJob::stride, out_per
inline int col_chunks(int w) { return (w + COL_PX - 1) / COL_PX; }
inline unsigned col_prepare_blocks(int w, int h) { return (unsigned)((h * col_chunks(w) + COL_THREADS - 1) / COL_THREADS); }
inline unsigned col_gather_blocks(int max_pts) { return (unsigned)(((max_pts + 3) / 4 + COL_THREADS - 1) / COL_THREADS); }
inline int col_row_stride(int pitch, bool decimate) { return decimate ? 2 * pitch : pitch; }
inline size_t col_bgr_per(int max_pts) { return ((size_t)3 * (size_t)(((max_pts + 3) / 4) * 4) + 15) & ~(size_t)15; }      // 12 bytes per 4 points

struct ColQ { uint32_t x, y, z, w; };
#if defined(__HIPCC__)
typedef uint32_t col_u4v __attribute__((ext_vector_type(4)));
typedef col_u4v col_u4v_ua __attribute__((aligned(1)));
typedef const __attribute__((address_space(1))) col_u4v_ua *col_gcptr128;
typedef __attribute__((address_space(1))) col_u4v_ua *col_gptr128;
// the images live in device (global) memory: say so, or the accesses become flat
__device__ __forceinline__ ColQ col_load16(const uint8_t *p)
{
    const col_u4v v = *(col_gcptr128)(reinterpret_cast<uintptr_t>(p));
    ColQ q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
    return q;
}
__device__ __forceinline__ void col_store16(uint8_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    col_u4v v; v.x = a; v.y = b; v.z = c; v.w = d;
    *(col_gptr128)(reinterpret_cast<uintptr_t>(p)) = v;
}
#else
__device__ __forceinline__ ColQ col_load16(const uint8_t *p) { ColQ q; memcpy(&q, p, 16); return q; }
__device__ __forceinline__ void col_store16(uint8_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t v[4] = { a, b, c, d };
    memcpy(p, v, 16);
}
#endif

// byte k (compile-time after unrolling) of a window held in dwords
#define COL_BYTE(q, k) (((q)[(k) >> 2] >> (8 * ((k) & 3))) & 0xffu)

// 16 pixels out of a window: pixel k is the three bytes at STEP * k + DELTA (b, g, r)
template <int STEP, int DELTA, int NDW>
__device__ __forceinline__ void col_convert(const uint32_t (&q)[NDW], uint32_t (&grey)[4], uint32_t (&bgr)[12])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) grey[i] = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) bgr[i] = 0;
#pragma unroll
    for (int k = 0; k < COL_PX; ++k) {
        const uint32_t b = COL_BYTE(q, STEP * k + DELTA), g = COL_BYTE(q, STEP * k + DELTA + 1), r = COL_BYTE(q, STEP * k + DELTA + 2);
        grey[k >> 2] |= (uint32_t)SVSLAM_GREY_FROM_RGB(r, g, b) << (8 * (k & 3));
        bgr[(3 * k) >> 2] |= b << (8 * ((3 * k) & 3));
        bgr[(3 * k + 1) >> 2] |= g << (8 * ((3 * k + 1) & 3));
        bgr[(3 * k + 2) >> 2] |= r << (8 * ((3 * k + 2) & 3));
    }
}

// task t of image `img`: row t / chunks, piece t % chunks (chunks = ceil(w / 16)).  grey: [n][grey_per] bytes, an image tight
// [h][w]; planes: [nplanes][h][w][3]
template <bool DECIMATE>
__device__ __forceinline__ void bgr_prepare_task(const BgrJob jb, int img, int t, int w, int h, int src_w, int chunks, uint8_t *grey,
                                                 size_t grey_per, uint8_t *planes)
{
    constexpr int NL = DECIMATE ? 6 : 3;          // 16-byte loads of a window
    constexpr int STEP = DECIMATE ? 6 : 3;        // source bytes from one output pixel to the next
    const int y = t / chunks, ck = t - y * chunks;
    if (y >= h) return;
    const int x0 = ck * COL_PX < w - COL_PX ? ck * COL_PX : (w - COL_PX > 0 ? w - COL_PX : 0);
    const uint8_t *row = jb.src + (size_t)y * (size_t)jb.stride;
    const int rb = 3 * src_w;                     // bytes of a source row
    uint8_t *go = grey + (size_t)img * grey_per + (size_t)y * w + x0;
    uint8_t *po = jb.plane >= 0 ? planes + (((size_t)jb.plane * h + y) * (size_t)w + x0) * 3 : nullptr;
    if (rb < 16 * NL || w < COL_PX) {
        // a row shorter than one window: byte by byte, each piece its own pixels
        const int xa = ck * COL_PX, xe = xa + COL_PX < w ? xa + COL_PX : w;
        go = grey + (size_t)img * grey_per + (size_t)y * w;
        po = jb.plane >= 0 ? planes + (((size_t)jb.plane * h + y) * (size_t)w) * 3 : nullptr;
        for (int x = xa; x < xe; ++x) {
            const uint8_t *s = row + (size_t)STEP * x;
            const uint32_t b = s[0], g = s[1], r = s[2];
            go[x] = (uint8_t)SVSLAM_GREY_FROM_RGB(r, g, b);
            if (po) { po[3 * x] = (uint8_t)b; po[3 * x + 1] = (uint8_t)g; po[3 * x + 2] = (uint8_t)r; }
        }
        return;
    }
    // the window [s, s + 16 NL) lies inside the row; want - s is 0, or 3 when the row ends three bytes before the window would
    const int want = STEP * x0, s = want < rb - 16 * NL ? want : rb - 16 * NL, delta = want - s;
    uint32_t q[4 * NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const ColQ v = col_load16(row + s + 16 * i);
        q[4 * i] = v.x; q[4 * i + 1] = v.y; q[4 * i + 2] = v.z; q[4 * i + 3] = v.w;
    }
    uint32_t gq[4], pq[12];
    if (DECIMATE && delta) col_convert<STEP, 3>(q, gq, pq);
    else col_convert<STEP, 0>(q, gq, pq);
    col_store16(go, gq[0], gq[1], gq[2], gq[3]);
    if (po) {
        col_store16(po, pq[0], pq[1], pq[2], pq[3]);
        col_store16(po + 16, pq[4], pq[5], pq[6], pq[7]);
        col_store16(po + 32, pq[8], pq[9], pq[10], pq[11]);
    }
}

// grid (ceil(h * chunks / COL_THREADS), n)
template <bool DECIMATE>
__global__ void __launch_bounds__(COL_THREADS)
k_bgr_prepare(const BgrJob *jobs, int w, int h, int src_w, int chunks, uint8_t *grey, size_t grey_per, uint8_t *planes)
{
    const int img = blockIdx.y;
    const int t = blockIdx.x * COL_THREADS + threadIdx.x;
    bgr_prepare_task<DECIMATE>(jobs[img], img, t, w, h, src_w, chunks, grey, grey_per, planes);
}

// points [4 i, 4 i + 4) of job j: three bytes each from the job's plane at pix, out as three dwords.  pix: [njobs][max_pts],
// n_points: stride `np_stride` ints (the n_points field of the DenseJob array), out: [njobs][out_per] bytes, out_per a multiple of
// 16 and >= 3 * ceil(max_pts / 4) * 4.  A job whose count exceeds max_pts has no list (k_dense_cloud wrote its count only).
__device__ __forceinline__ void colour_gather_task(int j, int i, const int *n_points, int np_stride, const int *plane_of, const int *pix,
                                                   int max_pts, const uint8_t *planes, size_t plane_bytes, uint8_t *out, size_t out_per)
{
    const int n = n_points[(size_t)j * np_stride];
    if (n > max_pts || 4 * i >= n) return;
    const uint8_t *pl = planes + (size_t)plane_of[j] * plane_bytes;
    const int *pj = pix + (size_t)j * max_pts;
    uint32_t o[3] = { 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = 4 * i + k;
        if (p < n) {
            const uint8_t *s = pl + 3 * (size_t)pj[p];
            o[(3 * k) >> 2] |= (uint32_t)s[0] << (8 * ((3 * k) & 3));
            o[(3 * k + 1) >> 2] |= (uint32_t)s[1] << (8 * ((3 * k + 1) & 3));
            o[(3 * k + 2) >> 2] |= (uint32_t)s[2] << (8 * ((3 * k + 2) & 3));
        }
    }
    uint32_t *d = reinterpret_cast<uint32_t *>(out + (size_t)j * out_per + 12 * (size_t)i);
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
}

// grid (ceil(ceil(max_pts / 4) / COL_THREADS), njobs)
__global__ void __launch_bounds__(COL_THREADS)
k_colour_gather(const int *n_points, int np_stride, const int *plane_of, const int *pix, int max_pts, const uint8_t *planes,
                size_t plane_bytes, uint8_t *out, size_t out_per)
{
    colour_gather_task(blockIdx.y, blockIdx.x * COL_THREADS + threadIdx.x, n_points, np_stride, plane_of, pix, max_pts, planes, plane_bytes,
                       out, out_per);
}
