// k_cloud_filter.h — the two PCL filters of run_dense_reconstruction (src/dense_reconstruction.cpp:175-209):
//   pcl::StatisticalOutlierRemoval  the exact k-nearest-neighbour mean distance of every point (k_cf_keys, k_cf_gather, k_cf_knn);
//                                    the statistics, the threshold and the mask are the host's (svslam_cloud_sor_batch)
//   pcl::VoxelGrid                   voxel index per point, run heads of the sorted (index, point) keys, one thread per voxel
//                                    summing its run in point order (k_vg_keys, k_vg_heads, k_vg_starts, k_vg_reduce)
// The numeric contract is tests/ref_cloud_filters.py.  The two sorts between the kernels are rocPRIM's, called from
// api_dense.h: this file has no library in it and no cross-lane operation, so tests/cpp/cf_host_emu runs it on the host.
//
// kNN.  Points get a 30-bit Morton key (10 bits per axis) over their segment's bounding box, in cubic cells of side h = largest
// extent / 1024; the key's upper bits hold the segment, so one sort orders a whole batch.  A query (one per lane, in sorted
// order, so that the lanes of a wave look at the same cells) keeps its k + 1 smallest squared distances in a statically indexed
// register array and scans the 3 x 3 x 3 block of cells of side h 2^s around its own cell, every cell being one contiguous range
// of the sorted keys (two binary searches).  A point outside the block differs from the query by at least `gap` along one axis,
// gap being the distance from the query to the nearest face of the block that has cells behind it; the block is accepted when the
// (k+1)-th distance is <= gap^2, otherwise s grows by one and the larger block is scanned from scratch.  At s = 9 the block is
// the whole segment.  The first s is a guess (the cell that still holds the query's k/2 + 1 Morton neighbours on either side,
// halved once): it decides the work, never the result.
//
// Why gap is safe in f32.  With u = fl(p - min) and t = fl(u * inv_h), cell q = min(1023, (int)t) is monotone in p.  A point with
// q' >= Q has t' >= Q, so u' >= Q h (1 - 2^-23) and p' - p >= Q h - u - 3 * 2^-23 * 1024 h; what f32 evaluation of Q h - u adds
// is of the same size (every term is <= 1024 h).  0.01 h is taken off (25 x those together) and the square is scaled by
// 1 - 1e-5 for its own roundings; a computed squared distance is never below the computed square of one of its axes.
//
// The host's part (cf_segments, cf_sor_decide, vg_plan) is plain C++ here too: api_dense.h and the host emulation call the same
// functions.  A refusal is the message, written into the caller's `msg` (CF_MSG bytes); nullptr otherwise.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>

#define CF_THREADS 256
#define CF_KMAX 64                 /* mean_k of svslam_cloud_sor_batch: 1 .. 64 */
#define CF_MORTON_MASK 0x3FFFFFFFull
#define CF_MSG 128

struct CfSeg { int ofs, n; float mn[3]; float inv_h, h; int pad; };       // a segment of the batch: points [ofs, ofs + n), its box and cell
struct VgParams { float inv; int min_b[3]; int mul[3]; };

// One host pass over the batch (points seg_ofs[0] .. seg_ofs[nseg] of xyz): every coordinate finite (PCL's branch for the others is not
// restated), the box and the cell of every segment; *any: some segment has the mean_k + 1 points a search needs
inline const char *cf_segments(int nseg, const int64_t *seg_ofs, const float *xyz, int mean_k, CfSeg *out, bool *any, char *msg)
{
    *any = false;
    for (int s = 0; s < nseg; ++s) {
        CfSeg &g = out[s];
        g.ofs = (int)(seg_ofs[s] - seg_ofs[0]); g.n = (int)(seg_ofs[s + 1] - seg_ofs[s]); g.pad = 0;
        float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
        const float *p = xyz + 3 * (size_t)seg_ofs[s];
        for (int i = 0; i < g.n; ++i, p += 3) {
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) {
                snprintf(msg, CF_MSG, "cloud_filter: point %d of segment %d has a non-finite coordinate", i, s);
                return msg;
            }
            for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], p[a]); mx[a] = std::max(mx[a], p[a]); }
        }
        float ext = 0.f;
        for (int a = 0; a < 3; ++a) { g.mn[a] = g.n ? mn[a] : 0.f; if (g.n) ext = std::max(ext, mx[a] - mn[a]); }
        g.inv_h = ext > 0.f ? 1024.0f / ext : 0.f;
        if (!std::isfinite(g.inv_h)) g.inv_h = 0.f;
        g.h = g.inv_h > 0.f ? 1.0f / g.inv_h : 0.f;
        *any = *any || g.n >= mean_k + 1;
    }
    return nullptr;
}

// PCL's statistics over the n mean distances of a segment, sequentially in index order: the threshold has the yardstick's bits by
// construction.  Returns the threshold, keep[i] = the point stays
inline double cf_sor_decide(int n, const float *d, int mean_k, double stddev_mul, uint8_t *keep)
{
    if (n < mean_k + 1) {                                  // no valid distance: 0 / 0, nothing is above a NaN
        for (int i = 0; i < n; ++i) keep[i] = 1;
        return std::nan("");
    }
    double sum = 0.0, sq_sum = 0.0;
    for (int i = 0; i < n; ++i) { sum += (double)d[i]; const float sq = d[i] * d[i]; sq_sum += (double)sq; }
    const double nv = (double)n, mean = sum / nv, var = (sq_sum - sum * sum / nv) / (nv - 1.0);
    const double thr = mean + stddev_mul * std::sqrt(var);
    for (int i = 0; i < n; ++i) keep[i] = !((double)d[i] > thr) ? 1 : 0;
    return thr;
}

// pcl::VoxelGrid's set-up for n points and a leaf > 0: the float reciprocal, the box, PCL's guard (*over: more than INT32_MAX cells ->
// "Leaf size is too small for the input dataset", the output is the input; P.min_b and P.mul are not set then), the index origin
// and the multipliers
inline const char *vg_plan(size_t n, const float *xyz, double leaf, VgParams &P, bool *over, char *msg)
{
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * i + a];
            if (!std::isfinite(v)) { snprintf(msg, CF_MSG, "cloud_filter: point %zu has a non-finite coordinate", i); return msg; }
            mn[a] = std::min(mn[a], v); mx[a] = std::max(mx[a], v);
        }
    P.inv = 1.0f / (float)leaf;
    if (!std::isfinite(P.inv) || !(P.inv > 0.f)) { snprintf(msg, CF_MSG, "cloud_filter: leaf %g has no float reciprocal", leaf); return msg; }
    int64_t cells[3];
    *over = false;
    for (int a = 0; a < 3; ++a) {
        const float e = (mx[a] - mn[a]) * P.inv;
        if (!(e < 9.0e18f)) *over = true; else cells[a] = (int64_t)e + 1;
    }
    if (!*over) *over = (__int128)cells[0] * cells[1] * cells[2] > (__int128)INT32_MAX;
    if (*over) return nullptr;
    int div_b[3];
    for (int a = 0; a < 3; ++a) {
        P.min_b[a] = (int)std::floor(mn[a] * P.inv);
        div_b[a] = (int)std::floor(mx[a] * P.inv) - P.min_b[a] + 1;
    }
    P.mul[0] = 1; P.mul[1] = div_b[0]; P.mul[2] = (int)((unsigned)div_b[0] * (unsigned)div_b[1]);
    return nullptr;
}

__device__ __forceinline__ int cf_cell(float p, float mn, float inv_h)
{
    const float t = (p - mn) * inv_h;                      // >= 0: mn is the minimum itself
    return min(1023, (int)t);
}
__device__ __forceinline__ unsigned cf_spread(unsigned v)
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ unsigned cf_morton(int x, int y, int z) { return cf_spread((unsigned)x) | (cf_spread((unsigned)y) << 1) | (cf_spread((unsigned)z) << 2); }

// the segment of point i: the last one that starts at or before it (empty segments share their successor's start)
__device__ __forceinline__ int cf_seg_of(const CfSeg *segs, int nseg, int i)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].ofs <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void cf_keys_one(int i, const float *xyz, const CfSeg *segs, int nseg, unsigned long long *keys, unsigned *vals)
{
    const int s = cf_seg_of(segs, nseg, i);
    const CfSeg g = segs[s];
    const unsigned m = cf_morton(cf_cell(xyz[3 * (size_t)i], g.mn[0], g.inv_h), cf_cell(xyz[3 * (size_t)i + 1], g.mn[1], g.inv_h),
                                 cf_cell(xyz[3 * (size_t)i + 2], g.mn[2], g.inv_h));
    keys[i] = ((unsigned long long)s << 30) | m;
    vals[i] = (unsigned)i;
}
__global__ __launch_bounds__(CF_THREADS) void k_cf_keys(const float *xyz, int total, const CfSeg *segs, int nseg, unsigned long long *keys, unsigned *vals)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < total) cf_keys_one(i, xyz, segs, nseg, keys, vals);
}

// the coordinates in sorted order, one array per axis
__device__ __forceinline__ void cf_gather_one(int j, const float *xyz, const unsigned *perm, float *sx, float *sy, float *sz)
{
    const size_t i = perm[j];
    sx[j] = xyz[3 * i]; sy[j] = xyz[3 * i + 1]; sz[j] = xyz[3 * i + 2];
}
__global__ __launch_bounds__(CF_THREADS) void k_cf_gather(const float *xyz, const unsigned *perm, int total, float *sx, float *sy, float *sz)
{
    const int j = blockIdx.x * CF_THREADS + threadIdx.x;
    if (j < total) cf_gather_one(j, xyz, perm, sx, sy, sz);
}

// first position in [lo, hi) whose key is >= k
__device__ __forceinline__ int cf_lower_bound(const unsigned long long *keys, int lo, int hi, unsigned long long k)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The query at sorted position j.  CAP = slots of the register array; the k + 1 tracked distances live in its LAST k + 1 slots,
// ascending, the slots in front of them hold -inf and let every candidate pass: the largest tracked one is a[CAP - 1] for any k.
template <int CAP>
__device__ __forceinline__ void cf_knn_one(int j, const unsigned long long *keys, const unsigned *perm, const float *sx, const float *sy, const float *sz,
                                           const CfSeg *segs, int k, float *mean_dist, unsigned *climbs)
{
    const unsigned long long kj = keys[j];
    const int sg = (int)(kj >> 30);
    const CfSeg g = segs[sg];
    if (g.n < k + 1) { mean_dist[perm[j]] = 0.f; return; }      // the search would return fewer than k + 1: PCL's distance 0
    const int base = g.ofs, end = g.ofs + g.n;
    const float px = sx[j], py = sy[j], pz = sz[j];
    const float u[3] = { px - g.mn[0], py - g.mn[1], pz - g.mn[2] };
    const int q[3] = { cf_cell(px, g.mn[0], g.inv_h), cf_cell(py, g.mn[1], g.inv_h), cf_cell(pz, g.mn[2], g.inv_h) };
    const float INF = __builtin_huge_valf();
    // first block: the finest cell that still holds the k/2 + 1 sorted neighbours on either side, halved once
    const int half = k / 2 + 1;
    const unsigned mk = (unsigned)(kj & CF_MORTON_MASK);
    const unsigned diff = (mk ^ (unsigned)(keys[max(base, j - half)] & CF_MORTON_MASK)) | (mk ^ (unsigned)(keys[min(end - 1, j + half)] & CF_MORTON_MASK));
    // (a segment without extent, inv_h = 0, is one cell: its only block is the whole segment)
    const int s0 = g.inv_h == 0.f ? 9 : diff ? min(9, (31 - __builtin_clz(diff)) / 3) : 0;
    float a[CAP];
    int s = s0;
    for (; s <= 9; ++s) {
#pragma unroll
        for (int t = 0; t < CAP; ++t) a[t] = t >= CAP - 1 - k ? INF : -INF;
        const int ncell = 1 << (10 - s);
        const int c[3] = { q[0] >> s, q[1] >> s, q[2] >> s };
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int X = c[0] + dx, Y = c[1] + dy, Z = c[2] + dz;
                    if (X < 0 || Y < 0 || Z < 0 || X >= ncell || Y >= ncell || Z >= ncell) continue;
                    const unsigned long long klo = ((unsigned long long)sg << 30) | ((unsigned long long)cf_morton(X, Y, Z) << (3 * s));
                    const int lo = cf_lower_bound(keys, base, end, klo);
                    const int hi = cf_lower_bound(keys, lo, end, klo + (1ull << (3 * s)));
                    for (int i = lo; i < hi; ++i) {
                        const float ex = px - sx[i], ey = py - sy[i], ez = pz - sz[i];
                        float d = ((ex * ex) + (ey * ey)) + (ez * ez);          // FLANN's L2_Simple
                        if (d < a[CAP - 1]) {
#pragma unroll
                            for (int t = 0; t < CAP; ++t) { const float lo_ = fminf(a[t], d); d = fmaxf(a[t], d); a[t] = lo_; }
                        }
                    }
                }
        if (s == 9) break;                                 // cells -1 .. 1 around a cell of a 2-cell axis: the whole segment
        float gap = INF;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const int qlo = (c[ax] - 1) * (1 << s), qhi = (c[ax] + 2) * (1 << s);          // cells < qlo and >= qhi are outside
            if (qlo > 0) gap = fminf(gap, u[ax] - (float)qlo * g.h);
            if (qhi <= 1023) gap = fminf(gap, (float)qhi * g.h - u[ax]);
        }
        const float gs = gap - 0.01f * g.h;
        if (gs > 0.f && a[CAP - 1] <= gs * gs * 0.99999f) break;
    }
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < CAP; ++t) if (t > CAP - 1 - k) sum += (double)sqrtf(a[t]);     // ascending; the smallest (the point itself) is skipped
    mean_dist[perm[j]] = (float)(sum / (double)k);
    if (climbs && s > s0) atomicAdd(climbs, 1u);           // measurement only: queries that went above their first block
}
template <int CAP>
__global__ __launch_bounds__(CF_THREADS) void k_cf_knn(const unsigned long long *keys, const unsigned *perm, const float *sx, const float *sy, const float *sz,
                                                        int total, const CfSeg *segs, int k, float *mean_dist, unsigned *climbs)
{
    const int j = blockIdx.x * CF_THREADS + threadIdx.x;
    if (j < total) cf_knn_one<CAP>(j, keys, perm, sx, sy, sz, segs, k, mean_dist, climbs);
}

// ---- pcl::VoxelGrid -----------------------------------------------------------------------------------------------------
// key = voxel index (int32, biased to sort as signed) : point index — sorted, a voxel is a run and its points are in input order
__device__ __forceinline__ void vg_keys_one(int i, const float *xyz, const VgParams &P, unsigned long long *keys)
{
    unsigned idx = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int ijk = (int)(floorf(xyz[3 * (size_t)i + ax] * P.inv) - (float)P.min_b[ax]);
        idx += (unsigned)ijk * (unsigned)P.mul[ax];
    }
    keys[i] = ((unsigned long long)(idx ^ 0x80000000u) << 32) | (unsigned)i;
}
__global__ __launch_bounds__(CF_THREADS) void k_vg_keys(const float *xyz, int n, VgParams P, unsigned long long *keys)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i < n) vg_keys_one(i, xyz, P, keys);
}
__global__ __launch_bounds__(CF_THREADS) void k_vg_heads(const unsigned long long *keys, int n, unsigned *flag)
{
    const int j = blockIdx.x * CF_THREADS + threadIdx.x;
    if (j < n) flag[j] = j == 0 || (keys[j] >> 32) != (keys[j - 1] >> 32) ? 1u : 0u;
}
// pos = inclusive sum of flag: the head of voxel v is where flag is set and pos = v + 1
__global__ __launch_bounds__(CF_THREADS) void k_vg_starts(const unsigned *flag, const unsigned *pos, int n, int *start)
{
    const int j = blockIdx.x * CF_THREADS + threadIdx.x;
    if (j < n && flag[j]) start[pos[j] - 1] = j;
}
// one thread per voxel: f32 sums in run order (= ascending point index), centroid = sum / (float)count, colour mean truncated
__device__ __forceinline__ void vg_reduce_one(int v, const unsigned long long *keys, const int *start, int m, int n, const float *xyz, const uint8_t *rgb,
                                              float *out_xyz, uint8_t *out_rgb)
{
    const int j0 = start[v], j1 = v + 1 < m ? start[v + 1] : n;
    float s[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    for (int j = j0; j < j1; ++j) {
        const size_t i = (unsigned)(keys[j] & 0xFFFFFFFFull);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { s[ax] = s[ax] + xyz[3 * i + ax]; s[3 + ax] = s[3 + ax] + (float)rgb[3 * i + ax]; }
    }
    const float cnt = (float)(j1 - j0);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        out_xyz[3 * (size_t)v + ax] = s[ax] / cnt;
        out_rgb[3 * (size_t)v + ax] = (uint8_t)(unsigned)(s[3 + ax] / cnt);
    }
}
__global__ __launch_bounds__(CF_THREADS) void k_vg_reduce(const unsigned long long *keys, const int *start, int m, int n, const float *xyz, const uint8_t *rgb,
                                                          float *out_xyz, uint8_t *out_rgb)
{
    const int v = blockIdx.x * CF_THREADS + threadIdx.x;
    if (v < m) vg_reduce_one(v, keys, start, m, n, xyz, rgb, out_xyz, out_rgb);
}
