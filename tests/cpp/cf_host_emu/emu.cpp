// csrc/k_cloud_filter.h compiled for the host (tests/test_host_emulation_cloud_filters.py): the HIP qualifiers vanish, a "thread" is a
// call of the per-thread function, the two radix sorts are std::sort.  The kernels of that file use no LDS and no cross-lane
// operation, so the emulation is a loop.  The segment set-up (box, cell size) restates the few host lines of
// svslam_cloud_sor_batch.
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>
using std::min; using std::max;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct Dim3 { unsigned x, y, z; };
static Dim3 threadIdx, blockIdx;
static inline unsigned atomicAdd(unsigned *p, unsigned v) { const unsigned o = *p; *p += v; return o; }
#include "../../../stereovision-slam_amd/csrc/k_cloud_filter.h"

extern "C" int emu_sor_mean_dist(int nseg, const long long *seg_ofs, const float *xyz, int k, float *out_md, unsigned *out_climbs)
{
    const int total = (int)seg_ofs[nseg];
    std::vector<CfSeg> segs((size_t)nseg);
    for (int s = 0; s < nseg; ++s) {
        CfSeg &g = segs[(size_t)s];
        g.ofs = (int)seg_ofs[s]; g.n = (int)(seg_ofs[s + 1] - seg_ofs[s]); g.pad = 0;
        float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int i = 0; i < g.n; ++i)
            for (int a = 0; a < 3; ++a) { const float v = xyz[3 * (size_t)(g.ofs + i) + a]; mn[a] = std::min(mn[a], v); mx[a] = std::max(mx[a], v); }
        float ext = 0.f;
        for (int a = 0; a < 3; ++a) { g.mn[a] = g.n ? mn[a] : 0.f; if (g.n) ext = std::max(ext, mx[a] - mn[a]); }
        g.inv_h = ext > 0.f ? 1024.0f / ext : 0.f;
        if (!std::isfinite(g.inv_h)) g.inv_h = 0.f;
        g.h = g.inv_h > 0.f ? 1.0f / g.inv_h : 0.f;
    }
    std::vector<unsigned long long> keys((size_t)total), skeys((size_t)total);
    std::vector<unsigned> vals((size_t)total), perm((size_t)total);
    for (int i = 0; i < total; ++i) cf_keys_one(i, xyz, segs.data(), nseg, keys.data(), vals.data());
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](unsigned a, unsigned b) { return keys[a] < keys[b]; });
    for (int j = 0; j < total; ++j) skeys[(size_t)j] = keys[perm[(size_t)j]];
    std::vector<float> soa(3 * (size_t)total + 1);
    float *sx = soa.data(), *sy = sx + total, *sz = sy + total;
    for (int j = 0; j < total; ++j) cf_gather_one(j, xyz, perm.data(), sx, sy, sz);
    unsigned climbs = 0;
    for (int j = 0; j < total; ++j) {
        if (k <= 50) cf_knn_one<51>(j, skeys.data(), perm.data(), sx, sy, sz, segs.data(), k, out_md, &climbs);
        else cf_knn_one<CF_KMAX + 1>(j, skeys.data(), perm.data(), sx, sy, sz, segs.data(), k, out_md, &climbs);
    }
    if (out_climbs) *out_climbs = climbs;
    return 0;
}

extern "C" int emu_voxel_grid(int n, const float *xyz, const uint8_t *rgb, float inv, const int *min_b, const int *mul, float *out_xyz, uint8_t *out_rgb)
{
    VgParams P;
    P.inv = inv;
    for (int a = 0; a < 3; ++a) { P.min_b[a] = min_b[a]; P.mul[a] = mul[a]; }
    std::vector<unsigned long long> keys((size_t)n);
    for (int i = 0; i < n; ++i) vg_keys_one(i, xyz, P, keys.data());
    std::sort(keys.begin(), keys.end());
    std::vector<int> start;
    for (int j = 0; j < n; ++j) if (j == 0 || (keys[(size_t)j] >> 32) != (keys[(size_t)j - 1] >> 32)) start.push_back(j);
    const int m = (int)start.size();
    for (int v = 0; v < m; ++v) vg_reduce_one(v, keys.data(), start.data(), m, n, xyz, rgb, out_xyz, out_rgb);
    return m;
}
