// csrc/k_cloud_filter.h compiled for the host (tests/test_host_emulation_cloud_filters.py): the HIP qualifiers vanish, a "thread" is a
// call of the per-thread function, the two radix sorts are std::sort.  The kernels of that file use no LDS and no cross-lane
// operation, so the emulation is a loop.  The segment set-up, the statistics and the voxel plan are the file's own host functions,
// the ones svslam_cloud_sor_batch and svslam_cloud_voxel_grid call.
#include "../hip_on_host.h"
#include <numeric>
#include <vector>
static Dim3 threadIdx, blockIdx;
#include "../../../stereovision-slam_amd/csrc/k_cloud_filter.h"

static char g_msg[CF_MSG];
extern "C" const char *emu_cf_error() { return g_msg; }

extern "C" double emu_cf_sor_decide(int n, const float *d, int k, double stddev_mul, uint8_t *keep) { return cf_sor_decide(n, d, k, stddev_mul, keep); }

// out_md: mean distance of point seg_ofs[0] + i at [i]; with out_segs the set-up alone (segs[nseg], any).  -1 and emu_cf_error(): refused
extern "C" int emu_sor_mean_dist(int nseg, const int64_t *seg_ofs, const float *xyz_all, int k, float *out_md, unsigned *out_climbs, CfSeg *out_segs, int *out_any)
{
    const int total = (int)(seg_ofs[nseg] - seg_ofs[0]);
    std::vector<CfSeg> segs((size_t)nseg);
    bool any = false;
    if (cf_segments(nseg, seg_ofs, xyz_all, k, segs.data(), &any, g_msg)) return -1;
    if (out_segs) { std::copy(segs.begin(), segs.end(), out_segs); *out_any = any; return 0; }
    const float *xyz = xyz_all + 3 * (size_t)seg_ofs[0];
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

// the voxel grid on the library's plan (*plan), the plan alone without out_xyz; -1 and emu_cf_error(): refused, -2: PCL's guard
extern "C" int emu_voxel_grid(int n, const float *xyz, const uint8_t *rgb, double leaf, VgParams *plan, float *out_xyz, uint8_t *out_rgb)
{
    VgParams &P = *plan;
    bool over = false;
    if (vg_plan((size_t)n, xyz, leaf, P, &over, g_msg)) return -1;
    if (over) return -2;
    if (!out_xyz) return 0;
    std::vector<unsigned long long> keys((size_t)n);
    for (int i = 0; i < n; ++i) vg_keys_one(i, xyz, P, keys.data());
    std::sort(keys.begin(), keys.end());
    std::vector<int> start;
    for (int j = 0; j < n; ++j) if (j == 0 || (keys[(size_t)j] >> 32) != (keys[(size_t)j - 1] >> 32)) start.push_back(j);
    const int m = (int)start.size();
    for (int v = 0; v < m; ++v) vg_reduce_one(v, keys.data(), start.data(), m, n, xyz, rgb, out_xyz, out_rgb);
    return m;
}
