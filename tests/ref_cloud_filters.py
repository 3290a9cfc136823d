"""CPU restatement (numpy) of the two PCL filters of the reference's second program (src/dense_reconstruction.cpp:175-209):
pcl::StatisticalOutlierRemoval (setMeanK(50), setStddevMulThresh(1.0)) and pcl::VoxelGrid (0.02 m leaf, all fields).

Parity with PCL and FLANN is UNPINNED: neither is installed where this project is developed or tested, so both filters are
restated from memory of filters/impl/statistical_outlier_removal.hpp and filters/impl/voxel_grid.hpp (like
tests/ref_stereo_bm.py for cv::StereoBM).  The HIP kernels (csrc/k_cloud_filter.h) are held to THIS file bit for bit.
The choices that a PCL binary could decide differently, each marked (unpinned) where it is made:
  * sqrt of a neighbour's squared distance: the float overload, correctly rounded;
  * the order of summation inside a voxel: ascending point index (PCL's std::sort on the voxel index alone is not stable);
  * that FLANN's exact search returns the k + 1 smallest L2_Simple distances (its kd-tree is exact with checks = -1 / eps = 0).
Non-finite points (PCL: mean distance 0, not counted, removed) are not restated: the cloud kernel never produces one and the
ABI rejects them.

Second opinions in this file: sor_mean_dist_kdtree (scipy's cKDTree, f64) and voxel_grid_loops (one Python loop per voxel)."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
f32 = np.float32


def sq_dists(q, pts):
    """FLANN's L2_Simple in f32: ((dx*dx) + (dy*dy)) + (dz*dz), dx = a.x - b.x, no contraction.  q [m, 3], pts [n, 3] -> [m, n]"""
    q = np.asarray(q, f32); pts = np.asarray(pts, f32)
    dx = q[:, None, 0] - pts[None, :, 0]
    dy = q[:, None, 1] - pts[None, :, 1]
    dz = q[:, None, 2] - pts[None, :, 2]
    assert dx.dtype == f32
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def sor_mean_dist(xyz, mean_k=50, rows=512):
    """mean distance of every point to its mean_k nearest neighbours (brute force in row chunks); zeros if n < mean_k + 1"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    out = np.zeros(n, f32)
    if n < mean_k + 1:
        return out                                         # the search returns fewer than k + 1 results: distance 0, not valid
    for r0 in range(0, n, rows):
        d2 = sq_dists(xyz[r0:r0 + rows], xyz)
        # the mean_k + 1 smallest, the point itself among them; the smallest (result 0 of the search) is skipped
        near = np.sort(np.partition(d2, mean_k, axis=1)[:, :mean_k + 1], axis=1)[:, 1:]
        d = np.sqrt(near)                                  # (unpinned) float sqrt, correctly rounded
        assert d.dtype == f32
        s = np.cumsum(d.astype(np.float64), axis=1)[:, -1]         # sequential, ascending
        out[r0:r0 + rows] = (s / mean_k).astype(f32)
    return out


def sor_threshold(mean_dist, n_valid, stddev_mul=1.0):
    """PCL's statistics: f64 accumulators filled in index order, the square taken in float"""
    d = np.asarray(mean_dist, f32)
    if n_valid == 0:
        with np.errstate(all="ignore"):
            return float(np.float64(0.0) / np.float64(0.0))        # 0 / 0: NaN, every comparison with it is false
    s = np.cumsum(d.astype(np.float64))[-1]
    sq = np.cumsum((d * d).astype(np.float64))[-1]         # f32 x f32 rounded to f32, then widened
    nv = np.float64(n_valid)
    mean = s / nv
    with np.errstate(all="ignore"):
        var = (sq - s * s / nv) / (nv - np.float64(1.0))
        return float(mean + np.float64(stddev_mul) * np.sqrt(var))


def sor(xyz, mean_k=50, stddev_mul=1.0):
    """-> (keep bool [n], mean_dist f32 [n], threshold f64).  Input order is kept: xyz[keep] is the filtered cloud."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    md = sor_mean_dist(xyz, mean_k)
    thr = sor_threshold(md, n if n >= mean_k + 1 else 0, stddev_mul)
    if n == 0:
        return np.zeros(0, bool), md, thr
    with np.errstate(invalid="ignore"):
        keep = ~(md.astype(np.float64) > thr)
    return keep, md, thr


def sor_mean_dist_kdtree(xyz, mean_k=50):
    """second opinion: cKDTree in f64 (selects by differently rounded distances: agrees to a few f32 ulp, not bit for bit)"""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    if len(p) < mean_k + 1:
        return np.zeros(len(p), f32)
    d, _ = cKDTree(p).query(p, k=mean_k + 1)
    return (d[:, 1:].sum(1) / mean_k).astype(f32)


def _voxel_setup(xyz, leaf):
    inv = f32(1.0) / f32(leaf)
    min_p = xyz.min(0); max_p = xyz.max(0)
    assert min_p.dtype == f32
    cells = [int(np.trunc((max_p[a] - min_p[a]) * inv)) + 1 for a in range(3)]          # (int64)(f32 product) + 1
    over = cells[0] * cells[1] * cells[2] > INT32_MAX
    min_b = np.floor(min_p * inv).astype(np.int64)         # (int)floorf(.)
    max_b = np.floor(max_p * inv).astype(np.int64)
    div_b = max_b - min_b + 1
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    return inv, min_b, mul, over


def _voxel_index(xyz, inv, min_b, mul):
    ijk = (np.floor(xyz * inv) - min_b.astype(f32)).astype(np.int64)       # (int)(floorf(p * inv) - (float)min_b)
    return (ijk * mul).sum(1).astype(np.int32)             # int32 arithmetic (wraps like the C expression would)


def voxel_grid(xyz, rgb, leaf=0.02):
    """-> (xyz f32 [m, 3], rgb u8 [m, 3], overflowed).  One point per occupied voxel in ascending voxel index: the f32 sums of
    the voxel's points in ascending point index (unpinned) divided by (float)n; colours summed in f32, mean truncated."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return xyz.copy(), rgb.copy(), False
    inv, min_b, mul, over = _voxel_setup(xyz, leaf)
    if over:
        return xyz.copy(), rgb.copy(), True                # "Leaf size is too small for the input dataset": output = input
    idx = _voxel_index(xyz, inv, min_b, mul)
    order = np.argsort(idx, kind="stable")                 # ascending idx, ascending point index inside a voxel
    si = idx[order]
    heads = np.flatnonzero(np.concatenate([[True], si[1:] != si[:-1]]))
    cnt = np.diff(np.concatenate([heads, [n]]))
    m = len(heads)
    vals = np.concatenate([xyz[order], rgb[order].astype(f32)], 1)
    acc = np.zeros((m, 6), f32)
    # sequential f32 sums: step t adds the t-th point of every voxel that has one
    for t in range(int(cnt.max())):
        live = cnt > t
        acc[live] = acc[live] + vals[heads[live] + t]
    assert acc.dtype == f32
    mean = acc / cnt.astype(f32)[:, None]
    return mean[:, :3].copy(), mean[:, 3:].astype(np.uint32).astype(np.uint8), False


def voxel_grid_loops(xyz, rgb, leaf=0.02):
    """voxel_grid one voxel at a time, in the shape of PCL's loop over the sorted index vector"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return xyz.copy(), rgb.copy(), False
    inv, min_b, mul, over = _voxel_setup(xyz, leaf)
    if over:
        return xyz.copy(), rgb.copy(), True
    idx = _voxel_index(xyz, inv, min_b, mul)
    pairs = sorted((int(v), i) for i, v in enumerate(idx))
    oxyz, orgb = [], []
    i = 0
    while i < n:
        j = i
        s = [f32(0)] * 6
        while j < n and pairs[j][0] == pairs[i][0]:
            p = pairs[j][1]
            for a in range(3):
                s[a] = s[a] + xyz[p, a]
                s[3 + a] = s[3 + a] + f32(rgb[p, a])
            j += 1
        c = f32(j - i)
        assert all(type(v) is f32 for v in s)
        oxyz.append([s[0] / c, s[1] / c, s[2] / c])
        orgb.append([int(np.uint32(s[3] / c)), int(np.uint32(s[4] / c)), int(np.uint32(s[5] / c))])
        i = j
    return np.array(oxyz, f32).reshape(-1, 3), np.array(orgb, np.uint8).reshape(-1, 3), False
