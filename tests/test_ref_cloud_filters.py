"""The numpy restatement of the two PCL filters (tests/ref_cloud_filters.py) against hand-checkable clouds and its own second
opinions, and the new ABI in the built library.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np

import ref_cloud_filters as rcf
from cloud_filter_cases import depth_cloud_cpu, voxel_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _line(n):
    return np.stack([np.arange(n, dtype=f32), np.zeros(n, f32), np.zeros(n, f32)], 1)


# ---- StatisticalOutlierRemoval
def test_sor_line_with_one_outlier():
    xyz = np.concatenate([_line(60), np.array([[29.0, 100.0, 0.0]], f32)])
    keep, md, thr = rcf.sor(xyz)
    assert keep[:60].all() and not keep[60]
    # an interior point has 25 neighbours on either side: (2 (1 + ... + 25)) / 50 = 13, exact in every format involved
    assert md[30] == f32(13.0) and md[25] == f32(13.0) and md[34] == f32(13.0)
    # the end point's neighbours are 1 .. 50 away: 25.5
    assert md[0] == f32(25.5) and md[59] == f32(25.5)
    assert md[60] > 100.0 and md[:60].max() < thr < md[60]


def test_sor_small_clouds_are_kept_whole():
    rng = np.random.default_rng(3)
    for n in (1, 2, 50):
        keep, md, thr = rcf.sor(rng.normal(size=(n, 3)).astype(f32))
        assert keep.all() and len(keep) == n and not md.any() and math.isnan(thr)
    keep, md, thr = rcf.sor(np.zeros((0, 3), f32))
    assert len(keep) == 0 and len(md) == 0 and math.isnan(thr)


def test_sor_51_points_is_the_first_filtering_size():
    xyz = _line(51)
    xyz[50, 1] = 500.0
    keep, md, thr = rcf.sor(xyz)
    assert not math.isnan(thr) and keep[:50].all() and not keep[50]
    # every point's 50 neighbours are all the others
    assert md[0] == f32((np.arange(1, 50).sum() + math.sqrt(50.0 ** 2 + 500.0 ** 2)) / 50)
    keep50, _, thr50 = rcf.sor(xyz[:50])
    assert math.isnan(thr50) and keep50.all()


def test_sor_coincident_points():
    keep, md, thr = rcf.sor(np.tile(np.array([[1.5, -2.0, 3.0]], f32), (51, 1)))
    assert not md.any() and thr == 0.0 and keep.all()


def test_sor_other_k_and_multiplier():
    xyz = np.concatenate([_line(60), np.array([[29.0, 100.0, 0.0]], f32)])
    _, md, _ = rcf.sor(xyz, mean_k=2)
    assert md[30] == f32(1.0) and md[0] == f32(1.5)
    keep, _, _ = rcf.sor(xyz, stddev_mul=100.0)
    assert keep.all()


def test_sor_statistics_are_sequential_with_a_float_square():
    d = (np.random.default_rng(9).random(20001) * 3).astype(f32)
    s = sq = 0.0
    for v in d:
        s += float(v); sq += float(f32(v * v))
    want = s / len(d) + 1.0 * math.sqrt((sq - s * s / len(d)) / (len(d) - 1.0))
    assert rcf.sor_threshold(d, len(d), 1.0) == want


def test_sor_brute_force_against_ckdtree(svs):
    xyz, _ = depth_cloud_cpu(svs, 300, 64)
    assert 5000 < len(xyz) < 9000
    md = rcf.sor_mean_dist(xyz)
    kd = rcf.sor_mean_dist_kdtree(xyz)
    ulp = np.spacing(np.maximum(md, kd))
    assert (np.abs(md.astype(np.float64) - kd.astype(np.float64)) <= 4 * ulp).all()
    keep, _, _ = rcf.sor(xyz)
    assert 0.02 < 1.0 - keep.mean() < 0.40


def test_the_gpu_test_cloud_is_bitten(svs):
    """the cloud tests/test_gpu_cloud_filters.py filters (a 200 x 60 crop): the yardstick removes between 2 % and 40 % of it"""
    xyz, _ = depth_cloud_cpu(svs, 200, 60)
    keep, _, _ = rcf.sor(xyz)
    assert len(xyz) > 1500 and 0.02 < 1.0 - keep.mean() < 0.40, (len(xyz), keep.mean())


# ---- VoxelGrid
def test_voxel_grid_equals_its_loop_twin(svs):
    cases = dict(voxel_cases())
    xyz, grey = depth_cloud_cpu(svs, 200, 60)
    rgb = np.repeat(grey[:, None], 3, 1)
    cases["depth-0.02"] = (xyz, rgb, 0.02); cases["depth-0.5"] = (xyz, rgb, 0.5)
    for name, (xyz, rgb, leaf) in cases.items():
        a, b = rcf.voxel_grid(xyz, rgb, leaf), rcf.voxel_grid_loops(xyz, rgb, leaf)
        assert a[2] is False and b[2] is False
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        assert 1 <= len(a[0]) <= len(xyz)
    many = rcf.voxel_grid(*cases["depth-0.5"])[0]
    assert len(many) * 2 < len(cases["depth-0.5"][0])            # the case means what its name says: several points per voxel
    assert len(rcf.voxel_grid(*cases["single-voxel"])[0]) == 1


def test_voxel_grid_floors_negative_coordinates():
    # -0.005 and +0.005 truncate to the same cell 0 but floor to cells -1 and 0
    xyz = np.array([[-0.005, 0.0, 0.0], [0.005, 0.0, 0.0]], f32)
    rgb = np.array([[10, 20, 30], [50, 60, 70]], np.uint8)
    oxyz, orgb, over = rcf.voxel_grid(xyz, rgb, 0.02)
    assert not over and np.array_equal(oxyz, xyz) and np.array_equal(orgb, rgb)
    # two points of the negative cell [-0.02, 0) merge
    xyz = np.array([[-0.015, 0.0, 0.0], [-0.005, 0.0, 0.0], [0.005, 0.0, 0.0]], f32)
    oxyz, _, _ = rcf.voxel_grid(xyz, np.zeros((3, 3), np.uint8), 0.02)
    assert len(oxyz) == 2 and oxyz[0, 0] == (f32(-0.015) + f32(-0.005)) / f32(2) and oxyz[1, 0] == f32(0.005)


def test_voxel_grid_face_between_two_points():
    inv = f32(1.0) / f32(0.02)
    lo = np.nextafter(f32(0.04), f32(0))
    while np.floor(lo * inv) >= 2:                          # the largest float still in cell 1
        lo = np.nextafter(lo, f32(0))
    hi = np.nextafter(lo, f32(1))
    assert np.floor(lo * inv) == 1 and np.floor(hi * inv) == 2
    xyz = np.array([[0.0, 0.0, 0.0], [lo, 0.0, 0.0], [hi, 0.0, 0.0]], f32)
    oxyz, _, _ = rcf.voxel_grid(xyz, np.zeros((3, 3), np.uint8), 0.02)
    assert len(oxyz) == 3 and np.array_equal(oxyz, xyz)
    oxyz, _, _ = rcf.voxel_grid(xyz[[0, 1, 1]], np.zeros((3, 3), np.uint8), 0.02)
    assert len(oxyz) == 2


def test_voxel_grid_overflow_guard():
    # leaf 1: cells = (int64)(extent) + 1 per axis
    rgb = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    # 46341^2 = 2147488281 > INT32_MAX >= 46340 x 46341 = 2147441940; with a third axis of 1 cell
    for ex, ey, want in ((46339.5, 46340.5, False), (46340.5, 46340.5, True)):
        xyz = np.array([[0.0, 0.0, 0.0], [ex, ey, 0.5]], f32)
        oxyz, orgb, over = rcf.voxel_grid(xyz, rgb, 1.0)
        assert over is want
        assert np.array_equal(oxyz, xyz) and np.array_equal(orgb, rgb)      # (not overflowed: two voxels of one point each, same order)
        assert rcf.voxel_grid_loops(xyz, rgb, 1.0)[2] is want
    # exactly at the limit: 2147483647 cells along x alone is not an overflow, one more is
    # (floats near 2^31 are 128 apart: 2147483520 is the float below 2^31, 2^31 the next)
    for ex, want in ((2147483520.0, False), (2147483648.0, True)):
        xyz = np.array([[0.0, 0.0, 0.0], [ex, 0.0, 0.0]], f32)
        cells = int(np.trunc(f32(ex))) + 1
        assert (cells > rcf.INT32_MAX) is want
        oxyz, _, over = rcf.voxel_grid(xyz, rgb, 1.0)
        assert over is want and np.array_equal(oxyz, xyz)
    # the reference's leaf on a map of 100 m x 100 m x 5 m is past the guard
    xyz = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 5.0]], f32)
    assert rcf.voxel_grid(xyz, rgb, 0.02)[2] is True


def test_voxel_grid_colour_mean_truncates():
    xyz = np.array([[0.001, 0.001, 0.001], [0.002, 0.002, 0.002]], f32)
    rgb = np.array([[1, 255, 0], [2, 254, 1]], np.uint8)
    oxyz, orgb, _ = rcf.voxel_grid(xyz, rgb, 0.02)
    assert len(oxyz) == 1 and orgb.tolist() == [[1, 254, 0]]


# ---- the ABI
def test_abi_has_the_cloud_filters(svs):
    svs.build()
    L = svs.load()
    for name in ("svslam_cloud_sor_batch", "svslam_cloud_voxel_grid"):
        assert hasattr(L, name) and name in svs.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "svslam.h")).read()
    assert re.search(r"\bsvslam_cloud_sor_batch\s*\(", hdr) and re.search(r"\bsvslam_cloud_voxel_grid\s*\(", hdr)
    # the timing family: appended after the last existing number, addressed by name
    assert svs.CLOUD_FAMILIES == {"cloud_filter": 12}
    used = [v for t in (svs.FAMILIES, svs.DENSE_FAMILIES, svs.DEBUG_FAMILIES, svs.KERNEL_FAMILIES) for v in t.values()]
    assert sorted(used) == list(range(12)) and "12 cloud_filter" in hdr
    out = subprocess.run(["strings", "-a", svs.lib_path()], capture_output=True, text=True).stdout
    for k in svs.FAMILY_KERNELS["cloud_filter"] + ["cloud_filter: "]:
        assert k in out, k
