"""svslam_cloud_sor_batch / svslam_cloud_voxel_grid (csrc/k_cloud_filter.h) against the numpy restatement of the two PCL filters
(tests/ref_cloud_filters.py), bit for bit: the statistics run on the host in the reference's order, so mean distance, threshold
and mask have no tolerance.  Clouds of at most a few thousand points: the sizes around mean_k + 1 and around the workgroup,
degenerate shapes (one point repeated, a plane, a line, tied distances), a density contrast of 10^4 with isolated far points
(queries that start at, or climb to, the scan of the whole cloud) and a depth cloud from Context.dense_cloud."""
import math

import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import ref_cloud_filters as rcf
from cloud_filter_cases import BASELINE, CAM, IDENT, POSE, depth_crop, sor_cases, voxel_cases

pytestmark = pytest.mark.gpu
KW = dict(max_pts=8, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
W, H = 200, 60


@pytest.fixture(scope="module")
def ctx(svs):
    c = svs.Context(W, H, max_slots=2, max_jobs=2, **KW)
    yield c
    c.close()


@pytest.fixture(scope="module")
def depth(svs, ctx):
    """(xyz, rgb) of the crop's cloud as the device makes it: image order, x outer"""
    left, right = depth_crop(svs, W, H)
    ctx.pyramid([0, 1], [left, right])
    (xyz, pix, _), = ctx.dense_cloud([(0, 1, POSE)], CAM, IDENT, BASELINE)
    return xyz, np.repeat(left.reshape(-1)[pix][:, None], 3, 1)


@pytest.fixture(scope="module")
def cases(svs, depth):
    c = sor_cases(svs, depth=False)
    c["depth"] = depth[0]
    return c


@pytest.fixture(scope="module")
def refs(cases):
    """the yardstick at k = 50, computed once"""
    return {n: rcf.sor(x) for n, x in cases.items()}


def _same(got, want, name):
    keep, md, thr = got
    wkeep, wmd, wthr = want
    assert md.dtype == np.float32 and len(md) == len(wmd) and len(keep) == len(wkeep), name
    assert np.array_equal(md, wmd), (name, int((md != wmd).sum()), len(md))
    assert (math.isnan(thr) and math.isnan(wthr)) or thr == wthr, (name, thr, wthr)
    assert np.array_equal(keep, wkeep), name


@pytest.mark.parametrize("name", ["n0", "n1", "n50", "n51", "n52", "n63", "n64", "n65", "n1000", "coincident", "plane", "line", "duplicates",
                                  "contrast", "depth"])
def test_sor_equals_the_restatement(ctx, cases, refs, name):
    (got,) = ctx.cloud_sor([cases[name]])
    _same(got, refs[name], name)
    n = len(cases[name])
    if n < 51:
        assert math.isnan(got[2]) and got[0].all() and not got[1].any()
    else:
        assert not math.isnan(got[2])


def test_the_filter_bites_the_depth_cloud(ctx, cases, refs):
    keep = refs["depth"][0]
    removed = 1.0 - keep.mean()
    print("depth cloud: %d points, the yardstick removes %.2f %%" % (len(keep), 100 * removed))
    assert len(keep) > 1500 and 0.02 < removed < 0.40
    (got,) = ctx.cloud_sor([cases["depth"]])
    assert np.array_equal(got[0], keep)


def test_far_points_scan_the_whole_cloud(ctx, cases, refs):
    """the 20 isolated points of the contrast cloud: their 50 neighbours are a cluster 40 m away; they are what the filter removes first"""
    ctx.cloud_sor_climbs()
    (got,) = ctx.cloud_sor([cases["contrast"]])
    queries, climbed = ctx.cloud_sor_climbs()
    print("contrast cloud: %d queries, %d went above their first block" % (queries, climbed))
    assert queries == len(cases["contrast"]) and 0 < climbed < queries // 4
    far = np.r_[2000:2010, 4010:4020]
    assert (got[1][far] > 30.0).all() and not got[0][far].any() and got[0].sum() >= 3900
    _same(got, refs["contrast"], "contrast")


@pytest.mark.parametrize("mean_k", [1, 7, 64])
def test_other_mean_k(ctx, cases, mean_k):
    for name in ("n65", "duplicates", "depth"):
        (got,) = ctx.cloud_sor([cases[name]], mean_k=mean_k, stddev_mul=0.5)
        _same(got, rcf.sor(cases[name], mean_k, 0.5), (name, mean_k))
    # 64 points have no 64 neighbours each
    (got,) = ctx.cloud_sor([cases["n64"]], mean_k=mean_k)
    assert math.isnan(got[2]) == (mean_k == 64)


def test_eight_segments_in_one_call(ctx, cases, refs):
    names = ["n1000", "plane", "n0", "depth", "n50", "contrast", "coincident", "n51"]
    got = ctx.cloud_sor([cases[n] for n in names])
    assert len(got) == 8
    for n, g in zip(names, got):
        (single,) = ctx.cloud_sor([cases[n]])
        _same(g, single, n)
        _same(g, refs[n], n)


def _vg_same(ctx, xyz, rgb, leaf, name):
    gx, gr, over = ctx.cloud_voxel_grid(xyz, rgb, leaf)
    wx, wr, wover = rcf.voxel_grid(xyz, rgb, leaf)
    assert over == wover, name
    assert gx.shape == wx.shape and np.array_equal(gx, wx) and np.array_equal(gr, wr), name
    return gx


def test_voxel_grid_equals_the_restatement(ctx, depth):
    xyz, rgb = depth
    fine = _vg_same(ctx, xyz, rgb, 0.02, "depth-0.02")
    coarse = _vg_same(ctx, xyz, rgb, 0.5, "depth-0.5")
    assert len(coarse) * 2 < len(xyz) and len(coarse) < len(fine) <= len(xyz)
    for name, (x, c, leaf) in voxel_cases().items():
        out = _vg_same(ctx, x, c, leaf, name)
        if name in ("single-voxel", "one-point"):
            assert len(out) == 1
    gx, gr, over = ctx.cloud_voxel_grid(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert len(gx) == 0 and len(gr) == 0 and not over


def test_voxel_grid_overflow_returns_the_input(ctx, depth):
    rgb = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    xyz = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 5.0], [3.0, 2.0, 1.0]], np.float32)       # 5001 x 5001 x 251 cells of 2 cm
    gx, gr, over = ctx.cloud_voxel_grid(xyz, rgb, 0.02)
    assert over and np.array_equal(gx, xyz) and np.array_equal(gr, rgb)
    assert rcf.voxel_grid(xyz, rgb, 0.02)[2] is True
    for ex, want in ((46339.5, False), (46340.5, True)):                  # 46340 x 46341 cells <= INT32_MAX < 46341 x 46341
        xyz = np.array([[0.0, 0.0, 0.0], [ex, 46340.5, 0.5]], np.float32)
        assert _vg_same(ctx, xyz, rgb[:2], 1.0, ex) is not None
        assert ctx.cloud_voxel_grid(xyz, rgb[:2], 1.0)[2] is want
    # the context goes on working after the early return
    _vg_same(ctx, depth[0], depth[1], 0.5, "after")


def test_the_kept_buffers_carry_nothing_over(svs):
    """on a fresh context: both filters on n51 (mean_k + 1 points), on the first 204 points of n1000, on n51 again.  Every buffer of
    the family holds a fixed number of bytes per point (12 xyz, 8 a key, 4 a value or a distance, 3 a colour) and a regrow takes a
    quarter plus 256 bytes more: 51 points ask for 612, 408, 204 and 153 bytes (the context then keeps 1021, 766, 511 and 447), 204
    points for 2448, 1632, 816 and 612, each more than 1.25 times the first request plus 256, so the second round replaces every
    per-point buffer and the third runs in what it left.  First and third round are the same bits, the bits of a context that has
    seen nothing else, and the restatement's."""
    c = sor_cases(svs, depth=False)
    small, big = c["n51"], np.ascontiguousarray(c["n1000"][:204])
    rgb = np.random.default_rng(3).integers(0, 256, (204, 3)).astype(np.uint8)
    a = gc.new_context(svs, 64, 32, max_slots=1, max_jobs=1, **KW)
    b = gc.new_context(svs, 64, 32, max_slots=1, max_jobs=1, **KW)
    try:
        rounds = [(x.cloud_sor([p])[0], x.cloud_voxel_grid(p, rgb[:len(p)], 0.5)) for x, p in ((a, small), (a, big), (a, small), (b, small))]
    finally:
        a.close(); b.close(); gc.settle_rotation(svs)
    for (sor, vg), p in zip(rounds, (small, big, small, small)):
        _same(sor, rcf.sor(p), len(p))
        assert not math.isnan(sor[2])
        wx, wr, wover = rcf.voxel_grid(p, rgb[:len(p)], 0.5)
        assert vg[2] == wover and np.array_equal(vg[0], wx) and np.array_equal(vg[1], wr) and 1 < len(wx) < len(p)
    for sor, vg in rounds[2:]:
        _same(sor, rounds[0][0], "again")
        assert all(np.array_equal(x, y) for x, y in zip(vg[:2], rounds[0][1][:2]))


def test_argument_errors_leave_the_context_usable(ctx, cases, refs):
    bad = cases["n65"].copy()
    bad[17, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        ctx.cloud_sor([cases["n51"], bad])
    bad[17, 1] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        ctx.cloud_voxel_grid(bad, np.zeros((65, 3), np.uint8))
    for k in (0, 65, -3):
        with pytest.raises(RuntimeError, match="mean_k"):
            ctx.cloud_sor([cases["n65"]], mean_k=k)
    for leaf in (0.0, -0.02, float("nan")):
        with pytest.raises(RuntimeError, match="leaf"):
            ctx.cloud_voxel_grid(cases["n65"], np.zeros((65, 3), np.uint8), leaf)
    (got,) = ctx.cloud_sor([cases["n65"]])
    _same(got, refs["n65"], "n65")


def test_timing_family_counts_points(ctx, cases):
    ctx.timing(True)
    try:
        ctx.cloud_sor([cases["n1000"], cases["plane"]])
        ms, launches, units = ctx.timing_get("cloud_filter")
        assert launches == 1 and units == 2500 and ms > 0
        ctx.cloud_voxel_grid(cases["plane"], np.zeros((1500, 3), np.uint8))
        ms2, launches, units = ctx.timing_get("cloud_filter")
        assert launches == 2 and units == 4000 and ms2 > ms
    finally:
        ctx.timing(False)
