"""The HIP block matcher and cloud kernels (csrc/k_stereo_bm.h: svslam_stereo_bm_batch, svslam_dense_cloud_batch)
against the numpy restatement tests/ref_stereo_bm.py: disparity maps bit for bit, the compacted cloud with its order
exactly and its coordinates within one f32 ulp."""
import numpy as np
import pytest

import common as cm
import ref_stereo_bm as rbm
from test_ref_stereo_bm import half_pixel_pair, hand_pairs

pytestmark = pytest.mark.gpu

KW = dict(max_pts=64, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
_cache = {}


def _pair(svs, seed=1, frame=0):
    k = ("pair", seed, frame)
    if k not in _cache:
        _cache[k] = svs.synth_pair(seed, frame, w=620, h=188)
    return _cache[k]


def _crop(svs, w, h, seed=1, frame=0):
    """a w x h crop of the synthetic pair (same window of both images, so the disparities stay)"""
    left, right = _pair(svs, seed, frame)
    y0, x0 = (188 - h) // 2, (620 - w) // 2
    return left[y0:y0 + h, x0:x0 + w].copy(), right[y0:y0 + h, x0:x0 + w].copy()


def _ref(key, left, right, prm):
    """the restatement, computed once per input and never modified"""
    if key not in _cache:
        d = rbm.stereo_bm(left, right, **prm)
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def _run(svs, left, right, prm):
    h, w = left.shape
    c = svs.Context(w, h, max_slots=2, max_jobs=2, **KW)      # (a pyramid call takes one job per image)
    try:
        c.pyramid([0, 1], [left, right])
        return c.stereo_bm([(0, 1)], **prm)[0]
    finally:
        c.close()


# width, height, num_disparities, block_size: the reference's shape; a small one; odd height and a width that is no multiple
# of the 64-column tile or of 4; a strip barely taller than the largest window; a region only nine columns wide (nd - 1 + r = 134,
# w - r = 143) — not yet OpenCV's early-out, that is EARLY_OUT below
SHAPES = [(620, 188, 128, 15), (200, 48, 64, 9), (97, 53, 32, 5), (161, 31, 16, 21), (150, 30, 128, 15)]


@pytest.mark.parametrize("w,h,nd,bs", SHAPES)
def test_disparity_is_bit_exact_on_crops(svs, w, h, nd, bs):
    left, right = _crop(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    ref = _ref(("crop", w, h, nd, bs), left, right, prm)
    got = _run(svs, left, right, prm)
    r = bs // 2
    assert nd - 1 + r < w - r and h >= 2 * r + 1
    assert (ref[r:h - r, nd - 1 + r:w - r] > 0).mean() > 0.3           # the case is not vacuous
    assert got.dtype == np.int16 and np.array_equal(got, ref), (np.argwhere(got != ref)[:8], got[got != ref][:8], ref[got != ref][:8])


# OpenCV's early-out: no column to compute (nd - 1 + r = 134 >= w - r = 133); the widest such image, w = nd + 2r - 1; no row to
# compute (h = 20 < 2r + 1 = 21, columns there would be).  The call succeeds, every pixel is -16 and the cloud is empty.
EARLY_OUT = [(140, 30, 128, 15), (141, 30, 128, 15), (97, 20, 16, 21)]


@pytest.mark.parametrize("w,h,nd,bs", EARLY_OUT)
def test_early_out_is_all_filtered_and_an_empty_cloud(svs, w, h, nd, bs):
    left, right = _crop(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    r = bs // 2
    assert nd - 1 + r >= w - r or h < 2 * r + 1
    assert (rbm.stereo_bm(left, right, **prm) == -16).all()
    c = svs.Context(w, h, max_slots=4, max_jobs=4, **KW)
    try:
        c.pyramid([0, 1, 2, 3], [left, right, right, left])
        assert c.stereo_bm_strip_rows(2, **prm) == 0                  # the matcher kernel is not launched
        got = c.stereo_bm([(0, 1), (2, 3)], **prm)
        assert got.shape == (2, h, w) and got.dtype == np.int16 and (got == -16).all()
        out = c.dense_cloud([(0, 1, None), (2, 3, _general_pose())], cm.CAM, cm.EXT_L, cm.BASELINE, **prm)
        for xyz, pix, disp in out:
            assert xyz.shape == (0, 3) and pix.shape == (0,) and (disp == -16).all()
        # max_pts_per_job = 1 is enough for no point, and the context computes again afterwards
        (xyz, pix, disp), = c.dense_cloud([(0, 1, None)], cm.CAM, cm.EXT_L, cm.BASELINE, max_pts_per_job=1, **prm)
        assert len(pix) == 0 and (disp == -16).all()
        assert (c.stereo_bm([(0, 1)], num_disparities=16, block_size=5)[0] > 0).any()
    finally:
        c.close()


def _distinct_pairs(svs, w, h):
    """four pairs of different content at one size: three crops of different synthetic frames and one with left and right swapped"""
    return [_crop(svs, w, h), _crop(svs, w, h, seed=7, frame=33), tuple(reversed(_crop(svs, w, h, seed=3, frame=5))), _crop(svs, w, h, seed=5, frame=12)]


# (w, h, nd, bs, njobs, strip rows): the strip height is chosen from the call's workgroup count (16 from 1024 workgroups on, else 8,
# else 4), so every call of the other tests runs strips of 4.  The reference's shape (620x188: 8 tiles, 174 rows) with 12 jobs is 8 x 11
# x 12 = 1056 workgroups of 16 rows, with 6 jobs 8 x 22 x 6 = 1056 of 8 rows; both leave a partial last strip (174 = 10 x 16 + 14 =
# 21 x 8 + 6).  The small shape (3 tiles, 40 rows) does the same with another window-word count and rows = 40 = 2 x 16 + 8; the
# largest window at the most disparities is the LDS limit of 16-row strips (2 tiles, 30 rows = 16 + 14).
STRIPS = [(620, 188, 128, 15, 12, 16), (620, 188, 128, 15, 6, 8), (200, 48, 64, 9, 114, 16), (200, 48, 64, 9, 69, 8),
          (340, 50, 256, 21, 256, 16), (340, 50, 256, 21, 2, 4)]


@pytest.mark.parametrize("w,h,nd,bs,njobs,th", STRIPS)
def test_every_strip_height_is_bit_exact(svs, w, h, nd, bs, njobs, th):
    pairs = _distinct_pairs(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    refs = [_ref(("strip", w, h, nd, bs, j), p[0], p[1], prm) for j, p in enumerate(pairs)]
    valid = [(x[bs // 2:h - bs // 2, nd - 1 + bs // 2:w - bs // 2] > 0).mean() for x in refs]
    assert min(valid[0], valid[1], valid[3]) > 0.5 and 0 < valid[2] < 0.5            # (the swapped pair matches little, by design)
    assert all(not np.array_equal(refs[i], refs[j]) for i in range(4) for j in range(i))
    c = svs.Context(w, h, max_slots=8, max_jobs=max(njobs, 8), **KW)
    try:
        c.pyramid(list(range(8)), [im for p in pairs for im in p])
        assert c.stereo_bm_strip_rows(njobs, **prm) == th              # the case runs the strip height it is here for
        order = [(3 * i + i // 4) % 4 for i in range(njobs)]           # neighbouring jobs differ, and not with period 4
        got = c.stereo_bm([(2 * j, 2 * j + 1) for j in order], **prm)
    finally:
        c.close()
    for i, j in enumerate(order):
        assert np.array_equal(got[i], refs[j]), (i, j, np.argwhere(got[i] != refs[j])[:8])


def test_half_pixel_pair_is_bit_exact(svs):
    left, right, prm = half_pixel_pair()
    assert np.array_equal(_run(svs, left, right, prm), _ref("half", left, right, prm))


@pytest.mark.parametrize("name", ["shift5", "constant", "period8"])
def test_hand_checkable_pairs(svs, name):
    left, right, prm, want = hand_pairs()[name]
    got = _run(svs, left, right, prm)
    assert np.array_equal(got, _ref(("hand", name), left, right, prm))
    h, w = left.shape
    r = prm["block_size"] // 2
    region = got[r:h - r, prm["num_disparities"] - 1 + r:w - r]
    assert (region >= want[0]).all() and (region <= want[1]).all()


def test_three_jobs_of_different_content(svs):
    pairs = [_crop(svs, 200, 48), _crop(svs, 200, 48, seed=7, frame=33), tuple(reversed(_crop(svs, 200, 48, seed=3, frame=5)))]
    prm = dict(num_disparities=64, block_size=9)
    c = svs.Context(200, 48, max_slots=6, max_jobs=6, **KW)
    try:
        c.pyramid(list(range(6)), [im for p in pairs for im in p])
        got = c.stereo_bm([(4, 5), (0, 1), (2, 3)], **prm)           # not in slot order
    finally:
        c.close()
    for i, j in enumerate((2, 0, 1)):
        assert np.array_equal(got[i], _ref(("jobs", j), pairs[j][0], pairs[j][1], prm)), (i, j)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def test_black_and_white_pair_saturates_the_prefilter(svs):
    rng = np.random.default_rng(11)
    h, w = 44, 130
    wide = (rng.random((h, w + 7)) < 0.5).astype(np.uint8) * 255
    wide = np.repeat(np.repeat(wide[:h // 2 + 1, :(w + 7) // 2 + 1], 2, 0), 2, 1)[:h, :w + 7]      # 2 x 2 blocks of 0 / 255
    left, right = np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, 7:])
    pf = rbm.prefilter_xsobel(left, 31)
    assert (pf == 0).any() and (pf == 62).any()
    prm = dict(num_disparities=32, block_size=11)
    assert np.array_equal(_run(svs, left, right, prm), _ref("bw", left, right, prm))


def _general_pose():
    from scipy.spatial.transform import Rotation
    return np.concatenate([Rotation.from_rotvec([0.11, -0.23, 0.07]).as_quat(), [1.7, -0.4, 12.5]])


@pytest.mark.parametrize("w,h,nd,bs", [(620, 188, 128, 15), (97, 53, 32, 5)])
@pytest.mark.parametrize("rig", ["kitti_identity", "general"])
def test_cloud_matches_the_reference_loop(svs, w, h, nd, bs, rig):
    left, right = _crop(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    if rig == "kitti_identity":
        cam, ext, T = cm.CAM, cm.EXT_L, np.array(svs.IDENT)
    else:
        cam, ext, T = cm.GENERAL_RIG[0], cm.GENERAL_RIG[1], _general_pose()
    ref_disp = _ref(("crop", w, h, nd, bs), left, right, prm)
    ref_xyz, ref_pix = rbm.dense_cloud(ref_disp, cam, ext, cm.BASELINE, T)
    assert len(ref_pix) > 0.2 * (h - bs) * (w - nd - bs)
    c = svs.Context(w, h, max_slots=2, max_jobs=2, **KW)
    try:
        c.pyramid([0, 1], [left, right])
        (xyz, pix, disp), = c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, **prm)
        assert np.array_equal(disp, ref_disp)
        assert len(pix) == len(ref_pix) and np.array_equal(pix, ref_pix)
        assert xyz.dtype == np.float32 and xyz.shape == ref_xyz.shape
        # one f32 ulp: the f64 evaluation order (quaternion rotation here, matrices there) may differ by rounding before
        # the final conversion to f32
        ulp = np.spacing(np.abs(ref_xyz))
        err = np.abs(xyz.astype(np.float64) - ref_xyz.astype(np.float64))
        print("cloud %dx%d %s: %d points, %d coordinates off by one ulp" % (w, h, rig, len(pix), int((err > 0).sum())))
        assert (err <= ulp).all(), float((err / ulp).max())
        # a cap of exactly the count passes, one below is an error — not a truncation
        n = len(ref_pix)
        (xyz2, pix2, _), = c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, max_pts_per_job=n, **prm)
        assert np.array_equal(pix2, pix) and np.array_equal(xyz2, xyz)
        with pytest.raises(RuntimeError, match="max_pts_per_job"):
            c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, max_pts_per_job=n - 1, **prm)
        # two jobs, different poses: each job's list starts at its own offset
        out = c.dense_cloud([(0, 1, None), (0, 1, T)], cam, ext, cm.BASELINE, **prm)
        assert np.array_equal(out[1][0], xyz) and np.array_equal(out[0][1], pix) and np.array_equal(out[1][1], pix)
        assert np.array_equal(out[0][0], xyz) == (rig == "kitti_identity")
    finally:
        c.close()


BAD = [dict(num_disparities=0), dict(num_disparities=-16), dict(num_disparities=24), dict(num_disparities=272),
       dict(block_size=4), dict(block_size=14), dict(block_size=3), dict(block_size=23),
       dict(pre_filter_cap=0), dict(pre_filter_cap=64), dict(texture_threshold=-1), dict(uniqueness_ratio=-1)]


def test_bad_parameters_are_errors_with_a_message(svs):
    left, right = _crop(svs, 97, 53)
    c = svs.Context(97, 53, max_slots=2, max_jobs=2, **KW)
    try:
        c.pyramid([0, 1], [left, right])
        for bad in BAD:
            for call in (lambda: c.stereo_bm([(0, 1)], **bad), lambda: c.dense_cloud([(0, 1, None)], cm.CAM, cm.EXT_L, cm.BASELINE, **bad)):
                with pytest.raises(RuntimeError) as e:
                    call()
                assert list(bad)[0] in str(e.value), (bad, str(e.value))
        for call in (lambda: c.stereo_bm([(0, 2)]), lambda: c.stereo_bm([(-1, 1)]), lambda: c.stereo_bm([(0, 1)] * 3),
                     lambda: c.dense_cloud([(0, 1, None)], cm.CAM, cm.EXT_L, 0.0), lambda: c.dense_cloud([(0, 1, None)], cm.CAM, cm.EXT_L, cm.BASELINE, min_depth=0.0),
                     lambda: c.dense_cloud([(0, 1, None)], cm.CAM, cm.EXT_L, cm.BASELINE, max_pts_per_job=0)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert len(str(e.value)) > 20
        # the context is still usable
        assert c.stereo_bm([(0, 1)], num_disparities=32, block_size=5).shape == (1, 53, 97)
    finally:
        c.close()


def test_timing_family_6_counts_the_jobs(svs):
    left, right = _crop(svs, 200, 48)
    c = svs.Context(200, 48, max_slots=2, max_jobs=4, **KW)
    try:
        c.pyramid([0, 1], [left, right])
        assert svs.DENSE_FAMILIES["stereo_bm"] == 6
        c.timing(True)
        c.stereo_bm([(0, 1)] * 4, num_disparities=64, block_size=9)
        c.stereo_bm([(0, 1)], num_disparities=64, block_size=9)
        ms, launches, units = c.timing_get("stereo_bm")
        assert launches == 2 and units == 5 and ms > 0
    finally:
        c.close()
