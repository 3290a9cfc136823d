"""The HIP block matcher and cloud kernels (csrc/k_stereo_bm.h: svslam_stereo_bm_batch, svslam_dense_cloud_batch)
against the numpy restatement tests/ref_stereo_bm.py: disparity maps bit for bit, the compacted cloud with its order
exactly and its coordinates within one f32 ulp."""
import numpy as np
import pytest

import common as cm
import ref_stereo_bm as rbm
from test_ref_stereo_bm import (band_pair, check_period8_ratio0, half_pixel_pair, hand_pairs, region_of, texture_ramp_pair, tie_pair,
                                uniqueness_ramp_pair)

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
    _check_cloud(svs, w, h, nd, bs, rig, 1.0)


def _check_cloud(svs, w, h, nd, bs, rig, min_depth, expect_points=None):
    left, right = _crop(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    if rig == "kitti_identity":
        cam, ext, T = cm.CAM, cm.EXT_L, np.array(svs.IDENT)
    else:
        cam, ext, T = cm.GENERAL_RIG[0], cm.GENERAL_RIG[1], _general_pose()
    ref_disp = _ref(("crop", w, h, nd, bs), left, right, prm)
    ref_xyz, ref_pix = rbm.dense_cloud(ref_disp, cam, ext, cm.BASELINE, T, min_depth=min_depth)
    if expect_points is None:
        assert len(ref_pix) > 0.2 * (h - bs) * (w - nd - bs)
    else:
        assert len(ref_pix) == expect_points
    md = dict(min_depth=min_depth)
    c = svs.Context(w, h, max_slots=2, max_jobs=2, **KW)
    try:
        c.pyramid([0, 1], [left, right])
        (xyz, pix, disp), = c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, **md, **prm)
        assert np.array_equal(disp, ref_disp)
        assert len(pix) == len(ref_pix) and np.array_equal(pix, ref_pix)
        assert xyz.dtype == np.float32 and xyz.shape == ref_xyz.shape
        # one f32 ulp: the f64 evaluation order (quaternion rotation here, matrices there) may differ by rounding before
        # the final conversion to f32
        ulp = np.spacing(np.abs(ref_xyz))
        err = np.abs(xyz.astype(np.float64) - ref_xyz.astype(np.float64))
        print("cloud %dx%d %s min_depth %r: %d points, %d coordinates off by one ulp" % (w, h, rig, min_depth, len(pix), int((err > 0).sum())))
        assert (err <= ulp).all(), float((err / ulp).max())
        # a cap of exactly the count passes, one below is an error — not a truncation
        n = len(ref_pix)
        (xyz2, pix2, _), = c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, max_pts_per_job=max(n, 1), **md, **prm)
        assert np.array_equal(pix2, pix) and np.array_equal(xyz2, xyz)
        if n > 1:                                      # (n = 0, the empty cloud of min_depth 1e9: no cap below the count exists)
            with pytest.raises(RuntimeError, match="max_pts_per_job"):
                c.dense_cloud([(0, 1, T)], cam, ext, cm.BASELINE, max_pts_per_job=n - 1, **md, **prm)
        # two jobs, different poses: each job's list starts at its own offset
        out = c.dense_cloud([(0, 1, None), (0, 1, T)], cam, ext, cm.BASELINE, **md, **prm)
        assert np.array_equal(out[1][0], xyz) and np.array_equal(out[0][1], pix) and np.array_equal(out[1][1], pix)
        assert np.array_equal(out[0][0], xyz) == (rig == "kitti_identity" or n == 0)
    finally:
        c.close()
    return len(pix)


BAD = [dict(num_disparities=0), dict(num_disparities=-16), dict(num_disparities=24), dict(num_disparities=272),
       dict(block_size=4), dict(block_size=14), dict(block_size=3), dict(block_size=23),
       dict(pre_filter_cap=0), dict(pre_filter_cap=64), dict(texture_threshold=-1), dict(uniqueness_ratio=-1),
       dict(uniqueness_ratio=10001), dict(num_disparities=8), dict(block_size=22)]


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


# ---- the parameter space beyond the reference's one point -------------------------------------------------------------------
def _valid(disp, nd, bs):
    return float((region_of(disp, nd, bs) > 0).mean())


def _differ(a, b, nd, bs):
    return float((region_of(a, nd, bs) != region_of(b, nd, bs)).mean())


def _bit_exact(got, ref):
    assert got.dtype == np.int16 and np.array_equal(got, ref), (np.argwhere(got != ref)[:8], got[got != ref][:8], ref[got != ref][:8])


# window words NWW = ceil(bs / 4) and bytes in the last word: 7 -> 2 / 3, 13 -> 4 / 1, 17 -> 5 / 1, 19 -> 5 / 3 (the other tests run 2 / 1,
# 3 / 1, 3 / 3, 4 / 3, 6 / 1).  Two disparity counts each; odd heights, odd widths, a partial last 64-column tile
BLOCKS = [(131, 37, 16, 7), (203, 41, 64, 7), (141, 39, 32, 13), (247, 45, 128, 13), (149, 43, 48, 17), (337, 51, 256, 17),
          (157, 47, 32, 19), (275, 55, 160, 19)]


@pytest.mark.parametrize("w,h,nd,bs", BLOCKS)
def test_block_sizes_7_13_17_19_are_bit_exact(svs, w, h, nd, bs):
    left, right = _crop(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    ref = _ref(("crop", w, h, nd, bs), left, right, prm)
    cols = w - 2 * (bs // 2) - (nd - 1)
    assert h % 2 == 1 and w % 4 != 0 and cols > 64 and cols % 64 != 0
    print("bs %d nd %d %dx%d: window words %d, last bytes %d, valid %.1f %%" % (bs, nd, w, h, (bs + 3) // 4, bs - 4 * ((bs + 3) // 4 - 1), 100 * _valid(ref, nd, bs)))
    assert _valid(ref, nd, bs) > 0.3
    _bit_exact(_run(svs, left, right, prm), ref)


# five window words at every strip height: 149x43 with bs 17 is 2 tiles x 27 rows (27 = 16 + 11 = 3 x 8 + 3 = 6 x 4 + 3: a partial last
# strip at every height), 157x47 with bs 19 is 2 tiles x 29 rows (16 + 13, 3 x 8 + 5, 7 x 4 + 1).  The height is 16 from 1024 workgroups
# of 16 rows on (2 x 2 x 256), 8 from 1024 workgroups of 8 rows on (2 x 4 x 128, which are 512 of 16 rows), else 4
STRIPS5 = [(149, 43, 48, 17, 256, 16), (149, 43, 48, 17, 128, 8), (149, 43, 48, 17, 2, 4),
           (157, 47, 32, 19, 256, 16), (157, 47, 32, 19, 128, 8), (157, 47, 32, 19, 3, 4)]


@pytest.mark.parametrize("w,h,nd,bs,njobs,th", STRIPS5)
def test_five_window_words_at_every_strip_height(svs, w, h, nd, bs, njobs, th):
    assert (bs + 3) // 4 == 5 and (h - 2 * (bs // 2)) % th != 0
    pairs = _distinct_pairs(svs, w, h)
    prm = dict(num_disparities=nd, block_size=bs)
    refs = [_ref(("strip", w, h, nd, bs, j), p[0], p[1], prm) for j, p in enumerate(pairs)]
    print("bs %d strips of %d: valid %s" % (bs, th, ["%.2f" % _valid(x, nd, bs) for x in refs]))
    assert all(not np.array_equal(refs[i], refs[j]) for i in range(4) for j in range(i))
    assert max(_valid(x, nd, bs) for x in refs) > 0.5
    c = svs.Context(w, h, max_slots=8, max_jobs=max(njobs, 8), **KW)
    try:
        c.pyramid(list(range(8)), [im for p in pairs for im in p])
        assert c.stereo_bm_strip_rows(njobs, **prm) == th
        order = [(3 * i + i // 4) % 4 for i in range(njobs)]
        got = c.stereo_bm([(2 * j, 2 * j + 1) for j in order], **prm)
    finally:
        c.close()
    for i, j in enumerate(order):
        assert np.array_equal(got[i], refs[j]), (i, j, np.argwhere(got[i] != refs[j])[:8])


def _band_width(nd, bs):
    """nd 240: the smallest width that leaves two tiles (65 computed columns); else 98 columns"""
    return nd - 1 + 2 * (bs // 2) + (65 if nd == 240 else 98)


@pytest.mark.parametrize("bs", [9, 15])
@pytest.mark.parametrize("nd", [48, 80, 112, 176, 240])
def test_disparity_counts_that_are_no_power_of_two(svs, nd, bs):
    """nd / 16 chunks dealt to four waves unevenly (3, 5, 7, 11, 15 chunks) and quarters of nd / 4 = 12, 20, 28, 44, 60 disparities that
    cut through the chunks.  The pair has four bands whose shifts lie one in each quarter, two of them at a quarter's edge."""
    w, h = _band_width(nd, bs), 59
    left, right = band_pair(w, h, nd)
    prm = dict(num_disparities=nd, block_size=bs)
    ref = _ref(("bands", nd, bs), left, right, prm)
    reg = region_of(ref, nd, bs)
    d = reg[reg > 0] >> 4
    hit = [int(((d >= q * nd // 4) & (d < (q + 1) * nd // 4)).sum()) for q in range(4)]
    print("nd %d bs %d %dx%d: valid %.1f %%, arg-min per quarter %s" % (nd, bs, w, h, 100 * _valid(ref, nd, bs), hit))
    assert (nd // 16) % 4 != 0 and min(hit) >= 100
    assert (w - 2 * (bs // 2) - (nd - 1) == 65) == (nd == 240)
    _bit_exact(_run(svs, left, right, prm), ref)


# ---- one parameter at a time -------------------------------------------------------------------------------------------------
PW, PH, PND, PBS = 340, 59, 32, 9          # the shape of the texture and uniqueness ramps: 5 tiles (the last 44 columns), 51 rows


def _param_input(svs, name):
    if name == "crop":
        return _crop(svs, 200, 47), dict(num_disparities=64, block_size=9)
    pair = texture_ramp_pair(PW, PH, PND) if name == "texture_ramp" else uniqueness_ramp_pair(PW, PH, PND)
    return pair, dict(num_disparities=PND, block_size=PBS)


def _param_case(svs, name, **changed):
    """(reference at the changed parameters, reference at the defaults, prm); the kernel is compared inside"""
    (left, right), prm = _param_input(svs, name)
    base = _ref((name, "defaults"), left, right, prm)
    prm2 = dict(prm, **changed)
    ref = _ref((name,) + tuple(sorted(changed.items())), left, right, prm2)
    _bit_exact(_run(svs, left, right, prm2), ref)
    return ref, base, prm


@pytest.mark.parametrize("name", ["crop", "texture_ramp"])
@pytest.mark.parametrize("cap", [1, 2, 15, 62, 63])
def test_pre_filter_cap(svs, cap, name):
    """the cap enters the prefilter's clamp and, as the byte the texture sum is taken against, the texture test: on the texture
    ramp the pixels whose window holds one faint dot are valid or not by that sum alone"""
    ref, base, prm = _param_case(svs, name, pre_filter_cap=cap)
    nd, bs = prm["num_disparities"], prm["block_size"]
    (left, right), _ = _param_input(svs, name)
    _, tex = rbm.sad_volume(left, right, nd, bs, cap)
    by_texture = float(((tex < 10) & (tex > 0)).mean())
    print("cap %d on %s: valid %.1f %%, differs from cap 31 in %.1f %%, filtered by a texture sum in 1..9: %.1f %%" %
          (cap, name, 100 * _valid(ref, nd, bs), 100 * _differ(ref, base, nd, bs), 100 * by_texture))
    assert _differ(ref, base, nd, bs) >= 0.02
    assert name != "texture_ramp" or by_texture >= 0.02


# texture_threshold on the texture ramp.  Read off the reference's texture sums over the computed region (cap 31): 22 % are 0 (the flat
# tenth and windows between dots), 11 % lie in 1..9, 8 is the sum of a window with one dot, the median is 163, the 70th percentile 737,
# the maximum 2378.  0 and 2379 are the extremes: nothing and everything filtered by texture
TEX = [1, 5, 8, 163, 737]


@pytest.mark.parametrize("tex", TEX)
def test_texture_threshold_discriminates(svs, tex):
    ref, base, prm = _param_case(svs, "texture_ramp", texture_threshold=tex)
    nd, bs = prm["num_disparities"], prm["block_size"]
    print("texture_threshold %d: valid %.1f %%, differs from 10 in %.1f %%" % (tex, 100 * _valid(ref, nd, bs), 100 * _differ(ref, base, nd, bs)))
    assert _differ(ref, base, nd, bs) >= 0.02 and 0.05 < _valid(ref, nd, bs) < 0.95


def test_texture_threshold_extremes(svs):
    (left, right), prm = _param_input(svs, "texture_ramp")
    _, tex = rbm.sad_volume(left, right, PND, PBS)
    top = int(tex.max()) + 1
    assert (tex < 0).mean() == 0.0 and (tex < top).mean() == 1.0 and (tex == 0).mean() > 0.05
    ref0, _, _ = _param_case(svs, "texture_ramp", texture_threshold=0)
    ref1, _, _ = _param_case(svs, "texture_ramp", texture_threshold=top)
    ref2, _, _ = _param_case(svs, "texture_ramp", texture_threshold=top - 1)
    print("texture_threshold 0: valid %.1f %%; %d: valid %.1f %%; %d: %d pixels valid" % (100 * _valid(ref0, PND, PBS), top, 100 * _valid(ref1, PND, PBS), top - 1,
                                                                                             int((region_of(ref2, PND, PBS) > 0).sum())))
    assert (ref1 == -16).all()
    # without the uniqueness test as well, threshold 0 leaves every pixel of the region valid, the flat tenth included (all SADs 0
    # there: the largest disparity, 16 x 31)
    ref3, _, _ = _param_case(svs, "texture_ramp", texture_threshold=0, uniqueness_ratio=0)
    assert _valid(ref3, PND, PBS) == 1.0 and (region_of(ref3, PND, PBS)[:, :20] == 16 * 31).all()
    ref4, _, _ = _param_case(svs, "texture_ramp", texture_threshold=1, uniqueness_ratio=0)
    assert (region_of(ref4, PND, PBS)[:, :20] == -16).all()


# uniqueness_ratio on the uniqueness ramp: the second-best SAD outside +-1 over the minimum falls from "anything" (minimum 0, last
# 12 %) towards 1 (the periodic end), so every ratio cuts the region at another column; 0 switches the test off
UNIQ = [0, 1, 5, 50, 100, 10000]


@pytest.mark.parametrize("uniq", UNIQ)
def test_uniqueness_ratio_discriminates(svs, uniq):
    ref, base, prm = _param_case(svs, "uniqueness_ramp", uniqueness_ratio=uniq)
    nd, bs = prm["num_disparities"], prm["block_size"]
    print("uniqueness_ratio %d: valid %.1f %%, differs from 15 in %.1f %%" % (uniq, 100 * _valid(ref, nd, bs), 100 * _differ(ref, base, nd, bs)))
    assert _differ(ref, base, nd, bs) >= 0.02 and 0.05 < _valid(ref, nd, bs) < 0.95


def test_two_combinations_at_the_limits(svs):
    left, right = _crop(svs, 340, 50)
    prm = dict(num_disparities=256, block_size=21, pre_filter_cap=63)
    ref = _ref("cap63-bs21-nd256", left, right, prm)
    base = _ref(("strip", 340, 50, 256, 21, 0), left, right, dict(num_disparities=256, block_size=21))
    print("cap 63, bs 21, nd 256: valid %.1f %%, differs from cap 31 in %.1f %%" % (100 * _valid(ref, 256, 21), 100 * _differ(ref, base, 256, 21)))
    assert _differ(ref, base, 256, 21) >= 0.02
    _bit_exact(_run(svs, left, right, prm), ref)
    for name in ("crop", "texture_ramp", "uniqueness_ramp"):
        ref, base, prm = _param_case(svs, name, pre_filter_cap=1, texture_threshold=0, uniqueness_ratio=0)
        nd, bs = prm["num_disparities"], prm["block_size"]
        print("cap 1, tex 0, uniq 0 on %s: valid %.1f %%, differs from the defaults in %.1f %%" % (name, 100 * _valid(ref, nd, bs), 100 * _differ(ref, base, nd, bs)))
        assert (region_of(ref, nd, bs) != -16).all() and _differ(ref, base, nd, bs) >= 0.02          # nothing filters: every pixel has a disparity


def test_period8_at_ratio_0(svs):
    """the hand pair whose minimum is tied at 0, 8, 16 and 24 — one disparity in each wave's quarter of 32: the largest survives"""
    left, right, prm, _ = hand_pairs()["period8"]
    prm = dict(prm, uniqueness_ratio=0)
    ref = _ref("period8-ratio0", left, right, prm)
    got = _run(svs, left, right, prm)
    _bit_exact(got, ref)
    check_period8_ratio0(region_of(got, 32, 9).astype(np.int32), 32, 0, rbm.sad_volume(left, right, 32, 9)[0])
    _bit_exact(_run(svs, left, right, dict(prm, uniqueness_ratio=1)), np.full_like(ref, -16))


@pytest.mark.parametrize("nd,bs", [(48, 9), (32, 5), (80, 7)])
def test_ties_between_the_quarters_go_to_the_largest_disparity(svs, nd, bs):
    """period nd / 2 ties quarter 0 with 2 and 1 with 3, the constant gradient ties all nd disparities; nothing filters them
    (texture_threshold 0, uniqueness_ratio 0).  Pins `<=` in each quarter's scan and in the merge of the four."""
    w, h = 127, 40
    left, right = tie_pair(w, h, nd)
    prm = dict(num_disparities=nd, block_size=bs, texture_threshold=0, uniqueness_ratio=0)
    ref = _ref(("ties", nd, bs), left, right, prm)
    sad, _ = rbm.sad_volume(left, right, nd, bs)
    at_min = sad == sad.min(0)[None]
    quarters = np.stack([at_min[q * nd // 4:(q + 1) * nd // 4].any(0) for q in range(4)])
    tied = quarters.sum(0) >= 2                                  # the minimum occurs in two quarters or more
    within = (at_min.sum(0) >= 2) & ~tied
    reg = region_of(ref, nd, bs)
    print("ties nd %d bs %d: %d pixels tied across quarters (%d across all four), %d only within one, valid %.1f %%, arg-min %s" %
          (nd, bs, int(tied.sum()), int((quarters.sum(0) == 4).sum()), int(within.sum()), 100 * _valid(ref, nd, bs), np.unique(reg >> 4).tolist()))
    assert tied.sum() >= 100 and (quarters.sum(0) == 4).sum() >= 100 and (reg != -16).all()
    # the rows whose window, and the image rows its prefilter reads, lie in the gradient (image row y >= h / 2 + r + 1 = region row
    # h / 2 + 1), but for the first and last column (whose windows meet the prefilter's cap columns 0 of R' and w - 1): the last disparity, no sub-pixel term
    assert (reg[h // 2 + 1:, 1:-1] == 16 * (nd - 1)).all() and reg[h // 2 + 1:, 1:-1].size >= 100
    _bit_exact(_run(svs, left, right, prm), ref)


# ---- the cloud's gate and its smallest image ---------------------------------------------------------------------------------
def _most_frequent_depth(ref_disp, fx):
    vals, counts = np.unique(ref_disp[ref_disp > 0], return_counts=True)
    d16 = int(vals[np.argmax(counts)])
    depth = (np.float32(fx) * np.float32(cm.BASELINE)) / (np.float32(d16) * np.float32(1.0 / 16.0))
    assert type(depth) is np.float32
    return d16, int(counts.max()), float(depth)


@pytest.mark.parametrize("rig", ["kitti_identity", "general"])
@pytest.mark.parametrize("which", ["0.25", "v", "v_plus_one_ulp", "1e9"])
def test_cloud_min_depth_gate(svs, which, rig):
    """min_depth is a double compared with the f32 depth as !(depth < min_depth): at v = the depth of the map's most frequent
    disparity those pixels are kept, one ulp of the double above they are dropped — exactly as many as the map holds"""
    w, h, nd, bs = 97, 53, 32, 5
    left, right = _crop(svs, w, h)
    ref_disp = _ref(("crop", w, h, nd, bs), left, right, dict(num_disparities=nd, block_size=bs))
    fx = (cm.CAM if rig == "kitti_identity" else cm.GENERAL_RIG[0])[0]
    d16, count, v = _most_frequent_depth(ref_disp, fx)
    up = float(np.nextafter(v, np.inf))
    # filtered pixels have depth 0 and are dropped by any positive min_depth; nearer than v means a larger disparity
    n_v = int(((ref_disp > 0) & (ref_disp <= d16)).sum())
    md, expect = {"0.25": (0.25, int((ref_disp > 0).sum())), "v": (v, n_v), "v_plus_one_ulp": (up, n_v - count), "1e9": (1e9, 0)}[which]
    print("min_depth %s = %r (disparity %d / 16 at %d pixels): %d points expected" % (which, md, d16, count, expect))
    assert count >= 10 and v > 1.0 and up > v
    assert _check_cloud(svs, w, h, nd, bs, rig, md, expect_points=expect) == expect


def test_cloud_of_the_smallest_image(svs):
    """20 x 16 is the smallest image with a computed pixel: svslam_create takes no side below 16, and nd 16, bs 5 need
    nd - 1 + r = 17 < w - r.  320 pixels on 1024 threads: `per` = 1, threads 320.. own an empty piece of the walk."""
    w, h, nd, bs = 20, 16, 16, 5
    assert w * h < 1024 and nd - 1 + bs // 2 < w - bs // 2 and not (nd - 1 + bs // 2 < (w - 1) - bs // 2) and h == 16
    rng = np.random.default_rng(71)
    wide = rng.integers(0, 256, (h, w + 3), dtype=np.uint8)
    left, right = wide[:, :w].copy(), wide[:, 3:].copy()
    prm = dict(num_disparities=nd, block_size=bs)
    ref_disp = _ref("smallest", left, right, prm)
    assert region_of(ref_disp, nd, bs).size == 12 and (region_of(ref_disp, nd, bs) > 0).sum() >= 6
    T = _general_pose()
    c = svs.Context(w, h, max_slots=2, max_jobs=2, **KW)
    try:
        c.pyramid([0, 1], [left, right])
        _bit_exact(c.stereo_bm([(0, 1)], **prm)[0], ref_disp)
        out = c.dense_cloud([(0, 1, None), (0, 1, T)], cm.GENERAL_RIG[0], cm.GENERAL_RIG[1], cm.BASELINE, **prm)
    finally:
        c.close()
    for (xyz, pix, disp), pose in zip(out, (np.array(svs.IDENT), T)):
        ref_xyz, ref_pix = rbm.dense_cloud(ref_disp, cm.GENERAL_RIG[0], cm.GENERAL_RIG[1], cm.BASELINE, pose)
        assert np.array_equal(disp, ref_disp) and len(ref_pix) >= 6 and np.array_equal(pix, ref_pix)
        err = np.abs(xyz.astype(np.float64) - ref_xyz.astype(np.float64))
        assert xyz.dtype == np.float32 and (err <= np.spacing(np.abs(ref_xyz))).all()
    print("smallest image %dx%d: %d points per job" % (w, h, len(out[0][1])))
    assert not np.array_equal(out[0][0], out[1][0])
