"""tests/ref_orb_desc.py held to facts it does not use itself: the exact signed permutations at the quarter turns, the descriptor of a
turned image at the turned centre and angle, the constant image, and ref_brief's rows at -1 degree on level 0."""
import numpy as np
import pytest

import ref_brief as rb
import ref_orb
import ref_orb_desc as rod

PAT = rb.default_pattern()


def test_quarter_turns_are_exact_signed_permutations():
    p = PAT.reshape(512, 2).astype(np.int64)
    # cos and sin of k * 90 degrees in f32 are within 1e-7 of 0 and +-1, |p| <= 13: the rounding gives the exact turn
    for ang, (m00, m01, m10, m11) in ((0.0, (1, 0, 0, 1)), (90.0, (0, -1, 1, 0)), (180.0, (-1, 0, 0, -1)), (270.0, (0, 1, -1, 0))):
        off = rod.offsets(PAT, ang)
        assert np.array_equal(off[:, 0], m00 * p[:, 0] + m01 * p[:, 1]) and np.array_equal(off[:, 1], m10 * p[:, 0] + m11 * p[:, 1]), ang


def test_reach_of_the_tables():
    assert rod.reach(PAT) == 19                                   # (13, 13) is not in the table; the farthest point is within 19
    t = np.array(PAT); t[0] = (13, 13, 0, 1)
    assert rod.reach(t) == 19 and 13 * 13 * 2 <= 19 * 19
    t[0] = (3, 4, 0, 1); t[1:] = (1, 0, 0, 1)
    assert rod.reach(t) == 5                                      # a perfect square: m^2 == px^2 + py^2
    for ang in np.random.default_rng(2).uniform(0, 360, 200):
        assert np.abs(rod.offsets(PAT, ang)).max() <= 19


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_turned_image_at_the_turned_centre_and_angle_gives_the_same_row(k):
    """np.rot90(img, k) turns the image k quarter turns counter-clockwise as displayed (y down): pixel (x, y) of an h x w image goes to
    (y, w - 1 - x).  An offset (dx, dy) then becomes (dy, -dx), which in the contract's rotation (ix = px a - py b, iy = px b + py a) is
    the angle -90: so the angle of the turned keypoint is angle - 90 k.  Exact, because the blur's taps are symmetric and separable."""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (96, 120), dtype=np.uint8)
    h, w = img.shape
    pts = [(40.0, 45.0, 0.0), (60.0, 50.0, 90.0), (55.0, 40.0, 180.0), (70.0, 48.0, 270.0)]
    kp = [(x, y, a, 0) for x, y, a in pts]
    want, idx = rod.describe(img, kp)
    assert len(idx) == len(kp)
    cur, cw, turned = img, w, kp
    for _ in range(k):
        cur = np.rot90(cur)
        turned = [(y, cw - 1 - x, (a - 90.0) % 360.0, o) for x, y, a, o in turned]
        cw = cur.shape[1]
    got, idx2 = rod.describe(np.ascontiguousarray(cur), turned)
    assert len(idx2) == len(kp) and np.array_equal(got, want)
    assert len({r.tobytes() for r in want}) == len(kp)


def test_a_constant_image_gives_zeros():
    img = np.full((120, 160), 137, np.uint8)
    d, idx = rod.describe(img, [(50.0, 50.0, 33.0, 0), (60.0, 60.0, 200.0, 1), (80.0, 60.0, 1.0, 2)])
    assert len(idx) == 3 and not d.any()


def test_minus_one_degree_on_level_0_is_ref_brief():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    xy = np.stack([rng.uniform(25, 135, 80), rng.uniform(25, 95, 80)], axis=1).astype(np.float32)
    xy = np.concatenate([xy, np.array([[128.99, 50.0], [129.0, 50.0], [31.0, 88.99], [30.99, 50.0], [40.5, 41.5]], np.float32)])
    d0, i0 = rb.describe(img, xy, angle_deg=-1.0)
    d1, i1 = rod.describe(img, [(x, y, -1.0, 0) for x, y in xy])
    assert len(i0) > 40 and np.array_equal(i0, i1) and np.array_equal(d0, d1)
    # and the offsets themselves: the C library's cos / sin against numpy's f32 ones, equal after the rounding (brief_cases asserts the margin)
    assert np.array_equal(rod.offsets(PAT, -1.0), rb.offsets(PAT, -1.0))


def test_levels_are_the_detectors():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    _, info = ref_orb.detect(img, None, nfeatures=50)
    lv, geo = rod.levels(img, 5)
    assert geo == ref_orb.level_geometry(160, 120, 6)
    for a, b in zip(lv, info["levels"]):
        assert np.array_equal(a, b)


def test_refusals_of_the_reference():
    img = np.zeros((120, 160), np.uint8)
    for kp, kw, words in (([(50, 50, 0, 8)], {}, "octave"), ([(50, 50, 0, -1)], {}, "octave"), ([(50, 50, np.nan, 0)], {}, "angle"),
                          ([(50, 50, 0, 0)], dict(nlevels=9), "nlevels"), ([(50, 50, 0, 0)], dict(edge=22), "edge"),
                          ([(50, 50, 0, 3)], dict(nlevels=3), "octave"), ([(50, 50, 0, 0)] * 1025, {}, "1024")):
        with pytest.raises(ValueError, match=words):
            rod.describe(img, kp, **kw)
    assert len(rod.describe(img, [(50, 50, 0, 2)], nlevels=3, edge=23)[1]) == 1
