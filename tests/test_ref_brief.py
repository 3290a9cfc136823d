"""tests/ref_brief.py held to facts it does not use itself: the taps, the blur against a direct 2-D integer convolution, the rotation
at angles whose result is known, the bit layout, and the properties of the default table."""
import numpy as np

import ref_brief as rb


def test_taps_sum_to_256_and_are_the_rounded_gaussian():
    assert int(rb.TAPS.sum()) == 256
    g = np.exp(-(np.arange(7) - 3.0) ** 2 / 8.0); g = 256.0 * g / g.sum()
    assert np.abs(rb.TAPS - g)[[0, 1, 2, 4, 5, 6]].max() <= 0.5           # the side taps are nearest integers
    assert abs(rb.TAPS[3] - g[3]) < 1.5 and tuple(rb.TAPS) == tuple(rb.TAPS[::-1])


def test_a_constant_image_blurs_to_itself():
    for v in (0, 1, 254, 255):
        assert (rb.blur(np.full((20, 23), v, np.uint8)) == v).all()


def test_blur_equals_the_direct_2d_convolution():
    rng = np.random.default_rng(3)
    im = rng.integers(0, 256, (31, 40), dtype=np.uint8)
    k2 = np.outer(rb.TAPS, rb.TAPS).astype(np.int64)
    assert k2.sum() == 65536
    want = np.zeros((25, 34), np.int64)
    for y in range(25):
        for x in range(34):
            want[y, x] = (int((k2 * im[y:y + 7, x:x + 7].astype(np.int64)).sum()) + 32768) >> 16
    assert np.array_equal(rb.blur(im), want)


def test_rotations_with_known_results():
    p = rb.default_pattern()
    pts = p.reshape(512, 2).astype(np.int64)
    assert np.array_equal(rb.offsets(p, 0.0), pts)
    assert np.array_equal(rb.offsets(p, -1.0), pts)          # |c| <= 13: a degree moves a coordinate by 0.23 at the most
    assert np.array_equal(rb.offsets(p, 90.0), np.stack([-pts[:, 1], pts[:, 0]], axis=1))
    assert np.array_equal(rb.offsets(p, 180.0), -pts)


def test_default_table_properties():
    p = rb.default_pattern()
    assert p.shape == (256, 4) and p.dtype == np.int8
    assert np.abs(p).max() <= 13
    assert len({tuple(r) for r in p.tolist()}) == 256
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()
    assert np.array_equal(p, rb.default_pattern())


def test_a_constant_image_gives_zero_descriptors():
    d, idx = rb.describe(np.full((80, 90), 77, np.uint8), [(40, 40), (45.5, 41), (2, 2)])
    assert d.shape == (2, 32) and not d.any() and idx.tolist() == [0, 1]


def test_bit_layout_is_little_endian_within_a_byte():
    rng = np.random.default_rng(5)
    im = rng.integers(0, 256, (80, 90), dtype=np.uint8)
    (d,), _ = rb.describe(im, [(44.0, 39.0)])
    B = rb.blur(im).astype(np.int64)
    off = rb.offsets(rb.default_pattern(), -1.0).reshape(256, 2, 2)
    bits = np.array([B[39 + o[0][1] - 3, 44 + o[0][0] - 3] < B[39 + o[1][1] - 3, 44 + o[1][0] - 3] for o in off])
    assert 40 < bits.sum() < 216                                         # a random image decides both ways
    assert np.array_equal(d, np.packbits(bits, bitorder="little"))


def test_filter_bounds_and_rounding():
    im = np.random.default_rng(6).integers(0, 256, (72, 96), dtype=np.uint8)
    pts = [(30.99, 35), (31, 35), (96 - 31 - 0.01, 35), (96 - 31, 35), (35, 30.99), (35, 31), (35, 72 - 31 - 0.01), (35, 72 - 31)]
    d, idx = rb.describe(im, pts)
    assert idx.tolist() == [1, 2, 5, 6]
    (a, b, c, e), _ = rb.describe(im, [(40.5, 35), (40, 35), (41.5, 35), (42, 35)])
    assert np.array_equal(a, b) and np.array_equal(c, e) and not np.array_equal(a, c)


def test_refusals():
    import pytest
    im = np.zeros((72, 96), np.uint8)
    with pytest.raises(ValueError, match="1024"):
        rb.describe(im, np.full((1025, 2), 35.0))
    with pytest.raises(ValueError, match="edge"):
        rb.describe(im, [(35, 35)], edge=16)
    rb.describe(im, [(35, 35)], edge=17)
    p = np.array(rb.default_pattern()); p[9, 2:] = p[9, :2]
    with pytest.raises(ValueError, match="coincide"):
        rb.describe(im, [(35, 35)], pattern=p)
