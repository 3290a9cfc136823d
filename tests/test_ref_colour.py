"""tests/ref_colour.py against facts that need no kernel: the grey of the primaries, of white, black and every grey, the size
rule at the sizes the colour tests use, and the decimation's last row and column."""
import numpy as np

import ref_colour as rc


def test_grey_of_the_primaries_white_black_and_greys():
    px = lambda b, g, r: np.array([[[b, g, r]]], np.uint8)
    assert rc.grey_from_bgr(px(255, 0, 0))[0, 0] == 29
    assert rc.grey_from_bgr(px(0, 255, 0))[0, 0] == 150
    assert rc.grey_from_bgr(px(0, 0, 255))[0, 0] == 76
    assert rc.grey_from_bgr(px(255, 255, 255))[0, 0] == 255
    assert rc.grey_from_bgr(px(0, 0, 0))[0, 0] == 0
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(rc.grey_from_bgr(np.stack([v, v, v], -1)), v)      # the weights sum to 2^14
    assert rc.WR + rc.WG + rc.WB == 1 << 14


def test_grey_is_the_integer_formula_on_every_channel_extreme():
    vals = np.array([0, 1, 2, 127, 128, 254, 255], np.uint8)
    b, g, r = np.meshgrid(vals, vals, vals, indexing="ij")
    img = np.stack([b, g, r], -1)
    want = [[[(int(r_) * 4899 + int(g_) * 9617 + int(b_) * 1868 + 8192) >> 14 for r_ in vals] for g_ in vals] for b_ in vals]
    assert np.array_equal(rc.grey_from_bgr(img), np.array(want, np.uint8))


def test_size_rule_rounds_half_to_even():
    assert rc.cv_round_half(401) == 200 and rc.cv_round_half(403) == 202
    assert rc.cv_round_half(1241) == 620 and rc.cv_round_half(376) == 188
    assert rc.cv_round_half(121) == 60 and rc.cv_round_half(123) == 62
    assert rc.halves_to(1241, 376) == (620, 188)


def test_decimation_reads_even_rows_and_columns():
    rng = np.random.default_rng(5)
    for (sw, sh) in ((401, 121), (403, 123)):
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        w, h = rc.halves_to(sw, sh)
        grey, plane = rc.prepare(img, w, h)
        assert plane.shape == (h, w, 3) and grey.shape == (h, w)
        for (x, y) in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 3)):
            assert np.array_equal(plane[y, x], img[2 * y, 2 * x])
        assert np.array_equal(grey, rc.grey_from_bgr(plane))
        # conversion first, decimation second: the same image
        assert np.array_equal(grey, rc.decimate(rc.grey_from_bgr(img), w, h))
    # 403 x 123 rounds up: the last output column and row are the last source column and row; 401 x 121 leaves them unused
    assert 2 * (202 - 1) == 403 - 1 and 2 * (62 - 1) == 123 - 1
    assert 2 * (200 - 1) < 401 - 1 and 2 * (60 - 1) < 121 - 1
    img = rng.integers(0, 256, (53, 97, 3), dtype=np.uint8)
    grey, plane = rc.prepare(img, 97, 53)
    assert np.array_equal(plane, img)
