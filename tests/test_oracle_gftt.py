"""CPU tests pinning the oracle's GFTT against an independent numpy float32 computation
of the declared operation order, and against the defining properties of the detector."""
import numpy as np

import common as cm
from ref_frontend import _eig_numpy, _greedy_python


def test_min_eig_map_bit_exact_vs_numpy(orc):
    rng = np.random.default_rng(0)
    for (h, w) in ((48, 64), (188, 620), (17, 23)):
        img = cm.textured(rng, h, w) if h > 20 else rng.integers(0, 256, (h, w), dtype=np.uint8)
        e = orc.min_eig_map(img)
        r = _eig_numpy(img)
        assert r.dtype == np.float32
        assert np.array_equal(e.view(np.uint32), r.view(np.uint32)), np.abs(e - r).max()


def test_mask_rounding_half_even_inclusive_clipped(orc):
    m = orc.gftt_mask(64, 48, np.array([[20.5, 10.5], [0.0, 0.0], [63.0, 47.0], [-30, -30]], np.float32))
    # 20.5-10 = 10.5 -> 10 (half to even), 20.5+10 = 30.5 -> 30 ; 10.5-10 = 0.5 -> 0 ; 10.5+10 = 20.5 -> 20
    assert m[0:21, 10:31].max() == 0 and m[21, 20] == 255 and m[10, 31] == 255 and m[10, 9] == 0
    assert m[0:11, 0:11].max() == 0            # clipped square around (0,0): [-10,10] -> [0,10]
    assert m[37:48, 53:64].max() == 0
    assert m[30, 40] == 255


def test_gftt_matches_python_selection(orc):
    rng = np.random.default_rng(3)
    img = cm.textured(rng, 60, 90)
    eig = orc.min_eig_map(img)
    rect = np.array([[30.2, 20.7], [70.5, 40.5]], np.float32)
    mask = orc.gftt_mask(90, 60, rect)
    for (mc, q, md) in ((40, 0.01, 8.0), (500, 0.002, 3.0), (25, 0.05, 12.0), (60, 0.01, 0.0)):
        got = orc.gftt(img, rect, mc, q, md)
        ref = _greedy_python(eig, mask, mc, q, md)
        assert np.array_equal(got, ref), (mc, q, md)


def test_gftt_properties_on_kitti_shaped_frame(orc, svs):
    l0, _ = svs.synth_pair(11, 0)
    c = orc.gftt(l0)
    assert len(c) == 150                                     # textured frame: the cap binds
    assert np.array_equal(c, np.rint(c))                     # integer pixel coordinates
    assert c[:, 0].min() >= 1 and c[:, 0].max() <= 618 and c[:, 1].min() >= 1 and c[:, 1].max() <= 186
    d = np.linalg.norm(c[:, None] - c[None], axis=2) + 1e9 * np.eye(len(c))
    assert d.min() >= 20.0
    e = orc.min_eig_map(l0)
    q = e[c[:, 1].astype(int), c[:, 0].astype(int)]
    assert np.all(np.diff(q) <= 0)                           # quality-descending
    # masked detection never returns a corner inside an exclusion square
    c2 = orc.gftt(l0, c[:50])
    m = orc.gftt_mask(620, 188, c[:50])
    assert m[c2[:, 1].astype(int), c2[:, 0].astype(int)].min() == 255
    # flat image: nothing
    assert len(orc.gftt(np.full((188, 620), 50, np.uint8))) == 0
