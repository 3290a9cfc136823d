"""CPU tests: the oracle's GFTT and LK against the plain references of tests/ref_frontend.py on the
frame geometries and selection parameters on which tests/test_gpu_frontend_geometries.py then holds
the HIP kernels to the oracle bit for bit.  Every comparison is exact but the one inherited LK bound."""
import itertools

import numpy as np

import ref_frontend as rf


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_geometry_list_covers_what_it_claims():
    ws = [g[0] for g in rf.GEOMETRIES]
    assert {w % 4 for w in ws} == {0, 1, 2, 3}                                   # k_lk's clamped staging: gxmax = (w + 12) & ~3
    assert any((w + 2 * rf.SVS_BORDER) % 16 == 0 for w in ws)                    # a pitch without slack
    res = {(w % rf.GE_COLS, h % rf.GE_ROWS) for w, h, _ in rf.GEOMETRIES}
    assert {(0, 0), (1, 1), (2, 2), (rf.GE_COLS - 1, rf.GE_ROWS - 1)} <= res     # last strips of 1, 2, all-but-one, no columns / rows
    assert {rf.nlevels(w, h) for w, h, _ in rf.GEOMETRIES} >= {1, 3, 4}     # LK level clamp: pyramids shorter than max_level + 1
    assert rf.selection_path(512, 256, 20) == "bitmap" and rf.selection_path(512, 257, 20) == "grid"
    assert rf.selection_path(512, 256, 31.5) == "grid" and rf.selection_path(640, 480, 7.4) == "list"


def test_min_eig_map_bit_exact_on_every_geometry(orc):
    rng = np.random.default_rng(100)
    for w, h, why in rf.GEOMETRIES:
        for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), rf.cm.textured(rng, h, w)):
            e = orc.min_eig_map(img)
            r = rf._eig_numpy(img)
            assert r.dtype == np.float32
            assert np.array_equal(_u32(e), _u32(r)), (w, h, why, np.abs(e - r).max())


def _grid(straddles):
    mds = rf.MIN_DISTS + [s[0] for s in straddles]
    return list(itertools.product(mds, rf.MAX_CORNERS, rf.QUALITIES))


def _check_gftt(orc, img, rect, cases, tag):
    eig = orc.min_eig_map(img)
    h, w = img.shape
    mask = orc.gftt_mask(w, h, rect) if rect is not None else np.full((h, w), 255, np.uint8)
    for md, mc, q in cases:
        got = orc.gftt(img, rect, mc, q, md)
        ref = rf._greedy_python(eig, mask, mc, q, md)
        assert got.shape == ref.shape, (tag, md, mc, q, got.shape, ref.shape)
        assert np.array_equal(got, ref), (tag, md, mc, q)


def test_gftt_matches_plain_selection_over_the_parameter_grid(orc):
    """the whole grid (min_dist x max_corners x quality, straddling values included), with and without
    mask rectangles on strip seams and image corners, on an odd small geometry and on config 3's"""
    straddles = rf.straddling_min_dists()
    assert len(straddles) >= 4
    cases = _grid(straddles)
    rng = np.random.default_rng(101)
    for (w, h) in ((117, 97), (613, 185)):
        imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8)]
        if w < 200:
            imgs.append(rf.cm.textured(rng, h, w))
        rect = rf.seam_rects(rng, w, h)
        for k, img in enumerate(imgs):
            _check_gftt(orc, img, None, cases, (w, h, k, "no mask"))
            _check_gftt(orc, img, rect, cases, (w, h, k, "mask"))


def test_gftt_matches_plain_selection_on_the_large_geometries(orc):
    """640x480 and 1241x376 (where the GPU's cell grid and its full-list fallback run): a thinned grid,
    the vectorised candidate search keeps the reference in seconds"""
    straddles = rf.straddling_min_dists()
    cases = [(0, 1024, 0.01), (1.0, 1024, 0.0005), (2.5, 1024, 0.0005), (7.4, 150, 0.01), (20, 1024, 0.0005),
             (31.5, 1024, 0.0005), (40, 1024, 0.01), (40, 1, 0.01), (straddles[0][0], 1024, 0.0005), (straddles[-1][0], 150, 0.0005)]
    rng = np.random.default_rng(102)
    for (w, h) in ((640, 480), (1241, 376)):
        noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
        rect = rf.seam_rects(rng, w, h)
        _check_gftt(orc, noise, None, cases, (w, h, "noise"))
        _check_gftt(orc, noise, rect, cases[3:7], (w, h, "noise, mask"))
        _check_gftt(orc, rf.lattice_image(w, h), None, cases[4:6], (w, h, "lattice"))
        img, _ = rf.straddle_scene(rng, w, h, straddles)
        _check_gftt(orc, img, None, [(s[0], 1024, 0.01) for s in straddles], (w, h, "straddle scene"))


def test_straddling_min_dist_decides_a_pair_in_double(orc):
    """min_dist = sqrt(k) whose double square is just above k and whose float square IS k: the later of
    two corners at squared distance exactly k is dropped (k < min_dist^2 in double, as in OpenCV's
    `minDistance *= minDistance` on a double — recalled, not pinned).  An oracle that rounds the square
    to float keeps it."""
    straddles = rf.straddling_min_dists()
    assert len(straddles) >= 4 and straddles[-1][0] > rf.BITMAP_MAX_DIST
    rng = np.random.default_rng(103)
    w, h = 620, 188
    img, pairs = rf.straddle_scene(rng, w, h, straddles)
    eig = orc.min_eig_map(img)
    mask = np.full((h, w), 255, np.uint8)
    cand = rf._candidates(eig, mask, 0.01).tolist()
    has = lambda r, p: bool((r == np.array(p, np.float32)).all(1).any())
    for (md, k, (dx, dy)), (a, b) in zip(straddles, pairs):
        assert md * md > k and np.float32(md * md) == np.float32(k)
        assert (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2 == k
        assert list(a) in cand and list(b) in cand and cand.index(list(a)) < cand.index(list(b))
        below = md
        while below * below > k:                       # the neighbouring double whose square does not exceed k
            below = float(np.nextafter(below, 0.0))
        ref = rf._greedy_python(eig, mask, 1024, 0.01, md)
        ref_below = rf._greedy_python(eig, mask, 1024, 0.01, below)
        assert has(ref, a) and not has(ref, b), k      # the pair decides: the later corner is dropped ...
        assert has(ref_below, a) and has(ref_below, b), k   # ... and would have been accepted one ulp below
        got = orc.gftt(img, None, 1024, 0.01, md)
        assert np.array_equal(got, ref), k
        assert np.array_equal(orc.gftt(img, None, 1024, 0.01, below), ref_below), k


def _check_lk_level0(orc, I, J, pts, guess, tag):
    q, st, _ = orc.lk(I, J, pts, guess, params=orc.lk_params(max_level=0))
    q_ref, st_ref = rf._ref_lk_single_level(I, J, pts, guess)
    assert np.array_equal(st, st_ref), (tag, np.nonzero(st != st_ref)[0])
    ok = st > 0
    assert ok.sum() >= 30, tag
    # the criterion of test_lk_level0_matches_independent_numpy: the only declared deviation (exact
    # integer sums vs float accumulation) is far below this
    assert np.abs(q[ok] - q_ref[ok]).max() < 2e-3, tag
    return q, st


def test_lk_level0_matches_numpy_on_large_flow_and_odd_geometries(orc):
    # the re-staging scene: windows walk 14-24 px at level 0
    n_far = 0
    for shift in rf.RESTAGE_SHIFTS:
        I, J, p = rf.restage_scene(117, 97, shift, n=80)
        q, st = _check_lk_level0(orc, I, J, p, p, ("restage", shift))
        n_far += int(rf.restaged(q, st, p).sum())
    assert n_far >= 16
    # two odd geometries (w mod 4 = 3 and 1), points over the whole range incl. the status thresholds
    for (w, h) in ((59, 49), (613, 185)):
        rng = np.random.default_rng(104 + w)
        I, J = rf.warp_pair(rng, w, h)
        p, g = rf.lk_full_range_points(rng, w, h, n=60)
        _check_lk_level0(orc, I, J, p, g, (w, h))


def test_restaging_scene_leaves_the_staged_region_on_every_geometry(orc):
    """the seed and sigma of ref_frontend.restage_scene are chosen so that, on the oracle's result alone,
    at least 16 tracked points end more than a region away from their guess (the GPU test asserts the same
    before it compares).  16x16 is exempt: a 32-wide region around any guess covers most of that image."""
    prm = orc.lk_params(max_level=0, max_iter=30, use_initial_flow=1)
    for w, h, _ in rf.GEOMETRIES:
        n = 0
        for shift in rf.RESTAGE_SHIFTS:
            I, J, p = rf.restage_scene(w, h, shift)
            q, st, _ = orc.lk(I, J, p, p, params=prm)
            n += int(rf.restaged(q, st, p).sum())
        if min(w, h) > 16:
            assert n >= 16, (w, h, n)
