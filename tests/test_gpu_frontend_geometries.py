"""GPU tests: k_gftt_eig3, k_gftt_select2 and k_lk through the C ABI against the CPU oracle, bit for
bit (float outputs compared as uint32), over the frame geometries and selection paths that the
kernels' control flow depends on.  tests/test_oracle_frontend_geometries.py pins the oracle against
plain references on the same inputs; tests/ref_frontend.py holds the geometry list, the kernels'
published rules restated in Python, and the seeded scenes."""
import itertools

import numpy as np
import pytest

import ref_frontend as rf

pytestmark = pytest.mark.gpu

GEOM_IDS = ["%dx%d" % (w, h) for w, h, _ in rf.GEOMETRIES]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_corners(got, ref, tag):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.array_equal(_u32(got), _u32(ref)), (tag, np.nonzero((got != ref).any(1))[0][:5])


def test_geometry_list_covers_what_it_claims():
    ws = [g[0] for g in rf.GEOMETRIES]
    assert {w % 4 for w in ws} == {0, 1, 2, 3}                                   # k_lk's clamped staging: gxmax = (w + 12) & ~3
    assert any((w + 2 * rf.SVS_BORDER) % 16 == 0 for w in ws)                    # a pitch without slack
    res = {(w % rf.GE_COLS, h % rf.GE_ROWS) for w, h, _ in rf.GEOMETRIES}
    assert {(0, 0), (1, 1), (2, 2), (rf.GE_COLS - 1, rf.GE_ROWS - 1)} <= res
    assert {rf.nlevels(w, h) for w, h, _ in rf.GEOMETRIES} >= {1, 3, 4}
    assert min(ws) == 16 and (512, 256) in [(w, h) for w, h, _ in rf.GEOMETRIES]


# ---------------------------------------------------------------------------- a. eigenvalue map and corners
@pytest.mark.parametrize("geom", rf.GEOMETRIES, ids=GEOM_IDS)
def test_eigmap_and_corners_on_geometry(svs, orc, geom):
    w, h, why = geom
    rng = np.random.default_rng(1000 + 7 * w + h)
    imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8), rf.cm.textured(rng, h, w)]
    rect = rf.seam_rects(rng, w, h)
    assert len(rect) >= 60
    c = svs.Context(w, h, max_slots=2, max_jobs=4, max_pts=512, max_corners=150, max_kf=0, max_lm=0, max_obs=0)
    try:
        c.pyramid([0, 1], imgs)
        for slot, img in enumerate(imgs):
            e = c.gftt_eigmap(slot)
            e_ref = orc.min_eig_map(img)
            bad = np.argwhere(_u32(e) != _u32(e_ref))
            assert len(bad) == 0, (why, slot, len(bad), bad[:6].tolist())        # (y, x) of the first differing pixels
        got = c.gftt([(0, None), (1, None), (0, rect), (1, rect)])
        for k, (img, r) in enumerate(((imgs[0], None), (imgs[1], None), (imgs[0], rect), (imgs[1], rect))):
            _same_corners(got[k], orc.gftt(img, r), (why, k))
        if w >= 58:
            assert len(got[0]) > 0 and len(got[2]) > 0
    finally:
        c.close()


# ---------------------------------------------------------------------------- b. selection paths
def _selection_cases():
    straddles = rf.straddling_min_dists()
    mds = rf.MIN_DISTS + [s[0] for s in straddles]
    return straddles, list(itertools.product(mds, rf.MAX_CORNERS, rf.QUALITIES))


def _dense(mc, q):
    """the cases on which the accepted corners must be dense enough for the search to meet neighbours"""
    return mc == 1024 and q == 0.0005


def test_selection_cases_cover_every_path():
    """from the kernel's own rule (rf.selection_path): what the case list of test_selection_paths reaches"""
    straddles, cases = _selection_cases()
    assert len(straddles) >= 4 and straddles[-1][0] > rf.BITMAP_MAX_DIST
    for md, k, _ in straddles:
        assert md * md > k and np.float32(md * md) == np.float32(k)
    count = {"bitmap": 0, "grid": 0, "list": 0, "none": 0}
    dense_grid = beyond31 = 0
    for (w, h) in rf.SELECTION_GEOMETRIES:
        for md, mc, q in cases:
            p = rf.selection_path(w, h, md)
            count[p] += 1
            dense_grid += p == "grid" and _dense(mc, q)
            beyond31 += md > rf.BITMAP_MAX_DIST and ((w + 31) >> 5) * h <= rf.GF_BITMAP_WORDS
    assert count["bitmap"] >= 4 and count["list"] >= 2 and beyond31 >= 2 and count["none"] >= 2
    assert dense_grid >= 6           # grid cases whose corner density test_selection_paths asserts
    # both sides of the bitmap's size limit
    assert rf.selection_path(512, 256, 20) == "bitmap" and rf.selection_path(512, 257, 20) == "grid"


@pytest.mark.parametrize("wh", rf.SELECTION_GEOMETRIES, ids=["%dx%d" % g for g in rf.SELECTION_GEOMETRIES])
def test_selection_paths(svs, orc, wh):
    """the parameter grid against the oracle on the bitmap path, the cell grid, the full-list fallback (too
    many cells) and min_dist > 31, every call twice in a row (the second finds the counters the first left).

    gf_greedy's grid_ok = false overflow (a fourth corner in one cell) is not constructed: the pixel centres
    of a cell lie in a square of side cvRound(md) - 1 <= md - 0.5, and of any four points in a square two
    are no farther apart than its side (the best spread of four points is the four corners), i.e. closer
    than md; three do fit in a large cell, which is why the kernel keeps three slots."""
    w, h = wh
    straddles, cases = _selection_cases()
    rng = np.random.default_rng(2000 + w + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)              # ~ one local maximum per 10 pixels: several slices
    textured = rf.cm.textured(rng, h, w)
    lattice = rf.lattice_image(w, h)                                  # equal values: the global-memory bitonic fallback
    scene, pairs = rf.straddle_scene(rng, w, h, straddles)
    imgs = [noise, textured, lattice, scene]
    rect = rf.seam_rects(rng, w, h)
    c = svs.Context(w, h, max_slots=4, max_jobs=4, max_pts=512, max_corners=1024, max_kf=0, max_lm=0, max_obs=0)
    has = lambda r, p: bool((r == np.array(p, np.float32)).all(1).any())
    try:
        c.pyramid([0, 1, 2, 3], imgs)
        for md, mc, q in cases:
            jobs = [(0, None), (0, rect)]
            if mc == 1024:
                jobs += [(1, None), (3, None)]
            ref = [orc.gftt(imgs[s], r, mc, q, md) for s, r in jobs]
            for rep in range(2):
                got = c.gftt(jobs, max_corners=mc, quality=q, min_dist=md)
                for k in range(len(jobs)):
                    _same_corners(got[k], ref[k], (w, h, md, mc, q, "job", k, "rep", rep))
            if rf.selection_path(w, h, md) == "grid" and _dense(mc, q):
                # otherwise the 3x3 cell search never meets a neighbour
                assert rf.grid_density(ref[0], md) > 3, (w, h, md, rf.grid_density(ref[0], md))
        # each straddling value decides its pair: the later corner is dropped (on the oracle, hence on the GPU)
        for (md, k, _), (a, b) in zip(straddles, pairs):
            r = orc.gftt(scene, None, 1024, 0.01, md)
            assert has(r, a) and not has(r, b), (w, h, k)
        # identical corners everywhere: one histogram bin holds everything
        for (mc, q, md) in ((1024, 0.01, 20.0), (1024, 0.0001, 2.0), (150, 0.01, 40.0), (1000, 0.5, 1.0), (1024, 0.01, 0.0)):
            for rep in range(2):
                got = c.gftt([(2, None), (2, rect)], max_corners=mc, quality=q, min_dist=md)
                _same_corners(got[0], orc.gftt(lattice, None, mc, q, md), (w, h, "lattice", mc, q, md, rep))
                _same_corners(got[1], orc.gftt(lattice, rect, mc, q, md), (w, h, "lattice, mask", mc, q, md, rep))
        # the eig-map hook leaves the counters clean as well
        assert np.array_equal(_u32(c.gftt_eigmap(0)), _u32(orc.min_eig_map(noise)))
        (g,) = c.gftt([(0, None)], max_corners=150)
        _same_corners(g, orc.gftt(noise), (w, h, "after eigmap"))
    finally:
        c.close()


# ---------------------------------------------------------------------------- c. LK
def _same_lk(got, ref, tag):
    (q, st, err), (q_ref, st_ref, err_ref) = got, ref
    assert np.array_equal(st, st_ref), (tag, "status", np.nonzero(st != st_ref)[0][:8])
    bad = np.nonzero((_u32(q) != _u32(q_ref)).any(1))[0]
    assert len(bad) == 0, (tag, "position", len(bad), bad[:8], q[bad[:3]], q_ref[bad[:3]])
    assert np.array_equal(_u32(err), _u32(err_ref)), (tag, "err")


@pytest.mark.parametrize("geom", rf.GEOMETRIES, ids=GEOM_IDS)
def test_lk_on_geometry(svs, orc, geom):
    w, h, why = geom
    nl = rf.nlevels(w, h)
    rng = np.random.default_rng(3000 + 7 * w + h)
    I, J = rf.warp_pair(rng, w, h)
    assert len(orc.pyramid(I)) == nl
    c = svs.Context(w, h, max_slots=6, max_jobs=6, max_pts=512, max_kf=0, max_lm=0, max_obs=0)
    try:
        scenes = [rf.restage_scene(w, h, shift) for shift in rf.RESTAGE_SHIFTS]
        c.pyramid([0, 1, 2, 3, 4, 5], [I, J, scenes[0][0], scenes[0][1], scenes[1][0], scenes[1][1]])
        # (i) points over the whole range and on the status thresholds of every level, default parameters
        p, g = rf.lk_full_range_points(rng, w, h)
        assert len(p) == 400 + 80 * nl
        (got,) = c.lk([(0, 1, p, g)])
        ref = orc.lk(I, J, p, g)
        _same_lk(got, ref, (why, "full range"))
        if w >= 58:
            assert 0 < ref[1].sum() < len(p)
        # (ii) the level clamp (max_level = 3 on a shorter pyramid), without initial flow; and fewer levels than there are
        for ml in sorted({3, 7, max(nl - 2, 0)}):
            prm = (ml, 30, 0.01, 1e-4, 0)
            (got,) = c.lk([(0, 1, p, g)], params=svs.LkParams(*prm))
            _same_lk(got, orc.lk(I, J, p, g, params=orc.lk_params(*prm)), (why, "max_level", ml))
        # (iii) level 0 alone, windows walking 14-24 px: the 32x32 J region is staged again on the way
        prm = (0, 30, 0.01, 1e-4, 1)
        n_far = 0
        for k, (Ir, Jr, pr) in enumerate(scenes):
            ref = orc.lk(Ir, Jr, pr, pr, params=orc.lk_params(*prm))
            n_far += int(rf.restaged(ref[0], ref[1], pr).sum())
            (got,) = c.lk([(2 + 2 * k, 3 + 2 * k, pr, pr)], params=svs.LkParams(*prm))
            _same_lk(got, ref, (why, "restage", rf.RESTAGE_SHIFTS[k]))
        if min(w, h) > 16:               # a 32-wide region around any guess covers most of a 16x16 image
            assert n_far >= 16, (why, n_far)
    finally:
        c.close()


def test_lk_batched_point_counts(svs, orc):
    """one call, jobs of 0, 1, 63, 64, 65 and 512 points (around the wave size; the grid is sized by the largest)"""
    w, h = 613, 185
    rng = np.random.default_rng(4000)
    I, J = rf.warp_pair(rng, w, h)
    I2, J2, _ = rf.restage_scene(w, h, rf.RESTAGE_SHIFTS[0])
    c = svs.Context(w, h, max_slots=4, max_jobs=8, max_pts=512, max_kf=0, max_lm=0, max_obs=0)
    try:
        c.pyramid([0, 1, 2, 3], [I, J, I2, J2])
        jobs, refs = [], []
        for k, n in enumerate((65, 0, 512, 1, 64, 63)):
            p = np.stack([rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n)], 1).astype(np.float32).reshape(-1, 2)
            g = p + rng.normal(0, 3, p.shape).astype(np.float32)
            a, b, A, B = (0, 1, I, J) if k % 2 == 0 else (2, 3, I2, J2)
            jobs.append((a, b, p, g))
            refs.append(orc.lk(A, B, p, g))
        got = c.lk(jobs)
        for k, (gk, rk) in enumerate(zip(got, refs)):
            assert gk[0].shape == rk[0].shape
            if len(rk[0]):
                _same_lk(gk, rk, ("batched job", k))
    finally:
        c.close()
