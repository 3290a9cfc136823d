"""The numpy restatement of cv::StereoBM (tests/ref_stereo_bm.py) against geometry and hand-checkable inputs.  It is
the yardstick of the HIP block matcher (tests/test_gpu_stereo_bm.py); OpenCV itself is not available, so these are
the checks that an inverted tie rule, a swapped sub-pixel sign or a shifted window would not pass."""
import numpy as np
import pytest

import ref_stereo_bm as rbm

XL, XR, YT, YB = -6.0, 6.5, -4.0, 1.65                   # the tunnel planes of csrc/synth_scene.h


def _true_disparity(svs, seed, frame, w, h):
    """fx B / depth of the left view's ray-cast (svs_synth_pixel's intersection, in float64)"""
    vl, _ = svs.synth_views(seed, frame)
    R = np.array(list(vl.R), np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xc, yc = (xs - vl.cx) / vl.fx, (ys - vl.cy) / vl.fy
    dx = R[0, 0] * xc + R[0, 1] * yc + R[0, 2]
    dy = R[1, 0] * xc + R[1, 1] * yc + R[1, 2]
    Cx, Cy = vl.C[0], vl.C[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.full((h, w), 1e9)
        for num, den, ok in (((XR - Cx), dx, dx > 1e-6), ((XL - Cx), dx, dx < -1e-6), ((YB - Cy), dy, dy > 1e-6),
                             ((YT - Cy), dy, dy < -1e-6)):
            t = np.where(ok, np.minimum(t, num / np.where(ok, den, 1.0)), t)
    # the ray is (xc, yc, 1) in the camera frame: its parameter is the depth
    return svs.KITTI00_HALF_CAM[0] * svs.KITTI00_BASELINE / t


@pytest.mark.parametrize("seed,frame", [(1, 0), (7, 33)])
def test_restatement_recovers_the_synthetic_scene(svs, seed, frame):
    w, h = 620, 188
    left, right = svs.synth_pair(seed, frame, w=w, h=h)
    disp = rbm.stereo_bm(left, right)
    nd, r = 128, 7
    region = disp[r:h - r, nd - 1 + r:w - r].astype(np.float64) / 16.0
    truth = _true_disparity(svs, seed, frame, w, h)[r:h - r, nd - 1 + r:w - r]
    assert (disp[:r] == -16).all() and (disp[h - r:] == -16).all() and (disp[:, :nd - 1 + r] == -16).all() and (disp[:, w - r:] == -16).all()
    valid = region > 0
    within = np.abs(region - truth)[valid] <= 1.0
    print("seed %d frame %d: valid %.2f %%, within 1 px %.2f %%" % (seed, frame, 100 * valid.mean(), 100 * within.mean()))
    assert valid.mean() >= 0.80
    assert within.mean() >= 0.95


def hand_pairs():
    """the three hand-checkable pairs, shared with the GPU test: name -> (left, right, params, expected values of the region)

    shift5: the integer disparity is 5 at every pixel of the region.  The 16 x value is 80 only up to the sub-pixel term:
    SAD(5) = 0 makes it (p - n) * 128 / max(p, n) in 1/256 px, and p - n is the difference of the window's two boundary
    columns (p and n are the same sum of |L'(c) - L'(c+1)| shifted by one column) — 2 x 9 terms against the 81 of p, a few
    percent of p on random texture — and the window that touches column w-1 sees the prefilter's cap column, so SAD(5) is
    not even 0 there.  The faithful algorithm therefore gives 80 or 81 at most pixels, never "80 everywhere".  Required at
    EVERY pixel: [79, 82], which is ((1280 + t + 15) >> 4 with) |t| <= 32, i.e. |p - n| <= max(p, n) / 4: a boundary-column
    difference of a quarter of the whole window sum does not happen on this texture, a sub-pixel term of the wrong scale
    or a wrong integer disparity leaves the band."""
    rng = np.random.default_rng(5)
    h, w, nd, bs = 40, 120, 32, 9
    # a point at left column x appears at right column x - 5: right[x - 5] = left[x]
    wide = rng.integers(0, 256, (h, w + 5), dtype=np.uint8)
    left, right = wide[:, :w].copy(), wide[:, 5:].copy()
    prm = dict(num_disparities=nd, block_size=bs)
    const = np.full((h, w), 93, np.uint8)
    # period 8, rows differ.  The prefilter forces columns 0 and w-1 to cap; with w = 121 both are columns = 0 (mod 8), whose
    # neighbours (entries 1 and 7) are equal, so cap is also what the periodic continuation gives there: SAD(d) = SAD(d + 8)
    # holds exactly at every pixel of the region, the last column included
    per = np.tile(np.array([10, 200, 40, 250, 90, 20, 160, 200], np.uint8), (h, 16))[:, :121].copy()
    per = (per.astype(np.int32) + (np.arange(h)[:, None] * 37) % 50).clip(0, 255).astype(np.uint8)
    return {"shift5": (left, right, prm, (79, 82)), "constant": (const, const.copy(), prm, (-16, -16)),
            "period8": (per, per.copy(), prm, (-16, -16))}


@pytest.mark.parametrize("name", ["shift5", "constant", "period8"])
def test_hand_checkable_pairs(name):
    left, right, prm, want = hand_pairs()[name]
    h, w = left.shape
    nd, r = prm["num_disparities"], prm["block_size"] // 2
    disp = rbm.stereo_bm(left, right, **prm)
    region = disp[r:h - r, nd - 1 + r:w - r]
    assert region.size > 0 and (region >= want[0]).all() and (region <= want[1]).all(), (name, np.unique(region))
    outside = np.ones((h, w), bool); outside[r:h - r, nd - 1 + r:w - r] = False
    assert (disp[outside] == -16).all()


def half_pixel_pair():
    """right = the left shifted by 5.5 px (the mean of the 5 px and the 6 px shift) on a texture smooth enough for that mean to be
    the half-pixel sample: (left, right, params)"""
    rng = np.random.default_rng(9)
    h, w, nd, bs, k = 40, 120, 32, 9, 3
    t = rng.random((h + k - 1, w + 6 + k - 1))
    t = sum(t[i:i + h] for i in range(k))                                 # 3 x 3 box
    t = sum(t[:, i:i + w + 6] for i in range(k))
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    left = np.rint(t[:, :w]).astype(np.uint8)
    right = np.rint(0.5 * (t[:, 5:5 + w] + t[:, 6:6 + w])).astype(np.uint8)
    return left, right, dict(num_disparities=nd, block_size=bs)


def test_half_pixel_shift_pins_the_sign_of_the_subpixel_term():
    """Disparity 5.5 is 88.  SAD(5) ~ SAD(6), so the arg-min is 5 or 6 and the sub-pixel term must move it half a pixel TOWARDS the
    other: a swapped sign gives 72 (from 5) or 104 (from 6), no sub-pixel term 80 or 96.  Required: 95 % of the region valid and
    95 % of the valid pixels within a quarter pixel of 88, [84, 92].  OpenCV's V-shaped fit is not exact on a texture that is only
    approximately linear between samples, and a smooth texture has the odd false match, hence neither "every pixel" nor a
    narrower band; a quarter pixel is half the distance to an integer-only result and a quarter of the distance to the swapped
    sign's, which would both leave the band empty."""
    left, right, prm = half_pixel_pair()
    h, w = left.shape
    nd, r = prm["num_disparities"], prm["block_size"] // 2
    region = rbm.stereo_bm(left, right, **prm)[r:h - r, nd - 1 + r:w - r]
    valid = region[region != -16]
    print("half pixel: valid %.2f %%, values %s" % (100.0 * valid.size / region.size, dict(zip(*np.unique(valid, return_counts=True)))))
    assert valid.size >= 0.95 * region.size
    assert ((valid >= 84) & (valid <= 92)).mean() >= 0.95


def test_prefilter_edges_and_odd_height():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (9, 20), dtype=np.uint8)
    pf = rbm.prefilter_xsobel(img, 31)
    assert (pf[-1] == 31).all()                                 # odd height: the unpaired last row
    assert (pf[:, 0] == 31).all() and (pf[:, -1] == 31).all()
    a = img.astype(np.int32)
    dx = lambda y, x: a[y, x + 1] - a[y, x - 1]
    assert pf[0, 5] == np.clip(dx(1, 5) + 2 * dx(0, 5) + dx(1, 5), -31, 31) + 31          # row -1 -> row 1
    assert pf[4, 7] == np.clip(dx(3, 7) + 2 * dx(4, 7) + dx(5, 7), -31, 31) + 31
    even = rbm.prefilter_xsobel(img[:8], 31)
    b = img[:8].astype(np.int32)
    dxb = lambda y, x: b[y, x + 1] - b[y, x - 1]
    assert even[7, 3] == np.clip(dxb(6, 3) + 2 * dxb(7, 3) + dxb(6, 3), -31, 31) + 31     # row h -> row h-2
    sat = rbm.prefilter_xsobel(np.tile(np.array([0, 0, 255, 255], np.uint8), (6, 4)), 31)
    assert set(np.unique(sat[:, 1:-1])) == {0, 62}                # saturates at -cap and +cap


def test_too_narrow_image_is_all_filtered():
    rng = np.random.default_rng(3)
    nd, bs = 32, 9
    w = nd + 2 * (bs // 2) - 1
    img = rng.integers(0, 256, (30, w), dtype=np.uint8)
    assert (rbm.stereo_bm(img, img, num_disparities=nd, block_size=bs) == -16).all()
    assert (rbm.stereo_bm(img[:8], img[:8], num_disparities=16, block_size=9) == -16).all()      # h < 2r + 1
    one = rbm.stereo_bm(np.hstack([img, img[:, :1]]), np.hstack([img, img[:, :1]]), num_disparities=nd, block_size=bs)
    assert one.shape == (30, w + 1)                              # one column wider: a computed column exists


def test_cloud_order_and_gate():
    disp = np.full((4, 5), -16, np.int16)
    disp[1, 3] = 16 * 10; disp[3, 1] = 16 * 20; disp[0, 3] = 16 * 5; disp[2, 2] = 0
    disp[2, 4] = 32767                                          # depth = fx B / 2047.9 < 1: dropped
    cam = (359.428, 359.428, 303.5964, 92.60785)
    xyz, pix = rbm.dense_cloud(disp, cam, [0, 0, 0, 1, 0, 0, 0], 0.537166, [0, 0, 0, 1, 0, 0, 0])
    assert pix.tolist() == [3 * 5 + 1, 0 * 5 + 3, 1 * 5 + 3]    # x outer, y inner
    z = np.float32(np.float32(cam[0]) * np.float32(0.537166)) / np.float32(20.0)
    assert xyz[0, 2] == z and xyz.dtype == np.float32


# ---- inputs built for a purpose, shared with the GPU sweep (tests/test_gpu_stereo_bm.py) ------------------------------------
def band_pair(w, h, nd, seed=21):
    """four horizontal bands of random texture with exact integer shifts, one per quarter of [0, nd): 2 (next to the
    SAD(-1) := SAD(1) end), the last disparity of quarter 1, the first of quarter 2, and nd - 1 (the SAD(nd) := SAD(nd - 2) end)"""
    rng = np.random.default_rng(seed)
    dq = nd // 4
    wide = rng.integers(0, 256, (h, w + nd), dtype=np.uint8)
    left, right = wide[:, :w].copy(), np.empty((h, w), np.uint8)
    edges = [round(k * h / 4) for k in range(5)]
    for k, s in enumerate((2, 2 * dq - 1, 2 * dq, nd - 1)):
        right[edges[k]:edges[k + 1]] = wide[edges[k]:edges[k + 1], s:s + w]       # right[x - s] = left[x]
    return left, right


def texture_ramp_pair(w, h, nd, shift=7, seed=31):
    """texture that grows with the column, for texture_threshold: over the computed region (x from nd on) a flat tenth (texture sum 0),
    then grey 100 with isolated +-1 dots whose density rises to 2 % (one dot alone in a window has the texture sum 2+2+4x1 = 8, an
    exact match and no second one: valid unless the texture test drops it), then noise whose amplitude doubles every 9 % of the
    width.  right = left shifted by `shift`."""
    rng = np.random.default_rng(seed)
    x = (np.arange(w + shift, dtype=np.float64) - nd) / (w - nd)
    u = rng.random((h, w + shift)); noise = rng.uniform(-1.0, 1.0, (h, w + shift))
    dots = np.sign(noise) * (u < np.clip((x - 0.10) / 0.35, 0, 1)[None] * 0.02)
    amp = np.where(x < 0.45, 0.0, 0.8 * np.exp(8.0 * (x - 0.45)))
    wide = np.clip(np.rint(100.0 + np.where(x[None] < 0.45, dots, amp[None] * noise)), 0, 255).astype(np.uint8)
    return wide[:, :w].copy(), wide[:, shift:].copy()


def uniqueness_ramp_pair(w, h, nd, shift=7, period=11, seed=41):
    """a second, weaker match that fades with the column, for uniqueness_ratio: over the computed region a flat tenth, then
    alpha P + (1 - alpha) N with P of period 11 along the row (a second match at shift + 11 and shift - 11... as good as the noise
    in the right image lets it be) and N random, alpha falling from 1 to 0 as a cube, the right image shifted and with +-6 grey
    levels of noise; the last 12 % are N alone without noise: min SAD = 0 there, unique at any ratio"""
    rng = np.random.default_rng(seed)
    n = w + shift
    x = (np.arange(n, dtype=np.float64) - nd) / (w - nd)
    P = np.tile(rng.uniform(-1, 1, (h, period)), (1, n // period + 1))[:, :n]
    N = rng.uniform(-1, 1, (h, n))
    alpha = 1.0 - np.clip((x - 0.10) / 0.78, 0.0, 1.0) ** 3
    wide = 128.0 + np.where(x < 0.10, 0.0, 60.0)[None] * (alpha[None] * P + (1 - alpha[None]) * N)
    left = np.clip(np.rint(wide[:, :w]), 0, 255).astype(np.uint8)
    eps = rng.uniform(-6.0, 6.0, (h, w)) * (x[shift:] < 0.88)[None]
    right = np.clip(np.rint(wide[:, shift:] + eps), 0, 255).astype(np.uint8)
    return left, right


def tie_pair(w, h, nd, shift=5, seed=51):
    """exact SAD ties between disparities of different quarters of [0, nd).  Upper half: every row has the period nd / 2 (rows
    differ), so SAD(d) = SAD(d + nd / 2): the minimum is tied between quarters 0 and 2 or 1 and 3.  Lower half: a constant
    gradient of 2 grey levels per column (w <= 128), whose prefiltered image is constant: every SAD is 0, all nd disparities tie."""
    rng = np.random.default_rng(seed)
    assert w <= 128 and nd % 4 == 0
    p = nd // 2
    top = np.tile(rng.integers(0, 256, (h, p), dtype=np.uint8), (1, (w + shift) // p + 1))[:, :w + shift]
    left, right = top[:, :w].copy(), top[:, shift:].copy()
    left[h // 2:] = right[h // 2:] = (2 * np.arange(w)).astype(np.uint8)[None]
    return left, right


def bw_pair(w, h, shift=7, seed=11):
    """2 x 2 blocks of 0 / 255: the prefilter saturates at both ends of [0, 2 cap]"""
    rng = np.random.default_rng(seed)
    wide = (rng.random((h // 2 + 1, (w + shift) // 2 + 1)) < 0.5).astype(np.uint8) * 255
    wide = np.repeat(np.repeat(wide, 2, 0), 2, 1)[:h, :w + shift]
    return np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, shift:])


def region_of(disp, nd, bs):
    r, (h, w) = bs // 2, disp.shape
    return disp[r:h - r, nd - 1 + r:w - r]


# ---- the brute-force twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [9, 8, 1])
def test_bruteforce_prefilter_equals_the_vectorised_one(h):
    rng = np.random.default_rng(60 + h)
    img = rng.integers(100, 116, (h, 23), dtype=np.uint8)                       # gradients of both signs, within and beyond every cap
    sat = np.tile(np.array([0, 0, 255, 255], np.uint8), (h, 6))[:, :23]
    for cap in (1, 31, 63):
        for im in (img, sat, img[:, :3], img[:, :2]):
            assert np.array_equal(rbm.prefilter_xsobel_bruteforce(im, cap), rbm.prefilter_xsobel(im, cap)), (h, cap, im.shape)
    if h > 1:
        assert len(np.unique(rbm.prefilter_xsobel(img, 31)[:h - (h & 1)])) > 31          # (more than half of [0, 62] occurs: not two constant images)


def _grid_input(svs, name, w, h, nd):
    if name == "synthetic":
        left, right = svs.synth_pair(1, 0, w=620, h=188)
        # a window of the pair where the scene's disparity is below 16: the far end of the tunnel, around the principal point
        y0, x0 = 92 - h // 2, 303 - w // 2
        return left[y0:y0 + h, x0:x0 + w].copy(), right[y0:y0 + h, x0:x0 + w].copy()
    if name == "black_white":
        return bw_pair(w, h)
    if name == "period8":
        per = hand_pairs()["period8"][0]
        return per[:h, :w].copy(), per[:h, 3:3 + w].copy()                               # shifted by 3: ties at 3, 11, 19, ..
    return tie_pair(w, h, nd)


@pytest.mark.parametrize("bs", [5, 7, 13])
@pytest.mark.parametrize("nd", [16, 48])
@pytest.mark.parametrize("name", ["synthetic", "black_white", "period8", "ties"])
def test_bruteforce_equals_the_restatement_bit_for_bit(svs, name, nd, bs):
    """The whole grid cap {1, 31, 63} x texture_threshold {0, 10, the region's median texture sum} x uniqueness_ratio {0, 1, 15, 100}
    on images of 12 (nd 16) or 8 (nd 48) computed columns and 7 or 8 computed rows (at most 67 x 20)."""
    r = bs // 2
    w, h = nd - 1 + 2 * r + (12 if nd == 16 else 8), 2 * r + 7 + (bs == 7)               # bs 7: an even height (14)
    left, right = _grid_input(svs, name, w, h, nd)
    seen, valid, maps = set(), [], {}
    for cap in (1, 31, 63):
        _, tex = rbm.sad_volume(left, right, nd, bs, cap)
        for thr in (0, 10, int(np.median(tex))):
            for uniq in (0, 1, 15, 100):
                prm = dict(num_disparities=nd, block_size=bs, pre_filter_cap=cap, texture_threshold=thr, uniqueness_ratio=uniq)
                ref = rbm.stereo_bm(left, right, **prm)
                got = rbm.stereo_bm_bruteforce(left, right, **prm)
                assert got.dtype == np.int16 and np.array_equal(got, ref), (prm, np.argwhere(got != ref)[:4])
                seen.add(ref.tobytes()); valid.append((region_of(ref, nd, bs) > 0).mean())
                maps[(cap, thr if thr in (0, 10) else "median", uniq)] = ref.tobytes()
    # which parameters decide anything here: two parameter sets that differ in that parameter alone give different maps
    axes = {name_: any(a != b for ka, a in maps.items() for kb, b in maps.items()
                       if ka[i] != kb[i] and all(ka[j] == kb[j] for j in range(3) if j != i))
            for i, name_ in enumerate(("cap", "tex", "uniq"))}
    print("%s nd %d bs %d (%dx%d): %d distinct maps of 36, valid share %.2f .. %.2f, deciding: %s" %
          (name, nd, bs, w, h, len(seen), min(valid), max(valid), [k for k, v in axes.items() if v]))
    assert max(valid) > 0.5                                     # something is matched
    # natural texture: all three parameters decide pixels.  Exact ties: the uniqueness test decides (ratio 0 against the rest) and,
    # in the constant-gradient half, the cap byte of the texture sum.  0 / 255 blocks saturate at every cap and match exactly
    # (minimum 0): only the median texture threshold cuts.  Period 8 is all-or-nothing on the ratio
    want = {"synthetic": {"cap", "tex", "uniq"}, "ties": {"uniq"}, "black_white": {"tex"}, "period8": {"uniq"}}[name]
    assert all(axes[k] for k in want), axes


def test_period8_at_ratio_0_keeps_the_largest_tied_disparity():
    """left = right with period 8: SAD(d) = SAD(d + 8) exactly, the minimum 0 at d = 0, 8, 16, 24.  OpenCV skips the uniqueness
    scan at uniquenessRatio 0 and its strict `<` over descending d keeps the largest: arg-min 24 = the largest d < nd = 32 that is
    congruent to the shift (0) modulo 8, at EVERY pixel; at ratio 1 every pixel is filtered.

    The arg-min is not `value >> 4`: value = (256 d + t + 15) >> 4 with the sub-pixel term t = 128 (p - n) / max(p, n), |t| <= 128,
    and p - n = SAD(23) - SAD(25) is the difference of the window's two boundary columns, not 0 (the window is 9 wide, the period
    8).  Here t is in [-31, 47]: the values are 383, 384 and 386, and 383 >> 4 = 23.  The integer disparity of a value is therefore
    taken as (value + 8) >> 4 (nearest, exact for |t| < 113), and the value is additionally held to 16 x 24 +- 8 (half a pixel),
    which is what |t| <= 128 allows and no more; and to the value worked out by hand from the window sums SAD(23) and SAD(25)."""
    left, right, prm, _ = hand_pairs()["period8"]
    nd, bs = prm["num_disparities"], prm["block_size"]
    shift = 0
    region = region_of(rbm.stereo_bm(left, right, uniqueness_ratio=0, **prm), nd, bs).astype(np.int32)
    print("period8, ratio 0: values", dict(zip(*np.unique(region, return_counts=True))))
    check_period8_ratio0(region, nd, shift, rbm.sad_volume(left, right, nd, bs)[0])
    assert (region_of(rbm.stereo_bm(left, right, uniqueness_ratio=1, **prm), nd, bs) == -16).all()
    sad, _ = rbm.sad_volume(left, right, nd, bs)
    assert (sad[0] == 0).all() and all(np.array_equal(sad[d], sad[d + 8]) for d in range(nd - 8))


def check_period8_ratio0(region, nd, shift, sad):
    d = (region + 8) >> 4
    assert region.size > 0 and (region > 0).all()                                        # every pixel of the region is valid
    assert (d % 8 == shift % 8).all() and (d >= nd - 8).all()
    assert (np.abs(region - 16 * d) <= 8).all()
    # the value by hand: arg-min D = the largest d < nd congruent to the shift, SAD(D) = 0, p = SAD(D - 1), n = SAD(D + 1) straight from
    # the window sums — nothing of the matcher's arg-min, uniqueness or sub-pixel code
    D = nd - 8 + shift % 8
    p, n = sad[D - 1], sad[D + 1]
    assert (sad[D] == 0).all() and (p > 0).all() and (n > 0).all()
    num, den = (p - n) * 256, p + n + np.abs(p - n)
    t = np.sign(num) * (np.abs(num) // den)                                              # C division
    assert np.array_equal(region, (D * 256 + t + 15) >> 4)


def test_ratio_0_only_adds_pixels_and_ratio_1_is_a_test():
    """on the uniqueness ramp: the map at ratio 0 equals the map at ratio 1 wherever that one is valid, and has more valid pixels"""
    left, right = uniqueness_ramp_pair(160, 31, 32)
    a = rbm.stereo_bm(left, right, num_disparities=32, block_size=9, uniqueness_ratio=0)
    b = rbm.stereo_bm(left, right, num_disparities=32, block_size=9, uniqueness_ratio=1)
    assert np.array_equal(a[b != -16], b[b != -16]) and (a != -16).sum() > (b != -16).sum() > 0
