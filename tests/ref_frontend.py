"""Plain references of the image-side kernels (GFTT, LK), written from the declared operation
order alone, plus the seeded scenes and the geometry list that the CPU tests (oracle against
these references) and the GPU tests (HIP against the oracle) share.

Not a conftest: imported explicitly by test_oracle_gftt.py, test_oracle_image.py,
test_oracle_frontend_geometries.py and test_gpu_frontend_geometries.py."""
import numpy as np
from scipy import ndimage

import common as cm


# ---------------------------------------------------------------------------- GFTT
def _eig_numpy(img):
    f = np.float32
    p = np.pad(img.astype(np.float32), 1, mode="reflect")
    s1 = f(1.0 / 3060.0); s2 = f(2.0 * (1.0 / 3060.0))
    c = lambda dy, dx: p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx]
    d0 = c(-1, 1) - c(-1, -1); d1 = c(0, 1) - c(0, -1); d2 = c(1, 1) - c(1, -1)
    Dx = (d0 + d2) * s1 + d1 * s2
    c0 = (s1 * c(-1, -1) + s2 * c(-1, 0)) + s1 * c(-1, 1)
    c2 = (s1 * c(1, -1) + s2 * c(1, 0)) + s1 * c(1, 1)
    Dy = c2 - c0
    assert Dx.dtype == np.float32 and Dy.dtype == np.float32
    out = []
    for m in (Dx * Dx, Dx * Dy, Dy * Dy):
        q = np.pad(m, 1, mode="reflect").astype(np.float64)
        s = np.zeros_like(m, dtype=np.float64)
        for j in range(3):           # same accumulation order as the oracle (rows outer)
            for i in range(3):
                s = s + q[j:j + m.shape[0], i:i + m.shape[1]]
        out.append(s.astype(np.float32))
    a = out[0] * f(0.5); b = out[1]; cc = out[2] * f(0.5)
    t = a - cc
    return (a + cc) - np.sqrt(t * t + b * b)


def _candidates(eig, mask, quality):
    """the sorted candidate list of goodFeaturesToTrack as (x, y) rows: masked maximum -> threshold
    (TOZERO) -> 3x3 local maximum of the thresholded map on interior pixels -> value descending,
    then pixel index descending.  The 3x3 test is nine shifted views instead of a pixel loop."""
    h, w = eig.shape
    mx = eig[mask > 0].max() if (mask > 0).any() else 0.0
    thr = np.float32(float(mx) * quality)
    if h < 3 or w < 3:
        return np.zeros((0, 2), np.int64)
    t = np.where(eig > thr, eig, np.float32(0))
    v = eig[1:-1, 1:-1]
    nbmax = np.zeros_like(v)
    for dy in range(3):
        for dx in range(3):
            nbmax = np.maximum(nbmax, t[dy:dy + h - 2, dx:dx + w - 2])
    ok = (v > thr) & (v != 0) & (mask[1:-1, 1:-1] > 0) & ~(nbmax > v)
    ys, xs = np.nonzero(ok)
    ys += 1; xs += 1
    val = eig[ys, xs]
    idx = ys.astype(np.int64) * w + xs
    order = np.lexsort((-idx, -val.astype(np.float64)))
    return np.stack([xs[order], ys[order]], 1).astype(np.int64)


def _greedy_python(eig, mask, max_corners, quality, min_dist):
    """the whole selection.  The greedy pass is the plain loop over the FULL list of accepted corners
    (no cell grid, no bitmap) with the comparison in double: dx^2 + dy^2 < min_dist * min_dist."""
    cand = _candidates(eig, mask, quality)
    md2 = float(min_dist) * float(min_dist)
    acc = np.zeros((max(max_corners, 1), 2), np.int64)
    n = 0
    for x, y in cand:
        if min_dist >= 1 and n:
            d = acc[:n] - (x, y)
            if ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64) < md2).any():
                continue
        acc[n] = (x, y)
        n += 1
        if n == max_corners:
            break
    return acc[:n].astype(np.float32).reshape(-1, 2)


# ---------------------------------------------------------------------------- LK
def _ref_lk_single_level(I, J, pts, guess, max_iter=30, eps=0.01, win=11):
    """independent numpy restatement of one LK level (OpenCV LKTrackerInvoker, level 0 only,
    float accumulators exactly like the scalar C++ code)"""
    W_BITS = 14
    h, w = I.shape
    B = win
    Ib = np.pad(I.astype(np.int64), B, mode="reflect")
    Jb = np.pad(J.astype(np.int64), B, mode="reflect")
    a = I.astype(np.int64)
    sm = np.array([3, 10, 3]); df = np.array([-1, 0, 1])
    dx = ndimage.correlate1d(ndimage.correlate1d(a, sm, axis=0, mode="mirror"), df, axis=1, mode="mirror")
    dy = ndimage.correlate1d(ndimage.correlate1d(a, df, axis=0, mode="mirror"), sm, axis=1, mode="mirror")
    dxb = np.pad(dx, B); dyb = np.pad(dy, B)
    half = np.float32((win - 1) * 0.5)
    out = guess.astype(np.float32).copy(); status = np.ones(len(pts), np.uint8)

    def weights(fx, fy):
        ix, iy = int(np.floor(fx)), int(np.floor(fy))
        a_ = np.float32(fx - np.float32(ix)); b_ = np.float32(fy - np.float32(iy))
        one = np.float32(1)
        w00 = int(np.rint(np.float32(np.float32((one - a_) * (one - b_)) * np.float32(1 << W_BITS))))
        w01 = int(np.rint(np.float32(np.float32(a_ * (one - b_)) * np.float32(1 << W_BITS))))
        w10 = int(np.rint(np.float32(np.float32((one - a_) * b_) * np.float32(1 << W_BITS))))
        return ix, iy, w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10

    def patch(img_b, ix, iy, ws, shift):
        y0, x0 = iy + B, ix + B
        p = img_b[y0:y0 + win + 1, x0:x0 + win + 1]
        v = p[:-1, :-1] * ws[0] + p[:-1, 1:] * ws[1] + p[1:, :-1] * ws[2] + p[1:, 1:] * ws[3]
        return (v + (1 << (shift - 1))) >> shift

    for n, (p, g) in enumerate(zip(pts.astype(np.float32), guess.astype(np.float32))):
        px, py = np.float32(p[0] - half), np.float32(p[1] - half)
        ix, iy, *ws = weights(px, py)
        if ix < -win or ix >= w or iy < -win or iy >= h:
            status[n] = 0
            continue
        Iw = patch(Ib, ix, iy, ws, W_BITS - 5); Ix = patch(dxb, ix, iy, ws, W_BITS); Iy = patch(dyb, ix, iy, ws, W_BITS)
        sc = np.float32(1.0 / (1 << 20))
        A11 = np.float32(np.float32((Ix * Ix).sum()) * sc); A12 = np.float32(np.float32((Ix * Iy).sum()) * sc)
        A22 = np.float32(np.float32((Iy * Iy).sum()) * sc)
        D = np.float32(A11 * A22 - A12 * A12)
        mine = (A22 + A11 - np.sqrt(np.float32((A11 - A22) ** 2 + np.float32(4) * A12 * A12))) / np.float32(2 * win * win)
        if mine < 1e-4 or D < np.finfo(np.float32).eps:
            status[n] = 0
            continue
        D = np.float32(1) / D
        nx, ny = np.float32(g[0] - half), np.float32(g[1] - half)
        pdx = pdy = np.float32(0)
        for j in range(max_iter):
            jx, jy, *wj = weights(nx, ny)
            if jx < -win or jx >= w or jy < -win or jy >= h:
                status[n] = 0
                break
            diff = patch(Jb, jx, jy, wj, W_BITS - 5) - Iw
            b1 = np.float32(np.float32((diff * Ix).sum()) * sc); b2 = np.float32(np.float32((diff * Iy).sum()) * sc)
            ddx = np.float32(np.float32(A12 * b2 - A22 * b1) * D); ddy = np.float32(np.float32(A12 * b1 - A11 * b2) * D)
            nx = np.float32(nx + ddx); ny = np.float32(ny + ddy)
            out[n] = (nx + half, ny + half)
            if float(ddx) ** 2 + float(ddy) ** 2 <= eps * eps:
                break
            if j > 0 and abs(float(ddx + pdx)) < 0.01 and abs(float(ddy + pdy)) < 0.01:
                out[n] -= np.array([ddx, ddy], np.float32) * np.float32(0.5)
                break
            pdx, pdy = ddx, ddy
        if status[n]:
            # the level-0 residual is sampled at the final position; a window that has left the image there clears the status
            fx, fy = int(np.floor(np.float32(out[n][0] - half))), int(np.floor(np.float32(out[n][1] - half)))
            if fx < -win or fx >= w or fy < -win or fy >= h:
                status[n] = 0
    return out, status


# ---------------------------------------------------------------------------- kernel constants, restated
GE_COLS, GE_ROWS = 58, 48            # k_gftt_eig3: output columns / rows of one wave's strip
GF_BITMAP_WORDS = 4096               # k_gftt_select2: one bit per pixel, rows padded to 32-bit words
GF_GRID_CELLS = 1280                 # ... or OpenCV's cell grid, if it has at most this many cells
BITMAP_MAX_DIST = 31                 # one disc row per lane
LK_WIN, LK_REG = 11, 32              # k_lk: window, side of the staged J region
SVS_BORDER = 16                      # stored REFLECT_101 border of every pyramid level


def _geom(w, h, why):
    return (w, h, why)


# (w, h, why): every entry is derived from one of the constants above
GEOMETRIES = [
    _geom(16, 16, "the minimum svslam_create accepts; one pyramid level"),
    _geom(30, 22, "one level (the next would be 15x11 <= the window); LK max_level=3 must clamp"),
    _geom(GE_COLS, GE_ROWS, "one exact strip"),
    _geom(GE_COLS + 1, GE_ROWS + 1, "1-column / 1-row last strips"),
    _geom(GE_COLS + 2, GE_ROWS + 2, "2-column / 2-row last strips"),
    _geom(2 * GE_COLS - 1, 2 * GE_ROWS - 1, "strip residues 57 / 47"),
    _geom(2 * GE_COLS, 2 * GE_ROWS, "two exact strips"),
    _geom(2 * GE_COLS + 1, 2 * GE_ROWS + 1, "two strips plus a 1-column / 1-row last strip"),
    _geom(613, 185, "config 3"),
    _geom(621, 188, "KITTI 1242x375 halved (cvRound(187.5) = 188)"),
    _geom(512, GF_BITMAP_WORDS // (512 // 32), "bitmap exactly full: 16 words x 256 rows"),
    _geom(512, GF_BITMAP_WORDS // (512 // 32) + 1, "one row more: first geometry on the grid path"),
    _geom(640, 480, "grid path; (w + 32) % 16 == 0: pitch without slack"),
    _geom(1241, 376, "undecimated frame; grid path"),
]
SELECTION_GEOMETRIES = [(512, 256), (512, 257), (640, 480), (1241, 376), (620, 188)]

MIN_DISTS = [0, 0.5, 1.0, 1.5, 2.5, 3.5, 7.4, 20, 31, 31.5, 40]
MAX_CORNERS = [1, 150, 1024]
QUALITIES = [0.0005, 0.01]


def nlevels(w, h, max_level=3):
    n = 1
    while n <= max_level and (w + 1) // 2 > LK_WIN and (h + 1) // 2 > LK_WIN:
        w, h = (w + 1) // 2, (h + 1) // 2
        n += 1
    return n


def selection_path(w, h, min_dist):
    """k_gftt_select2's published rule, restated: which exclusion structure the greedy pass uses"""
    if not min_dist >= 1:
        return "none"
    wp = (w + 31) >> 5
    if wp * h <= GF_BITMAP_WORDS and min_dist <= BITMAP_MAX_DIST:
        return "bitmap"
    cell = int(np.rint(min_dist))                          # cvRound: half to even
    if -(-w // cell) * -(-h // cell) <= GF_GRID_CELLS:
        return "grid"
    return "list"


def straddling_min_dists(count=3, big=True):
    """min_dist values sqrt(k) whose DOUBLE square lies just above the integer k while the FLOAT square
    rounds onto k: a corner pair at squared distance exactly k is too close in double (k < md^2) and far
    enough in float (k < (float)md^2 is false).  k = dx^2 + dy^2 with one offset >= 6, so that two
    single-pixel features at that offset have disjoint 5x5 eigenvalue supports.  Returns (md, k, (dx, dy)):
    the first `count` small ones and, with big, one above the bitmap's 31-pixel limit."""
    out, bigone = [], None
    for k in range(37, 1300):
        reps = [(a, b) for a in range(0, 37) for b in range(6, 37) if a * a + b * b == k and a <= b]
        if not reps:
            continue
        md = float(np.sqrt(np.float64(k)))
        if md * md > k and np.float32(md * md) == np.float32(k):
            if len(out) < count:
                out.append((md, k, reps[0]))
            elif big and k > 32 * 32 and bigone is None:
                bigone = (md, k, reps[0])
    return out + ([bigone] if big and bigone else [])


def straddle_scene(rng, w, h, straddles):
    """a noise image (corners everywhere, so the selection structures are full) with one flat window per straddling value; in it two single bright pixels at the
    offset (dx, dy), dx^2 + dy^2 = k, the first brighter than the second, both far brighter than the
    texture: the candidate list holds the pair in that order and nothing else is within min_dist of the
    second.  Returns (image, [(first_xy, second_xy)])."""
    img = (rng.integers(0, 256, (h, w)) * 3 // 8).astype(np.uint8)      # dense noise corners, well below the dots
    pairs = []
    x0 = 4
    for md, k, (dx, dy) in straddles:
        m = int(np.ceil(md)) + 4                           # flat margin: nothing of the texture within md (+ supports)
        ww, hh = dx + 2 * m + 1, dy + 2 * m + 1
        assert x0 + ww < w - 4 and 4 + hh < h - 4, "image too small for the straddle windows"
        img[4:4 + hh, x0:x0 + ww] = 0
        ax, ay = x0 + m, 4 + m
        img[ay, ax] = 255
        img[ay + dy, ax + dx] = 230
        pairs.append(((ax, ay), (ax + dx, ay + dy)))
        x0 += ww + 6
    return img, pairs


def seam_rects(rng, w, h, n=60):
    """~n mask-rectangle centres: on the strip seams (x ~ 58k +- 10.5, y ~ 48k +- 10.5; half-integer
    centres meet the round-half-even rule of Point2f -> Point), on the image corners, random, some off-image"""
    r = []
    for k in range(0, w // GE_COLS + 2):
        for s in (-10.5, 10.5, 0.5):
            r.append((GE_COLS * k + s, rng.uniform(-5, h + 5)))
    for k in range(0, h // GE_ROWS + 2):
        for s in (-10.5, 10.5, -0.5):
            r.append((rng.uniform(-5, w + 5), GE_ROWS * k + s))
    r = [r[i] for i in rng.permutation(len(r))[:max(n - 24, 12)]]
    r += [(GE_COLS - 10.5, GE_ROWS + 10.5), (GE_COLS + 10.5, GE_ROWS - 10.5), (0.0, 0.0), (w - 1.0, h - 1.0), (w - 0.5, 0.5),
          (-10.5, h + 9.5), (-30.0, -30.0), (w + 40.0, h / 2.0), (w / 2.0, -11.0), (w / 2.0, h + 10.49)]
    while len(r) < n:
        r.append((rng.uniform(-12, w + 12), rng.uniform(-12, h + 12)))
    return np.array(r, np.float32)


def grid_density(corners, min_dist):
    """mean number of accepted corners in the 3x3 cell neighbourhood of every occupied cell (the cells
    of cvRound(min_dist) pixels that OpenCV's search and gf_greedy use)"""
    if len(corners) == 0:
        return 0.0
    cell = int(np.rint(min_dist))
    c = (corners.astype(np.int64) // cell)
    occ, cnt = np.unique(c, axis=0, return_counts=True)
    table = {tuple(o): n for o, n in zip(occ.tolist(), cnt.tolist())}
    tot = 0
    for (cx, cy) in table:
        tot += sum(table.get((cx + i, cy + j), 0) for i in (-1, 0, 1) for j in (-1, 0, 1))
    return tot / len(table)


def lattice_image(w, h):
    lat = np.zeros((h, w), np.uint8)
    lat[(np.arange(h)[:, None] // 6 + np.arange(w)[None] // 6) % 2 == 0] = 200      # identical corners everywhere
    return lat


# ---------------------------------------------------------------------------- LK scenes
def warp_pair(rng, w, h, sigma=2.0, amp=3.0):
    """(I, J): J is I under a smooth warp of a few pixels (a low-frequency displacement field)"""
    I = cm.textured(rng, h, w, sigma=sigma)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 4)
    ux = amp * np.sin(2 * np.pi * xx / max(w, 40) + ph[0]) * np.cos(2 * np.pi * yy / max(h, 40) + ph[1]) + rng.uniform(-1.5, 1.5)
    uy = 0.6 * amp * np.cos(2 * np.pi * xx / max(w, 40) + ph[2]) * np.sin(2 * np.pi * yy / max(h, 40) + ph[3]) + rng.uniform(-1, 1)
    J = ndimage.map_coordinates(I.astype(np.float64), [yy - uy, xx - ux], order=3, mode="mirror")
    return I, np.clip(np.rint(J), 0, 255).astype(np.uint8)


def lk_threshold_lattice(w, h):
    """points on the window-corner status thresholds of every level the geometry has: the window corner
    floor(x * 2^-l - 5) takes the values -12, -11 (first inside), w_l - 1 (last inside), w_l there"""
    pts = []
    lw, lh = w, h
    for l in range(nlevels(w, h)):
        s = float(1 << l)
        xs = [-6.5, -6.0, -5.99, -5.5, lw + 3.99, lw + 4.0, lw + 4.99, lw + 5.0]
        ys = [-6.5, -6.0, -5.99, -5.5, lh + 3.99, lh + 4.0, lh + 4.99, lh + 5.0]
        for x in xs:
            for y in ys:
                pts.append((x * s, y * s))
        for x in xs:
            pts.append((x * s, 0.37 * h))
        for y in ys:
            pts.append((0.61 * w, y * s))
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
    return np.array(pts, np.float32)


def lk_full_range_points(rng, w, h, n=400):
    p = np.stack([rng.uniform(-8, w + 8, n), rng.uniform(-8, h + 8, n)], 1).astype(np.float32)
    p = np.concatenate([p, lk_threshold_lattice(w, h)])
    g = p + rng.normal(0, 3, p.shape).astype(np.float32)
    return p, g


RESTAGE_SEED, RESTAGE_SIGMA = 23, 9.0
RESTAGE_SHIFTS = ((16, -18), (-15, 19))             # (sy, sx): both signs on both axes


def restage_scene(w, h, shift, seed=RESTAGE_SEED, sigma=RESTAGE_SIGMA, n=240):
    """a texture smooth enough (cm.textured with a large sigma) for single-level LK to walk 14-24 px:
    I and J = I displaced by shift = (sy, sx) are two crops of one larger texture; random points inside
    the image, to be used as their own guesses (the undisplaced position)"""
    rng = np.random.default_rng(seed)
    big = cm.textured(rng, h + 64, w + 64, sigma=sigma)
    sy, sx = shift
    I = big[32:32 + h, 32:32 + w].copy()
    J = big[32 - sy:32 - sy + h, 32 - sx:32 - sx + w].copy()      # J(y, x) = I(y - sy, x - sx): content moves by +shift
    m = min(8, w // 4)
    p = np.stack([rng.uniform(m, w - m, n), rng.uniform(m, h - m, n)], 1).astype(np.float32)
    return I, J, p


def restaged(q_ref, st_ref, guess):
    """points whose window provably left the 32-wide J region staged at the guess (origin guess - 10,
    x aligned down by up to 3): the oracle's result alone decides"""
    d = q_ref - guess
    return (st_ref > 0) & ((np.abs(d[:, 1]) > 11) | (d[:, 0] < -14))
