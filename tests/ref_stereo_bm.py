"""CPU restatement (numpy) of the dense-reconstruction arithmetic of the reference's second program:
cv::StereoBM::compute with the settings of include/StereoVisionSLAM/dense_reconstruction.h:56-57 (StereoBM(128, 15):
PREFILTER_XSOBEL, preFilterCap 31, minDisparity 0, textureThreshold 10, uniquenessRatio 15, no speckle filter, no
disp12MaxDiff, CV_16S output = 16 x disparity) and the disparity -> depth -> map-frame loop of
src/dense_reconstruction.cpp:116-173.

Vectorised over the image with one loop over the disparity; nothing here knows about the kernel's tiles.
stereo_bm_bruteforce is its second opinion: the same function one pixel at a time, in the shape of OpenCV's loop.
Parity with OpenCV itself is UNPINNED: OpenCV is not installed where this project is developed, so the block matcher
is restated from memory of modules/calib3d/src/stereobm.cpp (like oracle/orc_gftt.c for GFTT) and checked against
geometry (tests/test_ref_stereo_bm.py), not against cv2."""
import numpy as np

FILTERED = -16                # (minDisparity - 1) << 4
DEFAULTS = dict(num_disparities=128, block_size=15, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15)


def prefilter_xsobel(img, cap=31):
    """u8 image in [0, 2 cap]: clamp(dx(row-1) + 2 dx(row) + dx(row+1), -cap, cap) + cap, dx(r)[x] = r[x+1] - r[x-1]; rows
    outside the image reflected without repeating the edge; columns 0 and w-1 = cap; OpenCV works on row pairs and fills a
    trailing odd last row with cap"""
    a = np.asarray(img, np.int32)
    h, w = a.shape
    out = np.full((h, w), cap, np.int32)
    if w >= 3:
        dx = np.zeros((h, w), np.int32)
        dx[:, 1:-1] = a[:, 2:] - a[:, :-2]
        up = np.concatenate([dx[1:2] if h > 1 else dx[0:1], dx[:-1]], 0)
        dn = np.concatenate([dx[1:], dx[h - 2:h - 1] if h > 1 else dx[0:1]], 0)
        v = np.clip(up + 2 * dx + dn, -cap, cap) + cap
        out[:, 1:-1] = v[:, 1:-1]
    if h & 1:
        out[h - 1, :] = cap
    return out.astype(np.uint8)


def _box(a, r):
    """sum over the (2r+1)^2 window, 'valid' part: out[y - r, x - r] = sum a[y-r..y+r, x-r..x+r]"""
    h, w = a.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    n = 2 * r + 1
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


def sad_volume(left, right, num_disparities=128, block_size=15, pre_filter_cap=31):
    """(sad int64 [nd, hc, wc], tex int64 [hc, wc]) over the computed region y in [r, h-r), x in [nd-1+r, w-r): the window sums
    of |L' - R'(. - d)| and of |L' - cap|.  The tests read their thresholds and tie counts off these."""
    left = np.asarray(left, np.uint8); right = np.asarray(right, np.uint8)
    h, w = left.shape
    nd, r, cap = int(num_disparities), int(block_size) // 2, int(pre_filter_cap)
    x0, x1 = nd - 1 + r, w - r
    assert x0 < x1 and h >= 2 * r + 1
    L = prefilter_xsobel(left, cap).astype(np.int32)
    R = prefilter_xsobel(right, cap).astype(np.int32)
    sad = np.zeros((nd, h - 2 * r, x1 - x0), np.int64)
    for d in range(nd):
        # columns x0-r .. x1+r-1 of L' against the same columns shifted by d of R'
        ad = np.abs(L[:, x0 - r:x1 + r] - R[:, x0 - r - d:x1 + r - d])
        sad[d] = _box(ad, r)
    return sad, _box(np.abs(L[:, x0 - r:x1 + r] - cap), r)


def stereo_bm(left, right, num_disparities=128, block_size=15, pre_filter_cap=31, texture_threshold=10,
              uniqueness_ratio=15):
    """int16 map [h, w] of 16 x disparity, FILTERED (-16) where OpenCV writes no disparity.

    uniqueness_ratio = 0 switches the uniqueness test off: findStereoCorrespondenceBM guards the scan with
    `if( uniquenessRatio > 0 )` (modules/calib3d/src/stereobm.cpp), so a minimum that is tied at a distant disparity is
    kept, at the largest of the tied disparities.  Like the rest of this file that line is restated from memory of the
    source and UNPINNED against a binary."""
    left = np.asarray(left, np.uint8); right = np.asarray(right, np.uint8)
    h, w = left.shape
    nd, r, cap = int(num_disparities), int(block_size) // 2, int(pre_filter_cap)
    out = np.full((h, w), FILTERED, np.int16)
    x0, x1 = nd - 1 + r, w - r
    if x0 >= x1 or h < 2 * r + 1:
        return out                                        # OpenCV's early-out
    sad, tex = sad_volume(left, right, nd, block_size, cap)        # the computed region: y in [r, h-r), x in [x0, x1)
    # ties resolve to the LARGEST disparity
    mind = nd - 1 - np.argmin(sad[::-1], axis=0)
    minsad = np.take_along_axis(sad, mind[None], 0)[0]
    if uniqueness_ratio > 0:
        thr = minsad + minsad * uniqueness_ratio // 100
        dd = np.arange(nd)[:, None, None]
        outside = (dd < mind[None] - 1) | (dd > mind[None] + 1)
        not_unique = ((sad <= thr[None]) & outside).any(0)
    else:
        not_unique = np.zeros(mind.shape, bool)           # if( uniquenessRatio > 0 ): 0 is "no test", not "no margin"
    pm = np.where(mind > 0, mind - 1, 1)                  # SAD(-1) := SAD(1)
    nm = np.where(mind < nd - 1, mind + 1, nd - 2)        # SAD(nd) := SAD(nd-2)
    p = np.take_along_axis(sad, pm[None], 0)[0]
    n = np.take_along_axis(sad, nm[None], 0)[0]
    den = p + n - 2 * minsad + np.abs(p - n)
    num = (p - n) * 256
    frac = np.where(den != 0, np.sign(num) * (np.abs(num) // np.where(den != 0, den, 1)), 0)   # C division: towards zero
    val = (mind * 256 + frac + 15) >> 4
    val = np.where((tex < texture_threshold) | not_unique, FILTERED, val)
    out[r:h - r, x0:x1] = val.astype(np.int16)
    return out


def prefilter_xsobel_bruteforce(img, cap=31):
    """prefilter_xsobel one pixel at a time, written as cv::prefilterXSobel walks the image: rows in pairs, the source rows
    of a pair picked with its border rule (row -1 -> row 1, row h -> row h - 2), the rest of an odd image filled with cap"""
    a = [[int(v) for v in row] for row in np.asarray(img, np.uint8)]
    h, w = len(a), len(a[0])
    out = [[cap] * w for _ in range(h)]
    y = 0
    while y < h - 1:                                      # the pair (y, y + 1); h - 1 is not reached when h is odd
        for yy in (y, y + 1):
            r0 = a[yy - 1 if yy > 0 else 1]
            r1 = a[yy]
            r2 = a[yy + 1 if yy < h - 1 else h - 2]
            for x in range(1, w - 1):
                v = (r0[x + 1] - r0[x - 1]) + 2 * (r1[x + 1] - r1[x - 1]) + (r2[x + 1] - r2[x - 1])
                out[yy][x] = (-cap if v < -cap else cap if v > cap else v) + cap
        y += 2
    return np.array(out, np.uint8).reshape(h, w)


def stereo_bm_bruteforce(left, right, num_disparities=128, block_size=15, pre_filter_cap=31, texture_threshold=10,
                         uniqueness_ratio=15):
    """stereo_bm again, written the way findStereoCorrespondenceBM is: two loops over the pixels, every SAD summed over its
    window, a running minimum over OpenCV's index order, Python integers throughout.  Independent of stereo_bm but for
    prefilter_xsobel (which has a twin of its own above): no cumulative sum, no argmin, no take_along_axis."""
    left = np.asarray(left, np.uint8); right = np.asarray(right, np.uint8)
    h, w = left.shape
    nd, r, cap = int(num_disparities), int(block_size) // 2, int(pre_filter_cap)
    out = [[FILTERED] * w for _ in range(h)]
    L = [[int(v) for v in row] for row in prefilter_xsobel(left, cap)]
    R = [[int(v) for v in row] for row in prefilter_xsobel(right, cap)]
    win = range(-r, r + 1)
    for y in range(r, h - r):
        for x in range(nd - 1 + r, w - r):                # empty on OpenCV's early-out
            tex = 0
            for j in win:
                for i in win:
                    tex += abs(L[y + j][x + i] - cap)
            sad = [0] * (nd + 2)                          # sad[1 + i]: OpenCV's index i = disparity nd - 1 - i; two border cells
            for i in range(nd):
                d = nd - 1 - i
                s = 0
                for j in win:
                    lrow, rrow = L[y + j], R[y + j]
                    for k in win:
                        s += abs(lrow[x + k] - rrow[x + k - d])
                sad[1 + i] = s
            minsad, mini = None, -1
            for i in range(nd):
                if minsad is None or sad[1 + i] < minsad:             # strict: the first index = the largest disparity wins a tie
                    minsad, mini = sad[1 + i], i
            if tex < texture_threshold:
                continue
            if uniqueness_ratio > 0:
                thresh = minsad + _cdiv(minsad * uniqueness_ratio, 100)
                if any((i < mini - 1 or i > mini + 1) and sad[1 + i] <= thresh for i in range(nd)):
                    continue
            sad[0] = sad[2]                               # sad[-1] = sad[1]
            sad[nd + 1] = sad[nd - 1]                     # sad[nd] = sad[nd - 2]
            p, n = sad[1 + mini + 1], sad[1 + mini - 1]
            den = p + n - 2 * minsad + abs(p - n)
            val = ((nd - 1 - mini) * 256 + (_cdiv((p - n) * 256, den) if den != 0 else 0) + 15) >> 4
            out[y][x] = val
    return np.array(out, np.int16).reshape(h, w)


def _cdiv(a, b):
    """C's integer division: towards zero (b > 0)"""
    return a // b if a >= 0 else -((-a) // b)


def quat_R(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def dense_cloud(disp16, cam_l, ext_l, baseline, T_cw, min_depth=1.0):
    """src/dense_reconstruction.cpp:116-173 with its types: returns (xyz f32 [n, 3], pix i32 [n] = y*w + x) in the
    reference's loop order, x outer and y inner"""
    disp16 = np.asarray(disp16, np.int16)
    h, w = disp16.shape
    fx32 = np.float32(cam_l[0]); b32 = np.float32(baseline)
    disp = disp16.astype(np.float32) * np.float32(1.0 / 16.0)
    depth = np.zeros((h, w), np.float32)
    pos = disp > 0
    depth[pos] = (fx32 * b32) / disp[pos]
    keep = ~(depth.astype(np.float64) < min_depth)
    xs, ys = np.nonzero(keep.T)                            # x outer, y inner
    z = depth[ys, xs].astype(np.float64)
    fx, fy, cx, cy = [float(v) for v in cam_l]
    pc = np.stack([(xs - cx) * z / fx, (ys - cy) * z / fy, z], 1)
    Re, te = quat_R(ext_l[:4]), np.asarray(ext_l[4:], np.float64)
    Rc, tc = quat_R(T_cw[:4]), np.asarray(T_cw[4:], np.float64)
    pr = (pc - te) @ Re                                    # ext_l^-1: Re^T (p - te)
    pw = (pr - tc) @ Rc                                    # T_cw^-1
    return pw.astype(np.float32), (ys * w + xs).astype(np.int32)
