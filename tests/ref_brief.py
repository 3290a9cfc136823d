"""Reference for svslam_brief_describe_batch: BRIEF-256 at given points of a 7x7 / sigma 2 blurred image, what
cv::ORB::compute does with provided keypoints whose angle is KeyPoint's default.  A numpy reading of the stated procedure, written
from the contract and not from csrc/k_brief.h; everything is integer or a written-out f32 step, so the comparison with the kernel
and with its host emulation is exact.  tests/test_ref_brief.py holds this module to facts it does not use itself."""
import numpy as np

MAX_PTS = 1024
SIGMA = 2.0


def _taps():
    """round-to-nearest of 256 g(sigma = 2), the centre tap absorbing what the rounding leaves"""
    g = np.exp(-(np.arange(7) - 3.0) ** 2 / (2.0 * SIGMA * SIGMA))
    t = np.rint(256.0 * g / g.sum()).astype(np.int64)
    t[3] += 256 - t.sum()
    return t


TAPS = _taps()
assert TAPS.sum() == 256 and tuple(TAPS) == (18, 34, 49, 54, 49, 34, 18)


# ---- the default table ------------------------------------------------------------------------------------------------------------
PATTERN_SEED = 0x42524946      # "BRIF"
PATTERN_REACH = 13


def _mix32(n):
    h = ((n * 0x9E3779B1) ^ PATTERN_SEED) & 0xFFFFFFFF
    h ^= h >> 16; h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15; h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def default_pattern():
    """[256, 4] int8 = x0, y0, x1, y1.  Candidate k = 0, 1, ... takes its four coordinates from the stateless hash of 4k .. 4k + 3,
    each (hash * 27) >> 32 minus 13 (uniform on -13 .. 13).  A candidate is dropped when its two points coincide or when it, or
    its reverse, is already in the table; the first 256 kept are the table."""
    out, seen, k = [], set(), 0
    span = 2 * PATTERN_REACH + 1
    while len(out) < 256:
        c = tuple(((_mix32(4 * k + j) * span) >> 32) - PATTERN_REACH for j in range(4))
        k += 1
        if c[:2] == c[2:] or c in seen or (c[2:] + c[:2]) in seen:
            continue
        seen.add(c)
        out.append(c)
    return np.array(out, np.int8)


def cv_round(v):
    """cvRound: round half to even, on f32"""
    return np.rint(np.asarray(v, np.float32)).astype(np.int64)


def rotated_f32(pattern, angle_deg):
    """the 512 table points after the rotation, before the rounding: [512, 2] f32"""
    p = np.asarray(pattern, np.int8).reshape(512, 2).astype(np.float32)
    ang = np.float32(angle_deg) * np.float32(np.pi / 180.0)
    a, b = np.cos(ang, dtype=np.float32), np.sin(ang, dtype=np.float32)
    x = (p[:, 0] * a).astype(np.float32) - (p[:, 1] * b).astype(np.float32)
    y = (p[:, 0] * b).astype(np.float32) + (p[:, 1] * a).astype(np.float32)
    return np.stack([x.astype(np.float32), y.astype(np.float32)], axis=1)


def offsets(pattern, angle_deg):
    """[512, 2] integer (ix, iy)"""
    return cv_round(rotated_f32(pattern, angle_deg))


def half_integer_margin(pattern, angle_deg):
    """the distance of the nearest rotated coordinate to a half-integer, in f64 arithmetic: where it is large, an ulp of difference
    between two cosf / sinf cannot change an offset"""
    p = np.asarray(pattern, np.int8).reshape(512, 2).astype(np.float64)
    ang = np.deg2rad(float(angle_deg))
    x = p[:, 0] * np.cos(ang) - p[:, 1] * np.sin(ang)
    y = p[:, 0] * np.sin(ang) + p[:, 1] * np.cos(ang)
    v = np.concatenate([x, y])
    return float(np.abs(v - np.floor(v) - 0.5).min())


def blur(img):
    """the blurred values of the pixels that have all their 49 taps inside the image: [h - 6, w - 6] u8, entry [y - 3, x - 3]"""
    im = np.asarray(img, np.uint8).astype(np.int64)
    h, w = im.shape
    if h < 7 or w < 7:
        return np.zeros((max(h - 6, 0), max(w - 6, 0)), np.uint8)
    hs = sum(int(TAPS[k]) * im[:, k:w - 6 + k] for k in range(7))            # <= 255 * 256 = 65280
    vs = sum(int(TAPS[k]) * hs[k:h - 6 + k, :] for k in range(7))
    return ((vs + 32768) >> 16).astype(np.uint8)


def check_table(pattern, angle_deg, edge):
    """the refusals that depend on the table alone; returns the offsets"""
    p = np.asarray(pattern, np.int8).reshape(256, 4)
    if ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any():
        raise ValueError("brief: the two points of a table entry coincide")
    off = offsets(p, angle_deg)
    maxoff = int(np.abs(off).max())
    if edge < maxoff + 4:
        raise ValueError("brief: edge %d is below the table's reach %d + 4" % (edge, maxoff))
    return off


def describe(img, xy, pattern=None, angle_deg=-1.0, edge=31):
    """one job: -> desc [n_desc, 32] u8, desc_pt [n_desc] int32"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    if len(xy) > MAX_PTS:
        raise ValueError("brief: a job has more than 1024 points")
    off = check_table(default_pattern() if pattern is None else pattern, angle_deg, edge)
    x, y = xy[:, 0], xy[:, 1]
    keep = (np.float32(edge) <= x) & (x < np.float32(w - edge)) & (np.float32(edge) <= y) & (y < np.float32(h - edge))
    idx = np.nonzero(keep)[0].astype(np.int32)
    desc = np.zeros((len(idx), 32), np.uint8)
    if len(idx):
        B = blur(img)
        cx, cy = cv_round(x[idx]), cv_round(y[idx])
        for r in range(len(idx)):
            v = B[cy[r] + off[:, 1] - 3, cx[r] + off[:, 0] - 3].astype(np.int64).reshape(256, 2)
            bits = v[:, 0] < v[:, 1]
            for t in np.nonzero(bits)[0]:
                desc[r, t >> 3] |= 1 << (t & 7)
    return desc, idx
