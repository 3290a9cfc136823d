"""Reference for svslam_orb_describe_batch: rBRIEF at keypoints that carry an angle and an octave, what cv::ORB::compute
does with the keypoints cv::ORB::detect returned.  Built from ref_orb (levels, resize) and ref_brief (taps, blur, table) and written
from the contract, not from csrc/k_orb_desc.h; every step is integer, a written-out f32 step or f64 on the host, so the comparison
with the kernel and with its host emulation is exact.  tests/test_ref_orb_desc.py holds this module to facts it does not use itself.

The contract (include/svslam.h):
  levels    scale_L, inv_L = 1.f / scale_L, w_L, h_L are ref_orb.level_geometry's; level L is ref_orb.resize of level L - 1; no mask
  filter    edge <= x < w - edge and edge <= y < h - edge (f32 compares, level 0); then cx = rint(x * inv_L), cy alike: one f32
            product, rounded half to even, inv_0 exactly 1; on a level L >= 1 kept iff edge <= cx < w_L - edge and
            edge <= cy < h_L - edge (on level 0 the first test is the whole filter, as in ref_brief: a centre may round to w - edge).
            Kept points keep their order; desc_pt[row] is the point's index inside the job
  rotation  r = angle * (float)(pi / 180) in f32; a = (float)cos((double)r), b = (float)sin((double)r) with the C library's cos and
            sin (math.cos, not numpy's vectorised one); ix = rint(px a - py b), iy = rint(px b + py a), each product and sum f32
  reach     the largest over the 512 table points of the smallest integer m with m^2 >= px^2 + py^2 (19 for the default table)
  blur, tests, packing   ref_brief's, on the level-`octave` image around (cx, cy)
  refused   npts > 1024, coinciding table points, edge < reach + 4, reach > 24, nlevels outside 1..8, an octave outside
            0 .. nlevels - 1, a non-finite angle (ranges and slots belong to the batch call)
  dropped   a point whose level has no interior; non-finite coordinates
Deviations from OpenCV, declared: the input order is kept (OpenCV sorts by level); a centre that fails the level-L border test is
dropped (OpenCV would read its reflected border) - for a detector keypoint rint(x * inv_L) is the integer it was found at, which
centre() lets a caller assert."""
import math

import numpy as np

import ref_brief as rb
import ref_orb

F = np.float32
MAX_PTS = 1024
MAX_REACH = 24


def reach(pattern):
    p = np.asarray(pattern, np.int8).reshape(512, 2).astype(np.int64)
    q = p[:, 0] ** 2 + p[:, 1] ** 2
    m = np.zeros(512, np.int64)
    while (m * m < q).any():
        m += m * m < q
    return int(m.max())


def rotation(angle_deg):
    """(a, b) as f32"""
    r = F(angle_deg) * F(np.pi / 180.0)
    assert r.dtype == np.float32
    return F(math.cos(float(r))), F(math.sin(float(r)))


def offsets(pattern, angle_deg):
    """[512, 2] integer (ix, iy)"""
    p = np.asarray(pattern, np.int8).reshape(512, 2).astype(np.float32)
    a, b = rotation(angle_deg)
    xa, yb, xb, ya = p[:, 0] * a, p[:, 1] * b, p[:, 0] * b, p[:, 1] * a
    x, y = xa - yb, xb + ya
    assert x.dtype == np.float32 and y.dtype == np.float32
    return np.stack([np.rint(x), np.rint(y)], axis=1).astype(np.int64)


def keypoints(kp):
    """x, y, angle f32 and octave int64 of an ORB keypoint array (ref_orb.KP) or of rows (x, y, angle, octave)"""
    if isinstance(kp, np.ndarray) and kp.dtype.names:
        return kp["x"].astype(np.float32), kp["y"].astype(np.float32), kp["angle"].astype(np.float32), kp["octave"].astype(np.int64)
    rows = np.asarray(kp, np.float64).reshape(-1, 4)
    return rows[:, 0].astype(np.float32), rows[:, 1].astype(np.float32), rows[:, 2].astype(np.float32), rows[:, 3].astype(np.int64)


def check(kp, pattern, edge, nlevels):
    """the refusals one job can show; returns the table, the edge and nlevels after the defaults"""
    p = np.asarray(rb.default_pattern() if pattern is None else pattern, np.int8).reshape(256, 4)
    edge = edge if edge else 31
    nlevels = nlevels if nlevels else 8
    x, y, ang, octv = keypoints(kp)
    if len(x) > MAX_PTS:
        raise ValueError("orb_desc: a job has more than 1024 points")
    if ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any():
        raise ValueError("orb_desc: the two points of a table entry coincide")
    m = reach(p)
    if edge < m + 4:
        raise ValueError("orb_desc: edge %d is below the table's reach %d + 4" % (edge, m))
    if m > MAX_REACH:
        raise ValueError("orb_desc: the table's reach %d is above 24" % m)
    if not 1 <= nlevels <= 8:
        raise ValueError("orb_desc: nlevels is outside 1..8")
    if ((octv < 0) | (octv >= nlevels)).any():
        raise ValueError("orb_desc: a keypoint's octave is outside 0..nlevels-1")
    if not np.isfinite(ang).all():
        raise ValueError("orb_desc: a keypoint's angle is not finite")
    return p, edge, nlevels


def levels(img, lmax):
    """[level 0 .. lmax] of the image, and their (scale, w, h)"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    geo = ref_orb.level_geometry(w, h, lmax + 1)
    out = [img]
    for lv in range(1, lmax + 1):
        out.append(ref_orb.resize(out[-1], geo[lv][1], geo[lv][2]))
    return out, geo


def centre(x, y, scale):
    """(cx, cy) on the level of that scale: one f32 product each, rounded half to even"""
    inv = F(1.0) if scale == F(1.0) else F(1.0) / F(scale)
    return int(np.rint(F(x) * inv)), int(np.rint(F(y) * inv))


def describe(img, kp, pattern=None, edge=0, nlevels=0):
    """one job: -> desc [n_desc, 32] u8, desc_pt [n_desc] int32"""
    p, edge, nlevels = check(kp, pattern, edge, nlevels)
    x, y, ang, octv = keypoints(kp)
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    lv, geo = levels(img, int(octv.max(initial=0)))
    blurred = {}
    rows, idx = [], []
    for i in range(len(x)):
        if not (F(edge) <= x[i] and x[i] < F(w - edge) and F(edge) <= y[i] and y[i] < F(h - edge)):
            continue
        L = int(octv[i])
        scale, lw, lh = geo[L]
        prod = (F(x[i]) * (F(1.0) / scale if L else F(1.0)), F(y[i]) * (F(1.0) / scale if L else F(1.0)))
        cx, cy = int(np.rint(prod[0])), int(np.rint(prod[1]))
        if L > 0 and not (edge <= cx < lw - edge and edge <= cy < lh - edge):
            continue
        if L not in blurred:
            blurred[L] = rb.blur(lv[L])
        off = offsets(p, ang[i])
        v = blurred[L][cy + off[:, 1] - 3, cx + off[:, 0] - 3].astype(np.int64).reshape(256, 2)
        bits = (v[:, 0] < v[:, 1]).astype(np.uint8)
        rows.append(np.packbits(bits, bitorder="little"))
        idx.append(i)
    desc = np.array(rows, np.uint8).reshape(-1, 32)
    return desc, np.array(idx, np.int32)
