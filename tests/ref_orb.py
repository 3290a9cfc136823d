"""A second reading of the ORB detector's contract (include/svslam.h, svslam_orb_detect_batch) in plain numpy, written
from the text and not from csrc/k_orb.h.  The kernel, its host build (tests/cpp/orb_host_emu) and this module meet bit for bit:
every step is integer, a written-out float32 step, or float64 where the contract says so.  Parity with OpenCV is unpinned.

detect(img, rects, ...) returns (keypoints, info): keypoints is a structured array (KP) in the declared order (level ascending,
row-major inside a level, not truncated), info holds the levels, the masks and the per-level counts the case tests ask about."""
import math

import numpy as np

F = np.float32
KP = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
DEFAULTS = dict(nfeatures=500, nlevels=8, fast_threshold=20, edge=31)
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]


def with_defaults(**prm):
    out = dict(DEFAULTS)
    for k, v in prm.items():
        if k not in DEFAULTS:
            raise KeyError(k)
        if v:
            out[k] = int(v)
    return out


def refusal(w, h, nslots, jobs, total_rects, max_out, **prm):
    """None, or why the call is refused; jobs: (slot, rect_ofs, nrect)"""
    p = with_defaults(**prm)
    if p["nfeatures"] < 1 or not 1 <= p["nlevels"] <= 8 or not 1 <= p["fast_threshold"] <= 254 or p["edge"] < 16 or max_out < 1:
        return "parameter"
    for slot, ofs, n in jobs:
        if slot < 0 or slot >= nslots:
            return "slot"
        if n < 0 or ofs < 0 or ofs + n > total_rects:
            return "rects"
    return None


def level_geometry(w, h, nlevels):
    """[(scale f32, w_L, h_L)]"""
    out = []
    for lv in range(nlevels):
        scale = F(math.pow(float(F(1.2)), float(lv)))
        if lv == 0:
            out.append((scale, w, h))
            continue
        inv = F(1.0) / scale
        out.append((scale, int(np.rint(F(w) * inv)), int(np.rint(F(h) * inv))))
    return out


def quotas(nfeatures, nlevels):
    factor = F(1.0 / float(F(1.2)))
    nd = F(nfeatures) * (F(1.0) - factor) / (F(1.0) - F(math.pow(float(factor), float(nlevels))))
    assert nd.dtype == np.float32
    out, total = [], 0
    for _ in range(nlevels - 1):
        n = int(np.rint(nd))
        out.append(n)
        total += n
        nd = F(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


def axis_table(src, dst):
    s = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = s * (d + 0.5) - 0.5
    i = np.floor(f)
    c1 = np.rint((f - i) * 256.0).astype(np.int64)
    i = i.astype(np.int64)
    i0, i1, c0 = i.copy(), i + 1, 256 - c1
    lo, hi = i < 0, i >= src - 1
    i0[lo] = 0; i1[lo] = 0; c0[lo] = 256; c1[lo] = 0
    i0[hi] = src - 1; i1[hi] = src - 1; c0[hi] = 256; c1[hi] = 0
    return i0, i1, c0, c1


def resize(img, dw, dh):
    sh, sw = img.shape
    x0, x1, cx0, cx1 = axis_table(sw, dw)
    y0, y1, cy0, cy1 = axis_table(sh, dh)
    p = img.astype(np.int64)
    t = p[:, x0] * cx0[None, :] + p[:, x1] * cx1[None, :]
    assert t.max(initial=0) <= 65280
    v = t[y0] * cy0[:, None] + t[y1] * cy1[:, None]
    return ((v + 32768) >> 16).astype(np.uint8)


def mask_level0(w, h, rects):
    m = np.full((h, w), 255, np.uint8)
    if rects is None:
        return m
    r = np.asarray(rects, np.float32).reshape(-1, 2)
    for cx, cy in r:
        xa, ya = np.rint(F(cx) - F(10.0)), np.rint(F(cy) - F(10.0))
        xb, yb = np.rint(F(cx) + F(10.0)), np.rint(F(cy) + F(10.0))
        xa, ya, xb, yb = max(xa, 0.0), max(ya, 0.0), min(xb, float(w - 1)), min(yb, float(h - 1))
        if xa <= xb and ya <= yb:
            m[int(ya):int(yb) + 1, int(xa):int(xb) + 1] = 0
    return m


def fast_scores(img, t):
    """the exhaustive definition: score map (int), 0 outside 3 <= x < w - 3, 3 <= y < h - 3 and at non-corners"""
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if w < 7 or h < 7:
        return out
    p = img.astype(np.int32)
    c = p[3:h - 3, 3:w - 3]
    d = np.stack([p[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])          # [16, H, W]
    d2 = np.concatenate([d, d[:8]])
    best = np.full(c.shape, -1000, np.int32)
    for k in range(16):
        arc = d2[k:k + 9]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    out[3:h - 3, 3:w - 3] = np.where(best > t, best - 1, 0)
    return out


def nms(score):
    """corners whose score is strictly above all 8 neighbours' (a neighbour outside the map scores 0)"""
    h, w = score.shape
    pad = np.zeros((h + 2, w + 2), np.int32)
    pad[1:-1, 1:-1] = score
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    return keep


def harris(img, ys, xs):
    p = img.astype(np.int32)
    h, w = p.shape
    ix = np.zeros((h, w), np.int32); iy = np.zeros((h, w), np.int32)
    ix[1:-1, 1:-1] = (p[1:-1, 2:] - p[1:-1, :-2]) * 2 + (p[:-2, 2:] - p[:-2, :-2]) + (p[2:, 2:] - p[2:, :-2])
    iy[1:-1, 1:-1] = (p[2:, 1:-1] - p[:-2, 1:-1]) * 2 + (p[2:, :-2] - p[:-2, :-2]) + (p[2:, 2:] - p[:-2, 2:])
    a = np.zeros(len(ys), np.int64); b = np.zeros(len(ys), np.int64); c = np.zeros(len(ys), np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            gx = ix[ys + dy, xs + dx].astype(np.int64); gy = iy[ys + dy, xs + dx].astype(np.int64)
            a += gx * gx; b += gy * gy; c += gx * gy
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0), np.abs(c).max(initial=0)) < 2 ** 31
    scale = F(1.0) / (F(4 * 7) * F(255.0))
    s4 = F(F(F(scale * scale) * scale) * scale)
    fa, fb, fc = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    det = fa * fb - fc * fc
    tr = fa + fb
    r = (det - F(0.04) * tr * tr) * s4
    assert r.dtype == np.float32 and np.all(np.isfinite(r))
    return r


def umax_table():
    half = 15
    vmax = int(math.floor(float(F(half) * np.sqrt(F(2.0)) / F(2.0) + F(1.0))))
    vmin = int(math.ceil(float(F(half) * np.sqrt(F(2.0)) / F(2.0))))
    u = [0] * (half + 2)
    for v in range(vmax + 1):
        u[v] = int(np.rint(math.sqrt(float(half * half - v * v))))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:16]


UMAX = umax_table()


def atan_deg(y, x):
    """OpenCV's fastAtan2 with the contract's constants, float32 step by step; arrays in, degrees out"""
    y = np.asarray(y, np.float32); x = np.asarray(x, np.float32)
    k = F(180.0 / math.pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * k, F(-0.3258083974640975) * k, F(0.1555786518463281) * k, F(-0.04432655554792128) * k
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    num = np.where(big, ay, ax); den = np.where(big, ax, ay) + eps
    c = (num / den).astype(np.float32)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(big, a, F(90.0) - a).astype(np.float32)
    a = np.where(x < 0, F(180.0) - a, a).astype(np.float32)
    a = np.where(y < 0, F(360.0) - a, a).astype(np.float32)
    return a


def orientation(img, ys, xs):
    p = img.astype(np.int64)
    m10 = np.zeros(len(ys), np.int64); m01 = np.zeros(len(ys), np.int64)
    for v in range(-15, 16):
        um = UMAX[abs(v)]
        for u in range(-um, um + 1):
            val = p[ys + v, xs + u]
            m10 += u * val; m01 += v * val
    return atan_deg(m01.astype(np.float32), m10.astype(np.float32))


def keep_top(values, k):
    """indices (ascending) of everything >= the k-th largest; all when there are no more than k; none when k == 0"""
    n = len(values)
    if k <= 0:
        return np.zeros(0, np.int64)
    if n <= k:
        return np.arange(n)
    thr = np.sort(values)[n - k]
    return np.nonzero(values >= thr)[0]


def detect(img, rects=None, **prm):
    p = with_defaults(**prm)
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    geo = level_geometry(w, h, p["nlevels"])
    quo = quotas(p["nfeatures"], p["nlevels"])
    edge = p["edge"]
    levels, masks, raw_masks = [img], [mask_level0(w, h, rects)], [None]
    for lv in range(1, p["nlevels"]):
        _, lw, lh = geo[lv]
        levels.append(resize(levels[-1], lw, lh))
        raw = resize(masks[-1], lw, lh)
        raw_masks.append(raw)
        masks.append(np.where(raw <= 254, 0, 255).astype(np.uint8))
    rows, per_level = [], []
    for lv in range(p["nlevels"]):
        scale, lw, lh = geo[lv]
        st = dict(level=lv, w=lw, h=lh, quota=quo[lv], nms=np.zeros((0, 2), np.int64), after_mask=0, after_cut1=0, after_cut2=0)
        per_level.append(st)
        if lw <= 2 * edge or lh <= 2 * edge:
            continue
        sc = fast_scores(levels[lv], p["fast_threshold"])
        keep = nms(sc)
        inb = np.zeros_like(keep)
        inb[edge:lh - edge, edge:lw - edge] = True
        keep &= inb
        st["nms"] = np.argwhere(keep)                      # (y, x) after the border filter, before the mask
        keep &= masks[lv] != 0
        ys, xs = np.nonzero(keep)                          # row-major
        st["after_mask"] = len(ys)
        sel = keep_top(sc[ys, xs], 2 * quo[lv])
        ys, xs = ys[sel], xs[sel]
        st["after_cut1"] = len(ys)
        if len(ys) == 0:
            continue
        resp = harris(levels[lv], ys, xs)
        sel = keep_top(resp, quo[lv])
        ys, xs, resp = ys[sel], xs[sel], resp[sel]
        st["after_cut2"] = len(ys)
        if len(ys) == 0:
            continue
        out = np.zeros(len(ys), KP)
        out["x"] = xs.astype(np.float32) * scale
        out["y"] = ys.astype(np.float32) * scale
        out["size"] = F(31.0) * scale
        out["angle"] = orientation(levels[lv], ys, xs)
        out["response"] = resp
        out["octave"] = lv
        rows.append(out)
    kps = np.concatenate(rows) if rows else np.zeros(0, KP)
    return kps, dict(levels=levels, masks=masks, raw_masks=raw_masks, per_level=per_level, geometry=geo, quotas=quo, params=p)
