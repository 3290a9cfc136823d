"""The cases of svslam_orb_describe_batch, shared by tests/test_host_emulation_orb_desc.py (csrc/k_orb_desc.h compiled for the host) and
tests/test_gpu_orb_desc.py (the device): the smallest shapes at which each boundary of the code exists, with tests/ref_orb_desc.py as
the reference.  A case is one call: images per slot, jobs (slot, pt_ofs, npts) into one keypoint array, a table, an edge, nlevels.

Unlike brief_cases.py no (table, angle) pair has to stay clear of half-integers: cos and sin are the host's, in the library and in the
reference alike, and the device's part of the rotation is four f32 products, two sums and a rounding."""
import ctypes as C
import functools
import os

import numpy as np

import ref_brief as rb
import ref_orb
import ref_orb_desc as rod

NSLOTS = 4
SIZES = {"63x63": (63, 63), "160x120": (160, 120), "300x240": (300, 240), "620x188": (620, 188)}
NPTS = (0, 1, 3, 4, 5, 64, 65, 1024)
KP = ref_orb.KP
ANGLES = (-1.0, 0.0, 90.0, 180.0, 270.0, 359.99, 45.0, 1e-3)


@functools.lru_cache(maxsize=None)
def images(size, kind="random"):
    """the NSLOTS images of a context of that size"""
    w, h = SIZES[size]
    rng = np.random.default_rng([w, h, len(kind), 17])
    out = []
    for s in range(NSLOTS):
        if kind == "random":
            im = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == "step":                   # a vertical step edge: flat on both sides, ties for the strict <
            im = np.full((h, w), 10 + s, np.uint8); im[:, w // 2 + s:] = 200
        elif kind == "checker":                # 0 / 255 cells of 1, 2, 5 and 9 pixels: rounding near 127.5 and at saturation
            c = (1, 2, 5, 9)[s]
            yy, xx = np.mgrid[0:h, 0:w]
            im = ((((xx // c) + (yy // c)) & 1) * 255).astype(np.uint8)
        else:
            raise KeyError(kind)
        im.setflags(write=False)
        out.append(im)
    return tuple(out)


def geometry(size):
    w, h = SIZES[size]
    return ref_orb.level_geometry(w, h, 8)


def kps(rows):
    """rows of (x, y, angle, octave) -> KP array"""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    out = np.zeros(len(rows), KP)
    out["x"], out["y"], out["angle"], out["octave"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3].astype(np.int32)
    out["size"], out["response"] = 31.0, 1e-4           # ignored
    return out


def on_level(size, level, xi, yi, angle):
    """the keypoint the detector would emit for pixel (xi, yi) of that level: x = (float)xi * scale_L"""
    scale = geometry(size)[level][0]
    return (float(np.float32(xi) * scale), float(np.float32(yi) * scale), float(angle), level)


def level_points(seed, size, level, n, edge=31, band=3, angles=None):
    """n detector-style keypoints on a level: integer pixels over the level's interior and a band around it (the band is dropped by
    one of the two border tests), random angles"""
    _, lw, lh = geometry(size)[level]
    rng = np.random.default_rng([seed, level])
    lo = edge - band
    xi = rng.integers(lo, max(lw - lo, lo + 1), n); yi = rng.integers(lo, max(lh - lo, lo + 1), n)
    ang = rng.uniform(0.0, 360.0, n) if angles is None else np.resize(np.asarray(angles, np.float64), n)
    return [on_level(size, level, x, y, a) for x, y, a in zip(xi, yi, ang)]


def tracked_points(seed, size, n, edge=31):
    """what a tracked feature carries: any float position, angle -1, octave 0"""
    w, h = SIZES[size]
    rng = np.random.default_rng(seed)
    lo = edge - 4.0
    x = rng.uniform(lo, max(w - lo, lo + 1), n); y = rng.uniform(lo, max(h - lo, lo + 1), n)
    return [(float(np.float32(a)), float(np.float32(b)), -1.0, 0) for a, b in zip(x, y)]


def mixed_points(seed, size, n, lmax, edge=31):
    """tracked and detected keypoints interleaved, octaves 0 .. lmax"""
    rng = np.random.default_rng([seed, 99])
    out = []
    det = {lv: level_points(seed + lv, size, lv, n, edge) for lv in range(lmax + 1)}
    trk = tracked_points(seed, size, n, edge)
    for i in range(n):
        out.append(trk[i] if rng.integers(0, 3) == 0 else det[int(rng.integers(0, lmax + 1))][i])
    return out


def level0_border(size, edge=31):
    w, h = SIZES[size]
    xs = [edge - 0.01, float(edge), w - edge - 0.01, float(w - edge)]
    ys = [edge - 0.01, float(edge), h - edge - 0.01, float(h - edge)]
    return [(x, y, a, o) for x in xs for y in ys for a, o in ((-1.0, 0), (33.0, 1))]


def level_border(size, level, edge=31):
    """centres at cx = edge - 1, edge, w_L - edge - 1, w_L - edge, and in y alike"""
    _, lw, lh = geometry(size)[level]
    xs = [edge - 1, edge, lw - edge - 1, lw - edge]; ys = [edge - 1, edge, lh - edge - 1, lh - edge]
    pts = [on_level(size, level, x, y, 10.0 * level + i) for i, (x, y) in enumerate((x, y) for x in xs for y in ys)]
    for (x, y, _, lv), (xi, yi) in zip(pts, ((x, y) for x in xs for y in ys)):
        assert rod.centre(x, y, geometry(size)[lv][0]) == (xi, yi)
    return pts


@functools.lru_cache(maxsize=None)
def half_integer_points(size):
    """level-0 coordinates whose f32 product with inv_L is exactly k + 0.5: they must round to the even neighbour"""
    out = []
    for lv in (1, 2, 3):
        scale, lw, lh = geometry(size)[lv]
        inv = np.float32(1.0) / scale
        found = {0: None, 1: None}
        for k in range(34, lw - 34):
            x = np.float32((k + 0.5) * float(scale))
            for _ in range(8):
                x = np.nextafter(x, np.float32(0))
            for _ in range(16):
                if float(x * inv) == k + 0.5 and found[k & 1] is None:
                    found[k & 1] = (float(x), k)
                x = np.nextafter(x, np.float32(1e9))
        for par in (0, 1):
            assert found[par] is not None, (size, lv, par)
            x, k = found[par]
            y = float(np.float32(40) * scale)
            assert rod.centre(x, y, scale)[0] == (k if k % 2 == 0 else k + 1)
            out += [(x, y, 77.0, lv), (y, x, 200.0, lv)] if x < SIZES[size][1] - 31 else [(x, y, 77.0, lv)]
    return out


@functools.lru_cache(maxsize=None)
def table_c15(seed=5):
    """256 distinct tests with |c| <= 15 that contain (15, 15): reach 22"""
    rng = np.random.default_rng(seed)
    rows, seen = [(15, 15, -3, 2)], {(15, 15, -3, 2)}
    while len(rows) < 256:
        r = tuple(int(v) for v in rng.integers(-15, 16, 4))
        if r[:2] == r[2:] or r in seen:
            continue
        seen.add(r); rows.append(r)
    t = np.array(rows, np.int8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def contraction_angles(want=6):
    """angles at which some point of the default table lands so close to a half-integer that a contracted multiply-add (one rounding
    for px a - py b instead of two) rounds it to the other integer.  For a table point at distance r and a half-integer t < r the
    angle with px cos - py sin = t is atan2(py, px) inverted; the f32 angles around it are tried with both arithmetics (the f64
    product of two f32 is exact, so one rounding of it is the fused result)."""
    pts = rb.default_pattern().reshape(512, 2).astype(np.float64)
    out = []
    for px, py in pts[::7]:
        r = np.hypot(px, py)
        for t in np.arange(0.5, r, 1.0):
            th = np.degrees(np.arccos(t / r) - np.arctan2(py, px)) % 360.0
            a32 = np.float32(th)
            cand = [a32]
            for _ in range(6):
                cand.append(np.nextafter(cand[-1], np.float32(1e9)))
            for ang in cand:
                a, b = rod.rotation(ang)
                plain = np.float32(np.float32(px) * a) - np.float32(np.float32(py) * b)
                fused = np.float32(float(np.float32(px)) * float(a) - float(np.float32(np.float32(py) * b)))
                if np.rint(plain) != np.rint(fused):
                    out.append(float(ang))
                    break
            if len(out) >= want:
                return tuple(out)
    return tuple(out)


DEFAULT = rb.default_pattern()
assert len(contraction_angles()) >= 3
assert rod.reach(DEFAULT) == 19 and rod.reach(table_c15()) == 22


def _case(size, jobs, kind="random", pattern=None, edge=0, nlevels=0, gaps=None):
    """jobs: list of (slot, rows of (x, y, angle, octave)); gaps[i] keypoints of filler in front of job i"""
    gaps = gaps or [0] * len(jobs)
    parts, j3, o = [], [], 0
    for (slot, rows), gap in zip(jobs, gaps):
        if gap:
            parts.append(kps([(50.0, 50.0, 5.0, 0)] * gap)); o += gap          # would be kept if a job read them
        k = kps(rows)
        j3.append((slot, o, len(k))); o += len(k); parts.append(k)
    allk = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, KP)
    return dict(size=size, kind=kind, jobs=j3, kps=allk, pattern=pattern, edge=edge, nlevels=nlevels)


def _sweep(size):
    rng = np.random.default_rng(360)
    ang = np.concatenate([np.array(ANGLES), rng.uniform(0.0, 360.0, 360)])
    lv = rng.integers(0, 4, len(ang))
    _, lw, lh = geometry(size)[3]
    return [on_level(size, int(l), int(rng.integers(31, geometry(size)[l][1] - 31)), int(rng.integers(31, geometry(size)[l][2] - 31)), a)
            for l, a in zip(lv, ang)]


CASES = {
    # levels 0-3 of 160 x 120 have an interior, level 4 (77 x 58) has none: its points are dropped
    "levels_160x120": lambda: _case("160x120", [(0, sum((level_points(1, "160x120", lv, 12) for lv in range(6)), []))]),
    # all eight levels have an interior; level 7 is 84 x 67, interior 22 x 5
    "all_levels_300x240": lambda: _case("300x240", [(1, sum((level_points(2, "300x240", lv, 10) for lv in range(8)), []))]),
    # level 6 is 208 x 63: one interior row; level 7 has none
    "one_row_620x188": lambda: _case("620x188", [(2, sum((level_points(3, "620x188", lv, 16) for lv in (0, 5, 6, 7)), []) +
                                                  [on_level("620x188", 6, x, y, 7.0 * x) for y in (30, 31, 32) for x in (30, 31, 100, 176, 177)])]),
    "one_centre_63x63": lambda: _case("63x63", [(1, [(31.0, 31.0, 12.0, 0), (31.4, 31.3, 300.0, 0), (30.99, 31.0, 0.0, 0), (31.0, 32.0, 1.0, 0),
                                                    (31.5, 31.5, 2.0, 0), (31.0, 31.0, 3.0, 1), (31.99, 31.99, 4.0, 0)])]),
    "level0_border": lambda: _case("160x120", [(2, level0_border("160x120"))]),
    "level_border": lambda: _case("300x240", [(3, level_border("300x240", 1) + level_border("300x240", 2) + level_border("300x240", 7))]),
    "half_integer_centres": lambda: _case("300x240", [(0, half_integer_points("300x240"))]),
    "angles": lambda: _case("160x120", [(1, [on_level("160x120", lv, 40 + i, 33 + lv, a) for lv in (0, 2) for i, a in enumerate(ANGLES)])]),
    "contraction_sensitive": lambda: _case("160x120", [(2, [on_level("160x120", lv, 45 + 3 * i, 40 - lv, a) for lv in (0, 1)
                                                            for i, a in enumerate(contraction_angles())])]),
    "angle_sweep": lambda: _case("160x120", [(3, _sweep("160x120"))]),
    "tracked_and_detected": lambda: _case("300x240", [(0, mixed_points(4, "300x240", 80, 5))]),
    "jobs_slots_gaps": lambda: _case("620x188", [(2, mixed_points(11, "620x188", 150, 5)), (0, mixed_points(12, "620x188", 5, 2)), (3, []),
                                                  (0, tracked_points(13, "620x188", 65)), (1, mixed_points(14, "620x188", 150, 6))],
                                     gaps=[3, 0, 7, 1, 0]),
    "step_edge": lambda: _case("160x120", [(s, mixed_points(20 + s, "160x120", 40, 3)) for s in range(4)], kind="step"),
    "checkerboard": lambda: _case("160x120", [(s, mixed_points(30 + s, "160x120", 40, 3)) for s in range(4)], kind="checker"),
    "reach22_edge26": lambda: _case("160x120", [(0, mixed_points(44, "160x120", 40, 3, edge=26)), (1, level0_border("160x120", edge=26))],
                                    pattern=table_c15(), edge=26),
    "explicit_defaults": lambda: _case("160x120", [(0, mixed_points(46, "160x120", 40, 3))], pattern=DEFAULT, edge=31, nlevels=8),
    "nlevels_3": lambda: _case("160x120", [(0, mixed_points(47, "160x120", 40, 2))], nlevels=3),
    "all_octave_0": lambda: _case("160x120", [(0, tracked_points(48, "160x120", 40)), (1, level_points(49, "160x120", 0, 40))]),
    "not_finite_coordinates": lambda: _case("160x120", [(0, [(np.nan, 50.0, 1.0, 0), (50.0, np.inf, 1.0, 1), (-np.inf, 50.0, 1.0, 0),
                                                             (50.0, 50.0, 1.0, 1), (np.nan, np.nan, 1.0, 2)])]),
}
for _n in NPTS:
    CASES["npts_%d" % _n] = (lambda n: lambda: _case("620x188", [(n % NSLOTS, mixed_points(100 + n, "620x188", n, 4))]))(_n)

# (what changes in the good call, the words the refusal must contain, the reference's words)
REFUSALS = {
    "npts_1025": (dict(jobs=[(0, 0, 1025)], total=1025), "1024"),
    "descending": (dict(jobs=[(0, 40, 40), (1, 0, 40)]), "ascend"),
    "overlap": (dict(jobs=[(0, 0, 40), (1, 39, 40)]), "ascend"),
    "leaves_the_arrays": (dict(jobs=[(0, 0, 40), (1, 41, 40)]), "leaves"),
    "negative_offset": (dict(jobs=[(0, -1, 40)]), "leaves"),
    "negative_npts": (dict(jobs=[(0, 0, -1)]), "leaves"),
    "slot_low": (dict(jobs=[(-1, 0, 40)]), "slot"),
    "slot_high": (dict(jobs=[(0, 0, 40), (NSLOTS, 40, 40)]), "slot"),
    "edge_25_reach_22": (dict(pattern=table_c15(), edge=25), "edge"),
    "edge_22_default": (dict(edge=22), "edge"),
    "coincident_entry": (dict(pattern="coincident"), "coincide"),
    "reach_25": (dict(pattern="reach25", edge=40), "24"),
    "nlevels_9": (dict(nlevels=9), "nlevels"),
    "nlevels_negative": (dict(nlevels=-1), "nlevels"),
    "octave_8": (dict(point=(7, "octave", 8)), "octave"),
    "octave_negative": (dict(point=(41, "octave", -1)), "octave"),
    "octave_at_nlevels": (dict(nlevels=3, point=(7, "octave", 3)), "octave"),
    "angle_nan": (dict(point=(79, "angle", np.nan)), "angle"),
    "angle_inf": (dict(point=(0, "angle", np.inf)), "angle"),
}
# the accepted neighbour of each refusal: the same call with the bound met
ACCEPTED = {
    "npts_1024": dict(jobs=[(0, 0, 1024)], total=1024),
    "touching_ranges": dict(jobs=[(0, 0, 40), (1, 40, 40)]),
    "gap_between_ranges": dict(jobs=[(0, 0, 39), (1, 41, 39)]),
    "last_slot": dict(jobs=[(0, 0, 40), (NSLOTS - 1, 40, 40)]),
    "edge_26_reach_22": dict(pattern=table_c15(), edge=26),
    "edge_23_default": dict(edge=23),
    "reach_24": dict(pattern="reach24", edge=40),
    "nlevels_8": dict(nlevels=8),
    "nlevels_1": dict(nlevels=1, all_octave=0),
    "octave_7": dict(point=(7, "octave", 7)),
    "octave_2_of_3": dict(nlevels=3, point=(7, "octave", 2), all_octave=1),
    "angle_huge": dict(point=(79, "angle", 3.0e38)),
    "angle_flt_max": dict(point=(3, "angle", float(np.finfo(np.float32).max))),
    "angle_minus_flt_max": dict(point=(44, "angle", -float(np.finfo(np.float32).max))),
    "bad_point_in_a_gap": dict(jobs=[(0, 0, 39), (1, 41, 39)], point=(40, "octave", 99)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """per job (desc, desc_pt)"""
    c = case(name)
    ims = images(c["size"], c["kind"])
    return tuple(rod.describe(ims[slot], c["kps"][o:o + n], c["pattern"], c["edge"], c["nlevels"]) for slot, o, n in c["jobs"])


def changed_call(change):
    """a good call on 160x120 (two jobs of 40 mixed keypoints) with the named change"""
    total = change.get("total", 80)
    pattern = change.get("pattern")
    if isinstance(pattern, str):
        t = np.array(DEFAULT)
        if pattern == "coincident":
            t[200, 2:] = t[200, :2]
        elif pattern == "reach24":
            t[0] = (24, 0, 1, 1)
        elif pattern == "reach25":
            t[0] = (24, 1, 1, 1)
        pattern = t
    k = np.resize(kps(mixed_points(50, "160x120", 80, 3, edge=change.get("edge", 0) or 31)), total)
    if "all_octave" in change:
        k["octave"] = np.minimum(k["octave"], change["all_octave"])
    if "point" in change:
        i, field, v = change["point"]
        k[field][i] = v
    return dict(size="160x120", kind="random", jobs=change.get("jobs", [(0, 0, 40), (1, 40, 40)]), kps=np.ascontiguousarray(k), pattern=pattern,
                edge=change.get("edge", 0), nlevels=change.get("nlevels", 0))


# ---- the ABI, for the device library and for the emulation -----------------------------------------------------------------------------
class Job(C.Structure):
    _fields_ = [("slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int), ("n_desc", C.c_int), ("reserved", C.c_int)]


class Params(C.Structure):
    _fields_ = [("pattern", C.c_void_p), ("edge", C.c_int), ("nlevels", C.c_int), ("reserved", C.c_int)]


FILL_DESC, FILL_PT, FILL_N = 0xEE, -7, -5


def abi_call(c, emu=None, ctx=None, budget=0):
    """one call through the C ABI of the emulation (emu: the CDLL; budget in bytes) or of the device library (ctx: a Context of the
    case's size whose slots hold the case's images; budget in MB through SVSLAM_ORB_BUDGET_MB) -> (rc, error text, [n_desc], desc,
    desc_pt); the outputs are pre-filled so that a refusal that writes, or rows written behind n_desc, show"""
    n = len(c["jobs"])
    arr = (Job * max(n, 1))()
    for i, (slot, o, k) in enumerate(c["jobs"]):
        arr[i].slot, arr[i].pt_ofs, arr[i].npts, arr[i].n_desc = slot, o, k, FILL_N
    kp = np.ascontiguousarray(c["kps"], KP)
    total = len(kp)
    pat = None if c["pattern"] is None else np.ascontiguousarray(c["pattern"], np.int8)
    P = Params(None if pat is None else pat.ctypes.data, int(c["edge"]), int(c["nlevels"]), 0)
    desc = np.full((max(total, 1), 32), FILL_DESC, np.uint8); dpt = np.full(max(total, 1), FILL_PT, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    kptr = ptr(kp) if total else None
    if emu is not None:
        w, h = SIZES[c["size"]]
        ims = np.ascontiguousarray(np.stack(images(c["size"], c["kind"])))
        emu.emu_orb_desc_error.restype = C.c_char_p
        rc = emu.emu_orb_desc_describe(w, h, NSLOTS, ptr(ims), n, arr, C.byref(P), total, kptr, ptr(desc), ptr(dpt), C.c_longlong(budget))
        err = emu.emu_orb_desc_error().decode() if rc else ""
    else:
        old = os.environ.get("SVSLAM_ORB_BUDGET_MB")
        if budget:
            os.environ["SVSLAM_ORB_BUDGET_MB"] = str(int(budget))
        try:
            rc = ctx.L.svslam_orb_describe_batch(ctx.h, n, arr, C.byref(P), total, kptr, ptr(desc), ptr(dpt))
        finally:
            if budget:
                if old is None:
                    del os.environ["SVSLAM_ORB_BUDGET_MB"]
                else:
                    os.environ["SVSLAM_ORB_BUDGET_MB"] = old
        err = ctx.L.svslam_last_error(ctx.h).decode() if rc else ""
    return rc, err, [arr[i].n_desc for i in range(n)], desc[:total], dpt[:total]


def emu_stats(emu):
    """of the emulation's last call: chunks, resize launches, bytes of level storage, the table's reach"""
    out = (C.c_longlong * 4)()
    emu.emu_orb_desc_stats(out)
    return dict(chunks=out[0], resizes=out[1], level_bytes=out[2], reach=out[3])


def compare(c, ref, result):
    """exact: n_desc, desc_pt and every descriptor byte of every job; nothing written outside the kept rows"""
    rc, err, nd, desc, dpt = result
    if rc != 0:
        return False, "refused: " + err
    touched = np.zeros(len(desc), bool)
    for (slot, o, n), (rd, rp), k in zip(c["jobs"], ref, nd):
        if k != len(rp):
            return False, "n_desc %d, reference %d" % (k, len(rp))
        if not np.array_equal(dpt[o:o + k], rp):
            return False, "desc_pt differs"
        if not np.array_equal(desc[o:o + k], rd):
            bad = np.nonzero((desc[o:o + k] != rd).any(axis=1))[0]
            return False, "descriptor rows %s of the job at %d differ" % (bad[:8].tolist(), o)
        touched[o:o + k] = True
    if not ((desc[~touched] == FILL_DESC).all() and (dpt[~touched] == FILL_PT).all()):
        return False, "rows outside the kept ones were written"
    return True, "n_desc %s" % nd


def untouched(result):
    rc, err, nd, desc, dpt = result
    return bool((desc == FILL_DESC).all() and (dpt == FILL_PT).all() and all(k == FILL_N for k in nd))


def kept_levels(name):
    """the octaves of the rows the reference keeps, all jobs together"""
    c = case(name)
    out = []
    for (slot, o, n), (_, rp) in zip(c["jobs"], reference(name)):
        out += c["kps"]["octave"][o:o + n][rp].tolist()
    return out
