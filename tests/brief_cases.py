"""The cases of svslam_brief_describe_batch, shared by tests/test_host_emulation_brief.py (csrc/k_brief.h compiled for the host) and
tests/test_gpu_brief.py (the device): the boundaries of the code on both sides of each, with tests/ref_brief.py as the reference.
A case is one call: images per slot, jobs (slot, pt_ofs, npts) into one point array, a table, an angle and an edge.

The comparison is exact, so every (table, angle) pair used here must be one for which an ulp of difference between two cosf / sinf
cannot move an offset: the module asserts that no rotated coordinate lies within 1e-3 of a half-integer.  The default table fails
that at 30 degrees (x = 0, y odd gives y / 2), so 30 and 45 degrees run on tables drawn here with such points left out."""
import ctypes as C
import functools

import numpy as np

import ref_brief as rb

NSLOTS = 4
SIZES = {"62x100": (62, 100), "63x63": (63, 63), "96x72": (96, 72), "620x188": (620, 188)}
NPTS = (0, 1, 3, 4, 5, 63, 64, 65, 150, 1024)


# ---- images -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def images(size, kind="random"):
    """the NSLOTS images of a context of that size"""
    w, h = SIZES[size]
    rng = np.random.default_rng([w, h, len(kind)])
    out = []
    for s in range(NSLOTS):
        if kind == "random":
            im = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == "step":                   # a vertical step edge through every patch: flat on both sides, ties for the strict <
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


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _clear_of_half_integers(pt, angle_deg, tol=0.02):
    ang = np.deg2rad(float(angle_deg))
    x = pt[0] * np.cos(ang) - pt[1] * np.sin(ang); y = pt[0] * np.sin(ang) + pt[1] * np.cos(ang)
    return all(abs(v - np.floor(v) - 0.5) > tol for v in (x, y))


@functools.lru_cache(maxsize=None)
def drawn_table(seed, c_max, angle_deg, reach_max, must):
    """256 distinct tests with |c| <= c_max whose rotated points stay clear of half-integers and inside reach_max; `must` is a point
    the table contains (the one that gives it its reach)"""
    rng = np.random.default_rng(seed)
    ang = np.deg2rad(float(angle_deg))

    def ok(pt):
        x = pt[0] * np.cos(ang) - pt[1] * np.sin(ang); y = pt[0] * np.sin(ang) + pt[1] * np.cos(ang)
        return _clear_of_half_integers(pt, angle_deg) and max(abs(round(x)), abs(round(y))) <= reach_max
    assert ok(must)
    rows, seen = [], set()
    while len(rows) < 256:
        a = tuple(int(v) for v in rng.integers(-c_max, c_max + 1, 2)); b = tuple(int(v) for v in rng.integers(-c_max, c_max + 1, 2))
        if len(rows) == 0:
            a = tuple(must)
        if a == b or not ok(a) or not ok(b) or (a + b) in seen:
            continue
        seen.add(a + b); rows.append(a + b)
    t = np.array(rows, np.int8)
    t.setflags(write=False)
    return t


DEFAULT = rb.default_pattern()
TABLE_30 = drawn_table(30, 13, 30.0, 99, (13, -13))
TABLE_45_R21 = drawn_table(45, 15, 45.0, 99, (15, 15))          # (15, 15) -> (0, 21.2): reach 21
TABLE_45_R20 = drawn_table(46, 15, 45.0, 20, (15, 13))          # (15, 13) -> (1.4, 19.8): reach 20, so edge 24 passes and 23 does not
PAIRS_USED = [(DEFAULT, -1.0), (DEFAULT, 0.0), (TABLE_30, 30.0), (DEFAULT, 90.0), (DEFAULT, 180.0), (TABLE_45_R21, 45.0),
              (TABLE_45_R20, 45.0)]
for _t, _a in PAIRS_USED:
    assert rb.half_integer_margin(_t, _a) > 1e-3, (_a, rb.half_integer_margin(_t, _a))
assert int(np.abs(rb.offsets(TABLE_45_R21, 45.0)).max()) == 21 and int(np.abs(rb.offsets(TABLE_45_R20, 45.0)).max()) == 20
assert int(np.abs(TABLE_45_R21).max()) == 15 and int(np.abs(TABLE_45_R20).max()) == 15


# ---- points -----------------------------------------------------------------------------------------------------------------------
def scattered(seed, size, n, edge=31):
    """points over the interior and a band of 6 pixels around it, so the filter drops some"""
    w, h = SIZES[size]
    rng = np.random.default_rng(seed)
    lo = edge - 6.0
    x = rng.uniform(lo, max(w - lo, lo + 1), n); y = rng.uniform(lo, max(h - lo, lo + 1), n)
    return np.stack([x, y], axis=1).astype(np.float32)


def boundary_points(size, edge=31):
    """each filter bound from both sides in x and in y, and the two half-integer centres"""
    w, h = SIZES[size]
    xs = [edge - 0.01, float(edge), w - edge - 0.01, float(w - edge)]
    ys = [edge - 0.01, float(edge), h - edge - 0.01, float(h - edge)]
    pts = [(x, y) for x in xs for y in ys]
    pts += [(40.5, 35.0), (41.5, 35.0), (35.0, 40.5), (35.0, 41.5), (40.5, 40.5), (41.5, 39.5)]
    return np.array(pts, np.float32)


def _case(size, jobs, kind="random", pattern=None, angle_deg=-1.0, edge=31, gaps=None):
    """jobs: list of (slot, xy); gaps[i] points of filler in front of job i"""
    gaps = gaps or [0] * len(jobs)
    parts, j3, o = [], [], 0
    for (slot, xy), gap in zip(jobs, gaps):
        if gap:
            parts.append(np.full((gap, 2), 50.0, np.float32)); o += gap          # would be kept if a job read them
        xy = np.asarray(xy, np.float32).reshape(-1, 2)
        j3.append((slot, o, len(xy))); o += len(xy); parts.append(xy)
    xy = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2), np.float32)
    return dict(size=size, kind=kind, jobs=j3, xy=xy, pattern=pattern, angle_deg=angle_deg, edge=edge)


def _every_second(size):
    p = scattered(7, size, 150); p[:, 0] = np.clip(p[:, 0], 31, SIZES[size][0] - 32); p[:, 1] = np.clip(p[:, 1], 31, SIZES[size][1] - 32)
    p[1::2, 0] = 3.0
    return p


CASES = {
    "no_interior_62x100": lambda: _case("62x100", [(0, scattered(1, "62x100", 40)), (1, [(31.0, 50.0), (30.0, 50.0)])]),
    "one_centre_63x63": lambda: _case("63x63", [(1, [(31.0, 31.0), (31.4, 31.3), (30.99, 31.0), (31.0, 32.0), (31.5, 31.5), (32.0, 31.0),
                                                    (31.99, 31.99)])]),
    "bounds_96x72": lambda: _case("96x72", [(2, boundary_points("96x72"))]),
    "bounds_620x188": lambda: _case("620x188", [(3, boundary_points("620x188"))]),
    "every_second_dropped": lambda: _case("620x188", [(0, _every_second("620x188"))]),
    "jobs_slots_gaps": lambda: _case("620x188", [(2, scattered(11, "620x188", 150)), (0, scattered(12, "620x188", 5)), (3, np.zeros((0, 2))),
                                                  (0, scattered(13, "620x188", 65)), (1, scattered(14, "620x188", 150))],
                                     gaps=[3, 0, 7, 1, 0]),
    "step_edge": lambda: _case("96x72", [(s, scattered(20 + s, "96x72", 40)) for s in range(4)], kind="step"),
    "checkerboard": lambda: _case("96x72", [(s, scattered(30 + s, "96x72", 40)) for s in range(4)], kind="checker"),
    "angle_0": lambda: _case("96x72", [(0, scattered(40, "96x72", 40))], angle_deg=0.0),
    "angle_30": lambda: _case("96x72", [(1, scattered(41, "96x72", 40))], pattern=TABLE_30, angle_deg=30.0),
    "angle_90": lambda: _case("96x72", [(2, scattered(42, "96x72", 40))], angle_deg=90.0),
    "angle_180": lambda: _case("96x72", [(3, scattered(43, "96x72", 40))], angle_deg=180.0),
    "reach21_at_45": lambda: _case("96x72", [(0, scattered(44, "96x72", 40)), (1, boundary_points("96x72"))], pattern=TABLE_45_R21, angle_deg=45.0),
    "reach20_edge24": lambda: _case("96x72", [(0, scattered(45, "96x72", 40, edge=24)), (1, boundary_points("96x72", edge=24))],
                                    pattern=TABLE_45_R20, angle_deg=45.0, edge=24),
    "explicit_default_table": lambda: _case("96x72", [(0, scattered(46, "96x72", 40))], pattern=DEFAULT),
}
for _n in NPTS:
    CASES["npts_%d" % _n] = (lambda n: lambda: _case("620x188", [(n % NSLOTS, scattered(100 + n, "620x188", n))]))(_n)

# (what changes in the good call, the words the refusal must contain)
REFUSALS = {
    "npts_1025": (dict(jobs=[(0, 0, 1025)], total=1025), "1024"),
    "descending": (dict(jobs=[(0, 40, 40), (1, 0, 40)], total=80), "ascend"),
    "overlap": (dict(jobs=[(0, 0, 40), (1, 39, 40)], total=80), "ascend"),
    "leaves_the_arrays": (dict(jobs=[(0, 0, 40), (1, 41, 40)], total=80), "leaves"),
    "negative_offset": (dict(jobs=[(0, -1, 40)], total=80), "leaves"),
    "slot_low": (dict(jobs=[(-1, 0, 40)], total=80), "slot"),
    "slot_high": (dict(jobs=[(0, 0, 40), (NSLOTS, 40, 40)], total=80), "slot"),
    "edge_23_reach_20": (dict(pattern=TABLE_45_R20, angle_deg=45.0, edge=23), "edge"),
    "edge_24_reach_21": (dict(pattern=TABLE_45_R21, angle_deg=45.0, edge=24), "edge"),
    "edge_16_default": (dict(edge=16), "edge"),
    "coincident_entry": (dict(pattern="coincident"), "coincide"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """per job (desc, desc_pt)"""
    c = case(name)
    ims = images(c["size"], c["kind"])
    return tuple(rb.describe(ims[slot], c["xy"][o:o + n], c["pattern"], c["angle_deg"], c["edge"]) for slot, o, n in c["jobs"])


def refusal_call(name):
    """the arguments of abi_call for a refusal: a good call on 96x72 with the named change"""
    change, words = REFUSALS[name]
    total = change.get("total", 80)
    pattern = change.get("pattern")
    if isinstance(pattern, str):
        pattern = np.array(DEFAULT); pattern[200, 2:] = pattern[200, :2]
    c = dict(size="96x72", kind="random", jobs=change.get("jobs", [(0, 0, 40), (1, 40, 40)]),
             xy=np.ascontiguousarray(np.resize(scattered(50, "96x72", 80), (total, 2))), pattern=pattern,
             angle_deg=change.get("angle_deg", -1.0), edge=change.get("edge", 31))
    return c, words


# ---- the ABI, for the device library and for the emulation -----------------------------------------------------------------------------
class Job(C.Structure):
    _fields_ = [("slot", C.c_int), ("pt_ofs", C.c_int), ("npts", C.c_int), ("n_desc", C.c_int), ("reserved", C.c_int)]


class Params(C.Structure):
    _fields_ = [("pattern", C.c_void_p), ("angle_deg", C.c_float), ("edge", C.c_int)]


FILL_DESC, FILL_PT, FILL_N = 0xEE, -7, -5


def abi_call(c, emu=None, ctx=None):
    """one call through the C ABI of the emulation (emu: the CDLL) or of the device library (ctx: a Context of the case's size whose
    slots hold the case's images) -> (rc, error text, [n_desc], desc, desc_pt); the outputs are pre-filled so that a refusal that
    writes, or rows written behind n_desc, show"""
    n = len(c["jobs"])
    arr = (Job * max(n, 1))()
    for i, (slot, o, k) in enumerate(c["jobs"]):
        arr[i].slot, arr[i].pt_ofs, arr[i].npts, arr[i].n_desc = slot, o, k, FILL_N
    xy = np.ascontiguousarray(c["xy"], np.float32)
    total = len(xy)
    pat = None if c["pattern"] is None else np.ascontiguousarray(c["pattern"], np.int8)
    P = Params(None if pat is None else pat.ctypes.data, float(c["angle_deg"]), int(c["edge"]))
    desc = np.full((total, 32), FILL_DESC, np.uint8); dpt = np.full(total, FILL_PT, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if emu is not None:
        w, h = SIZES[c["size"]]
        ims = np.ascontiguousarray(np.stack(images(c["size"], c["kind"])))
        emu.emu_brief_error.restype = C.c_char_p
        rc = emu.emu_brief_describe(w, h, NSLOTS, ptr(ims), n, arr, C.byref(P), total, ptr(xy), ptr(desc), ptr(dpt))
        err = emu.emu_brief_error().decode() if rc else ""
    else:
        rc = ctx.L.svslam_brief_describe_batch(ctx.h, n, arr, C.byref(P), total, ptr(xy), ptr(desc), ptr(dpt))
        err = ctx.L.svslam_last_error(ctx.h).decode() if rc else ""
    return rc, err, [arr[i].n_desc for i in range(n)], desc, dpt


def compare(c, ref, result):
    """exact: n_desc, desc_pt and every descriptor byte of every job; nothing written outside the kept rows"""
    rc, err, nd, desc, dpt = result
    if rc != 0:
        return False, "refused: " + err
    touched_d = np.zeros(len(desc), bool)
    for (slot, o, n), (rd, rp), k in zip(c["jobs"], ref, nd):
        if k != len(rp):
            return False, "n_desc %d, reference %d" % (k, len(rp))
        if not np.array_equal(dpt[o:o + k], rp):
            return False, "desc_pt differs"
        if not np.array_equal(desc[o:o + k], rd):
            bad = np.nonzero((desc[o:o + k] != rd).any(axis=1))[0]
            return False, "descriptor rows %s differ" % bad[:8].tolist()
        touched_d[o:o + k] = True
    if not ((desc[~touched_d] == FILL_DESC).all() and (dpt[~touched_d] == FILL_PT).all()):
        return False, "rows outside the kept ones were written"
    return True, "n_desc %s" % nd


def untouched(result):
    rc, err, nd, desc, dpt = result
    return (desc == FILL_DESC).all() and (dpt == FILL_PT).all() and all(k == FILL_N for k in nd)
