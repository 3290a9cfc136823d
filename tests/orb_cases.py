"""The ORB detector's cases (svslam_orb_detect_batch), shared by the host-emulation test and the GPU tests: the smallest
shapes at which the thing can go wrong, the reference's result per case (computed once), the packing of a case into the C-ABI's
arrays and the bit-for-bit comparison."""
import ctypes as C
import functools

import numpy as np

import ref_orb


class Case:
    def __init__(self, w, h, imgs, jobs, max_out=2000, **prm):
        self.w, self.h, self.imgs, self.jobs, self.max_out, self.prm = w, h, imgs, jobs, max_out, prm     # jobs: [(slot, rects or None)]


def blocks(w, h, seed):
    """random blocks of two sizes plus a little texture: corners at every scale of the pyramid"""
    r = np.random.RandomState(seed)
    big = np.kron(r.randint(0, 190, (h // 32 + 1, w // 32 + 1)), np.ones((32, 32), np.int64))[:h, :w]
    small = np.kron(r.randint(0, 60, (h // 9 + 1, w // 9 + 1)), np.ones((9, 9), np.int64))[:h, :w]
    return np.clip(big + small + r.randint(-3, 4, (h, w)), 0, 255).astype(np.uint8)


def squares(w, h):
    """identical bright squares on a dark ground (a checkerboard of isolated squares: the X junctions of a plain checkerboard are no
    FAST corners): every square corner has the same FAST score and the same response"""
    img = np.full((h, w), 40, np.uint8)
    for y in range(34, h - 40, 14):
        for x in range(34, w - 40, 14):
            img[y:y + 7, x:x + 7] = 220
            img[y:y + 7:6, x:x + 7:6] = 250          # the four corner pixels: alone above their neighbours' scores
    return img


def one_corner(w, h):
    """a bright square whose corner pixel is the image's centre"""
    img = np.full((h, w), 30, np.uint8)
    img[h // 2:h // 2 + 14, w // 2:w // 2 + 14] = 200
    img[h // 2, w // 2] = 240
    return img


def _case(w, h, seed=1, rects=None, **kw):
    return Case(w, h, [blocks(w, h, seed)], [(0, rects)], **kw)


def _corner_rects(w, h):
    return np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w / 2, h / 2]], np.float32)


@functools.lru_cache(maxsize=None)
def _between_pixels_rects():
    """a rect whose right edge falls between two level-1 pixels at a level-1 keypoint of the unmasked image: searched once"""
    w, h = 160, 120
    img = blocks(w, h, 1)
    kps, _ = ref_orb.detect(img, None, nfeatures=150)
    for k in kps[kps["octave"] == 1]:
        for dx in range(-4, 5):
            rect = np.array([[np.floor(k["x"]) + dx - 10, k["y"]]], np.float32)
            if between_pixels_shows(img, rect):
                return rect
    raise AssertionError("no rect found")


def between_pixels_shows(img, rect):
    """a level >= 1 point that the '<= 254 becomes 0' step removes and a nearest-neighbour mask would keep"""
    _, info = ref_orb.detect(img, rect, nfeatures=150)
    m0 = info["masks"][0]
    for lv in range(1, len(info["levels"])):
        scale = float(info["geometry"][lv][0])
        for y, x in info["per_level"][lv]["nms"]:
            if info["masks"][lv][y, x] == 0 and 0 < info["raw_masks"][lv][y, x] <= 254:
                ny, nx = min(int(round(y * scale)), m0.shape[0] - 1), min(int(round(x * scale)), m0.shape[1] - 1)
                if m0[ny, nx] == 255:
                    return True
    return False


def _jobs_slots_gaps():
    w, h = 160, 120
    imgs = [blocks(w, h, s) for s in (1, 2, 3, 4, 5, 6)]
    r = np.random.RandomState(9)
    many = np.stack([r.uniform(-5, w + 5, 40), r.uniform(-5, h + 5, 40)], axis=1).astype(np.float32)
    jobs = [(5, None), (0, np.array([[80, 60]], np.float32)), (3, many), (3, None), (1, many[:7])]
    return Case(w, h, imgs, jobs, nfeatures=150)


CASES = {
    "all_levels_300x230_n150": lambda: _case(300, 230, seed=2, nfeatures=150),
    "all_levels_300x230_n500": lambda: _case(300, 230, seed=2, nfeatures=500),
    "four_levels_160x120": lambda: _case(160, 120, nfeatures=150),
    "odd_161x121": lambda: _case(161, 121, seed=2, nfeatures=150),
    "no_interior_62x100": lambda: _case(62, 100, nfeatures=150),
    "one_interior_63x63": lambda: Case(63, 63, [one_corner(63, 63)], [(0, None)], nfeatures=150),
    "flat": lambda: Case(160, 120, [np.full((120, 160), 77, np.uint8)], [(0, None)], nfeatures=150),
    "checkerboard": lambda: Case(200, 160, [squares(200, 160)], [(0, None)], nfeatures=150),
    "nfeatures_1": lambda: _case(160, 120, nfeatures=1),
    "nfeatures_5": lambda: _case(160, 120, nfeatures=5),
    "nlevels_1": lambda: _case(160, 120, nfeatures=150, nlevels=1),
    "nlevels_3": lambda: _case(160, 120, nfeatures=150, nlevels=3),
    "fast_threshold_1": lambda: _case(160, 120, nfeatures=150, fast_threshold=1),
    "fast_threshold_254": lambda: _case(160, 120, nfeatures=150, fast_threshold=254),
    "edge_16": lambda: _case(160, 120, nfeatures=150, edge=16),
    "mask_corners": lambda: _case(160, 120, rects=_corner_rects(160, 120), nfeatures=150),
    "mask_outside": lambda: _case(160, 120, rects=np.array([[-30, -30], [-5, 60], [165, 118], [400, 400], [80, -10]], np.float32), nfeatures=150),
    "mask_between_pixels": lambda: _case(160, 120, rects=_between_pixels_rects(), nfeatures=150),
    "mask_everything": lambda: _case(160, 120, rects=np.array([[x, y] for y in range(0, 130, 20) for x in range(0, 170, 20)], np.float32),
                                     nfeatures=150),
    "jobs_slots_gaps": _jobs_slots_gaps,
    "max_out_truncates": lambda: _case(160, 120, nfeatures=150, max_out=37),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """per job (keypoints, info) of ref_orb, not truncated; computed once and left unchanged"""
    c = case(name)
    out = []
    for slot, rects in c.jobs:
        kps, info = ref_orb.detect(c.imgs[slot], rects, **c.prm)
        kps.setflags(write=False)
        out.append((kps, info))
    return out


def pack(c):
    """the C-ABI's arrays of a case: images [nslots, h, w], [(slot, rect_ofs, nrect)], rect_xy [total, 2]"""
    jobs, parts, o = [], [], 0
    for slot, rects in c.jobs:
        r = np.zeros((0, 2), np.float32) if rects is None else np.asarray(rects, np.float32).reshape(-1, 2)
        jobs.append((slot, o, len(r)))
        o += len(r)
        parts.append(r)
    rect = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(np.stack(c.imgs)), jobs, rect


def compare(got, n_found, ref_kps, max_out, what=""):
    """got: the rows a call wrote for one job (structured, ref_orb.KP); bit for bit the first min(n_found, max_out) rows of the reference"""
    assert n_found == len(ref_kps), "%s: n_found %d, the reference has %d" % (what, n_found, len(ref_kps))
    want = ref_kps[:max_out]
    assert len(got) == len(want), "%s: %d rows written, %d expected" % (what, len(got), len(want))
    for f in ref_orb.KP.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
        assert bad.size == 0, "%s: field %s differs at row %d: %r vs %r (%d rows differ)" % (what, f, bad[0], a[bad[0]], b[bad[0]], bad.size)


# every refusal with the accepted side next to it: (name, changes to a call that is accepted, is it refused)
BASE_CALL = dict(nfeatures=150, nlevels=8, fast_threshold=20, edge=31, max_out=100, slot=0, rect_ofs=0, nrect=2, total_rects=2)
REFUSALS = [
    ("nfeatures_minus_1", dict(nfeatures=-1), True), ("nfeatures_1", dict(nfeatures=1), False),
    ("nlevels_9", dict(nlevels=9), True), ("nlevels_minus_1", dict(nlevels=-1), True), ("nlevels_8", dict(nlevels=8), False), ("nlevels_1", dict(nlevels=1), False),
    ("fast_threshold_255", dict(fast_threshold=255), True), ("fast_threshold_minus_1", dict(fast_threshold=-1), True),
    ("fast_threshold_254", dict(fast_threshold=254), False), ("fast_threshold_1", dict(fast_threshold=1), False),
    ("edge_15", dict(edge=15), True), ("edge_16", dict(edge=16), False),
    ("max_out_0", dict(max_out=0), True), ("max_out_1", dict(max_out=1), False),
    ("slot_minus_1", dict(slot=-1), True), ("slot_nslots", dict(slot=2), True), ("slot_last", dict(slot=1), False),
    ("rects_past_end", dict(rect_ofs=1, nrect=2), True), ("rects_negative_ofs", dict(rect_ofs=-1, nrect=1), True),
    ("rects_negative_count", dict(nrect=-1), True), ("rects_to_the_end", dict(rect_ofs=1, nrect=1), False),
    ("defaults", dict(nfeatures=0, nlevels=0, fast_threshold=0, edge=0), False),
]


class _Job(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("slot", "rect_ofs", "nrect", "n_out", "n_found", "reserved")]


class _Prm(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nfeatures", "nlevels", "fast_threshold", "edge")]


SENTINEL = -7


def abi_call(w, h, imgs, jobs, rect, total_rects, max_out, prm, emu=None, ctx=None, budget=0):
    """one call through the raw C ABI of the host build (emu) or of the library (ctx: a Context of w x h whose slots hold imgs).
    jobs: [(slot, rect_ofs, nrect)].  Returns (rc, message, [(n_out, n_found)], out [njobs, rows] of ref_orb.KP); the outputs start
    from a sentinel, so that a refusal that wrote anything shows."""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = len(jobs)
    arr = (_Job * max(n, 1))(*[_Job(s, o, k, SENTINEL, SENTINEL, 0) for s, o, k in jobs])
    P = _Prm(*[int(prm.get(k, 0)) for k in ("nfeatures", "nlevels", "fast_threshold", "edge")])
    out = np.zeros((max(n, 1), max(max_out, 1)), ref_orb.KP)
    out.view(np.uint8)[...] = 0xC3
    rect = np.ascontiguousarray(rect, np.float32) if len(rect) else np.zeros((1, 2), np.float32)
    if emu is not None:
        emu.emu_orb_error.restype = C.c_char_p
        imgs = np.ascontiguousarray(imgs)
        rc = emu.emu_orb_detect(w, h, len(imgs), p(imgs), n, arr, C.byref(P), total_rects, p(rect), max_out, p(out), C.c_longlong(budget))
        msg = emu.emu_orb_error().decode() if rc else ""
    else:
        rc = ctx.L.svslam_orb_detect_batch(ctx.h, n, arr, C.byref(P), total_rects, p(rect), max_out, p(out))
        msg = ctx.L.svslam_last_error(ctx.h).decode() if rc else ""
    return rc, msg, [(arr[i].n_out, arr[i].n_found) for i in range(n)], out


def run_case(c, emu=None, ctx=None, budget=0):
    imgs, jobs, rect = pack(c)
    return abi_call(c.w, c.h, imgs, jobs, rect, len(rect), c.max_out, c.prm, emu=emu, ctx=ctx, budget=budget)


def compare_case(name, res):
    rc, msg, counts, out = res
    assert rc == 0, msg
    c = case(name)
    for j, (kps, _) in enumerate(reference(name)):
        n_out, n_found = counts[j]
        assert n_out == min(n_found, c.max_out)
        compare(out[j, :n_out], n_found, kps, c.max_out, "%s job %d" % (name, j))
        assert np.all(out[j, n_out:].view(np.uint8) == 0xC3), "%s job %d: rows behind n_out were written" % (name, j)


def refusal_call(changes, emu=None, ctx=None):
    """BASE_CALL with changes on two slots of 160 x 120; returns abi_call's result"""
    a = dict(BASE_CALL, **changes)
    imgs = np.stack([blocks(160, 120, 1), blocks(160, 120, 2)])
    rect = np.array([[50, 50], [90, 70]], np.float32)
    return abi_call(160, 120, imgs, [(a["slot"], a["rect_ofs"], a["nrect"])], rect, a["total_rects"], a["max_out"], a, emu=emu, ctx=ctx)


def untouched(res):
    _, _, counts, out = res
    return counts == [(SENTINEL, SENTINEL)] and bool(np.all(out.view(np.uint8) == 0xC3))
