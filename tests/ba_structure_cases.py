"""Local-BA problems placed on either side of the integer capacities that decide which code k_ba_build, BaHostStruct::build
and k_local_ba_t run (tests/ref_ba_structure.py has the rule and the constants).  A case is a pair of visibility masks
[nkf, nlm] (left, right camera), the context's max_kf, and the property it is named for as a predicate on the restated
structure.  tests/test_ref_ba_structure.py asserts every property on the CPU; tests/test_gpu_ba_structure.py builds the
problems (common.make_ba_problem_vis) and solves them.

Landmarks are written as block counts in the order the renumbering will put them (descending), then dealt to caller
numbers by a seeded permutation, so the renumbering is never the identity.

ll_boundary_cases(): the same for the low-latency solver (LLCase: masks in caller numbering, a shard count, a context and a predicate
on the restated shard table); tests/test_gpu_ll_structure.py solves them."""
import numpy as np

import ref_ba_structure as R

# what the case lists below are written for; test_ref_ba_structure.py asserts them against the formula
TILE_CAP = {10: 480, 12: 432, 20: 64}


class Case:
    def __init__(self, name, max_kf, nkf, vis_l, vis_r, prop, single_edge_ok=False):
        self.name, self.max_kf, self.nkf, self.vis_l, self.vis_r, self.prop = name, max_kf, nkf, vis_l, vis_r, prop
        self.nlm = vis_l.shape[1]
        self.single_edge_ok = single_edge_ok

    def edges(self):
        """(okf, olm) of the masks, landmark-major"""
        l, k, _ = np.nonzero(np.stack([self.vis_l, self.vis_r], 2).transpose(1, 0, 2))
        return k.astype(np.int32), l.astype(np.int32)

    def structure(self):
        okf, olm = self.edges()
        return R.structure(self.nkf, self.nlm, okf, olm, R.tile_cap(self.max_kf))

    def __repr__(self):
        return self.name


def window(m, i, nkf):
    """m keyframes in a row (mod nkf), starting at i: every keyframe is seen by as many landmarks as its neighbours, so no
    pose is left to a landmark or two"""
    return tuple(sorted((i + j) % nkf for j in range(m)))


def masks(nkf, lms, seed=1):
    """lms: list of (keyframes, cams); cams 'LR' both cameras in every block, 'L' / 'R' one camera only, 'auto': a landmark
    seen from one keyframe gets both cameras (one edge alone leaves its position to lambda), a multi-view landmark gets
    blocks of one edge (left) and of two edges.  Returns vis_l, vis_r in caller numbering (a seeded permutation of lms)."""
    nlm = len(lms)
    vl = np.zeros((nkf, nlm), bool); vr = np.zeros((nkf, nlm), bool)
    perm = np.random.default_rng(seed).permutation(nlm)
    for i, (kfs, cams) in enumerate(lms):
        l = perm[i]
        for k in kfs:
            vl[k, l] = cams != "R"
            vr[k, l] = cams in ("LR", "R") or (cams == "auto" and (len(kfs) == 1 or (i + k) % 3 != 0))
    return vl, vr


def counts(cs, nkf, singles_per_kf=0, cams="auto"):
    """landmarks with the block counts cs (windows of keyframes), then singles_per_kf single-view landmarks per keyframe"""
    lms = [(window(m, i, nkf), cams) for i, m in enumerate(cs)]
    lms += [((k,), "auto") for k in range(nkf) for _ in range(singles_per_kf)]
    return lms


def _tile_cases(max_kf):
    cap = TILE_CAP[max_kf]
    nkf = max_kf
    head = {10: [10] * 20 + [4] * 40, 20: [13] * 2 + [6] * 5}[max_kf]            # 360 / 56 blocks, grouped numbering
    rest = cap - sum(head)
    tag = "cap%d" % cap
    more = [2] * {10: 5, 20: 45}[max_kf]                                         # a second (and third) tile; at 20 keyframes they also tie every pose down
    out = []

    def add(name, cs, prop, nkf_=nkf, singles=2):
        out.append(Case("%s-%s" % (tag, name), max_kf, nkf_, *masks(nkf_, counts(cs, nkf_, singles)), prop))

    add("tile0-exactly-full", head + [2] * (rest // 2) + more,
        lambda s: s["grouped"] and s["ntile"] >= 2 and s["tile_blocks"][0] == cap and s["tile_lm"][1] < cap)
    add("one-short-then-two-blocks", head + [3] + [2] * ((rest - 4) // 2) + more,
        lambda s: s["ntile"] >= 2 and s["tile_blocks"][0] == cap - 1 and s["blocks_new"][s["tile_lm"][1]] == 2)
    full = {10: [10] * 50 + [3] * 10 + [2] * 20, 20: [20] * 5 + [2] * 50}[max_kf]
    add("all-keyframes-landmark-opens-a-tile", full,
        lambda s: s["ntile"] >= 2 and s["blocks_new"][s["tile_lm"][1]] == nkf and s["grouped"] == (max_kf == 10))
    if max_kf == 20:
        add("13-of-13-keyframes-landmark-opens-a-tile", [13] * 6 + [2] * 30,
            lambda s: s["grouped"] and s["ntile"] >= 2 and s["blocks_new"][s["tile_lm"][1]] == 13, nkf_=13)
    whole = {10: [10] * 30 + [4] * 45 + [2] * 240, 20: [13] * 2 + [6] * 5 + [2] * 4 + [2] * 64}[max_kf]
    nt = {10: 2, 20: 3}[max_kf]
    add("whole-tiles-only", whole, lambda s: s["ntile"] == nt and np.all(s["tile_blocks"] == cap))
    add("whole-tiles-and-one-block-pair-more", whole + [2],
        lambda s: s["ntile"] == nt + 1 and np.all(s["tile_blocks"][:-1] == cap) and s["tile_blocks"][-1] == 2
        and s["tile_lm"][-1] - s["tile_lm"][-2] == 1)
    if max_kf == 20:
        # 16 + 20 keys > BB_MAXKEYS: ungrouped, the single-view landmarks go through the tiles; a tile of cap of them is
        # full in landmarks and in blocks at once
        def both_caps(s):
            n = np.diff(s["tile_lm"])
            t = np.nonzero((n == cap) & (s["tile_blocks"] == cap))[0]
            return not s["grouped"] and s["nmv"] == s["nlm"] and len(t) >= 1 and t[0] + 1 < s["ntile"]
        add("ungrouped-single-views-meet-both-capacities", [16] + [2] * 24 + [2] * 32 + [1] * 130, both_caps, singles=0)
    return out


def _pit_cases():
    cap = R.BA_PIT_CAP
    out = []
    for n, cs in ((cap - 1, [10] * 37 + [2] * 4), (cap, [10] * 37 + [4] + [2]), (cap + 1, [10] * 36 + [9] + [6] + [2])):
        out.append(Case("pit-%d-items-in-one-tile" % n, 10, 10, *masks(10, counts(cs, 10, 2)),
                        lambda s, n=n: s["ntile"] == 1 and s["tile_items"][0] == n))
    out.append(Case("pit-long-tile-then-short-tile", 10, 10, *masks(10, counts([10] * 49 + [2] * 10, 10, 2)),
                    lambda s: s["ntile"] == 2 and s["tile_items"][0] > cap and 0 < s["tile_items"][1] < 100))
    return out


def _key_cases():
    out = []
    for top in (16, 17):
        lms = [(tuple(range(top)), "auto")] + counts([3] * 17 + [2] * 34, 17, 2)
        if top == 16:
            prop = lambda s: s["maxc"] + s["nkf"] == R.BB_MAXKEYS and s["grouped"] and s["nmv"] < s["nlm"]
        else:
            prop = lambda s: (s["maxc"] + s["nkf"] == R.BB_MAXKEYS + 1 and not s["grouped"] and s["nmv"] == s["nlm"]
                              and np.all(s["sv_start"] == s["nlm"]))
        out.append(Case("keys-%d-%s" % (17 + top, "grouped" if top == 16 else "ungrouped"), 20, 17, *masks(17, lms), prop))
    return out


def _chunk_cases():
    out = []
    for nt in (40, 41):
        cs = [4] * (16 * (nt - 1) + 1)                   # 16 four-block landmarks fill a tile of 64: nt - 1 full tiles and one landmark
        nl = nt * 210
        out.append(Case("lists-%d-%s" % (nl, "one-chunk" if nl <= R.LIST_CHUNK else "two-chunks"), 20, 20,
                        *masks(20, counts(cs, 20, 1)),
                        lambda s, nt=nt, nl=nl: s["na"] == 20 and s["ntile"] == nt and s["nlists"] == nl
                        and R.list_chunks(s) == (1 if nt == 40 else 2)))
    return out


def _empty_cases():
    out = []

    def add(name, nkf, lms, prop, **kw):
        out.append(Case("empty-" + name, 10, nkf, *masks(nkf, lms), prop, **kw))

    add("every-landmark-single-view", 6, counts([], 6, 14), lambda s: s["nmv"] == 0 and s["ntile"] == 0 and s["ncontrib"] == 0)
    add("no-single-view-landmark", 6, counts([5] * 10 + [3] * 30 + [2] * 40, 6),
        lambda s: s["grouped"] and s["nmv"] == s["nlm"] and np.all(s["sv_start"] == s["nlm"]))
    mv = counts([4] * 10 + [2] * 30, 6)
    add("single-views-all-on-last-keyframe", 6, mv + [((5,), "auto")] * 40,
        lambda s: np.all(s["sv_start"][:6] == s["nmv"]) and s["sv_start"][6] == s["nlm"] and s["nmv"] < s["nlm"])
    add("single-views-all-on-keyframe-0", 6, mv + [((0,), "auto")] * 40,
        lambda s: s["sv_start"][0] == s["nmv"] < s["nlm"] and np.all(s["sv_start"][1:] == s["nlm"]))
    add("one-active-keyframe", 5, [((3,), "auto")] * 60, lambda s: s["na"] == 1 and s["nmv"] == 0 and s["nblk"] == 60)
    live = [1, 2, 4, 5, 6]                                # keyframes 0, 3 and 7 of 8 without edges
    lms = [(tuple(live[(i + j) % 5] for j in range(m)), "auto") for i, m in enumerate([4] * 10 + [3] * 20 + [2] * 30 + [1] * 30)]
    add("keyframes-without-edges-front-middle-end", 8, lms, lambda s: s["na"] == 5 and s["nkf"] == 8)
    vl, vr = masks(6, counts([3] * 20 + [2] * 30, 6, 5))
    for l in (0, vl.shape[1] - 1):
        vl[:, l] = False; vr[:, l] = False
    out.append(Case("empty-landmarks-0-and-last-without-edges", 10, 6, vl, vr,
                    lambda s: s["blocks"][0] == 0 and s["blocks"][-1] == 0 and set(s["lm_orig"][-2:]) == {0, s["nlm"] - 1}))
    add("right-camera-only-landmark", 6, counts([3] * 20 + [2] * 30, 6, 5) + [((1, 2, 4), "R")], lambda s: s["nmv"] == 51)
    add("one-and-two-edge-blocks-in-a-landmark", 6, counts([4] * 30 + [2] * 30, 6, 5), lambda s: s["nmv"] == 60)
    # 2 of 120 landmarks with a single edge (one left, one right): their 3 x 3 block is singular but for lambda
    add("two-landmarks-with-a-single-edge", 6, counts([4] * 20 + [3] * 30 + [2] * 50, 6, 3) + [((2,), "L"), ((4,), "R")],
        lambda s: s["nlm"] == 120, single_edge_ok=True)
    return out


def _row_cases():
    """na = 10, 11, 12 of 12 keyframes: np = 60, 66, 72 rows, the same landmarks but for the edges of the last keyframes"""
    vl, vr = masks(12, counts([6] * 30 + [3] * 60 + [2] * 60, 12, 3))
    out = []
    for na in (10, 11, 12):
        a, b = vl.copy(), vr.copy()
        a[na:] = False; b[na:] = False
        one = a.sum(0) + b.sum(0) == 1                   # a landmark left with a single edge gets its block's other camera
        a[:, one] |= b[:, one]; b[:, one] |= a[:, one]
        out.append(Case("rows-%d" % (6 * na), 12, 12, a, b, lambda s, na=na: s["na"] == na and (6 * na > 64) == (na > 10)))
    return out


def all_cases():
    return _tile_cases(10) + _tile_cases(20) + _pit_cases() + _key_cases() + _chunk_cases() + _empty_cases() + _row_cases()


def ll_cases():
    """what goes through the low-latency solver as well: the tile-capacity, BA_PIT_CAP and empty-pass cases of a 10-keyframe
    window, and ten landmarks for sixteen shards (shards without edges whatever the dealing rule)"""
    few = Case("ll-ten-landmarks", 10, 10, *masks(10, counts([10] * 10, 10)), lambda s: s["nlm"] == 10 and s["nblk"] == 100)
    return [c for c in all_cases() if c.max_kf == 10 and c.name.startswith(("cap480-", "pit-", "empty-"))] + [few]


# --------------------------------------------------------------------------- the low-latency solver on its own boundaries
class LLCase:
    """a problem for the low-latency solver: visibility masks in CALLER numbering (the deal follows the caller's landmark
    order, so nothing is permuted here), the shard count, the context (max_kf, resident 0 | 1) and a predicate on the restated
    shard table (ref_ba_structure.ll_shards: one row of landmarks, edges, blocks, tiles, solver code, active poses, mask per
    shard).  lms: per landmark None (no edge) or a tuple of (keyframe, 'LR' | 'L')."""

    def __init__(self, name, max_kf, resident, W, nkf, lms, prop):
        self.name, self.max_kf, self.resident, self.W, self.nkf, self.prop = name, max_kf, resident, W, nkf, prop
        self.nlm = len(lms)
        self.vis_l = np.zeros((nkf, self.nlm), bool); self.vis_r = np.zeros((nkf, self.nlm), bool)
        for l, blocks in enumerate(lms):
            for k, cams in blocks or ():
                assert cams in ("LR", "L") and not self.vis_l[k, l]
                self.vis_l[k, l] = True
                self.vis_r[k, l] = cams == "LR"
        self._rows = None

    edges = Case.edges

    def shards(self):
        """(rows [W, 7], per-shard structures, the deal) of the restatement, computed once"""
        if self._rows is None:
            okf, olm = self.edges()
            self._rows = R.ll_shards(olm, okf, self.nkf, self.nlm, self.W, self.max_kf, self.resident)
        return self._rows

    def __repr__(self):
        return self.name


NLM, NOBS, NBLK, NTILE, CODE, NA, MASK = range(7)      # columns of the shard table


def _lm(i, nkf, cams):
    """landmark i of a list: blocks with the cameras `cams` on a window of len(cams) keyframes that starts at keyframe i"""
    return tuple(zip(window(len(cams), i, nkf), cams))


def _only(col, w, v):
    """shard w has v in column col, every other shard less"""
    return lambda t: t[w, col] == v and np.all(np.delete(t[:, col], w) < v)


def _ll_resident_cases():
    """max_kf 11: a shard of the resident kernel holds 256 blocks (min(tile_cap_ll, B) = min(256, 256)), 208 landmarks, 448
    edges.  All landmarks with edges of a list cost the same, so the cuts are where the list says; the `above` case changes the
    counted quantity without moving a cut — a block more at the same edge count, a landmark without edges — except for the
    edges, where the landmark of five edges is the first of its shard and the cuts stay by arithmetic (the predicate has them)."""
    out = []
    T3, T3b = ("LR", "L"), ("L", "L", "L")                     # three edges, cost 21: two blocks / three blocks

    def blocks(W, over, tag, resident=1):
        lms = [_lm(i, 6, T3) for i in range(128 * W)]
        if over is not None:
            lms[128 * over + 64] = _lm(128 * over + 64, 6, T3b)
        kind = "res" if resident else "stream"
        if over is None:
            prop = lambda t: np.all(t[:, NBLK] == 256) and np.all(t[:, NLM] == 128) and np.all(t[:, NTILE] == 1) and np.all(t[:, CODE] == (2 if resident else 1))
        else:
            prop = lambda t: _only(NBLK, over, 257)(t) and np.all(t[:, CODE] == 1) and t[over, NTILE] == 2 and np.all(np.delete(t[:, NTILE], over) == 1)
        out.append(LLCase("ll-%s-w%d-blocks-%s" % (kind, W, tag), 11, resident, W, 6, lms, prop))
    blocks(4, None, "256")
    blocks(4, 0, "257-in-shard-0"); blocks(4, 2, "257-in-a-middle-shard"); blocks(4, 3, "257-in-the-last-shard")
    for W in (8, 16):
        blocks(W, None, "256"); blocks(W, W // 2 - 1, "257-in-a-middle-shard")
    # the streaming kernel's own tile, in a context without the resident kernel (tile_cap_ll(11) = 256)
    blocks(4, None, "256", resident=0); blocks(4, 1, "257-in-a-middle-shard", resident=0)
    # landmarks: one stereo block each (two edges, cost 12), every fifth two left-only blocks (two edges as well)
    for n in (832, 833):
        lms = [_lm(i, 6, ("L", "L") if i % 5 == 0 else ("LR",)) for i in range(n)]
        if n == 832:
            prop = lambda t: np.all(t[:, NLM] == 208) and np.all(t[:, CODE] == 2) and t[:, NBLK].max() <= 256 and t[:, NOBS].max() <= 448
        else:
            prop = lambda t: _only(NLM, 0, 209)(t) and np.all(t[:, CODE] == 1) and t[:, NBLK].max() <= 256 and t[:, NOBS].max() <= 448
        out.append(LLCase("ll-res-w4-landmarks-%d" % (n // 4 + n % 4), 11, 1, 4, 6, lms, prop))
    # edges: two stereo blocks each (four edges, cost 32); above: the first landmark has a fifth edge (cost 45)
    for over in (False, True):
        lms = [_lm(i, 6, ("LR", "LR")) for i in range(448)]
        if over:
            lms[0] = _lm(0, 6, ("LR", "LR", "L"))
            prop = lambda t: _only(NOBS, 0, 449)(t) and np.all(t[:, NLM] == 112) and np.all(t[:, CODE] == 1) and t[:, NBLK].max() <= 256
        else:
            prop = lambda t: np.all(t[:, NOBS] == 448) and np.all(t[:, NLM] == 112) and np.all(t[:, CODE] == 2) and t[:, NBLK].max() <= 256
        out.append(LLCase("ll-res-w4-edges-%d" % (449 if over else 448), 11, 1, 4, 6, lms, prop))
    return out


def _ll_in_lds_cases():
    """max_kf 11 without the resident kernel: a shard's records and positions stay in LDS up to LL_ECAP = 704 edges and
    LL_LCAP = 448 landmarks, decided per shard.  The column checked is what ref_ba_structure.ll_shard_in_lds says of each shard."""
    out = []
    in_lds = lambda t: [R.ll_shard_in_lds(int(n), int(e)) for n, e in zip(t[:, NLM], t[:, NOBS])]
    for over in (False, True):
        lms = [_lm(i, 6, ("LR", "LR")) for i in range(4 * 176)]
        if over:
            lms[0] = _lm(0, 6, ("LR", "LR", "L"))
            prop = lambda t: _only(NOBS, 0, 705)(t) and np.all(t[1:, NOBS] == 704) and in_lds(t) == [False, True, True, True]
        else:
            prop = lambda t: np.all(t[:, NOBS] == 704) and in_lds(t) == [True] * 4
        out.append(LLCase("ll-stream-w4-in-lds-edges-%d" % (705 if over else 704), 11, 0, 4, 6, lms, prop))
    # 448 landmarks a shard: 352 of two edges (every eleventh two left-only blocks, the others one stereo block) and 96 without
    # edges behind the first 96; a shard's list starts and ends with a landmark that has edges, so the cuts are the lists' ends.
    # Above: one more landmark without edges inside shard 1
    for over in (False, True):
        lms = []
        for w in range(4):
            for i in range(352):
                lms.append(_lm(i, 6, ("L", "L") if i % 11 == 0 else ("LR",)))
                if i < 96 or (over and w == 1 and i == 200):
                    lms.append(None)
        if over:
            prop = lambda t: _only(NLM, 1, 449)(t) and np.all(t[:, NOBS] == 704) and in_lds(t) == [True, False, True, True]
        else:
            prop = lambda t: np.all(t[:, NLM] == 448) and np.all(t[:, NOBS] == 704) and in_lds(t) == [True] * 4
        out.append(LLCase("ll-stream-w4-in-lds-landmarks-%d" % (449 if over else 448), 11, 0, 4, 6, lms, prop))
    return out


def _ll_min_cases():
    """where the two capacities of ba_ll_tile_cap differ: max_kf 7 (tile_cap_ll 368, B 320) and 13 (176, 192).  Landmarks of four
    blocks and five edges (cost 45); above: one of them has its five edges in five blocks"""
    out = []
    P5, P5b = ("LR", "L", "L", "L"), ("L",) * 5

    def add(max_kf, resident, per_shard, over, prop):
        nkf = max_kf
        lms = [_lm(i, nkf, P5) for i in range(4 * per_shard)]
        if over:
            lms[2 * per_shard + 7] = _lm(2 * per_shard + 7, nkf, P5b)
        out.append(LLCase("ll-kf%d-%s-w4-blocks-%d" % (max_kf, "res" if resident else "stream", 4 * per_shard + over), max_kf, resident,
                          4, nkf, lms, prop))
    add(7, 1, 80, 0, lambda t: np.all(t[:, NBLK] == 320) and np.all(t[:, CODE] == 2) and np.all(t[:, NTILE] == 1))
    add(7, 1, 80, 1, lambda t: _only(NBLK, 2, 321)(t) and np.all(t[:, CODE] == 1) and t[:, NTILE].tolist() == [1, 1, 2, 1])
    add(7, 0, 92, 0, lambda t: np.all(t[:, NBLK] == 368) and np.all(t[:, CODE] == 1) and np.all(t[:, NTILE] == 1))
    add(7, 0, 92, 1, lambda t: _only(NBLK, 2, 369)(t) and np.all(t[:, CODE] == 1) and t[:, NTILE].tolist() == [1, 1, 2, 1])
    add(13, 1, 44, 0, lambda t: np.all(t[:, NBLK] == 176) and np.all(t[:, CODE] == 2) and np.all(t[:, NA] == 13))
    add(13, 1, 44, 1, lambda t: _only(NBLK, 2, 177)(t) and np.all(t[:, CODE] == 1) and t[:, NTILE].tolist() == [1, 1, 2, 1])
    return out


def _ll_window_cases():
    """max_kf 16, the widest window the shard solver is made for (64 blocks and 64 landmarks a shard in the resident kernel):
    2 to 16 keyframes, every one an active pose of every shard — 8, 5, 3, 2, 1, 1 sixteen-lane rows per pose in k_ba_ll's pass"""
    out = []
    cams = ("LR", "L", "LR", "L")
    for W in (4, 16):
        for nkf in (2, 3, 5, 8, 12, 16):
            m = min(nkf, 4)
            n = (60 * W) // m
            lms = [_lm(i, nkf, cams[:m]) for i in range(n)]
            out.append(LLCase("ll-kf16-res-w%d-%d-keyframes" % (W, nkf), 16, 1, W, nkf, lms,
                              lambda t, nkf=nkf, W=W: np.all(t[:, CODE] == 2) and np.all(t[:, NA] == nkf) and np.all(t[:, NBLK] == 60)
                              and t[:, NLM].max() <= 64 and t[0, MASK] == (1 << W) - 1))
    for over in (0, 1):
        lms = [_lm(i, 16, cams) for i in range(64)]
        if over:
            lms[40] = _lm(40, 16, ("LR", "L", "L", "L", "L"))
            prop = lambda t: _only(NBLK, 2, 65)(t) and np.all(t[:, CODE] == 1) and t[:, NTILE].tolist() == [1, 1, 2, 1] and np.all(t[:, NA] == 16)
        else:
            prop = lambda t: np.all(t[:, NBLK] == 64) and np.all(t[:, CODE] == 2) and np.all(t[:, NA] == 16)
        out.append(LLCase("ll-kf16-res-w4-blocks-%d" % (64 + over), 16, 1, 4, 16, lms, prop))
    return out


def _ll_mask_case():
    """16 shards, 10 keyframes: light landmarks (three edges, cost 21) around one that every keyframe sees in both cameras
    (20 edges, cost 480: four shares of the total), so several MIDDLE shards are empty ranges; landmarks without edges in front,
    across a cut and behind; the last landmark with edges costs more than a share (12 edges, cost 192), so the last shard's range
    holds nothing but the landmarks without edges behind it"""
    light = lambda i: _lm(i, 10, ("LR", "L"))
    lms = [None, None] + [light(i) for i in range(30)] + [_lm(0, 10, ("LR",) * 10)]
    for i in range(30):
        lms.append(light(30 + i))
        if i in (3, 4, 11, 19, 27):
            lms.append(None)
    lms += [_lm(3, 10, ("LR",) * 6), None, None, None]

    def prop(t):
        c = LL_MASK_CASE.shards()[2]["cut"]
        has = (LL_MASK_CASE.vis_l | LL_MASK_CASE.vis_r).any(0)
        mask = int(t[0, MASK])
        holes = [w for w in range(16) if not (mask >> w) & 1]
        heavy = int(np.argmax(LL_MASK_CASE.vis_l.sum(0) + LL_MASK_CASE.vis_r.sum(0)))
        hw = max(w for w in range(16) if c[w] <= heavy)
        middle = [w for w in holes if hw < w < 15 and any((mask >> v) & 1 for v in range(w + 1, 16))]
        straddle = any(0 < c[w] < len(has) and not has[c[w]] and has[c[w] - 1] and t[w, NOBS] > 0 for w in range(1, 16))
        return (len(middle) >= 3 and all(t[w, NLM] == 0 for w in middle) and mask & 1 and not has[0]
                and t[15, NLM] == 3 and t[15, NOBS] == 0 and 15 in holes and straddle and np.all(t[:, CODE] == 2))
    return LLCase("ll-res-w16-shard-mask-with-holes", 11, 1, 16, 10, lms, prop)


LL_MASK_CASE = _ll_mask_case()


def ll_boundary_cases():
    return _ll_resident_cases() + _ll_in_lds_cases() + _ll_min_cases() + _ll_window_cases() + [LL_MASK_CASE]


def edge_cache_masks():
    """~1,200 landmarks, ~15,000 edges, 10 keyframes: both cameras in every block"""
    return masks(10, counts(([10, 8, 6, 4, 3] * 240), 10, 0, cams="LR"), seed=3)


def edge_cache_partner_nlm(nlm, nobs, fits):
    """landmark count of a second problem that pushes bb_lds_ints(max_nlm) + nobs just past (fits False) / leaves it just
    inside (fits True) the edge cache's LDS"""
    n = nlm
    while R.edge_cache_fits(n + 1, nobs):
        n += 1
    return n if fits else n + 1
