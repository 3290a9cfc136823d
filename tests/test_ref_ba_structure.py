"""CPU: the restated structure rule of a local-BA problem (tests/ref_ba_structure.py) against brute force, over random small
problems and every designed case of tests/ba_structure_cases.py; every designed case has the property it is named for,
before it is ever sent to a GPU; the problem builder realises exactly the prescribed visibility."""
import numpy as np
import pytest

import ba_structure_cases as bc
import common as cm
import ref_ba_structure as R

CASES = bc.all_cases()


def _check_structure(s, okf, olm):
    nkf, nlm, cap = s["nkf"], s["nlm"], s["cap"]
    # the renumbering is a permutation, ordered as the rule says
    assert sorted(s["lm_orig"].tolist()) == list(range(nlm))
    b = s["blocks_new"]
    per_lm = [set() for _ in range(nlm)]
    for k, l in zip(okf.tolist(), olm.tolist()):
        per_lm[l].add(k)
    assert [len(per_lm[l]) for l in s["lm_orig"]] == b.tolist()
    assert s["grouped"] == (max(len(p) for p in per_lm) + nkf <= R.BB_MAXKEYS)
    if s["grouped"]:
        assert np.all(np.diff(b[:s["nmv"]]) <= 0) and np.all(b[:s["nmv"]] >= 2) and np.all(b[s["nmv"]:] <= 1)
        sv = s["sv_start"]
        assert sv[0] == s["nmv"] and np.all(np.diff(sv) >= 0) and sv[nkf] == nlm - int((b == 0).sum())
        for k in range(nkf):
            for j in range(sv[k], sv[k + 1]):
                assert per_lm[s["lm_orig"][j]] == {k}
        assert np.all(b[sv[nkf]:] == 0)
    else:
        assert np.all(np.diff(b) <= 0) and s["nmv"] == nlm and np.all(s["sv_start"] == nlm)
    for lo, hi in [(0, s["nmv"])] + ([(s["sv_start"][k], s["sv_start"][k + 1]) for k in range(nkf)] if s["grouped"] else []):
        same = [j for j in range(lo, hi - 1) if b[j] == b[j + 1]]
        assert all(s["lm_orig"][j] < s["lm_orig"][j + 1] for j in same), "not stable"
    assert s["na"] == len(set(okf.tolist())) and s["nblk"] == sum(len(p) for p in per_lm)
    # the tiles partition [0, nmv), respect both capacities and are maximal
    t = s["tile_lm"]
    if s["nmv"] == 0:
        assert s["ntile"] == 0
    else:
        assert t[0] == 0 and t[-1] == s["nmv"] and np.all(np.diff(t) >= 1) and s["ntile"] == len(t) - 1
    for i in range(s["ntile"]):
        nl, nb = t[i + 1] - t[i], int(b[t[i]:t[i + 1]].sum())
        assert nl <= cap and nb <= cap and nb == s["tile_blocks"][i]
        if t[i + 1] < s["nmv"]:
            assert nl + 1 > cap or nb + b[t[i + 1]] > cap, "tile %d could have taken the next landmark" % i
    # the items: a double loop over landmarks and keyframe pairs
    tile_of = np.searchsorted(t, np.arange(s["nmv"]), side="right") - 1 if s["ntile"] else np.zeros(0, np.int64)
    items = np.zeros(max(s["ntile"], 1), np.int64)
    for j in range(s["nmv"]):
        kfs = sorted(per_lm[s["lm_orig"][j]])
        for a in range(len(kfs)):
            for c in range(a, len(kfs)):
                items[tile_of[j]] += 1
    assert items[:s["ntile"]].tolist() == s["tile_items"].tolist() and s["ncontrib"] == int(items[:s["ntile"]].sum())


def test_constants_give_the_tile_capacities_the_cases_are_written_for():
    for max_kf, cap in bc.TILE_CAP.items():
        assert R.tile_cap(max_kf) == cap, (max_kf, R.tile_cap(max_kf))
    assert R.lds_fixed_bytes(10) + 27 * 8 * R.tile_cap(10) <= R.BA_LDS_LIMIT
    assert R.lds_fixed_bytes(20) + 27 * 8 * (R.tile_cap(20) + 16) > R.BA_LDS_LIMIT        # 64 is all that fits at 20 keyframes
    assert R.tile_cap(32) == 0
    assert R.LIST_CHUNK == 8448 and R.BA_PIT_CAP == 2048
    # the edge cache: 6 ints per landmark and one per edge against 150 KiB
    assert R.edge_cache_fits(1200, 15000) and not R.edge_cache_fits(2410, 15000) and R.edge_cache_fits(2409, 15000)
    assert R.bb_lds_bytes(2410) <= R.CREATE_BUILD_LDS_LIMIT


def test_random_small_problems():
    rng = np.random.default_rng(5)
    seen = dict(grouped=0, ungrouped=0, multi_tile=0, no_mv=0, edgeless=0)
    for it in range(200):
        nkf = int(rng.integers(1, 25)); nlm = int(rng.integers(1, 120)); cap = int(rng.choice([nkf, nkf + 1, 32, 64]))
        cap = max(cap, nkf)
        dens = float(rng.choice([0.02, 0.1, 0.3, 0.9]))
        vis = rng.random((nkf, nlm)) < dens
        if it % 7 == 0:
            vis[:, rng.integers(nlm)] = True                                   # a landmark seen from everywhere
        if not vis.any():
            vis[rng.integers(nkf), rng.integers(nlm)] = True
        okf, olm = np.nonzero(vis)
        dup = rng.random(len(okf)) < 0.5                                       # second (right) edge of a block
        okf = np.concatenate([okf, okf[dup]]); olm = np.concatenate([olm, olm[dup]])
        p = rng.permutation(len(okf))
        s = R.structure(nkf, nlm, okf[p], olm[p], cap)
        _check_structure(s, okf, olm)
        seen["grouped" if s["grouped"] else "ungrouped"] += 1
        seen["multi_tile"] += s["ntile"] > 1; seen["no_mv"] += s["nmv"] == 0; seen["edgeless"] += bool((s["blocks"] == 0).any())
    assert min(seen.values()) >= 10, seen


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_designed_case(case):
    okf, olm = case.edges()
    s = case.structure()
    assert s["cap"] == bc.TILE_CAP[case.max_kf] and case.nkf <= case.max_kf and case.nlm <= 1500
    _check_structure(s, okf, olm)
    assert case.prop(s), case.name
    # landmarks with a single edge only where the case is about them
    nedge = case.vis_l.sum(0) + case.vis_r.sum(0)
    n1 = int((nedge == 1).sum())
    assert (n1 > 0) == case.single_edge_ok and n1 <= 0.02 * case.nlm


def test_case_names_are_unique_and_cover_the_boundary_table():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for word in ("cap480-", "cap64-", "pit-2047", "pit-2048", "pit-2049", "pit-long", "keys-33", "keys-34", "lists-8400", "lists-8610",
                 "empty-", "rows-60", "rows-66", "rows-72", "ungrouped-single-views"):
        assert any(word in n for n in names), word
    by = {c.name: c for c in CASES}
    a, b = by["keys-33-grouped"], by["keys-34-ungrouped"]
    assert int((a.vis_l != b.vis_l).sum() + (a.vis_r != b.vis_r).sum()) <= 2, "the two key-space cases differ in one block"
    assert any("one-and-two-edge" in c.name and ((c.vis_l & ~c.vis_r).any(0) & (c.vis_l & c.vis_r).any(0)).any() for c in CASES)
    assert any("right-camera-only" in c.name and (c.vis_r.any(0) & ~c.vis_l.any(0)).any() for c in CASES)


def test_edge_cache_problem_and_partners():
    vl, vr = bc.edge_cache_masks()
    nlm, nobs = vl.shape[1], int(vl.sum() + vr.sum())
    assert 1100 <= nlm <= 1300 and 14000 <= nobs <= 16000
    assert R.edge_cache_fits(nlm, nobs)
    big, small = bc.edge_cache_partner_nlm(nlm, nobs, False), bc.edge_cache_partner_nlm(nlm, nobs, True)
    assert big == small + 1 and not R.edge_cache_fits(big, nobs) and R.edge_cache_fits(small, nobs)
    assert 4 * (R.bb_lds_ints(big) + nobs) - R.EDGE_CACHE_LIMIT <= 24           # "just past": one landmark's six ints
    assert R.bb_lds_bytes(big) <= R.CREATE_BUILD_LDS_LIMIT and big < 65536


# --------------------------------------------------------------------------- the low-latency solver: the deal, the capacities, the cases
LL_BOUNDARY = bc.ll_boundary_cases()


def _deal_one_landmark_at_a_time(olm, okf, nlm, W):
    """the dealing rule again, without prefix arrays: walk the landmarks once with a running cost, open shards as the walk
    reaches them"""
    total = 0
    for l in range(nlm):
        e = sum(1 for v in olm if v == l)
        total += e * (4 + e)
    cut, nl, no, nb = [0], [0] * W, [0] * W, [0] * W
    run = 0
    for l in range(nlm):
        kfs = [k for v, k in zip(olm, okf) if v == l]
        w = run * W // total
        if w > W - 1:
            w = W - 1
        while len(cut) - 1 < w:                  # the walk has passed into shard w: it, and every shard skipped, starts here
            cut.append(l)
        nl[w] += 1; no[w] += len(kfs); nb[w] += len(set(kfs))
        run += len(kfs) * (4 + len(kfs))
    while len(cut) < W + 1:
        cut.append(nlm)
    mask = 0
    for w in range(W):
        if no[w]:
            mask |= 1 << w
    return dict(cut=cut, nlm=nl, nobs=no, nblk=nb, mask=mask)


def test_ll_deal_against_the_loop_only_implementation():
    rng = np.random.default_rng(11)
    seen = dict(front=0, middle=0, end=0, hole=0, trailing_hole=0, edgeless_shard=0)
    for it in range(210):
        W = (4, 8, 16)[it % 3]
        nkf = int(rng.integers(2, 12)); nlm = int(rng.integers(1, 90))
        vis = rng.random((nkf, nlm)) < float(rng.choice([0.1, 0.4, 0.9]))
        if it % 5 == 0:
            vis[:, rng.integers(nlm)] = True                                   # a landmark that outweighs several shares
        bare = np.zeros(nlm, bool)
        if it % 2 == 0 and nlm >= 6:
            which = ("front", "middle", "end")[(it // 2) % 3]
            n = int(rng.integers(1, 4))
            bare[{"front": slice(0, n), "middle": slice(nlm // 2, nlm // 2 + n), "end": slice(nlm - n, nlm)}[which]] = True
        vis[:, bare] = False
        if not vis.any():
            vis[0, int(np.nonzero(~bare)[0][0])] = True
        has = vis.any(0)
        seen["front"] += not has[0]; seen["end"] += not has[-1]; seen["middle"] += bool((~has[1:-1]).any())
        olm, okf = np.nonzero(vis.T)                                           # landmark-major, keyframes ascending
        dup = rng.random(len(olm)) < 0.5                                       # the block's second edge
        o = np.lexsort((np.concatenate([okf, okf[dup]]), np.concatenate([olm, olm[dup]])))
        olm, okf = np.concatenate([olm, olm[dup]])[o], np.concatenate([okf, okf[dup]])[o]
        d = R.ll_deal(olm, okf, nlm, W)
        assert d == _deal_one_landmark_at_a_time(olm.tolist(), okf.tolist(), nlm, W), (it, W)
        c = d["cut"]
        assert c[0] == 0 and c[W] == nlm and all(c[w] <= c[w + 1] for w in range(W)), "the ranges partition [0, nlm) in order"
        assert [c[w + 1] - c[w] for w in range(W)] == d["nlm"]
        assert sum(d["nlm"]) == nlm and sum(d["nobs"]) == len(olm) and sum(d["nblk"]) == len(set(zip(olm.tolist(), okf.tolist())))
        assert d["mask"] == sum(1 << w for w in range(W) if d["nobs"][w] > 0)
        # nothing costs anything before the first landmark with edges, so it is dealt to shard 0: the leader (the lowest shard of
        # the mask, which writes the poses and the trace back) is always shard 0
        assert d["mask"] & 1, "shard 0 without edges"
        holes = [w for w in range(W) if d["nlm"][w] == 0]
        seen["hole"] += any(any(d["nobs"][v] for v in range(w + 1, W)) for w in holes)
        seen["trailing_hole"] += any(not any(d["nlm"][v] for v in range(w, W)) for w in holes)
        seen["edgeless_shard"] += any(d["nlm"][w] > 0 and d["nobs"][w] == 0 for w in range(W))
    assert min(seen.values()) >= 10, seen


def test_ll_capacity_table():
    """tile_cap_ll / ll_caps as the cases of ba_structure_cases.ll_boundary_cases are written for them; the shard solver exists
    up to max_kf 16; the two capacities of ba_ll_tile_cap differ on both sides"""
    want = {7: (368, (320, 208, 448)), 11: (256, (256, 208, 448)), 13: (176, (192, 208, 448)), 16: (64, (64, 208, 448)),
            17: (0, (0, 0, 0))}
    for max_kf, (t, caps) in want.items():
        assert (R.tile_cap_ll(max_kf), R.ll_caps(max_kf)) == (t, caps), (max_kf, R.tile_cap_ll(max_kf), R.ll_caps(max_kf))
    assert [R.ll_enabled(k) for k in (1, 7, 11, 16, 17, 20)] == [True, True, True, True, False, False]
    assert [R.ll_tile_cap(k, 1) for k in (7, 11, 13, 16)] == [320, 256, 176, 64]
    assert [R.ll_tile_cap(k, 0) for k in (7, 11, 13, 16)] == [368, 256, 176, 64]
    assert (R.LL_ECAP, R.LL_LCAP) == (704, 448)
    assert R.ll_shard_in_lds(448, 704) and not R.ll_shard_in_lds(449, 704) and not R.ll_shard_in_lds(448, 705)
    for max_kf in range(1, 33):
        if not R.ll_enabled(max_kf):
            continue
        B, L, E = R.ll_caps(max_kf)
        assert B >= 64 and R.ll_resident_lds_bytes(max_kf, B, L, E) <= R.BA_LDS_LIMIT
        # k_ba_ll stages min(ncontrib, BA_PIT_CAP) pair items in LDS and would read the others from g_pitem; a resident shard has
        # one tile of at most min(tile_cap_ll, B) blocks, a landmark of m <= max_kf blocks lists m (m + 1) / 2 items, so at most
        # B (max_kf + 1) / 2 items: below BA_PIT_CAP everywhere, the fallback is unreachable
        items = R.ll_tile_cap(max_kf, 1) * (max_kf + 1) // 2
        assert items < R.BA_PIT_CAP, (max_kf, items)
        if max_kf == 11:
            assert items == 1536


@pytest.mark.parametrize("case", LL_BOUNDARY, ids=repr)
def test_ll_boundary_case(case):
    okf, olm = case.edges()
    assert np.array_equal(np.lexsort((okf, olm)), np.arange(len(olm))), "edges are not landmark-major"
    assert R.ll_enabled(case.max_kf) and case.nkf <= case.max_kf and case.W in (4, 8, 16)
    assert case.nlm <= cm.LL_CTX_KW["max_lm"] and len(olm) <= cm.LL_CTX_KW["max_obs"]
    t, structs, d = case.shards()
    assert d == _deal_one_landmark_at_a_time(olm.tolist(), okf.tolist(), case.nlm, case.W)
    assert case.prop(t), (case.name, t.tolist())
    # which kernel: all shards inside the three resident capacities and the tile, in a context that has the resident kernel
    cap = R.ll_tile_cap(case.max_kf, case.resident)
    B, L, E = R.ll_caps(case.max_kf)
    fits = case.resident and t[:, 2].max() <= min(B, cap) and t[:, 0].max() <= min(L, cap) and t[:, 1].max() <= E
    assert np.all(t[:, 4] == (2 if fits else 1))
    for w, s in enumerate(structs):
        if s is not None:
            assert not s["grouped"] and s["nmv"] == s["nlm"] and s["na"] == case.nkf
            assert t[w, 3] == s["ntile"] >= 1 and (t[w, 4] == 1 or s["ntile"] == 1)
            assert s["ncontrib"] < R.BA_PIT_CAP or t[w, 4] == 1
    # no landmark with a single edge: nothing is excluded from the comparison with the oracle
    nedge = case.vis_l.sum(0) + case.vis_r.sum(0)
    assert not (nedge == 1).any() and (nedge >= 2).any(0)
    assert (case.vis_l | case.vis_r).any(1).all(), "a keyframe without edges"


def test_ll_boundary_case_names():
    names = [c.name for c in LL_BOUNDARY]
    assert len(set(names)) == len(names)
    for word in ("res-w4-blocks-256", "res-w4-blocks-257-in-shard-0", "257-in-a-middle-shard", "257-in-the-last-shard", "res-w8-blocks-25",
                 "res-w16-blocks-25", "stream-w4-blocks-256", "stream-w4-blocks-257", "landmarks-208", "landmarks-209", "edges-448",
                 "edges-449", "in-lds-edges-704", "in-lds-edges-705", "in-lds-landmarks-448", "in-lds-landmarks-449", "kf7-res-w4-blocks-320",
                 "kf7-res-w4-blocks-321", "kf7-stream-w4-blocks-368", "kf7-stream-w4-blocks-369", "kf13-res-w4-blocks-176",
                 "kf13-res-w4-blocks-177", "kf16-res-w4-blocks-64", "kf16-res-w4-blocks-65", "shard-mask-with-holes"):
        assert any(word in n for n in names), word
    for W in (4, 16):
        assert sorted(c.nkf for c in LL_BOUNDARY if c.name.startswith("ll-kf16-res-w%d-" % W) and "keyframes" in c.name) == [2, 3, 5, 8, 12, 16]


@pytest.mark.parametrize("name", ["cap64-tile0-exactly-full", "empty-right-camera-only-landmark", "rows-72"])
def test_problem_builder_realises_the_masks(name):
    """make_ba_problem_vis asserts that itself; here: at 20 keyframes there is room in the intersection of the frusta, the
    problem is deterministic in its seed, and make_ba_problem still returns what it returned before the two shared
    their trajectory and perturbation code"""
    case = next(c for c in CASES if c.name == name)
    p = cm.make_ba_problem_vis(np.random.default_rng(9), case.vis_l, case.vis_r)
    q = cm.make_ba_problem_vis(np.random.default_rng(9), case.vis_l, case.vis_r)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert len(p["okf"]) == int(case.vis_l.sum() + case.vis_r.sum()) and p["pts"].shape == (case.nlm, 3)
    job = cm.ba_job(p, sort=True)
    s = R.structure(case.nkf, case.nlm, job[2], job[3], R.tile_cap(case.max_kf))
    assert case.prop(s)


def test_make_ba_problem_is_unchanged():
    p = cm.make_ba_problem(np.random.default_rng(61), 7, 300)
    assert len(p["okf"]) == MAKE_BA_PROBLEM_PIN[0]
    assert abs(float(p["poses0"].sum()) - MAKE_BA_PROBLEM_PIN[1]) < 1e-9 and abs(float(p["pts0"].sum()) - MAKE_BA_PROBLEM_PIN[2]) < 1e-9
    assert abs(float(p["ouv"].astype(np.float64).sum()) - MAKE_BA_PROBLEM_PIN[3]) < 1e-3
    assert int(p["okf"].astype(np.int64) @ np.arange(len(p["okf"]))) == MAKE_BA_PROBLEM_PIN[4]


# recorded from make_ba_problem before this file existed: edges, sums of the initial values and measurements, an order-sensitive sum
MAKE_BA_PROBLEM_PIN = (2857, -10.420994878377892, 8506.592922835202, 998372.8532268032, 12053240)
