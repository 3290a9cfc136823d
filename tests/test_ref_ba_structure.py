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
