"""GPU: the batch local-BA solver (k_ba_build, BaHostStruct::build, k_local_ba_t<0>) on problems placed on either side of
the integer capacities that decide which code runs: blocks per LDS tile, BA_PIT_CAP staged pair items, the key space of
the landmark sort, the chunks the pair lists are emitted in, the edge cache of the build, 64 rows of the reduced system,
passes that run zero times.  tests/ba_structure_cases.py has the cases, tests/ref_ba_structure.py the rule; which side of a
boundary a problem ran on is read back through Context.ba_struct and asserted, never assumed.

Every case, in landmark-major and in shuffled edge order:
  (i)   Context.ba_struct == the restated structure, device build and host build; the case's own property holds;
  (ii)  device build == host build, every output bit;
  (iii) both == the oracle (jac_mode 0): iterations equal, translation 1e-6 m, quaternion 1e-7, points rtol / atol 1e-6,
        chi2 rtol 1e-5 atol 1e-6 (the tolerances of test_gpu_parity.py and test_gpu_general_rig.py);
  (iv)  the LM trajectory == the oracle's, trial by trial (lm_cases.assert_traces_agree).
Run with -s for the deviations from the oracle per case and their maxima."""
import os

import numpy as np
import pytest

import ba_structure_cases as bc
import common as cm
import lm_cases as lc
import ref_ba_structure as R

pytestmark = pytest.mark.gpu

RIG = cm.KITTI_RIG
CASES = bc.all_cases()
FIELDS = ("nblk", "na", "ncontrib", "ntile", "nmv")
WORST = dict(t=0.0, q=0.0, points=0.0, chi2=0.0)


def _context(svs, host_build, **kw):
    old = os.environ.get("SVSLAM_BA_HOST_BUILD")
    if host_build:
        os.environ["SVSLAM_BA_HOST_BUILD"] = "1"
    else:
        os.environ.pop("SVSLAM_BA_HOST_BUILD", None)
    try:
        c = svs.Context(cm.W, cm.H, max_slots=1, **kw)
    finally:
        if old is None:
            os.environ.pop("SVSLAM_BA_HOST_BUILD", None)
        else:
            os.environ["SVSLAM_BA_HOST_BUILD"] = old
    c.lm_trace(True)
    return c


@pytest.fixture(scope="module")
def contexts(svs):
    """(device build, host build) per max_kf, made when first asked for"""
    made = {}

    def get(max_kf):
        if max_kf not in made:
            kw = dict(max_jobs=2, max_kf=max_kf, max_lm=2048, max_obs=20000)
            made[max_kf] = (_context(svs, False, **kw), _context(svs, True, **kw))
        return made[max_kf]
    yield get
    for cd, ch in made.values():
        cd.close(); ch.close()
    print("\nlargest deviation from the oracle over the structure cases: t %.1e m, q %.1e, points %.1e (rel), chi2 %.1e (rel)"
          % (WORST["t"], WORST["q"], WORST["points"], WORST["chi2"]))


def _jobs(p):
    """the landmark-major and the shuffled statement of one problem, and the map between their edges"""
    srt, shuf = cm.ba_job(p, sort=True), cm.ba_job(p)
    o = np.lexsort((p["okf"], p["olm"]))
    assert not np.array_equal(o, np.arange(len(o))), "the shuffled order is in order"
    return [srt, shuf], o


def _solve(c, jobs):
    res = c.local_ba(jobs, *RIG)
    return res, c.ba_struct(len(jobs)), [c.lm_trace(job=i) for i in range(len(jobs))]


def _assert_struct(st, s, res, traces, host, cached, what):
    """(i): the descriptors the solver returned == the restatement"""
    for i, row in enumerate(st):
        got = dict(zip(FIELDS, row[:5].tolist()))
        assert got == {f: s[f] for f in FIELDS}, (what, i, got, {f: s[f] for f in FIELDS})
        assert row[5] == res[i][3] and row[6] == len(traces[i]) >= row[5], (what, i, row.tolist(), res[i][3], len(traces[i]))
        want = (1 if i == 0 else 0) | (4 if host else (2 if cached else 0))
        assert row[7] == want, (what, i, "flags", int(row[7]), want)


def _bit_equal(a, b, what):
    for i, ((pa, xa, ca, ia), (pb, xb, cb, ib)) in enumerate(zip(a, b)):
        assert ia == ib, (what, i)
        assert np.array_equal(pa, pb), (what, i, "poses", np.abs(pa - pb).max())
        assert np.array_equal(xa, xb), (what, i, "points", np.abs(xa - xb).max())
        assert np.array_equal(ca, cb), (what, i, "chi2", np.abs(ca - cb).max())


def _against_oracle(got, ref, what, skip_lm=None, skip_edge=None):
    """(iii), printed before it is asserted (common.against_oracle)"""
    cm.against_oracle(got, ref, what, WORST, skip_lm, skip_edge)


def test_tile_capacities(svs):
    """what the case list is written for: 480 blocks per tile at max_kf 10, 432 at 12, 64 at 20"""
    assert [R.tile_cap(k) for k in (10, 12, 20)] == [480, 432, 64] == [bc.TILE_CAP[k] for k in (10, 12, 20)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_structure_case(svs, orc, contexts, case):
    s = case.structure()
    assert case.prop(s), "the case lost the property it is named for"
    p = cm.make_ba_problem_vis(np.random.default_rng(1 + CASES.index(case)), case.vis_l, case.vis_r)
    jobs, o = _jobs(p)
    nobs = len(p["okf"])
    assert R.edge_cache_fits(case.nlm, nobs)
    cd, ch = contexts(case.max_kf)
    rd, sd, td = _solve(cd, jobs)
    rh, sh, th = _solve(ch, jobs)
    _assert_struct(sd, s, rd, td, False, True, case.name + ", device build")
    _assert_struct(sh, s, rh, th, True, False, case.name + ", host build")
    assert np.array_equal(sd[:, 5:7], sh[:, 5:7]), (case.name, "iterations / LM trials", sd[:, 5:7].tolist(), sh[:, 5:7].tolist())
    _bit_equal(rd, rh, case.name + ": device build vs host build")
    for a, b in zip(td, th):
        assert np.array_equal(a, b), (case.name, "LM trace, device build vs host build")
    # the two statements of the problem are one problem
    assert np.array_equal(rd[0][0], rd[1][0]) and np.array_equal(rd[0][1], rd[1][1]) and np.array_equal(rd[0][2], rd[1][2][o])
    ref = orc.local_ba_trace(*RIG, *jobs[0], jac_mode=0)
    # landmarks with a single edge: their position is held by lambda alone; the only exclusion, and only where the case is about it
    lonely = np.bincount(p["olm"], minlength=case.nlm) == 1
    assert lonely.any() == case.single_edge_ok and lonely.sum() <= 0.02 * case.nlm
    skip_lm = lonely if lonely.any() else None
    skip_ed = lonely[jobs[0][3]] if lonely.any() else None
    _against_oracle(rd[0], ref, case.name, skip_lm, skip_ed)
    shuffled = (rd[1][0], rd[1][1], rd[1][2][o], rd[1][3])
    _against_oracle(shuffled, ref, case.name + " (shuffled)", skip_lm, skip_ed)
    for tr, what in ((td[0], case.name), (td[1], case.name + " (shuffled)")):
        lc.assert_traces_agree(tr, ref[4], need_rejected=0, what=what)


# --------------------------------------------------------------------------- the low-latency solver on the same problems
LL_CASES = bc.ll_cases()
LL_MAX_KF = cm.LL_CTX_KW["max_kf"]
# With 4 shards these two problems have a shard of more blocks than the resident kernel holds (263 / 264 against 256 at max_kf 11)
# and go to the streaming kernel; every other case, and every case with 16 shards, is resident.  Written down so that a change of
# the dealing rule or of the capacities that leaves one of the two kernels unexercised fails here instead of passing in silence.
LL_STREAMING = {(4, "cap480-whole-tiles-only"), (4, "cap480-whole-tiles-and-one-block-pair-more")}


@pytest.fixture(scope="module", params=[4, 16], ids=lambda w: "%dshards" % w)
def ll_ctx(svs, request):
    c = cm.make_ll_ctx(svs, request.param, 1)
    c.shards = request.param
    yield c
    c.close()


@pytest.mark.parametrize("case", LL_CASES, ids=repr)
def test_structure_case_low_latency(ll_ctx, orc, case):
    """submit / collect with the problem dealt to 4 and to 16 shards: what Context.ll_shards reports — landmarks, edges, blocks,
    tiles, solver (2 resident k_ba_ll, 1 streaming k_local_ba_t<2>), active poses and shard mask of every shard — equals the
    restatement of the dealing rule, of k_ba_build's shard structure and of k_ba_split's fit test (ref_ba_structure.ll_shards;
    ll_deal is held to a loop-only second implementation in test_ref_ba_structure.py), a shard without edges is missing from the
    shard mask, results and LM trajectory are the oracle's.  LL_STREAMING names the cases that must meet the streaming kernel.
    The shard solvers' own boundaries are in tests/test_gpu_ll_structure.py."""
    by_name = {c.name: k for k, c in enumerate(CASES)}
    p = cm.make_ba_problem_vis(np.random.default_rng(1 + by_name.get(case.name, len(CASES))), case.vis_l, case.vis_r)
    job = cm.ba_job(p, sort=True)
    ll_ctx.host_counters()
    (got,) = ll_ctx.local_ba([job], *RIG, split=True)
    cnt = ll_ctx.host_counters()
    assert cnt[6] == 1 and cnt[7] == 0, "the low-latency solver did not take the problem, or gave it up: %s" % cnt[6:]
    sh = ll_ctx.ll_shards(1)[0]
    tr = ll_ctx.lm_trace(job=0)
    assert sh.shape[0] == ll_ctx.shards
    assert sh[:, 0].sum() == case.nlm and sh[:, 1].sum() == len(job[2]) and sh[:, 2].sum() == case.structure()["nblk"]
    want, _, deal = R.ll_shards(job[3], job[2], case.nkf, case.nlm, ll_ctx.shards, LL_MAX_KF, 1)
    assert np.array_equal(sh[:, :7], want), (case.name, "shards (landmarks, edges, blocks, tiles, solver, poses, mask)", sh[:, :7].tolist(), want.tolist(), deal["cut"])
    assert int(sh[0, 4]) == (1 if (ll_ctx.shards, case.name) in LL_STREAMING else 2), (case.name, ll_ctx.shards, "solver", int(sh[0, 4]), sh[:, :3].tolist())
    mask = int(sh[0, 6])
    assert np.all(sh[:, 6] == mask) and [(mask >> w) & 1 for w in range(ll_ctx.shards)] == (sh[:, 1] > 0).astype(int).tolist()
    if case.name == "ll-ten-landmarks" and ll_ctx.shards == 16:
        assert bin(mask).count("1") <= 10, "ten landmarks with edges in more than ten shards"
    print("%-50s %2d shards: solver %d, %2d with edges, largest %3d landmarks %3d edges %3d blocks"
          % (case.name, ll_ctx.shards, sh[0, 4], bin(mask).count("1"), sh[:, 0].max(), sh[:, 1].max(), sh[:, 2].max()))
    ref = orc.local_ba_trace(*RIG, *job, jac_mode=0)
    lonely = np.bincount(p["olm"], minlength=case.nlm) == 1
    assert lonely.any() == case.single_edge_ok and lonely.sum() <= 0.02 * case.nlm
    _against_oracle(got, ref, "%s, %d shards" % (case.name, ll_ctx.shards), lonely if lonely.any() else None,
                    lonely[job[3]] if lonely.any() else None)
    lc.assert_traces_agree(tr, ref[4], need_rejected=0, what="%s, %d shards" % (case.name, ll_ctx.shards))


def test_edge_cache_used_or_not_gives_the_same_bits(svs, orc):
    """k_ba_build reads the edges from its LDS cache, or through srt from global memory when the batch's largest landmark
    count and largest edge count no longer leave room: one problem alone (cached), beside a mostly edgeless problem of just
    enough landmarks to lose the cache, and beside one with a landmark fewer (cached again) — the same bits each time"""
    vl, vr = bc.edge_cache_masks()
    p = cm.make_ba_problem_vis(np.random.default_rng(70), vl, vr)
    nlm, nobs = vl.shape[1], len(p["okf"])
    big, small = bc.edge_cache_partner_nlm(nlm, nobs, False), bc.edge_cache_partner_nlm(nlm, nobs, True)
    assert R.edge_cache_fits(nlm, nobs) and not R.edge_cache_fits(big, nobs) and R.edge_cache_fits(small, nobs) and big == small + 1

    def partner(n):
        vis = np.zeros((3, n), bool)
        vis[:, 5:n:97] = True                                    # a few three-view landmarks, the rest without edges
        return cm.ba_job(cm.make_ba_problem_vis(np.random.default_rng(71), vis, vis), sort=True)
    kw = dict(max_jobs=3, max_kf=10, max_lm=big, max_obs=16384)
    assert R.bb_lds_bytes(big) <= R.CREATE_BUILD_LDS_LIMIT and nobs <= 16384
    (srt, shuf), o = _jobs(p)
    cd, ch = _context(svs, False, **kw), _context(svs, True, **kw)
    try:
        alone, st_alone, _ = _solve(cd, [srt, shuf])
        host, st_host, _ = _solve(ch, [srt, shuf])
        past, st_past, _ = _solve(cd, [srt, shuf, partner(big)])
        under, st_under, _ = _solve(cd, [srt, shuf, partner(small)])
    finally:
        cd.close(); ch.close()
    assert st_alone[:, 7].tolist() == [3, 2] and st_host[:, 7].tolist() == [5, 4]
    assert st_past[:, 7].tolist() == [1, 0, 1], "the edge cache was used beside a problem of %d landmarks" % big
    assert st_under[:, 7].tolist() == [3, 2, 3], "the edge cache was not used beside a problem of %d landmarks" % small
    s = R.structure(10, nlm, srt[2], srt[3], R.tile_cap(10))
    for st in (st_alone, st_host, st_past, st_under):
        for row in st[:2]:
            assert dict(zip(FIELDS, row[:5].tolist())) == {f: s[f] for f in FIELDS}
    assert s["ntile"] >= 10 and s["nblk"] * 2 == nobs
    _bit_equal(alone, host, "cached device build vs host build")
    _bit_equal(alone, past[:2], "edge cache used vs not used")
    _bit_equal(alone, under[:2], "alone vs just under the limit")
    assert past[2][3] == under[2][3]
    _against_oracle(alone[0], orc.local_ba(*RIG, *srt, jac_mode=0), "edge cache problem (%d landmarks, %d edges)" % (nlm, nobs))
