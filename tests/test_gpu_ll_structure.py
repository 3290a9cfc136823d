"""GPU: the low-latency local BA (k_ba_split, k_ba_build for a shard, k_ba_ll, k_local_ba_t<2, W>) on problems placed on either
side of the integer capacities that decide which of its kernels solves a problem and which path a shard takes inside it: blocks,
landmarks and edges of a resident shard, the streaming kernel's tile, a shard in LDS or in global memory, the smaller of the two
tile capacities at max_kf 7 and 13, windows of up to 16 keyframes, a shard mask with holes in the middle.
tests/ba_structure_cases.py::ll_boundary_cases has the cases, tests/ref_ba_structure.py the dealing rule and the capacities;
tests/test_ref_ba_structure.py asserts every case's predicate on the CPU.

Every case, on the context it names (max_kf, shard count, with or without the resident kernel):
  (1) the low-latency solver took the problem and did not give it up (host_counters()[6] == 1, [7] == 0);
  (2) Context.ll_shards == the restatement, per shard: landmarks, edges, blocks, tiles, solver code, active poses, mask;
  (3) poses, points and chi2 == the oracle's (jac_mode 0) at common.against_oracle's tolerances, the LM trajectory == the oracle's
      trial by trial (lm_cases.assert_traces_agree);
  (4) the same call again gives the same bits;
  (5) LL_PAIRS: the two cases of a boundary reach the two solver codes / tile counts written there.
Run with -s for the deviations from the oracle per case and their maxima."""
import numpy as np
import pytest

import ba_structure_cases as bc
import common as cm
import lm_cases as lc
import ref_ba_structure as R

pytestmark = pytest.mark.gpu

RIG = cm.KITTI_RIG
CASES = bc.ll_boundary_cases()
BY_NAME = {c.name: c for c in CASES}
WORST = dict(t=0.0, q=0.0, points=0.0, chi2=0.0)
WORST_WIDE = dict(t=0.0, q=0.0, points=0.0, chi2=0.0)          # the cases of 12 and 16 keyframes alone
SEEN = {}                                                      # case name -> [W, 8] as the library reported it

# (case on / below the boundary, case above it, what differs): "solver" — 2 (resident k_ba_ll) on, 1 (streaming
# k_local_ba_t<2>) above; "tiles" — the largest tile count of a shard, 1 on, 2 above (both streaming); "in LDS" — both streaming,
# told apart by the sizes alone (ref_ba_structure.ll_shard_in_lds of the reported rows: all shards in, one out).
# Literal, so that a change of the capacities or of the dealing rule that leaves one side of a boundary unexercised fails here.
LL_PAIRS = [
    ("ll-res-w4-blocks-256", "ll-res-w4-blocks-257-in-shard-0", "solver"),
    ("ll-res-w4-blocks-256", "ll-res-w4-blocks-257-in-a-middle-shard", "solver"),
    ("ll-res-w4-blocks-256", "ll-res-w4-blocks-257-in-the-last-shard", "solver"),
    ("ll-res-w8-blocks-256", "ll-res-w8-blocks-257-in-a-middle-shard", "solver"),
    ("ll-res-w16-blocks-256", "ll-res-w16-blocks-257-in-a-middle-shard", "solver"),
    ("ll-res-w4-landmarks-208", "ll-res-w4-landmarks-209", "solver"),
    ("ll-res-w4-edges-448", "ll-res-w4-edges-449", "solver"),
    ("ll-stream-w4-blocks-256", "ll-stream-w4-blocks-257-in-a-middle-shard", "tiles"),
    ("ll-stream-w4-in-lds-edges-704", "ll-stream-w4-in-lds-edges-705", "in LDS"),
    ("ll-stream-w4-in-lds-landmarks-448", "ll-stream-w4-in-lds-landmarks-449", "in LDS"),
    ("ll-kf7-res-w4-blocks-320", "ll-kf7-res-w4-blocks-321", "solver"),
    ("ll-kf7-stream-w4-blocks-368", "ll-kf7-stream-w4-blocks-369", "tiles"),
    ("ll-kf13-res-w4-blocks-176", "ll-kf13-res-w4-blocks-177", "solver"),
    ("ll-kf16-res-w4-blocks-64", "ll-kf16-res-w4-blocks-65", "solver"),
]

# Contexts take the library's 16 pooled streams in rotation and test_gpu_low_latency_pipeline.py depends on which streams its
# contexts get (tests/global_desc_cases.py, "the contexts these device tests make"): this module counts the contexts it makes
# and its last test makes the rest of a multiple of 16.
ROTATION = 16
_made = [0]


def _count(c):
    _made[0] += 1
    return c


@pytest.fixture(scope="module")
def contexts(svs):
    """low-latency contexts by (max_kf, shards, resident), made when first asked for"""
    made = {}

    def get(max_kf, shards, resident):
        key = (max_kf, shards, resident)
        if key not in made:
            made[key] = _count(cm.make_ll_ctx(svs, shards, resident, max_kf=max_kf))
        return made[key]
    yield get
    for c in made.values():
        c.close()
    for what, w in (("low-latency boundary cases", WORST), ("cases of 12 and 16 keyframes", WORST_WIDE)):
        print("\nlargest deviation from the oracle over the %s: t %.1e m, q %.1e, points %.1e (rel), chi2 %.1e (rel)"
              % (what, w["t"], w["q"], w["points"], w["chi2"]))


def _problem(case):
    p = cm.make_ba_problem_vis(np.random.default_rng(500 + CASES.index(case)), case.vis_l, case.vis_r)
    job = cm.ba_job(p, sort=True)
    assert not (np.bincount(p["olm"], minlength=case.nlm) == 1).any(), "a landmark with a single edge"
    return job


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_ll_boundary_case(contexts, orc, case):
    want, _, deal = case.shards()
    assert case.prop(want), "the case lost the property it is named for"
    job = _problem(case)
    c = contexts(case.max_kf, case.W, case.resident)
    c.host_counters()
    (got,) = c.local_ba([job], *RIG)
    cnt = c.host_counters()
    assert cnt[6] == 1 and cnt[7] == 0, "the low-latency solver did not take the problem, or gave it up: %s" % cnt[6:]
    sh = c.ll_shards(1)[0]
    tr = c.lm_trace(job=0)
    SEEN[case.name] = sh.copy()
    assert sh.shape[0] == case.W
    assert np.array_equal(sh[:, :7], want), (case.name, "shards (landmarks, edges, blocks, tiles, solver, poses, mask)",
                                             sh[:, :7].tolist(), want.tolist(), deal["cut"])
    assert np.all(sh[sh[:, 1] > 0, 5] == case.nkf)
    print("%-50s %2d shards: solver %d, mask %s, largest %3d landmarks %3d edges %3d blocks %d tiles"
          % (case.name, case.W, sh[0, 4], bin(int(sh[0, 6])), sh[:, 0].max(), sh[:, 1].max(), sh[:, 2].max(), sh[:, 3].max()))
    ref = orc.local_ba_trace(*RIG, *job, jac_mode=0)
    dev = cm.against_oracle(got, ref, case.name, WORST)
    if case.nkf >= 12:
        WORST_WIDE.update({k: max(WORST_WIDE[k], float(v)) for k, v in dev.items()})
    lc.assert_traces_agree(tr, ref[4], need_rejected=0, what=case.name)
    # landmarks without edges stay where they were
    bare = ~(case.vis_l | case.vis_r).any(0)
    assert np.array_equal(got[1][bare], job[1][bare])
    # (4) again: the same bits, and still not given up
    (again,) = c.local_ba([job], *RIG)
    cnt = c.host_counters()
    assert cnt[6] == 1 and cnt[7] == 0, cnt[6:]
    assert again[3] == got[3] and all(np.array_equal(a, b) for a, b in zip(again[:3], got[:3])), (case.name, "not deterministic")
    assert np.array_equal(c.lm_trace(job=0), tr)


@pytest.mark.parametrize("on,above,what", LL_PAIRS, ids=[p[1] for p in LL_PAIRS])
def test_ll_pair_reaches_both_sides(on, above, what):
    """(5), from what the library reported in test_ll_boundary_case"""
    assert on in SEEN and above in SEEN, "run the whole module: the pair's cases have not been solved"
    a, b = SEEN[on], SEEN[above]
    if what == "solver":
        assert np.all(a[:, 4] == 2) and np.all(b[:, 4] == 1), (a[:, 4].tolist(), b[:, 4].tolist())
        assert np.all(a[:, 3] == 1) and b[:, 3].max() == (2 if "blocks" in above else 1), (a[:, 3].tolist(), b[:, 3].tolist())
    elif what == "tiles":
        assert np.all(a[:, 4] == 1) and np.all(b[:, 4] == 1)
        assert a[:, 3].max() == 1 and sorted(b[:, 3].tolist())[-2:] == [1, 2], (a[:, 3].tolist(), b[:, 3].tolist())
    else:
        assert np.all(a[:, 4] == 1) and np.all(b[:, 4] == 1)
        ia = [R.ll_shard_in_lds(int(n), int(e)) for n, e in a[:, :2]]
        ib = [R.ll_shard_in_lds(int(n), int(e)) for n, e in b[:, :2]]
        assert all(ia) and ib.count(False) == 1, (ia, ib)


def test_window_of_17_keyframes_goes_to_the_batch_solver(svs, orc):
    """max_kf 17: tile_cap_ll is 0, svslam_set_low_latency makes no shard solver, the call is the batch solver's — no problem
    counted for the low-latency solver, the result that of a context that never asked for it, bit for bit, and the oracle's"""
    case = BY_NAME["ll-kf16-res-w4-16-keyframes"]
    job = _problem(case)
    cl = _count(cm.make_ll_ctx(svs, 4, 1, max_kf=17))
    cb = _count(svs.Context(cm.W, cm.H, **dict(cm.LL_CTX_KW, max_kf=17)))
    try:
        assert cl.ll_limits()[:2] == [0, 0]
        cl.host_counters()
        (a,) = cl.local_ba([job], *RIG)
        cnt = cl.host_counters()
        assert cnt[6] == 0 and cnt[7] == 0, cnt[6:]
        (b,) = cb.local_ba([job], *RIG)
        assert a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        cm.against_oracle(a, orc.local_ba_trace(*RIG, *job, jac_mode=0), "17-keyframe context, batch solver")
    finally:
        cl.close(); cb.close()


def test_the_stream_rotation_is_left_where_it_was(svs):
    """the last test of this module: the contexts it made, and as many small ones as bring the count to a multiple of 16"""
    n = (-_made[0]) % ROTATION
    for _ in range(n):
        svs.Context(32, 32, max_slots=1, max_jobs=1).close()
    _made[0] = 0
