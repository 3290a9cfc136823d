"""svslam_local_fusion_batch on the device against tests/ref_local_fusion.py, bit for bit (f64 products and sums in a stated order,
contraction off): every call of local_fusion_cases.py through Context.local_fusion; the jobs of a call alone and together, a second
identical call; every refusal with the C arrays untouched; gaps between the jobs; the timing family."""
import ctypes as C

import numpy as np
import pytest

import local_fusion_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(svs):
    c = svs.Context(64, 32, max_slots=1, max_jobs=2)
    yield c
    c.close()


def _raw(ctx, arr, n, P, X, OP, OK, K):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx.L.svslam_local_fusion_batch(ctx.h, n, arr, 0 if P is None else len(P), p(P), 0 if X is None else len(X), p(X), p(OP),
                                         0 if OK is None else len(OK), p(OK), p(K))
    return rc, ctx.L.svslam_last_error(ctx.h).decode()


@pytest.mark.parametrize("name", list(lc.calls()))
def test_against_the_reference_bit_for_bit(ctx, name):
    jobs = lc.calls()[name]
    got = ctx.local_fusion(jobs)
    why = lc.same_bits(got, lc.reference(name))
    assert why is None, why
    why = lc.same_bits(ctx.local_fusion(jobs), got)                 # the same call again: the same bits
    assert why is None, why


def test_batch_independence(ctx):
    """all jobs of all cases in one call (more jobs than max_jobs: the family is not bounded by it), and every job alone"""
    names = [n for n in lc.calls() if lc.calls()[n]]
    jobs = [j for n in names for j in lc.calls()[n]]
    ref = [r for n in names for r in lc.reference(n)]
    together = ctx.local_fusion(jobs)
    why = lc.same_bits(together, ref)
    assert why is None, why
    for i in (0, 5, len(jobs) - 1):
        (alone,) = ctx.local_fusion([jobs[i]])
        assert lc.same_bits([alone], [together[i]]) is None, i


def test_gaps_between_the_jobs_come_back_untouched(ctx):
    jobs = lc.refusal_base()
    arr, P, X, OP, OK = lc.pack(jobs)
    P2 = np.concatenate([P[:4], np.full((3, 7), 7.5), P[4:]]); X2 = np.concatenate([X[:20], np.full((5, 3), -3.25), X[20:]])
    OP2 = np.concatenate([OP[:21], np.full(5, OP[20], np.int32), OP[21:]])
    arr[1].kf_ofs += 3; arr[1].pt_ofs += 5
    K = np.full(len(X2), -7, np.int32)
    rc, err = _raw(ctx, arr, 2, P2, X2, OP2, OK, K)
    assert rc == 0, err
    assert (P2[4:7] == 7.5).all() and (X2[20:25] == -3.25).all() and (K[20:25] == -7).all()
    ref = [lc.rlf.fuse(j) for j in jobs]
    assert np.array_equal(P2[:4], ref[0]["poses"]) and np.array_equal(P2[7:], ref[1]["poses"])
    assert np.array_equal(X2[:20], ref[0]["pts"]) and np.array_equal(X2[25:], ref[1]["pts"])
    assert np.array_equal(K[:20], ref[0]["pt_kf"]) and np.array_equal(K[25:], ref[1]["pt_kf"])
    assert np.array_equal(np.array(arr[0].T_cur), jobs[0]["T_cur"])          # an inactive cur is written nowhere


def test_refusals_write_nothing(ctx):
    for name, edit, text in lc.refusals():
        arr, P, X, OP, OK = lc.pack(lc.refusal_base())
        K = np.full(len(X), -7, np.int32)
        edit(arr, P, X, OP, OK)
        keep = (P.copy(), X.copy(), K.copy(), bytes(arr))
        rc, err = _raw(ctx, arr, 2, P, X, OP, OK, K)
        assert rc != 0 and text in err and err.startswith("local_fusion: "), (name, err)
        assert np.array_equal(P, keep[0]) and np.array_equal(X, keep[1]) and np.array_equal(K, keep[2]) and bytes(arr) == keep[3], name
    arr, P, X, OP, OK = lc.pack(lc.refusal_base())
    K = np.full(len(X), -7, np.int32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)

    def call(**change):
        args = dict(njobs=2, jobs=arr, total_kf=len(P), poses=p(P), total_pts=len(X), pts=p(X), obs_ptr=p(OP), total_obs=len(OK),
                    obs_kf=p(OK), pt_kf=p(K))
        args.update(change)
        return ctx.L.svslam_local_fusion_batch(ctx.h, *args.values()), ctx.L.svslam_last_error(ctx.h).decode()
    for k in ("jobs", "poses", "pts", "obs_ptr", "obs_kf", "pt_kf"):
        rc, err = call(**{k: None})
        assert rc != 0 and "null" in err, (k, err)
    for k in ("njobs", "total_kf", "total_pts", "total_obs"):
        rc, err = call(**{k: -1})
        assert rc != 0 and "negative count" in err, (k, err)
    assert (K == -7).all()
    assert ctx.L.svslam_local_fusion_batch(ctx.h, 0, None, 0, None, 0, None, None, 0, None, None) == 0       # njobs == 0 is success
    # and the context still works
    why = lc.same_bits(ctx.local_fusion(lc.refusal_base()), [lc.rlf.fuse(j) for j in lc.refusal_base()])
    assert why is None, why


def test_timing_family_counts_jobs(ctx, svs):
    assert svs.LOOP_FAMILIES["local_fusion"] == 19 and svs.FAMILY_KERNELS["local_fusion"] == ["k_local_fusion"]
    assert sorted(svs.FAMILIES.values()) == [0, 1, 2, 3, 4, 5]           # what bench.py sums over has nothing new
    ctx.timing(True)
    ctx.local_fusion(lc.calls()["three_jobs"])
    ctx.local_fusion(lc.calls()["obs_lists"])
    ctx.local_fusion([])
    ms, launches, units = ctx.timing_get("local_fusion")
    ctx.timing(False)
    assert launches == 2 and units == 5 and ms > 0
