"""svslam_pose_graph_batch on the device against tests/ref_pose_graph.py (closed-form Jacobians, the mode the kernel uses): the LM
decisions exact, lambda / chi2 / poses / points within the tolerances of pose_graph_cases.py; determinism and independence of
the jobs of a call; the ABI's refusals; the timing family."""
import numpy as np
import pytest

import pose_graph_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(svs):
    c = svs.Context(64, 32, max_slots=1, max_jobs=32)
    c.lm_trace(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ties():
    """cases that used the tie rule (one trial each): at most two in the whole module, checked once when the module is done"""
    used = []
    yield used
    assert len(used) <= 2, "more than two cases needed the tie rule: %s" % used


@pytest.mark.parametrize("name", list(pc.cases()))
def test_against_the_reference(ctx, ties, name):
    job = pc.cases()[name]
    ref = pc.reference(name)
    (got,) = ctx.pose_graph([job], iters=pc.ITERS[name])
    got["trace"] = ctx.lm_trace(job=0)
    if name in pc.CHI2_BEFORE_ONLY_ON_DEVICE:       # theta = pi: the Jacobian is 0 / 0 (pose_graph_cases._pi).  A finite residual of the
        # right norm is all this sees: not the sign of the branch, which the host emulation checks
        d = abs(got["chi2_before"] - ref["chi2_before"]) / ref["chi2_before"]
        print(name, "chi2_before differs by", d)
        assert d <= pc.TOL_SMALL["chi2"], (name, got["chi2_before"], ref["chi2_before"])
        return
    ok, tied, msg = pc.compare(got, ref, pc.tol_of(name), allow_tie=True)
    print(name, msg)
    if tied:
        ties.append(name)
    assert ok, msg
    if name == "ten_failed":
        assert got["iters"] == 1 and got["trials"] == 10 and not got["trace"][:, 5].any()       # the ten-failed-trials stop
    if name in ("empty", "n1", "edgeless", "optimum", "zero_chain", "ten_failed"):
        assert np.array_equal(got["poses"], np.asarray(job["poses"]).reshape(-1, 7))          # the input bits
    if name == "optimum":
        assert got["iters"] == 1 and got["trials"] == 1 and got["trace"][0, 4] == 0.0          # stopped by the rho == 0 rule
    if name in ("empty", "n1", "edgeless"):
        assert got["iters"] == 0 and got["trials"] == 0 and got["chi2_before"] == 0.0 and got["chi2_after"] == 0.0

    def run(jobs, iters):
        out = ctx.pose_graph(jobs, iters=iters)
        for i, o in enumerate(out):
            o["trace"] = ctx.lm_trace(job=i)
        return out
    pc.check_new_case(name, job, got, run, same_libm=False)


@pytest.mark.parametrize("name", pc.FULL_RUN_CASES)
def test_final_state_at_the_reference_s_22_iterations(ctx, name):
    """the caller's real iters: decisions past convergence are noise and not compared, the converged state is"""
    (got,) = ctx.pose_graph([pc.cases()[name]], iters=22)
    ok, msg = pc.compare_final(got, pc.reference22(name), pc.tol_of(name))
    print(name, msg)
    assert ok, msg


def test_batch_independence_and_determinism(ctx):
    """every case in one call (empty and edgeless jobs included), the same call again, and every job alone: the same bits.
    (Calls of at most 32 jobs, the context's max_jobs, so that every job of a call has a trace; test_jobs_beyond_max_jobs is about more.)"""
    c = pc.cases()
    for lo in range(0, len(c), 32):
        _together_again_alone(ctx, c, list(c)[lo:lo + 32])


def _together_again_alone(ctx, c, names):
    together = ctx.pose_graph([c[n] for n in names], iters=22)
    traces = [ctx.lm_trace(job=i) for i in range(len(names))]
    again = ctx.pose_graph([c[n] for n in names], iters=22)
    for i, n in enumerate(names):
        (alone,) = ctx.pose_graph([c[n]], iters=22)
        assert np.array_equal(ctx.lm_trace(job=0), traces[i]), n
        assert len(traces[i]) == together[i]["trials"], n
        for k in ("poses", "pts"):
            assert np.array_equal(alone[k], together[i][k]) and np.array_equal(again[i][k], together[i][k]), (n, k)
        for k in ("iters", "trials", "chi2_before", "chi2_after"):
            assert alone[k] == together[i][k] == again[i][k], (n, k)


def _same_bits(a, b, what):
    for k in ("poses", "pts"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("iters", "trials", "chi2_before", "chi2_after"):
        assert a[k] == b[k], (what, k)


def test_jobs_beyond_max_jobs(ctx):
    """40 jobs on a context with max_jobs = 32 and the trace on: jobs 32 .. 39 have no trace slot (the kernel's trace pointer is
    null for them) and return the bits they return alone, reading their trace is refused, jobs 0 .. 31 are traced as ever"""
    c = pc.cases()
    small = ["n2", "n3_loop_to_fixed", "span2", "reversed", "fixed_last", "theta_0.5", "duplicate_edge", "isolated_free"]
    names = [small[i % 8] for i in range(32)] + small[3:] + small[:3]
    got = ctx.pose_graph([c[n] for n in names], iters=4)
    traces = [ctx.lm_trace(job=i) for i in range(32)]
    for j in (32, 39, 40):
        with pytest.raises(RuntimeError, match="out of range"):
            ctx.lm_trace(job=j)
    for i in range(32):
        assert len(traces[i]) == got[i]["trials"] > 0 and traces[i][0, 2] == got[i]["chi2_before"], (i, names[i])
        assert np.array_equal(traces[i], traces[i % 8]), (i, names[i])
    for i in range(32, 40):
        (alone,) = ctx.pose_graph([c[names[i]]], iters=4)
        _same_bits(got[i], alone, (i, names[i]))
        assert alone["trials"] > 0


def test_the_kept_scratch_carries_nothing_over(svs):
    """on a fresh context: a small graph, n65 (which makes the context replace its buffer by a larger one, kept from then on), the
    small graph again, now in memory that n65 left its solver state in: the first and third results are the same bits, trace included"""
    c = pc.cases()
    ctx = svs.Context(64, 32, max_slots=1, max_jobs=2)
    ctx.lm_trace(True)
    try:
        _small_big_small(ctx, c)
    finally:
        ctx.close()


def _small_big_small(ctx, c):
    (first,) = ctx.pose_graph([c["reversed"]], iters=22); t1 = ctx.lm_trace(job=0)
    (big,) = ctx.pose_graph([c["n65"]], iters=pc.ITERS["n65"])
    (third,) = ctx.pose_graph([c["reversed"]], iters=22); t3 = ctx.lm_trace(job=0)
    assert big["trials"] > 0 and first["trials"] > 0
    _same_bits(first, third, "reversed")
    assert np.array_equal(t1, t3)


def test_refusals_write_nothing(ctx):
    base = pc.cases()["span2"]
    ea, eb, meas = base["edges"]

    def refused(word, **change):
        job = dict(base); job.update(change)
        with pytest.raises(RuntimeError, match=word):
            ctx.pose_graph([pc.cases()["n2"], job], iters=5)
    bad = ea.copy(); bad[2] = 8
    refused("out of its job's range", edges=(bad, eb, meas))
    bad = ea.copy(); bad[2] = -1
    refused("out of its job's range", edges=(bad, eb, meas))
    bad = eb.copy(); bad[3] = ea[3]
    refused("to itself", edges=(ea, bad, meas))
    refused("none of them is fixed", fixed=np.zeros(8, np.uint8))
    p = np.array(base["poses"]); p[4, :4] *= 1 + 2e-6
    refused("unit length", poses=p)
    m = meas.copy(); m[1, :4] *= 1 - 2e-6
    refused("unit length", edges=(ea, eb, m))
    import ctypes as C
    svs_mod = __import__("importlib").import_module("stereovision-slam_amd")
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    tab, P, F, A, B, M, AN, X = pc.pack([pc.cases()["n2"], base])
    for change, word in (((1, 0, 0), "ascend"), ((1, 1, 0), "no vertices")):      # job 1 starts inside job 0's vertices; job 1 has edges but nkf = 0
        t = tab.copy(); t[change[0], change[1]] = change[2]
        arr = (svs_mod.PgJob * 2)(*[svs_mod.PgJob(*[int(v) for v in r], 0, 0, 0.0, 0.0) for r in t])
        keep = P.copy()
        rc = ctx.L.svslam_pose_graph_batch(ctx.h, 2, arr, len(P), p_(P), p_(F), len(A), p_(A), p_(B), p_(M), len(X), p_(AN), p_(X), 5)
        assert rc != 0 and word in ctx.L.svslam_last_error(ctx.h).decode() and np.array_equal(P, keep)
    # the C arrays themselves are untouched by a refused call
    tab, P, F, A, B, M, AN, X = pc.pack([base])
    A[2] = 8
    arr = (svs_mod.PgJob * 1)(svs_mod.PgJob(*[int(v) for v in tab[0]], 7, 7, 7.0, 7.0))
    keep = P.copy()
    rc = ctx.L.svslam_pose_graph_batch(ctx.h, 1, arr, len(P), p_(P), p_(F), len(A), p_(A), p_(B), p_(M), len(X), p_(AN), p_(X), 5)
    assert rc != 0 and np.array_equal(P, keep) and arr[0].iters_done == 7 and arr[0].chi2_after == 7.0
    # and the context still works
    (got,) = ctx.pose_graph([base], iters=pc.ITERS["span2"])
    assert got["chi2_after"] < got["chi2_before"]


def test_timing_family_counts_jobs(ctx):
    c = pc.cases()
    ctx.timing(True)
    ctx.pose_graph([c["n2"], c["span2"], c["empty"]], iters=3)
    ctx.pose_graph([c["n17"]], iters=3)
    ms, launches, units = ctx.timing_get("pose_graph")
    ctx.timing(False)
    assert launches == 2 and units == 4 and ms > 0
