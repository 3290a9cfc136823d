"""svslam_loopdb_* and svslam_loop_candidates_batch on the device against tests/ref_loop_candidates.py on every case of
loop_candidates_cases.py, exactly: every refusal with its outputs untouched, every status, id and count, the bits of every similarity and
of every stored row; then Context's methods and the timing family."""
import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import loop_candidates_cases as lc
import ref_loop_candidates as rl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv(svs):
    d = lc.AbiDriver(svs)
    yield d
    d.close()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_against_the_reference(svs, drv, name):
    print(name, lc.check(name, drv))


def test_the_kept_staging_carries_nothing_over(svs):
    """on a fresh context with two streams of dim 128: one row appended to stream 0 and one query of it, eight rows appended to stream
    1, the query of stream 0 again.  A call stages its structs rounded up to 256 bytes, then 512 bytes per vector: 256 + 512 = 768
    bytes for the one-row append and for the query (the context then keeps 960), 256 + 8 * 512 = 4352 for the eight rows, more than
    1.25 * 768 + 256 = 1216, so that append replaces the buffer and the second query runs in what it left there.  Both queries give
    the same bits, the bits of a context that has seen only the first append, and the reference's; the eight rows are stored right."""
    dim = 128
    one, eight, ids8 = lc.vecs(61, 1, dim), lc.vecs(62, 8, dim), list(range(3, 27, 3))
    q = lc.near(one[0], 3, 0.005)[None]
    key = lambda g: (g["status"], g["cand_kf"], lc.bits(g["best_sim"]), g["best_kf"], g["n_weak"], g["n_compared"])
    ref = rl.Store(); ref.configure(2, 8, dim)
    assert ref.append([0], [2], one) is None and ref.append([1] * 8, ids8, eight) is None
    (want,) = ref.candidates([(0, 120)], q)
    a = gc.new_context(svs, 64, 48, max_slots=1, max_jobs=1)
    b = gc.new_context(svs, 64, 48, max_slots=1, max_jobs=1)
    try:
        for c in (a, b):
            c.loopdb_configure(2, 8, dim)
            c.loopdb_append([0], [2], one)
        (first,) = a.loop_candidates([(0, 120)], q)
        a.loopdb_append([1] * 8, ids8, eight)
        (third,) = a.loop_candidates([(0, 120)], q)
        (alone,) = b.loop_candidates([(0, 120)], q)
        ids, rows = a.loopdb_read(1)
    finally:
        a.close(); b.close(); gc.settle_rotation(svs)
    assert key(first) == key(third) == key(alone) == lc._result(want) and first["n_compared"] == 1 and first["status"] == rl.FOUND
    rid, rrows = ref.read(1)
    assert np.array_equal(ids, rid) and np.array_equal(rows.view(np.uint32), rrows.view(np.uint32))


def test_python_interface_and_timing_family(svs):
    ctx = svs.Context(64, 48, max_slots=1, max_jobs=1)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            ctx.loopdb_append([0], [0], np.ones((1, 4)))
        with pytest.raises(RuntimeError, match="dim must be"):
            ctx.loopdb_configure(1, 4, 4097)
        ctx.loopdb_configure(3, 40, 1280)
        ref = rl.Store(); ref.configure(3, 40, 1280)
        counts = (33, 0, 7)
        for s, n in enumerate(counts):
            if n:
                v = lc.vecs(50 + s, n, 1280); ids = list(range(2, 2 + 3 * n, 3))
                ctx.loopdb_append([s] * n, ids, v)
                assert ref.append([s] * n, ids, v) is None
        q = np.stack([lc.near(lc.vecs(50, 33, 1280)[4], 1, 0.005), lc.vecs(9, 1, 1280)[0], lc.near(lc.vecs(52, 7, 1280)[6], 2, 0.005)])
        jobs = [(0, 120), (1, 120), (2, 35)]
        ctx.timing(True)
        got = ctx.loop_candidates(jobs, q)
        ms, launches, units = ctx.timing_get("loop_candidates")
        ctx.timing(False)
        want = ref.candidates(jobs, q)
        assert [g["status"] for g in got] == [rl.FOUND, rl.NONE, rl.BELOW_STRONG] == [w[0] for w in want]
        for g, w in zip(got, want):
            assert (g["status"], g["cand_kf"], lc.bits(g["best_sim"]), g["best_kf"], g["n_weak"], g["n_compared"]) == lc._result(w)
        assert launches == 1 and ms > 0 and units == sum(g["n_compared"] for g in got) == 33 + 0 + 5
        assert svs.LC_STATUS[got[0]["status"]] == "FOUND" and got[0]["cand_kf"] == 14
        got = ctx.loop_candidates(jobs, q, min_gap=0, strong=0.5, weak=0.4)
        assert [lc._result(w) for w in ref.candidates(jobs, q, min_gap=0, strong=0.5, weak=0.4)] == \
            [(g["status"], g["cand_kf"], lc.bits(g["best_sim"]), g["best_kf"], g["n_weak"], g["n_compared"]) for g in got]
        assert got[2]["cand_kf"] == 20
        for s in range(3):
            ids, rows = ctx.loopdb_read(s)
            rid, rrows = ref.read(s)
            assert ctx.loopdb_count(s) == counts[s] and np.array_equal(ids, rid) and np.array_equal(rows.view(np.uint32), rrows.view(np.uint32))
        assert ctx.loop_candidates([], np.zeros((0, 1280))) == []
        with pytest.raises(TypeError, match="unknown parameter"):
            ctx.loop_candidates(jobs, q, gap=3)
        with pytest.raises(RuntimeError, match="above the stream's last stored id"):
            ctx.loop_candidates([(0, 98)], q[:1])
        with pytest.raises(RuntimeError, match="BAD_VECTOR"):
            ctx.loopdb_append([1], [0], np.zeros((1, 1280)))
        assert ctx.loopdb_count(1) == 0
    finally:
        ctx.close()
