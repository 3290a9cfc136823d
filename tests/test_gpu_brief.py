"""svslam_brief_describe_batch on the device against tests/ref_brief.py on every case of brief_cases.py, exactly: n_desc, desc_pt and
every descriptor byte; the default table against the reference's generator; the refusals with the outputs untouched; two calls giving
the same bits; a job giving the same result alone and among others; Context.brief_describe; the timing family."""
import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import brief_cases as bc
import ref_brief as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(svs):
    """one context per image size, made when first asked for; which images its slots hold"""
    made = {}

    def get(size, kind):
        if size not in made:
            w, h = bc.SIZES[size]
            made[size] = [svs.Context(w, h, max_slots=bc.NSLOTS, max_jobs=bc.NSLOTS), None]
        ent = made[size]
        if ent[1] != kind:
            ent[0].pyramid(list(range(bc.NSLOTS)), list(bc.images(size, kind)))
            ent[1] = kind
        return ent[0]
    yield get
    for c, _ in made.values():
        c.close()


def test_slots_hold_the_images(contexts):
    ctx = contexts("96x72", "checker")
    for s, im in enumerate(bc.images("96x72", "checker")):
        assert np.array_equal(ctx.pyramid_read(s, 0), im)


def test_default_table_is_the_generated_one(contexts):
    assert np.array_equal(contexts("96x72", "random").brief_default_pattern(), rb.default_pattern())


@pytest.mark.parametrize("name", list(bc.CASES))
def test_against_the_reference(contexts, name):
    c = bc.case(name)
    ok, msg = bc.compare(c, bc.reference(name), bc.abi_call(c, ctx=contexts(c["size"], c["kind"])))
    print(name, msg)
    assert ok, msg


@pytest.mark.parametrize("name", list(bc.REFUSALS))
def test_refusals_write_nothing(contexts, name):
    c, words = bc.refusal_call(name)
    res = bc.abi_call(c, ctx=contexts(c["size"], c["kind"]))
    assert res[0] != 0 and words in res[1], res[:2]
    assert bc.untouched(res)


def test_the_accepted_side_of_each_refusal(contexts):
    ctx = contexts("96x72", "random")
    c, _ = bc.refusal_call("edge_16_default")
    for edge, good in ((17, True), (16, False)):
        assert (bc.abi_call(dict(c, edge=edge), ctx=ctx)[0] == 0) == good
    c, _ = bc.refusal_call("npts_1025")
    assert bc.abi_call(dict(c, jobs=[(0, 0, 1024)]), ctx=ctx)[0] == 0
    assert bc.abi_call(dict(c, jobs=[]), ctx=ctx)[0] == 0               # njobs == 0


def test_two_calls_same_bits_and_a_job_alone_or_among_others(contexts):
    c = bc.case("jobs_slots_gaps")
    ctx = contexts(c["size"], c["kind"])
    together = bc.abi_call(c, ctx=ctx)
    again = bc.abi_call(c, ctx=ctx)
    assert together[0] == 0 and together[2] == again[2] and np.array_equal(together[3], again[3]) and np.array_equal(together[4], again[4])
    for i, (slot, o, n) in enumerate(c["jobs"]):
        alone = bc.abi_call(dict(c, jobs=[(slot, 0, n)], xy=c["xy"][o:o + n]), ctx=ctx)
        k = together[2][i]
        assert alone[2] == [k] and np.array_equal(alone[3][:k], together[3][o:o + k]) and np.array_equal(alone[4][:k], together[4][o:o + k])


def test_the_kept_buffer_carries_nothing_over(svs):
    """on a fresh context: npts_1, npts_63, npts_1 again.  br_layout takes, rounded up to 16 each, 16 n + 8 n + 1024 (the table) +
    16 jobs + 4 n + 32 n: 1120 bytes for one point of one job (the context then keeps 1400) and 4832 for 63 points, more than
    1.25 * 1120 + 256 = 1656, so the second call replaces the buffer and the third runs in what the second left there.  The first and
    third results are the same bits, and the bits of the case on a context that has seen nothing else; every call is the reference's."""
    small, big = bc.case("npts_1"), bc.case("npts_63")
    assert small["size"] == big["size"] == "620x188" and small["kind"] == big["kind"]
    w, h = bc.SIZES["620x188"]
    a = gc.new_context(svs, w, h, max_slots=bc.NSLOTS, max_jobs=bc.NSLOTS)
    b = gc.new_context(svs, w, h, max_slots=bc.NSLOTS, max_jobs=bc.NSLOTS)
    try:
        for c in (a, b):
            c.pyramid(list(range(bc.NSLOTS)), list(bc.images("620x188", small["kind"])))
        first, second, third = bc.abi_call(small, ctx=a), bc.abi_call(big, ctx=a), bc.abi_call(small, ctx=a)
        alone = bc.abi_call(small, ctx=b)
    finally:
        a.close(); b.close(); gc.settle_rotation(svs)
    for c, name, res in ((small, "npts_1", first), (big, "npts_63", second), (small, "npts_1", third), (small, "npts_1", alone)):
        ok, msg = bc.compare(c, bc.reference(name), res)
        assert ok, (name, msg)
    assert first[2] == [1] and second[2][0] > 1
    for res in (third, alone):
        assert res[2] == first[2] and np.array_equal(res[3], first[3]) and np.array_equal(res[4], first[4])


def test_python_interface_and_timing_family(contexts):
    name = "jobs_slots_gaps"
    c = bc.case(name)
    ctx = contexts(c["size"], c["kind"])
    ctx.timing(True)
    shared = ctx.brief_describe(c["jobs"], c["xy"])
    ms, launches, units = ctx.timing_get("brief")
    ctx.timing(False)
    assert launches == 1 and units == len(c["xy"]) and ms > 0
    own = ctx.brief_describe([(slot, c["xy"][o:o + n]) for slot, o, n in c["jobs"]])
    for (d, p, k), (d2, p2, k2), (rd, rp) in zip(shared, own, bc.reference(name)):
        assert k == k2 == len(rp) and np.array_equal(d, rd) and np.array_equal(p, rp) and np.array_equal(d2, rd) and np.array_equal(p2, rp)
    assert ctx.brief_describe([]) == []
    with pytest.raises(RuntimeError, match="1024"):
        ctx.brief_describe([(0, np.full((1025, 2), 40.0))])
