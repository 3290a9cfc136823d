"""svslam_orb_describe_batch on the device against tests/ref_orb_desc.py on every case of orb_desc_cases.py, exactly: n_desc, desc_pt and
every descriptor byte; alone, batched, repeated, split into chunks and as 256 copies of one job; the refusals with the outputs
untouched and their accepted neighbours; the rows of angle -1 / octave 0 against svslam_brief_describe_batch on the device;
Context.orb_describe; the timing family."""
import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import orb_desc_cases as dc
import ref_orb_desc as rod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(svs):
    """one context per image size, made when first asked for; which images its slots hold"""
    made = {}

    def get(size, kind="random"):
        if size not in made:
            w, h = dc.SIZES[size]
            made[size] = [gc.new_context(svs, w, h, max_slots=dc.NSLOTS, max_jobs=dc.NSLOTS), None]
        ent = made[size]
        if ent[1] != kind:
            ent[0].pyramid(list(range(dc.NSLOTS)), list(dc.images(size, kind)))
            ent[1] = kind
        return ent[0]
    yield get
    for c, _ in made.values():
        c.close()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_against_the_reference(contexts, name):
    c = dc.case(name)
    ok, msg = dc.compare(c, dc.reference(name), dc.abi_call(c, ctx=contexts(c["size"], c["kind"])))
    print(name, msg)
    assert ok, msg


@pytest.mark.parametrize("name", list(dc.REFUSALS))
def test_refusals_write_nothing(contexts, name):
    change, words = dc.REFUSALS[name]
    res = dc.abi_call(dc.changed_call(change), ctx=contexts("160x120"))
    assert res[0] != 0 and words in res[1], res[:2]
    assert dc.untouched(res)


@pytest.mark.parametrize("name", list(dc.ACCEPTED))
def test_the_accepted_neighbour_of_each_refusal(contexts, name):
    c = dc.changed_call(dc.ACCEPTED[name])
    ims = dc.images("160x120")
    ref = tuple(rod.describe(ims[slot], c["kps"][o:o + n], c["pattern"], c["edge"], c["nlevels"]) for slot, o, n in c["jobs"])
    ok, msg = dc.compare(c, ref, dc.abi_call(c, ctx=contexts("160x120")))
    assert ok, msg


def test_no_jobs_and_no_points_are_valid_calls(contexts):
    ctx = contexts("160x120")
    res = dc.abi_call(dc.changed_call(dict(jobs=[])), ctx=ctx)
    assert res[0] == 0 and dc.untouched(res)
    res = dc.abi_call(dc.changed_call(dict(jobs=[(0, 0, 0), (1, 40, 0)])), ctx=ctx)
    assert res[0] == 0 and res[2] == [0, 0] and (res[3] == dc.FILL_DESC).all()


def test_two_calls_same_bits_a_job_alone_or_among_others_and_in_chunks(contexts):
    name = "jobs_slots_gaps"
    c = dc.case(name)
    ctx = contexts(c["size"], c["kind"])
    together = dc.abi_call(c, ctx=ctx)
    again = dc.abi_call(c, ctx=ctx)
    assert together[0] == 0 and together[2] == again[2] and np.array_equal(together[3], again[3]) and np.array_equal(together[4], again[4])
    for i, (slot, o, n) in enumerate(c["jobs"]):
        alone = dc.abi_call(dict(c, jobs=[(slot, 0, n)], kps=c["kps"][o:o + n]), ctx=ctx)
        k = together[2][i]
        assert alone[2] == [k] and np.array_equal(alone[3][:k], together[3][o:o + k]) and np.array_equal(alone[4][:k], together[4][o:o + k])
    # 1 MB holds levels 1 .. 6 of two jobs of 620 x 188 (about 0.3 MB each) and not of all five: the call runs in chunks
    split = dc.abi_call(c, ctx=ctx, budget=1)
    ok, msg = dc.compare(c, dc.reference(name), split)
    assert ok, msg
    assert np.array_equal(split[3], together[3]) and np.array_equal(split[4], together[4])


def test_256_copies_of_one_job(contexts):
    ctx = contexts("160x120")
    one = dc.kps(dc.mixed_points(70, "160x120", 40, 3))
    ref = rod.describe(dc.images("160x120")[2], one)
    assert 10 < len(ref[1]) < 40
    c = dict(size="160x120", kind="random", jobs=[(2, 40 * i, 40) for i in range(256)], kps=np.tile(one, 256), pattern=None, edge=0, nlevels=0)
    ok, msg = dc.compare(c, (ref,) * 256, dc.abi_call(c, ctx=ctx))
    assert ok, msg


def test_minus_one_degree_on_level_0_is_the_plain_brief_row(contexts):
    """the contract's property, on the device: default table, every point at angle -1, octave 0 -> the rows of
    svslam_brief_describe_batch(angle_deg = -1), bit for bit"""
    for size, n in (("620x188", 150), ("160x120", 40), ("63x63", 7)):
        ctx = contexts(size)
        k = dc.kps(dc.tracked_points(80, size, n) + ([(31.5, 31.5, -1.0, 0), (31.99, 31.0, -1.0, 0)] if size == "63x63" else []))
        jobs = [(s, k) for s in range(dc.NSLOTS)]
        plain = ctx.brief_describe([(s, np.stack([k["x"], k["y"]], axis=1)) for s in range(dc.NSLOTS)], angle_deg=-1.0)
        oriented = ctx.orb_describe(jobs)
        assert sum(p[2] for p in plain) > 0
        for (d, p, m), (d2, p2, m2) in zip(plain, oriented):
            assert m == m2 and np.array_equal(p, p2) and np.array_equal(d, d2)


def test_python_interface_and_timing_family(contexts):
    name = "jobs_slots_gaps"
    c = dc.case(name)
    ctx = contexts(c["size"], c["kind"])
    ctx.timing(True)
    out = ctx.orb_describe([(slot, c["kps"][o:o + n]) for slot, o, n in c["jobs"]])
    ms, launches, units = ctx.timing_get("orb_desc")
    ctx.timing(False)
    assert launches == 1 and units == sum(n for _, _, n in c["jobs"]) and ms > 0
    rows = ctx.orb_describe([(slot, [(k["x"], k["y"], k["angle"], k["octave"]) for k in c["kps"][o:o + n]]) for slot, o, n in c["jobs"]])
    for (d, p, k), (d2, p2, k2), (rd, rp) in zip(out, rows, dc.reference(name)):
        assert k == k2 == len(rp) and np.array_equal(d, rd) and np.array_equal(p, rp) and np.array_equal(d2, rd) and np.array_equal(p2, rp)
    assert ctx.orb_describe([]) == []
    with pytest.raises(RuntimeError, match="1024"):
        ctx.orb_describe([(0, np.zeros(1025, dc.KP))])


def test_leave_the_stream_rotation_as_it_was(svs, contexts):
    assert 0 <= gc.settle_rotation(svs) < gc.ROTATION
