"""csrc/k_brief.h itself, compiled for the host (tests/cpp/brief_host_emu, -ffp-contract=off), against tests/ref_brief.py over every case
of brief_cases.py, exactly: n_desc, desc_pt and every descriptor byte, and each refusal.  The filter, the compaction, the offsets, the
LDS layout, both blur passes, the tests and the packing are checked here without a device.  Not a replacement for
tests/test_gpu_brief.py: the compiler, the ISA, the barriers, LDS and the launches are not in it."""
import ctypes as C

import numpy as np
import pytest

import brief_cases as bc
import ref_brief as rb


@pytest.fixture(scope="module")
def emu(svs):
    return C.CDLL(svs._build.build_emu("brief"))


def test_default_table_is_the_generated_one(emu):
    out = np.zeros((256, 4), np.int8)
    emu.emu_brief_default_pattern(out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out, rb.default_pattern())


@pytest.mark.parametrize("name", list(bc.CASES))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    c = bc.case(name)
    ok, msg = bc.compare(c, bc.reference(name), bc.abi_call(c, emu=emu))
    print(name, msg)
    assert ok, msg


def test_cases_reach_what_they_are_for():
    nd = {n: [len(p) for _, p in bc.reference(n)] for n in bc.CASES}
    assert nd["no_interior_62x100"] == [0, 0]
    assert [p.tolist() for _, p in bc.reference("one_centre_63x63")] == [[0, 1, 4, 6]]
    assert nd["npts_0"] == [0] and nd["npts_1024"][0] > 800 and nd["npts_1024"][0] < 1024
    pt = bc.reference("every_second_dropped")[0][1]
    assert pt.tolist() == list(range(0, 150, 2))
    assert all(0 < k < 16 for k in nd["bounds_96x72"][:1])
    for n in ("step_edge", "checkerboard"):                         # ties and rounding decide bits there, and not all the same way
        d = np.concatenate([d for d, _ in bc.reference(n)])
        assert len(d) > 40 and 0 < np.unpackbits(d).mean() < 0.5


@pytest.mark.parametrize("name", list(bc.REFUSALS))
def test_refusals_write_nothing(emu, name):
    c, words = bc.refusal_call(name)
    res = bc.abi_call(c, emu=emu)
    assert res[0] != 0 and words in res[1], res[:2]
    assert bc.untouched(res)


def test_the_accepted_side_of_each_refusal(emu):
    c, _ = bc.refusal_call("edge_16_default")
    for edge, good in ((17, True), (16, False)):
        assert (bc.abi_call(dict(c, edge=edge), emu=emu)[0] == 0) == good
    c, _ = bc.refusal_call("npts_1025")
    assert bc.abi_call(dict(c, jobs=[(0, 0, 1024)]), emu=emu)[0] == 0
    c, _ = bc.refusal_call("overlap")
    assert bc.abi_call(dict(c, jobs=[(0, 0, 40), (1, 40, 40)]), emu=emu)[0] == 0
    assert bc.abi_call(dict(c, jobs=[]), emu=emu)[0] == 0              # njobs == 0


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    c = bc.case("jobs_slots_gaps")
    together = bc.abi_call(c, emu=emu)
    again = bc.abi_call(c, emu=emu)
    assert np.array_equal(together[3], again[3]) and np.array_equal(together[4], again[4]) and together[2] == again[2]
    for i, (slot, o, n) in enumerate(c["jobs"]):
        alone = bc.abi_call(dict(c, jobs=[(slot, 0, n)], xy=c["xy"][o:o + n]), emu=emu)
        k = together[2][i]
        assert alone[2] == [k] and np.array_equal(alone[3][:k], together[3][o:o + k]) and np.array_equal(alone[4][:k], together[4][o:o + k])


def test_non_finite_coordinates_are_dropped(emu):
    c = bc.case("angle_0")
    xy = np.array(c["xy"]); xy[3] = (np.nan, 40.0); xy[5] = (40.0, np.inf); xy[7] = (-np.inf, 40.0)
    res = bc.abi_call(dict(c, xy=xy), emu=emu)
    assert res[0] == 0 and not ({3, 5, 7} & set(res[4][:res[2][0]].tolist()))
