"""csrc/k_orb_desc.h itself, compiled for the host (tests/cpp/orb_desc_host_emu, -ffp-contract=off), against tests/ref_orb_desc.py over
every case of orb_desc_cases.py, bit for bit: n_desc, desc_pt, every descriptor byte, and each refusal with its accepted neighbour.
The plan, the levels, the filter's compaction and the describe kernel's phases are checked here without a device.  Not a replacement
for tests/test_gpu_orb_desc.py: the compiler, the ISA, the barriers, LDS and the launches are not in it."""
import ctypes as C

import numpy as np
import pytest

import orb_desc_cases as dc
import ref_orb_desc as rod


@pytest.fixture(scope="module")
def emu(svs):
    return C.CDLL(svs._build.build_emu("orb_desc"))


@pytest.mark.parametrize("name", list(dc.CASES))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    c = dc.case(name)
    ok, msg = dc.compare(c, dc.reference(name), dc.abi_call(c, emu=emu))
    assert ok, msg


def test_cases_reach_what_they_are_for():
    from collections import Counter
    g = dc.geometry("160x120")
    assert g[3][1:] == (93, 69) and g[4][1:] == (77, 58)
    lv = Counter(dc.kept_levels("levels_160x120"))
    assert all(lv[k] > 0 for k in range(4)) and lv[4] == 0 and lv[5] == 0
    assert (dc.case("levels_160x120")["kps"]["octave"] == 4).sum() == 12
    g = dc.geometry("300x240")
    assert g[7][1:] == (84, 67)
    lv = Counter(dc.kept_levels("all_levels_300x240"))
    assert all(lv[k] > 0 for k in range(8)), lv
    g = dc.geometry("620x188")
    assert g[6][1:] == (208, 63) and g[7][2] <= 62
    lv = Counter(dc.kept_levels("one_row_620x188"))
    assert lv[6] > 0 and lv[7] == 0 and lv[5] > 0
    # level-0 border: of the four values per axis exactly the two inner ones pass at octave 0; at octave 1 those centres are outside
    # the level's interior
    d, p = dc.reference("level0_border")[0]
    assert len(p) == 4 and (dc.case("level0_border")["kps"]["octave"][p] == 0).all()
    # level-L border: cx = 30 and w_L - 31 fail, 31 and w_L - 32 pass, in x and y: 4 of 16 on levels 1 and 2; level 7 of 300 x 240 too
    k = dc.case("level_border")["kps"]
    _, p = dc.reference("level_border")[0]
    assert Counter(k["octave"][p].tolist()) == {1: 4, 2: 4, 7: 4}
    assert len(dc.reference("half_integer_centres")[0][1]) == len(dc.case("half_integer_centres")["kps"])
    assert len(dc.reference("angle_sweep")[0][1]) == 368
    # the rotation matters: the same centre at two angles gives different rows
    d, p = dc.reference("angles")[0]
    assert len(p) == 16 and len({r.tobytes() for r in d}) == 16
    lv = Counter(dc.kept_levels("tracked_and_detected"))
    assert len(lv) == 6
    counts = [len(p) for _, p in dc.reference("jobs_slots_gaps")]
    assert len(counts) == 5 and counts[2] == 0 and min(counts[:2] + counts[3:]) > 0
    for n in ("step_edge", "checkerboard"):
        rows = np.concatenate([d for d, _ in dc.reference(n)])
        assert len(rows) > 60 and 0 < np.unpackbits(rows).mean() < 0.5          # ties of the strict < leave zeros
    assert set(dc.kept_levels("all_octave_0")) == {0}
    assert [len(p) for _, p in dc.reference("not_finite_coordinates")] == [1]
    for n in dc.NPTS:
        assert sum(len(p) for _, p in dc.reference("npts_%d" % n)) > (0 if n < 3 else n // 3) or n == 0


def test_one_centre_rows_are_the_expected_points():
    _, p = dc.reference("one_centre_63x63")[0]
    # (30.99, 31) fails in x, (31, 32) in y; (31.5, 31.5) and (31.99, 31.99) pass the float test and have their centre at 32, as in
    # svslam_brief_describe_batch; the octave-1 point's level (52 x 52) has no interior
    assert p.tolist() == [0, 1, 4, 6], p.tolist()


@pytest.mark.parametrize("name", list(dc.REFUSALS))
def test_refusals_write_nothing(emu, name):
    change, words = dc.REFUSALS[name]
    c = dc.changed_call(change)
    res = dc.abi_call(c, emu=emu)
    assert res[0] != 0 and words in res[1], res[:2]
    assert dc.untouched(res)
    if "jobs" not in change:                                                   # the reference refuses what one job can show
        with pytest.raises(ValueError, match=words):
            half = change["point"][0] // 40 if "point" in change else 0
            rod.describe(dc.images("160x120")[half], c["kps"][40 * half:40 * half + 40], c["pattern"], c["edge"], c["nlevels"])


@pytest.mark.parametrize("name", list(dc.ACCEPTED))
def test_the_accepted_neighbour_of_each_refusal(emu, name):
    c = dc.changed_call(dc.ACCEPTED[name])
    ims = dc.images("160x120")
    ref = tuple(rod.describe(ims[slot], c["kps"][o:o + n], c["pattern"], c["edge"], c["nlevels"]) for slot, o, n in c["jobs"])
    ok, msg = dc.compare(c, ref, dc.abi_call(c, emu=emu))
    assert ok, msg


def test_no_jobs_and_no_points_are_valid_calls(emu):
    c = dc.changed_call(dict(jobs=[]))
    res = dc.abi_call(c, emu=emu)
    assert res[0] == 0 and dc.untouched(res)
    res = dc.abi_call(dict(c, kps=np.zeros(0, dc.KP)), emu=emu)
    assert res[0] == 0
    c = dc.changed_call(dict(jobs=[(0, 0, 0), (1, 40, 0)]))
    res = dc.abi_call(c, emu=emu)
    assert res[0] == 0 and res[2] == [0, 0] and (res[3] == dc.FILL_DESC).all()


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    c = dc.case("jobs_slots_gaps")
    together = dc.abi_call(c, emu=emu)
    again = dc.abi_call(c, emu=emu)
    assert together[0] == 0 and together[2] == again[2] and np.array_equal(together[3], again[3]) and np.array_equal(together[4], again[4])
    for i, (slot, o, n) in enumerate(c["jobs"]):
        alone = dc.abi_call(dict(c, jobs=[(slot, 0, n)], kps=c["kps"][o:o + n]), emu=emu)
        k = together[2][i]
        assert alone[2] == [k] and np.array_equal(alone[3][:k], together[3][o:o + k]) and np.array_equal(alone[4][:k], together[4][o:o + k])


def test_a_small_budget_splits_the_call_into_chunks_with_the_same_bits(emu):
    c = dc.case("jobs_slots_gaps")
    whole = dc.abi_call(c, emu=emu)
    assert dc.emu_stats(emu)["chunks"] == 1
    seen = set()
    for budget in (1, 700000, 1100000):
        split = dc.abi_call(c, emu=emu, budget=budget)
        seen.add(dc.emu_stats(emu)["chunks"])
        ok, msg = dc.compare(c, dc.reference("jobs_slots_gaps"), split)
        assert ok, (budget, msg)
        assert split[2] == whole[2] and np.array_equal(split[3], whole[3]) and np.array_equal(split[4], whole[4])
    assert 5 in seen and len(seen) >= 2, seen                                  # budget 1: a chunk per job


def test_a_call_of_octave_0_builds_no_level(emu):
    c = dc.case("all_octave_0")
    assert dc.abi_call(c, emu=emu)[0] == 0
    st = dc.emu_stats(emu)
    assert st["resizes"] == 0 and st["level_bytes"] == 0 and st["reach"] == 19
    c = dc.case("levels_160x120")                                              # octaves up to 5: five launches, levels 1 .. 5 stored
    assert dc.abi_call(c, emu=emu)[0] == 0
    st = dc.emu_stats(emu)
    g = dc.geometry("160x120")
    assert st["resizes"] == 5 and st["level_bytes"] >= sum(g[l][1] * g[l][2] for l in range(1, 6))
    assert dc.abi_call(dc.case("reach22_edge26"), emu=emu)[0] == 0 and dc.emu_stats(emu)["reach"] == 22


def test_the_host_rotation_is_the_references(emu):
    ab = (C.c_float * 2)()
    for a in list(dc.ANGLES) + np.random.default_rng(1).uniform(-720, 720, 500).tolist():
        emu.emu_orb_desc_rotation(C.c_float(a), ab)
        want = rod.rotation(a)
        assert (np.float32(ab[0]), np.float32(ab[1])) == want, a


def test_minus_one_degree_on_level_0_is_the_plain_brief_row(emu, svs):
    """the property the contract states: default table, every point at angle -1, octave 0 -> svslam_brief_describe_batch(-1)'s rows"""
    import brief_cases as bc
    bemu = C.CDLL(svs._build.build_emu("brief"))
    for name in ("jobs_slots_gaps", "bounds_620x188", "checkerboard", "one_centre_63x63"):
        b = bc.case(name)
        want = bc.abi_call(b, emu=bemu)
        assert want[0] == 0
        k = np.zeros(len(b["xy"]), dc.KP)
        k["x"], k["y"], k["angle"] = b["xy"][:, 0], b["xy"][:, 1], -1.0
        w, h = bc.SIZES[b["size"]]
        ims = np.ascontiguousarray(np.stack(bc.images(b["size"], b["kind"])))
        arr = (dc.Job * len(b["jobs"]))()
        for i, (slot, o, n) in enumerate(b["jobs"]):
            arr[i].slot, arr[i].pt_ofs, arr[i].npts = slot, o, n
        P = dc.Params(None, 0, 0, 0)
        desc = np.full((len(k), 32), bc.FILL_DESC, np.uint8); dpt = np.full(len(k), bc.FILL_PT, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = emu.emu_orb_desc_describe(w, h, bc.NSLOTS, ptr(ims), len(arr), arr, C.byref(P), len(k), ptr(k), ptr(desc), ptr(dpt), C.c_longlong(0))
        assert rc == 0 and [a.n_desc for a in arr] == want[2] and np.array_equal(desc, want[3]) and np.array_equal(dpt, want[4]), name
