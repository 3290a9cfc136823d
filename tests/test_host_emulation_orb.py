"""csrc/k_orb.h itself, compiled for the host (tests/cpp/orb_host_emu, -ffp-contract=off), against tests/ref_orb.py over every case of
orb_cases.py, bit for bit: counts, every field of every keypoint, every level and mask, and each refusal.  The plan, the resize
tables, the kernels' bodies with their scans, histograms and compactions are checked here without a device.  Not a replacement for
tests/test_gpu_orb.py: the compiler, the ISA, the barriers, LDS, the atomics and the launches are not in it."""
import ctypes as C

import numpy as np
import pytest

import orb_cases as oc
import ref_orb


@pytest.fixture(scope="module")
def emu(svs):
    return C.CDLL(svs._build.build_emu("orb"))


def read_level(emu, job, level):
    w, h = C.c_int(0), C.c_int(0)
    assert emu.emu_orb_read_level(job, level, None, None, C.byref(w), C.byref(h)) == 0
    img = np.zeros((h.value, w.value), np.uint8); mask = np.zeros((h.value, w.value), np.uint8)
    assert emu.emu_orb_read_level(job, level, img.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h)) == 0
    return img, mask


@pytest.mark.parametrize("name", list(oc.CASES))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    oc.compare_case(name, oc.run_case(oc.case(name), emu=emu))
    for j, (_, info) in enumerate(oc.reference(name)):                 # levels and masks byte for byte
        for lv in range(len(info["levels"])):
            img, mask = read_level(emu, j, lv)
            assert np.array_equal(img, info["levels"][lv]), (name, j, lv)
            assert np.array_equal(mask, info["masks"][lv]), (name, j, lv)


def test_cases_reach_what_they_are_for():
    def per_level(name, job=0):
        return [s["after_cut2"] for s in oc.reference(name)[job][1]["per_level"]]
    for n in ("all_levels_300x230_n150", "all_levels_300x230_n500"):
        info = oc.reference(n)[0][1]
        assert info["geometry"][7][1:] == (84, 64) and all(k > 0 for k in per_level(n)), per_level(n)
    assert all(k > 0 for k in per_level("four_levels_160x120")[:4]) and per_level("four_levels_160x120")[4:] == [0, 0, 0, 0]
    assert len(oc.reference("odd_161x121")[0][0]) > 40
    assert len(oc.reference("no_interior_62x100")[0][0]) == 0
    one = oc.reference("one_interior_63x63")[0][0]
    assert len(one) == 1 and (one["x"][0], one["y"][0], one["octave"][0]) == (31.0, 31.0, 0)
    assert len(oc.reference("flat")[0][0]) == 0
    # ties: more than 2 n_L through the first cut and more than n_L through the second, on level 0 of the squares
    st = oc.reference("checkerboard")[0][1]["per_level"][0]
    assert st["after_cut1"] > 2 * st["quota"] and st["after_cut2"] > st["quota"]
    assert len(oc.reference("checkerboard")[0][0]) > 150
    assert oc.reference("nfeatures_1")[0][1]["quotas"] == [0, 0, 0, 0, 0, 0, 0, 1]
    assert oc.reference("nfeatures_5")[0][1]["quotas"] == [1, 1, 1, 1, 1, 0, 0, 0] and per_level("nfeatures_5")[:4] == [1, 1, 1, 1]
    assert len(per_level("nlevels_1")) == 1 and len(per_level("nlevels_3")) == 3 and min(per_level("nlevels_3")) > 0
    assert len(oc.reference("fast_threshold_1")[0][0]) > len(oc.reference("four_levels_160x120")[0][0])
    assert len(oc.reference("fast_threshold_254")[0][0]) == 0
    assert all(k > 0 for k in per_level("edge_16"))                      # with edge 16 every level of 160 x 120 has an interior
    plain = oc.reference("four_levels_160x120")[0][0]
    for n in ("mask_corners", "mask_between_pixels"):            # the rects take keypoints away
        assert 0 < len(oc.reference(n)[0][0]) < len(plain)
    mc = oc.reference("mask_corners")[0][1]["masks"][0]
    assert mc[0, 0] == 0 and mc[10, 10] == 0 and mc[11, 11] == 255 and mc[119, 159] == 0 and mc[60, 80] == 0
    m0 = oc.reference("mask_outside")[0][1]["masks"][0]
    assert m0[60, 0] == 0 and m0[60, 6] == 255 and m0[0, 80] == 0 and m0[1, 80] == 255 and m0[119, 159] == 0 and m0[0, 0] == 255
    c = oc.case("mask_between_pixels")
    assert oc.between_pixels_shows(c.imgs[0], c.jobs[0][1])
    assert len(oc.reference("mask_everything")[0][0]) == 0 and not oc.reference("mask_everything")[0][1]["masks"][0].any()
    counts = [len(k) for k, _ in oc.reference("jobs_slots_gaps")]
    assert len(counts) == 5 and min(counts) > 0 and len(set(counts)) > 2
    assert len(oc.reference("max_out_truncates")[0][0]) > oc.case("max_out_truncates").max_out


@pytest.mark.parametrize("name,changes,refused", oc.REFUSALS, ids=[r[0] for r in oc.REFUSALS])
def test_refusals_write_nothing_and_their_accepted_side_runs(emu, name, changes, refused):
    res = oc.refusal_call(changes, emu=emu)
    a = dict(oc.BASE_CALL, **changes)
    want = ref_orb.refusal(160, 120, 2, [(a["slot"], a["rect_ofs"], a["nrect"])], a["total_rects"], a["max_out"],
                           **{k: a[k] for k in ref_orb.DEFAULTS})
    assert (want is not None) == refused
    if refused:
        assert res[0] != 0 and res[1] and oc.untouched(res), res[:3]
    else:
        assert res[0] == 0, res[1]
        assert res[2][0][0] == min(res[2][0][1], a["max_out"])


def test_no_jobs_is_a_valid_call(emu):
    rc, msg, counts, out = oc.abi_call(160, 120, np.zeros((1, 120, 160), np.uint8), [], np.zeros((0, 2), np.float32), 0, 10, dict(nfeatures=150), emu=emu)
    assert rc == 0 and np.all(out.view(np.uint8) == 0xC3)


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    c = oc.case("jobs_slots_gaps")
    together = oc.run_case(c, emu=emu)
    again = oc.run_case(c, emu=emu)
    assert together[2] == again[2] and together[3].tobytes() == again[3].tobytes()                 # repeatable
    imgs, jobs, rect = oc.pack(c)
    for j, job in enumerate(jobs):
        alone = oc.abi_call(c.w, c.h, imgs, [job], rect, len(rect), c.max_out, c.prm, emu=emu)
        assert alone[0] == 0 and alone[2][0] == together[2][j] and alone[3][0].tobytes() == together[3][j].tobytes(), j
    # split into chunks of one and two jobs by a small byte budget: the same bits
    for budget in (1, 700000):
        split = oc.run_case(c, emu=emu, budget=budget)
        assert split[2] == together[2] and split[3].tobytes() == together[3].tobytes()


def test_the_plan_splits_a_large_call_under_the_budget(emu):
    lw, lh, q = (C.c_int * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    P = oc._Prm(150, 0, 0, 0)
    one = emu.emu_orb_plan(620, 188, 4096, C.byref(P), 150, C.c_longlong(1 << 40), lw, lh, q)
    many = emu.emu_orb_plan(620, 188, 4096, C.byref(P), 150, C.c_longlong(1 << 30), lw, lh, q)
    assert one == 1 and 2 <= many <= 16
    geo = ref_orb.level_geometry(620, 188, 8)
    assert [(lw[i], lh[i]) for i in range(8)] == [g[1:] for g in geo] and list(q) == ref_orb.quotas(150, 8)


def test_umax_table_is_what_its_rule_gives(emu):
    table, rule = (C.c_int * 16)(), (C.c_int * 16)()
    emu.emu_orb_umax(table, rule)
    assert list(table) == list(rule) == ref_orb.umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_atan_deg_against_the_numpy_restatement(emu):
    r = np.random.RandomState(4)
    big = r.randint(-2800000, 2800001, (4000, 2)).astype(np.float32)
    small = r.randint(-6, 7, (600, 2)).astype(np.float32)
    axes = np.array([[0, 0], [0, 1], [0, -1], [1, 0], [-1, 0], [1, 1], [-1, 1], [1, -1], [-1, -1], [5, 5], [-5, 5], [2711925, 1],
                     [1, 2711925], [-2711925, -1], [-1, -2711925], [3, -3]], np.float32)
    yx = np.ascontiguousarray(np.concatenate([axes, small, big]))
    y, x = np.ascontiguousarray(yx[:, 0]), np.ascontiguousarray(yx[:, 1])
    out = np.zeros(len(y), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    emu.emu_orb_atan_deg(len(y), p(y), p(x), p(out))
    want = ref_orb.atan_deg(y, x)
    assert out.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert out[0] == 0.0 and np.all((out >= 0) & (out <= 360))
    # rows are (y, x): (1, 0) is 90 degrees, (-1, 0) 270, (0, -1) 180, (1, 1) 45; the polynomial is good to about 0.01 degree
    assert abs(out[3] - 90) < 0.02 and abs(out[4] - 270) < 0.02 and abs(out[2] - 180) < 0.02 and abs(out[5] - 45) < 0.02
