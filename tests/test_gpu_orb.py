"""svslam_orb_detect_batch on the device against tests/ref_orb.py on every case of orb_cases.py, bit for bit: the counts, every field of
every keypoint, every level and mask through the read hook; the refusals with the outputs untouched; a job alone, among others, twice,
split into chunks; 256 copies of one job in one call; Context.orb_detect; the timing family."""
import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import orb_cases as oc
import ref_orb

pytestmark = pytest.mark.gpu
NSLOTS = 6


@pytest.fixture(scope="module")
def contexts(svs):
    """one context per image size, made when first asked for; which case's images its slots hold"""
    made = {}

    def get(c, key):
        size = (c.w, c.h)
        if size not in made:
            made[size] = [gc.new_context(svs, c.w, c.h, max_slots=NSLOTS, max_jobs=NSLOTS), None]
        ent = made[size]
        if ent[1] != key:
            ent[0].pyramid(list(range(len(c.imgs))), list(c.imgs))
            ent[1] = key
        return ent[0]
    yield get
    for c, _ in made.values():
        c.close()


@pytest.mark.parametrize("name", list(oc.CASES))
def test_against_the_reference(contexts, name):
    c = oc.case(name)
    ctx = contexts(c, name)
    oc.compare_case(name, oc.run_case(c, ctx=ctx))
    for j, (_, info) in enumerate(oc.reference(name)):                 # levels and masks byte for byte
        for lv in range(len(info["levels"])):
            img, mask = ctx.orb_read_level(j, lv)
            assert np.array_equal(img, info["levels"][lv]), (name, j, lv)
            assert np.array_equal(mask, info["masks"][lv]), (name, j, lv)


@pytest.mark.parametrize("name", ["all_levels_300x230_n150", "jobs_slots_gaps", "max_out_truncates", "mask_everything"])
def test_context_orb_detect(contexts, name):
    c = oc.case(name)
    got = contexts(c, name).orb_detect(c.jobs, max_out=c.max_out, **c.prm)
    for (kps, n_found), (ref, _) in zip(got, oc.reference(name)):
        assert kps.dtype == ref_orb.KP
        oc.compare(kps, n_found, ref, c.max_out, name)


class _Two:
    """the two 160 x 120 images the refusal calls run on"""
    w, h = 160, 120
    imgs = [oc.blocks(160, 120, 1), oc.blocks(160, 120, 2)]


@pytest.mark.parametrize("name,changes,refused", oc.REFUSALS, ids=[r[0] for r in oc.REFUSALS])
def test_refusals_write_nothing_and_their_accepted_side_runs(contexts, name, changes, refused):
    ctx = contexts(_Two, "refusals")
    changes = dict(changes)
    if changes.get("slot") == 2:
        changes["slot"] = NSLOTS                      # the first slot this context does not have
    a = dict(oc.BASE_CALL, **changes)
    res = oc.refusal_call(changes, ctx=ctx)
    if refused:
        assert res[0] != 0 and res[1].startswith("orb: ") and oc.untouched(res), res[:3]
    else:
        assert res[0] == 0, res[1]
        assert res[2][0][0] == min(res[2][0][1], a["max_out"])


def test_no_jobs_is_a_valid_call(contexts):
    ctx = contexts(_Two, "refusals")
    rc, msg, counts, out = oc.abi_call(160, 120, None, [], np.zeros((0, 2), np.float32), 0, 10, dict(nfeatures=150), ctx=ctx)
    assert rc == 0 and np.all(out.view(np.uint8) == 0xC3)
    assert ctx.orb_detect([]) == []


def test_alone_batched_repeated_and_in_chunks(contexts, monkeypatch):
    c = oc.case("jobs_slots_gaps")
    ctx = contexts(c, "jobs_slots_gaps")
    together = oc.run_case(c, ctx=ctx)
    oc.compare_case("jobs_slots_gaps", together)
    again = oc.run_case(c, ctx=ctx)
    assert together[2] == again[2] and together[3].tobytes() == again[3].tobytes()
    imgs, jobs, rect = oc.pack(c)
    for j, job in enumerate(jobs):
        alone = oc.abi_call(c.w, c.h, imgs, [job], rect, len(rect), c.max_out, c.prm, ctx=ctx)
        assert alone[0] == 0 and alone[2][0] == together[2][j] and alone[3][0].tobytes() == together[3][j].tobytes(), j
    monkeypatch.setenv("SVSLAM_ORB_BUDGET_MB", "1")               # a few jobs per chunk: the five jobs take more than one
    split = oc.run_case(c, ctx=ctx)
    assert split[2] == together[2] and split[3].tobytes() == together[3].tobytes()
    with pytest.raises(RuntimeError, match="last chunk"):         # job 0 left with the first chunk
        ctx.orb_read_level(0, 1)
    img, mask = ctx.orb_read_level(4, 1)
    info = oc.reference("jobs_slots_gaps")[4][1]
    assert np.array_equal(img, info["levels"][1]) and np.array_equal(mask, info["masks"][1])


def test_256_copies_of_one_job_in_one_call(contexts, svs):
    c = oc.case("mask_corners")
    ctx = contexts(c, "mask_corners")
    ref = oc.reference("mask_corners")[0][0]
    ctx.timing(True)
    got = ctx.orb_detect([c.jobs[0]] * 256, max_out=c.max_out, **c.prm)
    t = ctx.timing_get("orb")
    ctx.timing(False)
    assert len(got) == 256
    for kps, n_found in got:
        assert n_found == len(ref) and kps.tobytes() == ref.tobytes()
    assert svs.ORB_FAMILIES == {"orb": 20} and sorted(svs.FAMILIES.values()) == [0, 1, 2, 3, 4, 5]      # what bench.py sums over has nothing new
    assert "k_orb_fast" in svs.FAMILY_KERNELS["orb"]
    assert t[0] > 0 and t[2] >= 256, t


def test_leave_the_stream_rotation_as_it_was(svs):
    assert 0 <= gc.settle_rotation(svs) < gc.ROTATION
