"""CPU: the plain map model of tests/ref_dmap.py on maps small enough to check by eye, and every generated case of
tests/dmap_cases.py against the preconditions the kernels of csrc/k_dmap.h take for granted (a case that breaks one tests
nothing on the GPU, so it fails here)."""
import ctypes as C

import numpy as np
import pytest

import dmap_cases as dc
import ref_dmap as rd


def tiny():
    """3 keyframe slots x 4 features, 4 landmark slots.
    slot 0: keyframe 7 (features a0 a1 a2), slot 1: empty, slot 2: keyframe 3 (features b0 b1).
    landmark slot 0: id 9, slot 1: id 2, slot 2: free, slot 3: id 5 (outside the window).
      a0: left -> id 9, right -> id 9      a1: right -> id 2       a2: left -> id 5
      b0: left -> id 2, right -> id 2      b1: left -> id 9"""
    s = dict(kf_frame=np.array([70, -1, 30], np.int64), kf_id=np.array([7, 0, 3], np.int32), kf_pose=np.zeros((3, 7)), kf_n=np.array([3, 0, 2], np.int32),
             f_xy=np.arange(24, dtype=np.float32).reshape(3, 4, 2), f_xyr=100 + np.arange(24, dtype=np.float32).reshape(3, 4, 2),
             f_lm=np.array([[0, -1, 3, -1], [-1] * 4, [1, 0, -1, -1]], np.int32), f_lmr=np.array([[0, 1, -1, -1], [-1] * 4, [1, -1, -1, -1]], np.int32),
             f_fl=np.array([[1, 1, 0, 0], [0] * 4, [1, 0, 0, 0]], np.uint8), lm_pos=np.arange(12, dtype=np.float64).reshape(4, 3),
             lm_id=np.array([9, 2, -1, 5], np.int32), lm_obs=np.array([3, 3, 0, 1], np.int32), lm_state=np.array([1, 1, 0, 2], np.uint8),
             lm_stamp=np.array([1, 1, -1, 0], np.int32), next_lm_id=np.array([10], np.int32))
    s["kf_pose"][:, 3] = 1
    return s


def test_round_trip_and_observation_order():
    s = tiny()
    m = rd.MapModel.from_state(s)
    for k, v in m.to_state(s).items():
        assert np.array_equal(v, s[k]), k
    # chronological: keyframe 3 before keyframe 7, left before right
    assert [(o[0], o[1]) for o in m.lms[9].obs] == [(3, 0), (7, 0), (7, 1)]
    assert [(o[0], o[1]) for o in m.lms[2].obs] == [(3, 0), (3, 1), (7, 1)]
    assert [(o[0], o[1]) for o in m.lms[5].obs] == [(7, 0)]


def test_problem_of_optimize_by_hand():
    m = rd.MapModel.from_state(tiny())
    p = m.ba_problem(2, 6)
    assert [kf.kf_id for kf in p["kfs"]] == [3, 7] and [kf.slot for kf in p["kfs"]] == [2, 0]
    assert [lm.id for lm in p["verts"]] == [2, 9]                # id order; id 5 is outside the window: no vertex, its feature no edge
    got = [(e["v"], e["a"], e["right"], e["kf_slot"], e["feat"], tuple(float(x) for x in e["uv"])) for e in p["edges"]]
    assert got == [(0, 0, 0, 2, 0, (16.0, 17.0)), (0, 0, 1, 2, 0, (116.0, 117.0)), (0, 1, 1, 0, 1, (102.0, 103.0)),
                   (1, 0, 0, 2, 1, (18.0, 19.0)), (1, 1, 0, 0, 0, (0.0, 1.0)), (1, 1, 1, 0, 0, (100.0, 101.0))]
    assert not p["skipped"] and m.ba_problem(2, 5)["skipped"] and m.ba_problem(1, 6)["skipped"]


def test_threshold_loop_and_removal_by_hand():
    s = tiny()
    m = rd.MapModel.from_state(s)
    p = m.ba_problem(2, 6)
    # th 5.991: 4 of 6 outliers -> doubled once (11.982): 2 outliers (> is strict: 11.982 itself stays)
    chi2 = [1.0, 6.0, 2 * 5.991, 1.0, 50.0, 70.0]
    outs = m.ba_apply(dict(dead=0, kf_slot=0), p, chi2, [[0, 0, 0, 1, 1, 2, 3], [0, 0, 0, 1, 4, 5, 6]], [[1, 1, 1], [2, 2, 2]], 4, 5.991, 11, 12)
    assert outs["ba_iters"] == 4 and outs["pose"] == [0, 0, 0, 1, 4, 5, 6] and (outs["ba_npair"], outs["ba_ntrial"]) == (11, 12)
    t = m.to_state(s)
    assert t["f_lm"][0].tolist() == [-1, -1, 3, -1] and t["f_lmr"][0].tolist() == [-1, 1, -1, -1]     # both edges of a0 gone
    assert t["lm_obs"].tolist() == [1, 3, 0, 1] and t["lm_state"].tolist() == [1, 1, 0, 2]
    assert t["lm_pos"][1].tolist() == [1, 1, 1] and t["lm_pos"][0].tolist() == [2, 2, 2] and t["lm_pos"][3].tolist() == [9, 10, 11]
    assert t["kf_pose"][2].tolist() == [0, 0, 0, 1, 1, 2, 3]
    # exactly half outliers doubles; five doublings at the most; a failed solve applies nothing
    m = rd.MapModel.from_state(s)
    m.ba_apply(dict(dead=0, kf_slot=0), m.ba_problem(2, 6), [1, 1, 1, 7, 7, 100], [[0] * 7] * 2, [[0] * 3] * 2, 1, 5.991)
    assert m.to_state(s)["lm_obs"].tolist() == [2, 3, 0, 1]
    m = rd.MapModel.from_state(s)
    m.ba_apply(dict(dead=0, kf_slot=0), m.ba_problem(2, 6), [32 * 5.991] * 3 + [32 * 5.991 * 1.01] * 3, [[0] * 7] * 2, [[0] * 3] * 2, 1, 5.991)
    assert m.to_state(s)["lm_obs"].tolist() == [0, 3, 0, 1] and m.lms[9].active
    m = rd.MapModel.from_state(s)
    assert m.ba_apply(dict(dead=0, kf_slot=0), m.ba_problem(2, 6), [100.0] * 6, None, None, -1, 5.991) == dict(ba_iters=-1)


def test_begin_by_hand():
    s = tiny()
    m = rd.MapModel.from_state(s)
    job = dict(is_init=0, kf_slot=1, remove_slot=2, kf_id=8, frame_id=80, pose=[0, 0, 0, 1, 0, 0, 0], npts=2, stamp=6)
    outs, cands = m.begin(job, np.array([[1, 2], [3, 4]], np.float32), [3, -1])
    # keyframe 3 retires: id 9 keeps 2 observations, id 2 keeps 1; the tracked list names id 5: observed again and stamped
    t = m.to_state(s)
    assert t["kf_frame"].tolist() == [70, 80, -1] and t["kf_n"].tolist() == [3, 2, 2]
    assert t["lm_obs"].tolist() == [2, 1, 0, 2] and t["lm_stamp"].tolist() == [1, 1, -1, 6] and t["lm_state"].tolist() == [1, 1, 0, 2]
    assert t["f_lm"][1, :2].tolist() == [3, -1] and cands == [] and outs["ok"] == 1 and outs["n_features"] == 2
    # retire keyframe 7 instead, carry nothing: id 5 loses its only observation, was outside the window already -> candidate;
    # with the step's stamp it would stay
    m = rd.MapModel.from_state(s)
    outs, cands = m.begin(dict(job, remove_slot=0, npts=0), np.zeros((0, 2), np.float32), [])
    assert cands == [5]
    after = m.to_state(s); after["lm_id"][3] = -1; after["lm_state"][3] = 0
    assert m.check_eviction(cands, 1, [(5, 9.0, 10.0, 11.0)], after) == {5}
    assert m.to_state(s)["lm_id"].tolist() == [9, 2, -1, -1]
    with pytest.raises(AssertionError):
        rd.MapModel.from_state(s).check_eviction([5], 1, [], after)            # a candidate and room for it: it must go
    m = rd.MapModel.from_state(s)
    assert m.begin(dict(job, remove_slot=0, npts=0, stamp=0), np.zeros((0, 2), np.float32), [])[1] == []


def test_commit_prep_finish_by_hand():
    s = tiny()
    m = rd.MapModel.from_state(s)
    job = dict(is_init=0, dead=0, kf_slot=2, kf_id=3, n_tri_in=2, stamp=6, flags=0, npts=2)
    outs = m.commit(job, [1, 0], [1, 1], [[1, 2, 3], [4, 5, 6]])
    assert outs == dict(n_tri_ok=1, flags=2)                     # one free slot, two accepted
    t = m.to_state(s)
    assert t["lm_id"].tolist() == [9, 2, 10, 5] and t["lm_obs"][2] == 2 and t["next_lm_id"][0] == 11 and t["f_lm"][2, 1] == 2 == t["f_lmr"][2, 1]
    m = rd.MapModel.from_state(s)
    outs, prev, nxt = m.stereo_prep(dict(job, flags=0), [(1, 1), (2, 2), (3, 3)], [0, 0, 0, 1, 0, 0, 0], (2.0, 2.0, 1.0, 1.0))
    assert outs == dict(flags=1, corners_dropped=1, n_corners=2, n_features=4)          # 4 features per keyframe: the third corner goes
    assert nxt[0] == (np.float32(2.0 * 3 / 5 + 1), np.float32(2.0 * 4 / 5 + 1)) and nxt[2] == prev[2] == (1.0, 1.0)
    outs, tri = m.stereo_finish(dict(job, is_init=0, n_features=4), [(1, 1), (5, 1), (1, 5), (-0.0, 4.9)], [1, 1, 1, 1], 5, 5, 3)
    assert outs == dict(n_right_ok=2, dead=0, n_tri_in=1) and tri == [3]              # feature 0 has a map point
    assert rd.MapModel.from_state(s).stereo_finish(dict(job, is_init=1, n_features=2), [(1, 1), (9, 9)], [1, 1], 5, 5, 2)[0]["dead"] == 1


def test_projection_against_a_rotation_matrix():
    r = np.random.RandomState(0)
    for _ in range(20):
        T = dc.rand_pose(r); X = r.uniform(-3, 3, 3) + [0, 0, 9]
        x, y, z, w = T[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        p = R @ X + T[4:]
        assert np.allclose(rd.project(T, dc.CAM_R, X), (20 * p[0] / p[2] + 8, 21 * p[1] / p[2] + 7.5), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- the generated cases
def all_states():
    for name, KW, NL, nv in dc.gather_cases():
        yield "gather-" + name, dc.gather_case(KW, NL, nv)["state"]
    for nobs in dc.SCATTER_NOBS:
        yield "scatter-%d" % nobs, dc.edges_case(4, 256, nobs)["state"]
    for NL in (256, 4096):
        for n in dc.begin_counts(NL):
            yield "begin-%d-%d" % (NL, n), dc.begin_case(4, NL, n)["state"]
    for NL in dc.MAX_LM:
        for n in (255, 256, 257, 320):
            yield "commit-%d-%d" % (NL, n), dc.commit_case(4, NL, n, 100)["state"]
    for npts in (170, 200, 300, 320):
        yield "features-%d" % npts, dc.feature_case(4, 256, npts)["state"]
    yield "chain", dc.chain_case()["state"]
    yield "neighbour", dc.neighbour_state(11, 1024, 3)


def test_every_generated_case_meets_the_preconditions():
    n = 0
    for name, state in all_states():
        try:
            rd.check_preconditions(state)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        n += 1
    assert n >= 80


def test_generated_cases_have_the_counts_they_promise():
    for name, KW, NL, nv in dc.gather_cases():
        st = dc.gather_case(KW, NL, nv)["state"]
        p = rd.MapModel.from_state(st).ba_problem(12, 1 << 30)
        assert len(p["verts"]) == nv, name
        ids = [lm.id for lm in p["verts"]]
        assert ids == sorted(ids) and (nv < 8 or [lm.slot for lm in p["verts"]] != sorted(lm.slot for lm in p["verts"])), name
        assert nv < 200 or max(ids) > 2 ** 31 - 1 - 3 * NL, name
        assert ((st["lm_state"] == 2) & (st["lm_obs"] > 0)).any() or nv + 40 > NL, name       # a carried landmark outside the window
    assert all(KW == 11 or NL == 4096 or NL in dc.vertex_counts(KW, NL) for KW in dc.MAX_KF for NL in dc.MAX_LM)
    assert 4096 in dc.vertex_counts(11, 4096) and 4095 in dc.vertex_counts(11, 4096)
    for NL in (256, 4096):
        for n in dc.begin_counts(NL):
            c = dc.begin_case(4, NL, n)
            assert len(rd.MapModel.from_state(c["state"]).begin(c["job"], c["xy"], c["mp"])[1]) == n


def test_preconditions_catch_broken_maps():
    def broken(change):
        s = tiny()
        change(s)
        with pytest.raises(AssertionError):
            rd.check_preconditions(s)
    broken(lambda s: s["f_lm"].__setitem__((0, 1), 0))           # id 9 named by two left features of keyframe 7
    broken(lambda s: s["lm_obs"].__setitem__(0, 2))              # count != links

    def two_features(s):                                          # id 2: right at a1 and now left at a2 of keyframe 7, counted
        s["f_lm"][0, 2] = 1; s["lm_obs"][1] = 4; s["lm_obs"][3] = 0
    broken(two_features)
    broken(lambda s: s["lm_id"].__setitem__(3, 9))               # id twice
    broken(lambda s: s["lm_state"].__setitem__(2, 1))            # state without an id
    broken(lambda s: s["f_lm"].__setitem__((2, 0), 2))           # a link to a free slot
    broken(lambda s: s["f_lm"].__setitem__((1, 3), 4))           # a stale link outside the arena


def test_the_bindings_mirror_the_header(svs):
    assert C.sizeof(svs.DmapJob) == 1008 and C.sizeof(svs.DmapStageIO) == 72 + 22 * 8 and C.sizeof(svs.DmapState) == 15 * 8
    assert len(svs.DMAP_BADEV) == svs.DMAP_BADEV_INTS == 21
