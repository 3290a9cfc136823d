"""The kernels of the device-resident map (csrc/k_dmap.h), ONE at a time, on maps the test seeds, against the plain model of
tests/ref_dmap.py (written from the reference's Map / Frontend / Backend, not from the kernels).

tests/test_gpu_device_map.py runs the whole pipeline on video with the map on the host and on the device and asks for equal
bits: strong where natural runs go.  Here the map is put where they do not go — vertex counts at the sort's powers of two, ids
near 2^31, the BA capacities hit exactly, the outlier rule at its equalities, landmark slots running out, the eviction quota at
its boundary — through the test hooks svslam_debug_dmap_write / _read / _stage, which launch the kernels by the very functions
the keyframe path launches them with.

Every comparison is exact (np.array_equal on the raw arrays; no tolerance anywhere).  After every stage the WHOLE map of every
stream is read back: the seeded stream must equal the model, the streams beside it what they held before, byte for byte — all
arrays live in one allocation, so an index that strays shows there.  Outputs are pre-filled with a pattern, so what a kernel
must not write is compared as well."""
import ctypes as C

import numpy as np
import pytest

import dmap_cases as dc
import ref_dmap as rd

pytestmark = pytest.mark.gpu

NF = dc.NF
PAT_I = 0x5A5A5A5A
PAT_F = -12345.5
CHI2_TH = 5.991


# ------------------------------------------------------------------------------------------------------------ the rig
@pytest.fixture(scope="module")
def rigs(svs):
    made = {}

    def get(KW, NL, S=3):
        if (KW, NL, S) not in made:
            made[(KW, NL, S)] = svs.Context(dc.W, dc.H, max_slots=2, max_jobs=8, max_pts=NF, max_corners=150, max_kf=KW, max_lm=NL,
                                            max_obs=2048, max_streams=S, device_map=1)
        return Rig(svs, made[(KW, NL, S)], KW, NL, S)
    yield get
    for c in made.values():
        c.close()


class Rig:
    """a context whose streams all hold a known map: `seed` the ones under test, the others get neighbour maps"""

    def __init__(self, svs, ctx, KW, NL, S):
        self.svs, self.ctx, self.KW, self.NL, self.S = svs, ctx, KW, NL, S
        self.held = {}
        for s in range(S):
            self.seed(s, dc.neighbour_state(KW, NL, 100 + s))

    def seed(self, stream, state):
        rd.check_preconditions(state)
        self.ctx.dmap_state_write(stream, state)
        self.held[stream] = {k: v.copy() for k, v in state.items()}

    def check(self, expected=None):
        """every stream, every array: `expected` {stream: state} where the model says so, else what was seeded"""
        for s in range(self.S):
            got = self.ctx.dmap_state_read(s)
            want = (expected or {}).get(s, self.held[s])
            for k in want:
                assert np.array_equal(got[k], want[k]), ("stream %d, %s" % (s, k), np.argwhere(got[k] != want[k])[:5].tolist())
        return got

    def jobs(self, dicts):
        arr = (self.svs.DmapJob * len(dicts))()
        C.memset(arr, 0x5A, C.sizeof(arr))                       # outputs the kernel must write show; inputs are set below
        for j, d in zip(arr, dicts):
            j.stream = d.get("stream", 1); j.slot_cur = 0; j.slot_right = 1; j.is_init = d.get("is_init", 0)
            j.kf_slot = d.get("kf_slot", 0); j.remove_slot = d.get("remove_slot", -1); j.kf_id = d.get("kf_id", 0); j.npts = d.get("npts", 0)
            j.frame_id = d.get("frame_id", 0); j.stamp = d.get("stamp", dc.STAMP); j.dead = d.get("dead", 0); j.flags = d.get("flags", 0)
            j.n_features = d.get("n_features", j.npts); j.n_tri_in = d.get("n_tri_in", 0)
            for name in ("pose", "T_camr_w", "T_wc"):
                v = d.get(name, (0, 0, 0, 1, 0, 0, 0))
                for i in range(7):
                    getattr(j, name)[i] = float(v[i])
        return arr

    def stage(self, stage, jobs, arrays=None, **scalars):
        self.ctx.dmap_stage(stage, jobs, arrays, **scalars)


def job_dict(j):
    out = {}
    for name, _ in type(j)._fields_:
        v = getattr(j, name)
        if name == "win_pose":
            v = [[v[a][i] for i in range(7)] for a in range(12)]
        elif hasattr(v, "__len__"):
            v = list(v)
        out[name] = v
    return out


def expect_job(before, outs, hook_buf=0):
    """the job as it must come back: as it went in (src_buf / dst_buf placed by the hook), with the model's outputs"""
    want = dict(before)
    want["src_buf"] = want["dst_buf"] = hook_buf
    for k, v in outs.items():
        if k == "win_pose":
            want["win_pose"] = [list(r) for r in before["win_pose"]]
            for a, p in v.items():
                want["win_pose"][a] = list(p)
        elif k == "win_slot":
            want["win_slot"] = list(before["win_slot"])
            for a, s in enumerate(v):
                want["win_slot"][a] = s
        else:
            want[k] = list(v) if isinstance(v, (list, tuple, np.ndarray)) else v
    return want


def assert_job(j, want):
    got = job_dict(j)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])


def pat(shape, dtype):
    a = np.empty(shape, dtype)
    a[...] = PAT_F if np.dtype(dtype).kind == "f" else (PAT_I if np.dtype(dtype).itemsize == 4 else 0x5A)
    return a


# ------------------------------------------------------------------------------------------------------------ gather
BD = {name: i for i, name in enumerate(("kf_ofs", "nkf", "lm_ofs", "nlm", "obs_ofs", "nobs", "nblk", "na", "ncontrib", "ntile", "aux_ofs",
                                        "iters_done", "rec_ofs", "lay_nblk", "lay_na", "lay_ntile", "nmv", "reserved", "lm_base", "shmask", "ntrial"))}
# (aux_ofs and lay_ntile are functions of the solver's scratch layout, which tests/test_gpu_ba_structure.py covers: not compared)
BD_COMPARED = [i for n, i in BD.items() if n not in ("aux_ofs", "lay_ntile")]


def gather_arrays(n, NL, MK, MO):
    return dict(badev=pat((n, len(BD)), np.int32), poses=pat((n, MK, 7), np.float64), pts=pat((n, NL, 3), np.float64),
                packed=pat((n, MO), np.uint32), uv=pat((n, MO, 2), np.float32), edge_ref=pat((n, MO), np.int32),
                lm_slot_of=pat((n, NL), np.int32))


def gather_expect(want, j, prob, dead=False):
    """fills job j's part of the pattern-filled arrays with what the model's problem says"""
    n, MK = want["poses"].shape[:2]
    NL, MO = want["pts"].shape[1], want["packed"].shape[1]
    bd = want["badev"][j]
    bd[:] = 0
    bd[BD["kf_ofs"]] = j * MK; bd[BD["lm_ofs"]] = j * NL; bd[BD["obs_ofs"]] = j * MO; bd[BD["rec_ofs"]] = 2 * j * MO; bd[BD["reserved"]] = 1
    if dead or prob["skipped"]:
        return
    kfs, verts, edges = prob["kfs"], prob["verts"], prob["edges"]
    bd[BD["nkf"]] = bd[BD["lay_na"]] = len(kfs); bd[BD["nlm"]] = len(verts); bd[BD["nobs"]] = bd[BD["lay_nblk"]] = len(edges)
    for a, kf in enumerate(kfs):
        want["poses"][j, a] = kf.pose
    for v, lm in enumerate(verts):
        want["pts"][j, v] = lm.pos
        want["lm_slot_of"][j, v] = lm.slot
    for e, ed in enumerate(edges):
        want["packed"][j, e] = ed["v"] | (ed["a"] << 16) | (ed["right"] << 24)
        want["uv"][j, e] = ed["uv"]
        want["edge_ref"][j, e] = (ed["kf_slot"] << 16) | (ed["feat"] << 1) | ed["right"]


def gather_job_outs(prob, flags=0):
    if prob["skipped"]:
        return dict(flags=flags | rd.FLAG_BA_SKIPPED)
    return dict(ba_nkf=len(prob["kfs"]), ba_nlm=len(prob["verts"]), ba_nobs=len(prob["edges"]), win_slot=[kf.slot for kf in prob["kfs"]])


def run_gather(rig, threads, state, MK, MO, dead=0, flags=0):
    rig.seed(1, state)
    prob = rd.MapModel.from_state(state).ba_problem(MK, MO)
    jobs = rig.jobs([dict(stream=1, dead=dead, flags=flags)])
    before = job_dict(jobs[0])
    arr = gather_arrays(1, rig.NL, MK, MO)
    want = {k: v.copy() for k, v in arr.items()}
    gather_expect(want, 0, prob, dead=bool(dead))
    rig.stage("ba_gather", jobs, arr, threads=threads, max_kf=MK, max_obs=MO, chi2_th=CHI2_TH)
    assert np.array_equal(arr["badev"][:, BD_COMPARED], want["badev"][:, BD_COMPARED]), (arr["badev"], want["badev"])
    for k in ("poses", "pts", "packed", "uv", "edge_ref", "lm_slot_of"):
        assert np.array_equal(arr[k], want[k]), (k, np.argwhere(arr[k] != want[k])[:5].tolist())
    assert_job(jobs[0], expect_job(before, {} if dead else gather_job_outs(prob, flags)))
    rig.check()                                                  # the gather writes nothing into any map
    return prob


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("name,KW,NL,nv", dc.gather_cases(), ids=[c[0] for c in dc.gather_cases()])
def test_gather_vertex_and_edge_order(rigs, name, KW, NL, nv, threads):
    """vertex counts around the sort's and the scans' powers of two, ids shuffled against slots and near 2^31 - 1, landmarks of
    state 2 / without observations between the vertices, a window with an empty slot and ids out of slot order, right-only links.
    max_obs is the problem's edge count exactly: nobs == max_obs gathers."""
    rig = rigs(KW, NL)
    state = dc.gather_case(KW, NL, nv)["state"]
    nobs = len(rd.MapModel.from_state(state).ba_problem(12, 1 << 30)["edges"])
    prob = run_gather(rig, threads, state, KW, max(nobs, 1))
    assert not prob["skipped"] and len(prob["verts"]) == nv and len(prob["edges"]) == nobs


@pytest.mark.parametrize("threads", [512, 1024])
def test_gather_skips_over_the_capacities_and_not_at_them(rigs, threads):
    rig = rigs(4, 256)
    state = dc.gather_case(4, 256, 255)["state"]
    full = rd.MapModel.from_state(state).ba_problem(12, 1 << 30)
    nobs, nkf = len(full["edges"]), len(full["kfs"])
    assert not run_gather(rig, threads, state, nkf, nobs)["skipped"]
    assert run_gather(rig, threads, state, nkf, nobs - 1, flags=2)["skipped"]        # nobs == max_obs + 1: flag 4 joins flag 2, bd.nobs == 0
    assert run_gather(rig, threads, state, nkf - 1, nobs)["skipped"]                 # nkf == max_kf + 1
    run_gather(rig, threads, state, nkf, nobs, dead=1)                               # a dead job: the descriptor zeroed, nothing else written


@pytest.mark.parametrize("threads", [512, 1024])
def test_gather_two_jobs_keep_to_their_strides(rigs, threads):
    rig = rigs(4, 256, 6)
    states = {2: dc.gather_case(4, 256, 257 - 1, seed=5)["state"], 4: dc.gather_case(4, 256, 3, seed=6)["state"]}
    MK, MO = 5, 1000
    jobs = rig.jobs([dict(stream=2), dict(stream=4)])
    arr = gather_arrays(2, 256, MK, MO)
    want = {k: v.copy() for k, v in arr.items()}
    wj = []
    for j, s in enumerate((2, 4)):
        rig.seed(s, states[s])
        prob = rd.MapModel.from_state(states[s]).ba_problem(MK, MO)
        assert not prob["skipped"]
        gather_expect(want, j, prob)
        wj.append(expect_job(job_dict(jobs[j]), gather_job_outs(prob)))
    rig.stage("ba_gather", jobs, arr, threads=threads, max_kf=MK, max_obs=MO, chi2_th=CHI2_TH)
    assert np.array_equal(arr["badev"][:, BD_COMPARED], want["badev"][:, BD_COMPARED])
    for k in ("poses", "pts", "packed", "uv", "edge_ref", "lm_slot_of"):
        assert np.array_equal(arr[k], want[k]), k
    for j in range(2):
        assert_job(jobs[j], wj[j])
    rig.check()


# ------------------------------------------------------------------------------------------------------------ scatter
def scatter_inputs(prob, NL, MK, MO, r, iters_done=7):
    """what the gather and the solver hand to the scatter for one job, from the MODEL's problem; new poses and positions"""
    arr = gather_arrays(1, NL, MK, MO)
    gather_expect(arr, 0, prob)
    del arr["packed"], arr["uv"]
    arr["badev"][0, BD["iters_done"]] = iters_done; arr["badev"][0, BD["ncontrib"]] = 321; arr["badev"][0, BD["ntrial"]] = 9
    poses = r.uniform(-1, 1, (len(prob["kfs"]), 7)); pts = r.uniform(-30, 30, (len(prob["verts"]), 3))
    arr["poses"][0, :len(poses)] = poses; arr["pts"][0, :len(pts)] = pts
    arr["chi2"] = pat((1, MO), np.float64)
    return arr, poses, pts


def run_scatter(rig, state, chi2_of, iters_done=7, dead=0, kf_slot=None, zero_nobs=False):
    """chi2_of(prob) -> per-edge chi2.  Returns (model after, problem, chi2)"""
    rig.seed(1, state)
    m = rd.MapModel.from_state(state)
    MK = rig.KW
    prob = m.ba_problem(MK, 1 << 30)
    MO = max(len(prob["edges"]), 1) + 3
    arr, poses, pts = scatter_inputs(prob, rig.NL, MK, MO, np.random.RandomState(len(prob["edges"])), iters_done)
    chi2 = np.asarray(chi2_of(prob), np.float64)
    arr["chi2"][0, :len(chi2)] = chi2
    if zero_nobs:
        arr["badev"][0, BD["nobs"]] = 0
    kf_slot = prob["kfs"][-1].slot if kf_slot is None else kf_slot
    jobs = rig.jobs([dict(stream=1, dead=dead, kf_slot=kf_slot)])
    for a, kf in enumerate(prob["kfs"]):
        jobs[0].win_slot[a] = kf.slot
    before = job_dict(jobs[0])
    keep = {k: v.copy() for k, v in arr.items()}
    outs = {} if zero_nobs else m.ba_apply(dict(dead=dead, kf_slot=kf_slot), prob, chi2, poses, pts, iters_done, CHI2_TH, 321, 9)
    rig.stage("ba_scatter", jobs, arr, max_kf=MK, max_obs=MO, chi2_th=CHI2_TH)
    for k in keep:
        assert np.array_equal(arr[k], keep[k]), k                   # inputs only
    assert_job(jobs[0], expect_job(before, outs))
    rig.check({1: m.to_state(state)})
    return m, prob, chi2


@pytest.mark.parametrize("nobs", dc.SCATTER_NOBS)
def test_scatter_edge_counts_across_the_chunk(rigs, nobs):
    """1, 255, 256 and 257 edges, a third of them outliers: which feature loses its link, which landmark an observation"""
    state = dc.edges_case(4, 256, nobs)["state"]
    m, prob, chi2 = run_scatter(rigs(4, 256), state, lambda p: [100.0 if e % 3 == 1 else 0.5 for e in range(len(p["edges"]))])
    assert sum(len(lm.obs) for lm in m.lms.values()) == nobs - sum(1 for e in range(nobs) if e % 3 == 1)


def test_scatter_half_outliers_doubles_the_threshold(rigs):
    """256 edges, exactly 128 above the threshold: the ratio is 0.5 and `> 0.5` is strict, so the threshold doubles; 64 of the
    128 lie between the two thresholds and end as inliers"""
    def chi2_of(p):
        return [(7.0 if e % 4 == 0 else 100.0) if e % 2 == 0 else 1.0 for e in range(len(p["edges"]))]
    m, prob, chi2 = run_scatter(rigs(4, 256), dc.edges_case(4, 256, 256)["state"], chi2_of)
    assert sum(len(lm.obs) for lm in m.lms.values()) == 256 - 64


def test_scatter_equal_to_the_threshold_is_an_inlier(rigs):
    """chi2 == th is no outlier, in the count (129 of 257 would be a majority of outliers) and in the removal"""
    def chi2_of(p):
        return [CHI2_TH if e % 2 == 0 else 0.25 for e in range(len(p["edges"]))]
    m, prob, chi2 = run_scatter(rigs(4, 256), dc.edges_case(4, 256, 257)["state"], chi2_of)
    assert sum(len(lm.obs) for lm in m.lms.values()) == 257
    # ... and after a doubling: a strict majority above th, all of them equal to 2 th or to 4 th
    def chi2_of2(p):
        return [(2 * CHI2_TH if e % 4 == 0 else 4 * CHI2_TH) if e % 2 == 0 else 0.25 for e in range(len(p["edges"]))]
    m, prob, chi2 = run_scatter(rigs(4, 256), dc.edges_case(4, 256, 257)["state"], chi2_of2)
    assert sum(len(lm.obs) for lm in m.lms.values()) == 257 - 64     # th ends at 2 th0: the edges at 4 th0 go


def test_scatter_five_doublings_and_no_more(rigs):
    """all edges far out: five doublings, th = 32 th0.  153 edges at 20 th0 are inliers under 32 th0 (four doublings would call them
    outliers); the others, at 1e9, go — with both edges of one feature, and both observations of landmarks that keep state 1 at 0"""
    def chi2_of(p):
        return [20 * CHI2_TH if e % 5 < 3 else 1e9 for e in range(len(p["edges"]))]
    state = dc.edges_case(4, 256, 255)["state"]
    m, prob, chi2 = run_scatter(rigs(4, 256), state, chi2_of)
    assert sum(len(lm.obs) for lm in m.lms.values()) == 153
    # all of it gone: every landmark loses all its observations, stays active (CleanMap runs with the next retirement only)
    m, prob, chi2 = run_scatter(rigs(4, 256), state, lambda p: [1e9] * len(p["edges"]))
    assert all(not lm.obs and lm.active for lm in m.lms.values()) and len(m.lms) == 64
    assert all(ft.lm is None and ft.lmr is None for kf in m.kfs.values() for ft in kf.feats)


def test_scatter_applies_nothing_for_a_failed_solve_a_dead_job_or_an_empty_problem(rigs):
    state = dc.edges_case(4, 256, 256)["state"]
    chi2_of = lambda p: [100.0 if e % 3 == 0 else 1.0 for e in range(len(p["edges"]))]
    m, _, _ = run_scatter(rigs(4, 256), state, chi2_of, iters_done=-1)          # reports -1, touches nothing
    for k, v in m.to_state(state).items():
        assert np.array_equal(v, state[k])
    run_scatter(rigs(4, 256), state, chi2_of, dead=1)
    run_scatter(rigs(4, 256), state, chi2_of, zero_nobs=True)                   # bd.nobs == 0 with chi2 behind it
    run_scatter(rigs(11, 1024), dc.gather_case(11, 1024, 257)["state"], chi2_of, kf_slot=7)       # a job whose keyframe is mid-window


# ------------------------------------------------------------------------------------------------------------ begin
def run_begin(rig, cases, quota):
    """cases: {stream: begin_case}.  Returns per stream the evicted id set"""
    streams = sorted(cases)
    models, cands, wants, dicts = {}, {}, [], []
    for s in streams:
        c = cases[s]
        rig.seed(s, c["state"])
        rig.ctx.rtrack_upload([(s, c["xy"], c["mp"], c["xyz"])])
        models[s] = rd.MapModel.from_state(c["state"])
        dicts.append(dict(c["job"], stream=s))
    jobs = rig.jobs(dicts)
    for j, s in enumerate(streams):
        outs, cands[s] = models[s].begin(dicts[j], cases[s]["xy"], cases[s]["mp"])
        wants.append(expect_job(job_dict(jobs[j]), outs))
    n = len(streams)
    ev = pat((n * quota, 4), np.int32)
    cur = np.zeros(1, np.int32)
    rig.stage("begin", jobs, dict(evicted=ev, ev_cursor=cur), ev_quota=quota)
    after = {s: rig.ctx.dmap_state_read(s) for s in streams}
    sets, ranges = {}, []
    for j, s in enumerate(streams):
        ofs, cnt = jobs[j].ev_ofs, jobs[j].ev_n
        assert cnt == min(len(cands[s]), quota) and 0 <= ofs and ofs + cnt <= cur[0]
        ranges.append((ofs, ofs + cnt))
        recs = [(int(ev[i, 0]),) + tuple(ev[i, 1:].view(np.float32)) for i in range(ofs, ofs + cnt)]
        sets[s] = models[s].check_eviction(cands[s], quota, recs, after[s])
        wants[j]["ev_ofs"], wants[j]["ev_n"] = (ofs, cnt) if cnt else (0, 0)
        assert_job(jobs[j], wants[j])
    live = sorted(r for r in ranges if r[1] > r[0])
    assert sum(b - a for a, b in live) == cur[0] and all(live[i][1] == live[i + 1][0] for i in range(len(live) - 1))     # disjoint, no gap
    assert (ev[cur[0]:] == PAT_I).all()
    rig.check({s: models[s].to_state(cases[s]["state"]) for s in streams})
    return sets


@pytest.mark.parametrize("NL", [256, 4096])
@pytest.mark.parametrize("which", range(6))
def test_begin_retires_inserts_and_evicts_up_to_the_quota(rigs, NL, which):
    """candidates 0, 1, quota - 1, quota, quota + 1, 3 quota: a subset of the candidates of size min(candidates, quota) leaves, as
    (id, float32 position); the same subset on a repeat; whatever else was a candidate is untouched; the landmark the tracked list
    names is stamped and stays although it is outside the window and unobserved"""
    quota, ncand = dc.begin_quota(NL), dc.begin_counts(NL)[which]
    rig = rigs(4, NL)
    case = dc.begin_case(4, NL, ncand)
    first = run_begin(rig, {1: case}, quota)
    assert len(first[1]) == min(ncand, quota)
    assert run_begin(rig, {1: case}, quota) == first


def test_begin_four_jobs_share_one_cursor(rigs):
    rig = rigs(4, 256, 6)
    cases = {s: dc.begin_case(4, 256, n, seed=20 + s) for s, n in ((1, 9), (2, 0), (3, 5), (4, 30))}
    sets = run_begin(rig, cases, 8)
    assert [len(sets[s]) for s in (1, 2, 3, 4)] == [8, 0, 5, 8]


def test_begin_of_an_init_job_resets_the_job_and_nothing_else(rigs):
    rig = rigs(4, 256)
    case = dc.begin_case(4, 256, 5)
    case["job"] = dict(case["job"], is_init=1, npts=0)
    case["xy"], case["mp"], case["xyz"] = case["xy"][:0], case["mp"][:0], case["xyz"][:0]
    assert run_begin(rig, {1: case}, 8) == {1: set()}


# ------------------------------------------------------------------------------------------------------------ commit
def run_commit(rig, case, open_slots=()):
    state = case["state"]
    rig.seed(1, state)
    m = rd.MapModel.from_state(state, open_slots=open_slots)
    jobs = rig.jobs([dict(case["job"], stream=1)])
    before = job_dict(jobs[0])
    n = case["job"]["n_tri_in"]
    arr = dict(tri_idx=np.zeros((1, NF), np.int32), tri_ok=np.ones((1, NF), np.uint8), tri_xyz=pat((1, NF, 3), np.float64))
    arr["tri_idx"][0, :n] = case["tri_idx"]; arr["tri_ok"][0, :n] = case["tri_ok"]; arr["tri_xyz"][0, :n] = case["tri_xyz"]
    keep = {k: v.copy() for k, v in arr.items()}
    outs = m.commit(before, case["tri_idx"], case["tri_ok"], case["tri_xyz"])
    rig.stage("commit", jobs, arr)
    for k in keep:
        assert np.array_equal(arr[k], keep[k]), k
    assert_job(jobs[0], expect_job(before, outs))
    rig.check({1: m.to_state(state)})
    return outs


@pytest.mark.parametrize("NL", [256, 1024, 4096])
@pytest.mark.parametrize("n_tri_in", [255, 256, 257, 320])
def test_commit_deals_free_slots_in_order_and_flags_a_shortage(rigs, NL, n_tri_in):
    """free slots scattered through the arena: 0, one below, equal to and one above the accepted count and, where the arena has
    that many, at least max_pts.  Ids are next_lm_id + rank, slots ascending, both feature links set, flag 2 exactly when
    accepted > free"""
    rig = rigs(4, NL)
    acc = dc.commit_case(4, NL, n_tri_in, 0)["accepted"]
    for nfree in [0, acc - 1, acc, acc + 1] + ([NF, NL - 7] if NL > NF + 7 else []):
        nfree = min(nfree, NL)
        case = dc.commit_case(4, NL, n_tri_in, nfree)
        outs = run_commit(rig, case)
        a = case["accepted"]
        assert a == acc
        assert outs["n_tri_ok"] == min(a, nfree) and (outs.get("flags", 0) == rd.FLAG_LM_FULL) == (a > nfree), (nfree, a, outs)


def test_commit_init_job_writes_the_header_and_a_dead_job_nothing(rigs):
    rig = rigs(11, 1024)
    case = dc.commit_case(11, 1024, 257, 400, is_init=True)
    outs = run_commit(rig, case, open_slots=(1,))
    assert outs["n_tri_ok"] == case["accepted"]
    got = rig.ctx.dmap_state_read(1)
    assert got["kf_frame"][1] == 5 and got["kf_id"][1] == 0
    case = dc.commit_case(11, 1024, 257, 400, is_init=True)
    case["job"]["dead"] = 1
    assert run_commit(rig, case, open_slots=(1,)) == {}


# ------------------------------------------------------------------------------------------------------------ prep, finish, refresh
@pytest.mark.parametrize("npts,ncorners", [(300, 150), (320, 40), (170, 150), (200, 0)])
def test_stereo_prep_appends_corners_and_projects_start_guesses(rigs, npts, ncorners):
    """room for corners: negative is impossible (npts <= max_pts), zero (320), partial (300 + 150, 20 kept and 130 dropped), ample;
    the start guess of a feature with a map point is the landmark's projection into the right camera in doubles, rounded to float"""
    rig = rigs(4, 256)
    case = dc.feature_case(4, 256, npts)
    state, slot = case["state"], case["slot"]
    rig.seed(1, state)
    m = rd.MapModel.from_state(state)
    r = np.random.RandomState(npts)
    T = dc.rand_pose(r); T[4:] = (0.1, -0.2, 0.3)
    MC = 150
    corners = pat((1, MC, 2), np.float32); corners[0, :ncorners] = r.uniform(0, 600, (ncorners, 2))
    ncor = np.array([ncorners], np.int32)
    jobs = rig.jobs([dict(stream=1, kf_slot=slot, npts=npts, T_camr_w=T, flags=2)])
    before = job_dict(jobs[0])
    arr = dict(corners=corners, ncorners=ncor, lkjobs=pat((1, 4), np.int32), prev_xy=pat((1, NF, 2), np.float32), next_xy=pat((1, NF, 2), np.float32))
    outs, prev, nxt = m.stereo_prep(before, [tuple(c) for c in corners[0, :ncorners]], T, dc.CAM_R)
    want_prev, want_next = arr["prev_xy"].copy(), arr["next_xy"].copy()
    want_prev[0, :len(prev)] = prev; want_next[0, :len(nxt)] = nxt
    rig.stage("stereo_prep", jobs, arr, max_corners=MC, cam_r=dc.CAM_R)
    assert np.array_equal(arr["prev_xy"], want_prev) and np.array_equal(arr["next_xy"], want_next)
    assert arr["lkjobs"][0].tolist() == [0, 1, 0, len(prev)]                     # prev_slot, next_slot, pt_ofs, npts
    assert_job(jobs[0], expect_job(before, outs))
    assert outs["n_corners"] == min(ncorners, NF - npts) and (outs.get("flags", 2) == 3) == (ncorners > NF - npts)
    rig.check({1: m.to_state(state)})


@pytest.mark.parametrize("is_init,good", [(0, 120), (1, 99), (1, 100)])
def test_stereo_finish_image_test_init_threshold_and_triangulation_list(rigs, is_init, good):
    """the in-image test at x == w and y == h (out), at -0.0 (in) and just below 0 (out); StereoInit's threshold at
    num_features_init - 1 (dead: no list) and at num_features_init; the list in feature order across the 256-thread chunks"""
    rig = rigs(4, 256)
    npts = 300
    case = dc.feature_case(4, 256, npts, with_mp=not is_init)
    state, slot = case["state"], case["slot"]
    if is_init:
        state["kf_frame"][slot] = -1
    rig.seed(1, state)
    m = rd.MapModel.from_state(state, open_slots=(slot,))
    r = np.random.RandomState(good)
    nxt = pat((1, NF, 2), np.float32)
    nxt[0, :npts] = r.uniform(0.5, 15.5, (npts, 2))
    status = np.zeros((1, NF), np.uint8); status[0, NF - 10:] = 1
    below = np.nextafter(np.float32(0), np.float32(-1))
    edge = [(16.0, 5.0), (5.0, 16.0), (-0.0, 5.0), (5.0, -0.0), (below, 5.0), (5.0, below), (np.nextafter(np.float32(16), np.float32(0)), 1.0)]
    for i, e in enumerate(edge):                                 # spread over both chunks, status set
        p = 250 + 2 * i
        nxt[0, p] = e; status[0, p] = 1
    n_edge_in = 3
    others = [p for p in r.permutation(npts) if not (250 <= p < 250 + 2 * len(edge))][:good - n_edge_in]
    status[0, others] = 1
    jobs = rig.jobs([dict(stream=1, kf_slot=slot, is_init=is_init, npts=0 if is_init else npts, n_features=npts, T_wc=dc.rand_pose(r))])
    before = job_dict(jobs[0])
    outs, tri = m.stereo_finish(before, nxt[0], status[0], dc.W, dc.H, 100)
    assert outs["n_right_ok"] == good
    arr = dict(next_xy=nxt, status=status, trijobs=pat((1, 9), np.float64), uv_l=pat((1, NF, 2), np.float32), uv_r=pat((1, NF, 2), np.float32),
               tri_idx=pat((1, NF), np.int32))
    want = {k: arr[k].copy() for k in ("uv_l", "uv_r", "tri_idx")}
    kf = m.kfs[slot]
    for q, p in enumerate(tri):
        want["uv_l"][0, q] = kf.feats[p].xy; want["uv_r"][0, q] = kf.feats[p].xyr; want["tri_idx"][0, q] = p
    rig.stage("stereo_finish", jobs, arr, num_features_init=100, zmax=123.5)
    for k in want:
        assert np.array_equal(arr[k], want[k]), k
    tj = arr["trijobs"][0]
    assert tj[:1].view(np.int32).tolist() == [0, len(tri)] and tj[1:8].tolist() == before["T_wc"] and tj[8] == (0.0 if is_init else 123.5)
    assert_job(jobs[0], expect_job(before, outs))
    assert outs["dead"] == (1 if is_init and good < 100 else 0)
    assert (tri == []) if outs["dead"] else (min(tri) < 256 <= max(tri) and tri == sorted(tri))       # both 256-thread chunks, feature order
    rig.check({1: m.to_state(state)})


def test_refresh_and_refresh_xyz(rigs):
    """the keyframe's features become the resident list (landmark slot, position; (0, 0, 1) without a map point); refresh_xyz
    rewrites the positions of the entries that name a landmark and skips mp < 0"""
    rig = rigs(4, 256)
    npts = 300
    case = dc.feature_case(4, 256, npts)
    state, slot = case["state"], case["slot"]
    rig.seed(1, state)
    m = rd.MapModel.from_state(state)
    r = np.random.RandomState(1)
    rig.ctx.rtrack_upload([(1, pat((NF, 2), np.float32), np.full(NF, -1, np.int32), pat((NF, 3), np.float64))])
    # (the upload leaves xyz of entries without a map point as it was: read the list before, compare what must not change)
    xy0, mp0, xyz0 = rig.ctx.rtrack_read(1)
    jobs = rig.jobs([dict(stream=1, kf_slot=slot, npts=npts, n_features=npts)])
    before = job_dict(jobs[0])
    rig.stage("refresh", jobs)
    assert_job(jobs[0], expect_job(before, {}))
    xy, mp, xyz = rig.ctx.rtrack_read(1)
    for i, (p, l, X) in enumerate(m.resident_list(slot)):
        xy0[i] = p; mp0[i] = l; xyz0[i] = X
    assert np.array_equal(xy, xy0) and np.array_equal(mp, mp0) and np.array_equal(xyz, xyz0)
    rig.check()
    # the landmarks move (a local BA landed); the list keeps its features, the named positions follow
    moved = {k: v.copy() for k, v in state.items()}
    moved["lm_pos"] += r.uniform(-1, 1, moved["lm_pos"].shape)
    rig.seed(1, moved)
    m2 = rd.MapModel.from_state(moved)
    jobs = rig.jobs([dict(stream=1, npts=npts - 3)])               # the last three entries are not part of the list any more
    rig.stage("refresh_xyz", jobs)
    xy, mp, xyz = rig.ctx.rtrack_read(1)
    for i in range(npts - 3):
        if mp0[i] >= 0:
            xyz0[i] = m2.position_at(int(mp0[i]))
    assert np.array_equal(xy, xy0) and np.array_equal(mp, mp0) and np.array_equal(xyz, xyz0)
    rig.check()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_optimise_only_job_equals_model_gather_solver_model_scatter(rigs, svs):
    """through the public API: a seeded three-keyframe map, one optimise-only job (is_init == 2).  The map afterwards must be the
    model's gather -> svslam_local_ba_batch on that problem -> the model's scatter on its chi2, bit for bit"""
    rig = rigs(4, 256)
    ctx = rig.ctx
    case = dc.chain_case(4, 256)
    state = case["state"]
    rig.seed(1, state)
    m = rd.MapModel.from_state(state)
    prob = m.ba_problem(4, 2048)
    assert not prob["skipped"] and len(prob["kfs"]) == 3 and len(prob["edges"]) > 300
    ed = prob["edges"]
    (poses, pts, chi2, iters), = ctx.local_ba([(np.array([kf.pose for kf in prob["kfs"]]), np.array([lm.pos for lm in prob["verts"]]),
                                                [e["a"] for e in ed], [e["v"] for e in ed], [e["right"] for e in ed],
                                                np.array([e["uv"] for e in ed], np.float32))],
                                              case["cam"], case["ext_l"], case["cam"], case["ext_r"], huber_delta=CHI2_TH, iters=10)
    st = ctx.ba_struct(1)
    assert iters > 0 and not np.array_equal(poses, np.array([kf.pose for kf in prob["kfs"]]))
    ctx.rtrack_upload([(1, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros((0, 3)))])
    jobs = rig.jobs([dict(stream=1, is_init=2, npts=0, kf_slot=0)])
    prm = svs.DmapParams(150, 100, 3, 10, 300.0, CHI2_TH, 0, 0)
    cam = (C.c_double * 4)(*case["cam"])
    nul = (C.c_void_p * 1)(None); strides = (C.c_int * 1)(0)
    el, er = (C.c_double * 7)(*case["ext_l"]), (C.c_double * 7)(*case["ext_r"])
    rc = ctx.L.svslam_dmap_keyframe_batch(ctx.h, 1, jobs, nul, nul, strides, 1, cam, el, cam, er, C.byref(prm))
    assert rc == 0, ctx.L.svslam_last_error(ctx.h).decode()
    outs = m.ba_apply(dict(dead=0, kf_slot=-1), prob, chi2, poses, pts, iters, CHI2_TH, int(st[0][2]), int(st[0][6]))
    j = jobs[0]
    assert (j.ba_nkf, j.ba_nlm, j.ba_nobs, j.ba_iters, j.flags) == (3, len(prob["verts"]), len(ed), iters, 0)
    assert [j.win_slot[a] for a in range(3)] == [kf.slot for kf in prob["kfs"]]
    for a in range(3):
        assert [j.win_pose[a][i] for i in range(7)] == outs["win_pose"][a]
    assert (j.ba_npair, j.ba_ntrial) == (outs["ba_npair"], outs["ba_ntrial"])
    rig.check({1: m.to_state(state)})
