"""GPU: the geometry and bundle-adjustment kernels on a general stereo rig (common.GENERAL_RIG: both extrinsics rotated,
fx != fy, cam_l != cam_r) against the CPU oracle at the tolerances of SURVEY 8d, through the C ABI.

Every other GPU test uses the reference's rig, where six of the nine entries of each extrinsic rotation are zeros, fx == fy
and both cameras share their intrinsics: a transposed Re, an fx / fy mix-up or a wrong camera selection passes them all.
The reference side of these tests is pinned on the CPU in tests/test_oracle_general_rig.py.

The library has two instantiations of every BA kernel: EID when both extrinsic quaternions are exactly (0,0,0,1), the general
one otherwise.  (0,0,0,-1) is the same rotation — exactly the identity matrix — but not that quaternion, so
common.KITTI_RIG_NEG_W runs the general code on the reference's rig: the two must agree bit for bit (k_ba.h, ba_project)."""
import importlib

import numpy as np
import pytest

import common as cm
import lm_cases as lc
from test_gpu_ll_ba import _make_ctx

pytestmark = pytest.mark.gpu

RIG = cm.GENERAL_RIG
LL_CONTEXTS = [(16, 1), (16, 0), (8, 1), (4, 0)]
LL_IDS = ["%dshards-%s" % (w, "resident" if r else "streaming") for w, r in LL_CONTEXTS]


def _check_against_oracle(got, ref, what):
    """iterations equal, translation 1e-6 m, quaternion 1e-7, points rtol / atol 1e-6, chi2 rtol 1e-5 atol 1e-6"""
    (poses, pts, chi2, it), (pr, xr, cr, itr) = got, ref[:4]
    dev = (np.abs(poses[:, 4:] - pr[:, 4:]).max(), np.abs(poses[:, :4] - pr[:, :4]).max(),
           (np.abs(pts - xr) / (1 + np.abs(xr))).max(), (np.abs(chi2 - cr) / (0.1 + np.abs(cr))).max() if len(cr) else 0.0)
    print("%-60s vs oracle: t %.1e m, q %.1e, points %.1e (rel), chi2 %.1e (rel)" % ((what,) + dev))
    assert it == itr, what
    assert np.allclose(poses[:, 4:], pr[:, 4:], atol=1e-6), (what, dev)
    assert np.allclose(poses[:, :4], pr[:, :4], atol=1e-7), (what, dev)
    assert np.allclose(pts, xr, rtol=1e-6, atol=1e-6), (what, dev)
    assert np.allclose(chi2, cr, rtol=1e-5, atol=1e-6), (what, dev)


def _bit_equal(a, b, what):
    for i, ((pa, xa, ca, ia), (pb, xb, cb, ib)) in enumerate(zip(a, b)):
        assert ia == ib, (what, i)
        assert np.array_equal(pa, pb), (what, i, "poses", np.abs(pa - pb).max())
        assert np.array_equal(xa, xb), (what, i, "points", np.abs(xa - xb).max())
        assert np.array_equal(ca, cb), (what, i, "chi2", np.abs(ca - cb).max())


def _batch_jobs(rig):
    """sizes of test_local_ba, a 4 x 7 problem, and np = 72 > 64 rows of the reduced system; edges in shuffled order"""
    rng = np.random.default_rng(61)
    mk = lambda nkf, nlm, **kw: cm.make_ba_problem(rng, nkf, nlm, rig=rig, **kw)
    a, b, c, d, e = mk(7, 300), mk(10, 1200), mk(3, 40), mk(4, 7, outlier_frac=0.0), mk(12, 600)
    return [cm.ba_job(a), cm.ba_job(b, rng.random(len(b["okf"])) < 0.3), cm.ba_job(c), cm.ba_job(d),
            cm.ba_job(e, rng.random(len(e["okf"])) < 0.25)]


def _ll_jobs(rig):
    """landmark-major problems: a thinned full window, a mid-size one, fewer landmarks than shards, and one with a keyframe
    and three landmarks (first, middle, last) without edges; returns (jobs, the ragged problem's dict)"""
    rng = np.random.default_rng(62)
    mk = lambda nkf, nlm, **kw: cm.make_ba_problem(rng, nkf, nlm, rig=rig, **kw)
    a, b, c, g = mk(10, 700), mk(7, 300), mk(4, 7, outlier_frac=0.0), mk(6, 200)
    keep = (g["okf"] != 2) & ~np.isin(g["olm"], (0, 77, 199))
    return [cm.ba_job(a, rng.random(len(a["okf"])) < 0.35, sort=True), cm.ba_job(b, sort=True), cm.ba_job(c, sort=True),
            cm.ba_job(g, keep, sort=True)], g


_oracle_cache = {}


def _oracle(orc, key, rig, jobs):
    """the oracle's answers (with the LM trace) for a job list: computed once, shared between the tests and contexts"""
    if key not in _oracle_cache:
        _oracle_cache[key] = [orc.local_ba_trace(*rig, *job, jac_mode=0) for job in jobs]
    return _oracle_cache[key]


BATCH_KW = dict(max_slots=1, max_jobs=8, max_kf=12, max_lm=2048, max_obs=20000)


# --------------------------------------------------------------------------- a. batch solver
def test_batch_ba_on_the_general_rig(svs, orc, monkeypatch):
    """k_local_ba_t<0, 1, false> with rotations that have no zero entry and two different cameras, structure built on the device
    and on the host"""
    jobs = _batch_jobs(RIG)
    assert len(jobs[4][0]) * 6 > 64
    cd = svs.Context(cm.W, cm.H, **BATCH_KW)
    monkeypatch.setenv("SVSLAM_BA_HOST_BUILD", "1")
    ch = svs.Context(cm.W, cm.H, **BATCH_KW)
    monkeypatch.delenv("SVSLAM_BA_HOST_BUILD")
    try:
        rd = cd.local_ba(jobs, *RIG)
        rh = ch.local_ba(jobs, *RIG)
    finally:
        cd.close(); ch.close()
    for i, (got, ref) in enumerate(zip(rd, _oracle(orc, "batch general", RIG, jobs))):
        _check_against_oracle(got, ref, "batch, general rig, problem %d (%d x %d)" % (i, len(jobs[i][0]), len(jobs[i][1])))
        assert (got[2] < 5.991).mean() > 0.75
    _bit_equal(rd, rh, "device build vs host build")


# --------------------------------------------------------------------------- b. one term at a time
def _rot_only(ext, t):
    return np.concatenate([ext[:4], t])


ONE_THING = {
    "fy": ((cm.CAM[0], 371.9, cm.CAM[2], cm.CAM[3]), cm.EXT_L, (cm.CAM[0], 371.9, cm.CAM[2], cm.CAM[3]), cm.EXT_R),
    "cam_r": (cm.CAM, cm.EXT_L, RIG[2], cm.EXT_R),
    "ext_r-rotation": (cm.CAM, cm.EXT_L, cm.CAM, _rot_only(RIG[3], cm.EXT_R[4:])),
}


@pytest.mark.parametrize("name", list(ONE_THING))
def test_batch_ba_with_one_thing_changed(svs, orc, name):
    """the KITTI rig with only fy, only the right camera's intrinsics, or only the right extrinsic's rotation changed: a failure
    here names the term — CT[13] against CT[12], the camera an edge selects, Re"""
    rig = ONE_THING[name]
    job = cm.ba_job(cm.make_ba_problem(np.random.default_rng(63), 6, 200, rig=rig))
    c = svs.Context(cm.W, cm.H, **BATCH_KW)
    try:
        (got,) = c.local_ba([job], *rig)
    finally:
        c.close()
    _check_against_oracle(got, orc.local_ba(*rig, *job, jac_mode=0), "batch, only %s changed" % name)


# --------------------------------------------------------------------------- c. low-latency solver
@pytest.mark.parametrize("shards,resident", LL_CONTEXTS, ids=LL_IDS)
def test_ll_ba_on_the_general_rig(svs, orc, shards, resident):
    """k_ba_ll<W, false> (resident) and k_local_ba_t<2, W, false> (streaming): the oracle's answers and its LM trajectory trial
    by trial, the batch kernel's answers to the rounding of another summation order, vertices without edges untouched"""
    jobs, ragged = _ll_jobs(RIG)
    refs = _oracle(orc, "ll general", RIG, jobs)
    c = _make_ctx(svs, shards, resident)
    cb = svs.Context(cm.W, cm.H, max_slots=1, max_jobs=16, max_kf=11, max_lm=4096, max_obs=16384)
    try:
        c.host_counters()
        res = c.local_ba(jobs, *RIG)
        assert c.host_counters()[6] == len(jobs), "the low-latency solver did not take the call"
        sh = c.ll_shards(len(jobs))
        traces = [c.lm_trace(job=i) for i in range(len(jobs))]
        batch = cb.local_ba(jobs, *RIG)
    finally:
        c.close(); cb.close()
    assert sh.shape[1] == shards
    if not resident:
        assert np.all(sh[:, :, 4] == 1)
    elif shards == 16:
        assert np.all(sh[:, :, 4] == 2), "a K <= 10 window over 16 workgroups fits the resident layout: %s" % sh[:, :, 4].tolist()
    assert int(np.count_nonzero(sh[2, :, 1])) <= 7              # 7 landmarks: shards without edges
    for i, (got, ref, tr, bat) in enumerate(zip(res, refs, traces, batch)):
        what = "low latency %d shards %s, general rig, problem %d" % (shards, "resident" if resident else "streaming", i)
        _check_against_oracle(got, ref, what)
        n, _ = lc.assert_traces_agree(tr, ref[4], need_rejected=0, what=what)
        assert n >= 3, (what, "significant prefix", n)
        (pa, xa, ca, ia), (pb, xb, cb2, ib) = got, bat
        assert ia == ib
        assert np.allclose(pa, pb, atol=1e-9), (what, np.abs(pa - pb).max())
        assert np.allclose(xa, xb, rtol=1e-8, atol=1e-8), (what, np.abs(xa - xb).max())
        assert np.allclose(ca, cb2, rtol=1e-6, atol=1e-8), what
    poses, pts = res[3][0], res[3][1]
    assert np.array_equal(poses[2], ragged["poses0"][2]), ("a keyframe without edges moved", np.abs(poses[2] - ragged["poses0"][2]).max())
    for l in (0, 77, 199):
        assert np.array_equal(pts[l], ragged["pts0"][l]), "a landmark without edges moved"
    assert np.array_equal(batch[3][0][2], ragged["poses0"][2]) and np.array_equal(batch[3][1][77], ragged["pts0"][77])


# --------------------------------------------------------------------------- d. EID == general, bit for bit
def _pipeline_job():
    p = lc.pipeline_problems()[0]
    neg = p["ext_r"].astype(np.float64).copy()
    assert np.array_equal(neg[:4], [0, 0, 0, 1])
    neg[:4] = [0, 0, 0, -1]
    return (p["poses0"], p["pts0"], p["okf"], p["olm"], p["ori"], p["ouv"]), p["cam"], p["ext_r"], neg


def test_eid_equals_general_batch(svs):
    """the batch kernel's two instantiations on the same problems, device build: every output bit"""
    jobs = _batch_jobs(cm.KITTI_RIG)
    pj, cam, ext_r, ext_r_neg = _pipeline_job()
    c = svs.Context(cm.W, cm.H, **BATCH_KW)
    try:
        eid = c.local_ba(jobs, *cm.KITTI_RIG)
        gen = c.local_ba(jobs, *cm.KITTI_RIG_NEG_W)
        p_eid = c.local_ba([pj], cam, cm.EXT_L, cam, ext_r)
        p_gen = c.local_ba([pj], cam, cm.EXT_L, cam, ext_r_neg)
    finally:
        c.close()
    assert all(r[3] >= 3 for r in eid)
    _bit_equal(eid, gen, "batch: EID vs general")
    _bit_equal(p_eid, p_gen, "batch, captured pipeline problem: EID vs general")


@pytest.mark.parametrize("shards,resident", [(16, 1), (8, 1), (16, 0), (4, 0)], ids=["16shards-resident", "8shards-resident", "16shards-streaming", "4shards-streaming"])
def test_eid_equals_general_low_latency(svs, shards, resident):
    """the same for k_ba_ll<W, EID> and k_local_ba_t<2, W, EID>"""
    jobs, _ = _ll_jobs(cm.KITTI_RIG)
    pj, cam, ext_r, ext_r_neg = _pipeline_job()
    c = _make_ctx(svs, shards, resident)
    try:
        c.host_counters()
        eid = c.local_ba(jobs, *cm.KITTI_RIG)
        sh_e = c.ll_shards(len(jobs))
        gen = c.local_ba(jobs, *cm.KITTI_RIG_NEG_W)
        sh_g = c.ll_shards(len(jobs))
        p_eid = c.local_ba([pj], cam, cm.EXT_L, cam, ext_r)
        p_gen = c.local_ba([pj], cam, cm.EXT_L, cam, ext_r_neg)
        assert c.host_counters()[6] == 2 * len(jobs) + 2, "the low-latency solver did not take every call"
    finally:
        c.close()
    assert np.array_equal(sh_e[:, :, 4], sh_g[:, :, 4])
    if not resident:
        assert np.all(sh_g[:, :, 4] == 1)
    elif shards == 16:
        assert np.all(sh_g[:, :, 4] == 2), "the resident kernel did not take the problems: %s" % sh_g[:, :, 4].tolist()
    assert all(r[3] >= 3 for r in eid)
    _bit_equal(eid, gen, "low latency: EID vs general")
    _bit_equal(p_eid, p_gen, "low latency, captured pipeline problem: EID vs general")


# --------------------------------------------------------------------------- e. shared-map engine, one rank
def test_shared_map_engine_on_the_general_rig(svs, orc):
    """k_local_ba_t<1>'s phases driven from the host (one rank, no collective) == the single-launch local BA"""
    sdist = importlib.import_module("stereovision-slam_amd.dist")
    sba = importlib.import_module("stereovision-slam_amd.shared_ba")
    rng = np.random.default_rng(64)
    p = cm.make_ba_problem(rng, 7, 900, rig=RIG)
    m = rng.random(len(p["okf"])) < 0.5
    m &= np.bincount(p["olm"][m], minlength=900)[p["olm"]] >= 2
    job = cm.ba_job(p, m)
    c = svs.Context(cm.W, cm.H, max_slots=1, max_jobs=1, max_kf=11, max_lm=2048, max_obs=20000)
    try:
        (ref,) = c.local_ba([job], *RIG)
        eng = sba.HipEngine(c, *RIG, *job)
        it1, lam1 = sba.shared_map_ba(eng, sdist.Rank(0, 0, 1), len(job[0]), iters=10)
        P1, X1, C1 = eng.close()
    finally:
        c.close()
    pr, xr, cr, itr = ref
    assert it1 == itr
    assert np.allclose(P1, pr, atol=1e-9), np.abs(P1 - pr).max()
    assert np.allclose(X1, xr, atol=1e-8), np.abs(X1 - xr).max()
    assert np.allclose(C1, cr, rtol=1e-7, atol=1e-9)
    _check_against_oracle(ref, orc.local_ba(*RIG, *job, jac_mode=0), "batch, general rig, shared-map problem")


# --------------------------------------------------------------------------- f. triangulation
def epipolar_distance(rig, l, r):
    """pixels between each match and the epipolar line of its partner, the larger of the two images' — what the vertical
    disparity is on a rectified rig"""
    cam_l, ext_l, cam_r, ext_r = rig
    K = lambda c: np.array([[c[0], 0, c[2]], [0, c[1], c[3]], [0, 0, 1.0]])
    Rl, Rr = cm.quat_R(ext_l[:4]), cm.quat_R(ext_r[:4])
    R = Rr @ Rl.T; t = ext_r[4:] - R @ ext_l[4:]                         # x_r = R x_l + t
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K(cam_r)).T @ tx @ R @ np.linalg.inv(K(cam_l))
    hl = np.concatenate([l, np.ones((len(l), 1))], 1).astype(np.float64); hr = np.concatenate([r, np.ones((len(r), 1))], 1).astype(np.float64)
    lr = hl @ F.T; ll = hr @ F                                            # lines in the right / left image
    s = np.abs((hr * lr).sum(1))
    return np.maximum(s / np.hypot(lr[:, 0], lr[:, 1]), s / np.hypot(ll[:, 0], ll[:, 1]))


def triangulation_case(rig):
    """192 matches with 0.3 px noise; every third left feature integer with the match on exactly the same row (on the reference's
    rig: an exactly singular DLT system), one match with zero disparity"""
    rng = np.random.default_rng(77)
    n = 192
    P = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 1.5, n), rng.uniform(3, 60, n)], 1)
    l = cm.project(rig[0], cm.EXT_L, rig[1], P)[0] + rng.normal(0, 0.3, (n, 2))
    r = cm.project(rig[2], cm.EXT_L, rig[3], P)[0] + rng.normal(0, 0.3, (n, 2))
    l = l.astype(np.float32); r = r.astype(np.float32)
    l[::3] = np.round(l[::3])
    r[::3, 1] = l[::3, 1]
    r[5] = l[5]
    return l, r


def test_triangulate_on_the_general_rig(svs, orc):
    l, r = triangulation_case(RIG)
    T = cm.random_pose(np.random.default_rng(2))
    jobs = [(l, r, None, 0.0), (l, r, T, 40.0)]
    c = svs.Context(cm.W, cm.H, max_slots=1, max_jobs=2, max_pts=256, max_kf=0, max_lm=0, max_obs=0)
    try:
        res = c.triangulate(jobs, *RIG)
    finally:
        c.close()
    for (xyz, ok), (ul, ur, Tj, zmax) in zip(res, jobs):
        xyz_ref, ok_ref = orc.triangulate(*RIG, ul, ur, Tj, zmax)
        assert np.array_equal(ok, ok_ref)
        m = ok_ref > 0
        assert m.sum() > (100 if Tj is None else 60) and not m.all()
        print("triangulation, general rig: max relative deviation from the oracle %.1e" % (np.abs(xyz[m] - xyz_ref[m]) / (1e-9 + np.abs(xyz_ref[m]))).max())
        assert np.allclose(xyz[m], xyz_ref[m], rtol=1e-9, atol=1e-9)
    # the accepted points re-project onto both pixels within a fraction of what the two measurements disagree by (the bound of
    # test_full_size_batch_properties_without_oracle; the disagreement of a match on a rig that is not rectified is its
    # distance from the epipolar line, which on the reference's rig is the vertical disparity)
    xyz, ok = res[0]
    m = ok > 0
    d = epipolar_distance(RIG, l[m], r[m])
    ul, zl = cm.project(RIG[0], cm.EXT_L, RIG[1], xyz[m])
    ur, zr = cm.project(RIG[2], cm.EXT_L, RIG[3], xyz[m])
    assert (zl > 0).all() and (zr > 0).all()
    assert (np.abs(ul - l[m]).max(1) <= 0.6 * d + 1e-3).all(), (np.abs(ul - l[m]).max(1) / (d + 1e-9)).max()
    assert (np.abs(ur - r[m]).max(1) <= 0.6 * d + 1e-3).all(), (np.abs(ur - r[m]).max(1) / (d + 1e-9)).max()


# --------------------------------------------------------------------------- g. pose-only and the fused track, fx != fy
@pytest.mark.parametrize("low_latency", [0, 1])
def test_pose_only_with_fx_not_fy(svs, orc, low_latency):
    """both kernel shapes with the left camera of the general rig (CT[13] is not CT[12] in the residual and the Jacobian)"""
    cam = RIG[0]
    rng = np.random.default_rng(21)
    jobs, truths = [], []
    for n in (230, 64, 5, 0, 400, 257, 512, 130):
        T_true, P, uv = cm.pose_problem(rng, n, cam)
        jobs.append((cm.EXT_L.copy(), P, uv)); truths.append(T_true)
    c = svs.Context(cm.W, cm.H, max_slots=1, max_jobs=8, max_pts=512, max_kf=0, max_lm=0, max_obs=0)
    try:
        c.low_latency(bool(low_latency))
        res = c.pose_only(jobs, cam)
        res2 = c.pose_only(jobs[::-1], cam)[::-1]
    finally:
        c.close()
    for (T, outl, ninl), (T2, outl2, ninl2), (T0, P, uv), T_true in zip(res, res2, jobs, truths):
        T_ref, outl_ref, ninl_ref = orc.pose_only(cam, T0, P, uv)
        assert np.allclose(T[4:], T_ref[4:], atol=1e-6), np.abs(T - T_ref).max()
        assert np.allclose(T[:4], T_ref[:4], atol=1e-7)
        assert np.array_equal(outl, outl_ref)
        assert ninl == ninl_ref
        if len(P) >= 64:
            assert np.linalg.norm(T[4:] - T_true[4:]) < 0.05
        assert np.array_equal(T, T2) and np.array_equal(outl, outl2) and ninl == ninl2


def test_track_fused_with_fx_not_fy(svs, orc):
    """svslam_track_batch (LK + pose-only in one call) with that camera == the oracle's LK followed by its pose-only"""
    cam = RIG[0]
    l0, r0 = svs.synth_pair(7, 0)
    l1, _ = svs.synth_pair(7, 1)
    pts = orc.gftt(l0)
    q, st, _ = orc.lk(l0, r0, pts, pts)
    xyz, ok = orc.triangulate(cam, cm.EXT_L, cam, cm.EXT_R, pts, q)
    has_mp = ((st > 0) & (ok > 0)).astype(np.uint8)
    c = svs.Context(cm.W, cm.H, max_slots=2, max_jobs=1, max_pts=512, max_corners=200, max_kf=0, max_lm=0, max_obs=0)
    try:
        c.pyramid([0], [l0])
        (r,) = c.track([(0, 1, l1, cm.EXT_L.copy(), pts, pts, has_mp, xyz)], cam)
    finally:
        c.close()
    q1, st1, _ = orc.lk(l0, l1, pts, pts)
    inb = (q1[:, 0] >= 0) & (q1[:, 0] < cm.W) & (q1[:, 1] >= 0) & (q1[:, 1] < cm.H)
    keep = (st1 > 0) & inb
    assert np.array_equal(r["status"], keep.astype(np.uint8))
    assert np.array_equal(r["next_xy"].view(np.uint32), q1.view(np.uint32))
    e = keep & (has_mp > 0)
    T_ref, outl_ref, ninl_ref = orc.pose_only(cam, cm.EXT_L, xyz[e], q1[e])
    T_kitti, _, _ = orc.pose_only(cm.CAM, cm.EXT_L, xyz[e], q1[e])
    assert np.abs(T_ref - T_kitti).max() > 1e-4              # the camera matters to the answer
    assert e.sum() > 60 and ninl_ref > 40
    assert r["n_tracked"] == keep.sum()
    assert r["n_inlier"] == ninl_ref
    assert np.allclose(r["pose"], T_ref, atol=1e-6), np.abs(r["pose"] - T_ref).max()
    assert np.array_equal(r["outlier"][e], outl_ref)
