"""The cases of the loop-verification tests, each built from a seed: a camera with fx != fy behind a rotated ext_l, a true
pose, landmarks in front of it (float32, like the reference's cv::Point3f), their projections rounded to float32, a planted share of
wrong matches whose pixels are at least 50 px away, and 256-bit descriptors with a chosen number of flipped bits.

reference(name) runs tests/ref_loop_verify.py once per case (cached, never modified by a test) and asserts the margins that make
discrete outcomes comparable between implementations that round differently:
  * for every hypothesis, no point's squared error lies within 1e-6 relative of the threshold;
  * the winner's inlier count is not tied with a hypothesis that has a different inlier set;
  * no gate value lies within 1e-6 relative of its threshold;
  * Hamming distances are integers: d_min, the threshold and every comparison with them are exact.
A seed that violates a margin is replaced HERE (change the seed in CASES), never skipped at run time."""
import ctypes as C
import functools

import numpy as np

import ref_loop_verify as rl
from ref_pose_graph import quat_to_R, se3_exp, se3_inv, se3_mul

CAM = np.array([718.856, 705.3, 607.19, 185.2])
EXT_L = se3_exp(np.array([0.05, -0.02, 0.01, 0.02, -0.03, 0.01]))
TOL_T, TOL_Q, TOL_D = 1e-6, 1e-7, 1e-6            # DESIGN 3's tolerances of a pose (metres, quaternion components); d: the issue's 1e-6
# tests/test_ref_loop_verify.py: the refined pose against the truth on the noise-free cases.  The pixels are rounded to float32
# (half an ulp at 1000 px = 3e-5 px), which is what the deviation measures; measured on this file's cases: translation 2.93e-7 m
# (inliers_at), quaternion 7.51e-9 (n63_65), each the largest over the ACCEPTED cases — bounded at ten times that, DESIGN 10's
# convention for a figure with no other source
MEASURED_T, MEASURED_Q = 2.93e-7, 7.51e-9


def _project(T_pnp, X):
    pc = X @ quat_to_R(T_pnp[:4]).T + T_pnp[4:]
    return np.stack([CAM[0] * pc[:, 0] / pc[:, 2] + CAM[2], CAM[1] * pc[:, 1] / pc[:, 2] + CAM[3]], axis=1), pc[:, 2]


def _flip(rng, row, k):
    out = np.unpackbits(row)
    out[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(out)


def build(seed, nc, nq, n_match, wrong=0.0, no_lm=0, d_min=0, mirror=False, collinear=None, dcur=0.1, dcand=3.0, at_thr=True):
    """n_match candidate rows carry the descriptor of a current row with d_min .. thr flipped bits (one of them exactly d_min, and with
    at_thr one at thr and one at thr + 1, which is dropped); the other candidate rows are random (about 128 bits from everything)."""
    rng = np.random.default_rng(seed)
    T_corr = se3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-0.2, 0.2, 3)]))
    T_pnp = se3_mul(EXT_L, T_corr)
    Ti = se3_inv(T_pnp); Ri = quat_to_R(Ti[:4])

    def landmarks(n):
        pc = rng.uniform([-8, -2, 4], [8, 2, 40], (n, 3))
        if collinear == "all" or (collinear == "some" and n > 12):
            k = n if collinear == "all" else 12
            pc[:k] = np.array([-6.0, 1.0, 8.0]) + np.linspace(0, 1, k)[:, None] * np.array([9.0, -1.5, 21.0])
        return (pc @ Ri.T + Ti[4:]).astype(np.float32).astype(np.float64)

    dup = nq >= 8                                    # the last current row repeats row 0's descriptor: a Hamming tie, lowest index wins
    n_own = nq - 1 if dup else nq
    Lq = landmarks(max(nq, 1))[:nq]
    uv_q, z = _project(T_pnp, Lq) if nq else (np.zeros((0, 2)), None)
    desc_q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    if dup:
        desc_q[nq - 1] = desc_q[0]; uv_q[nq - 1] = uv_q[0] + [120.0, -60.0]
    uv_q = uv_q.astype(np.float32)
    thr = max(2 * d_min, 30)
    desc_c = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    xyz_c = landmarks(max(nc, 1))[:nc]
    has = np.ones(nc, np.uint8)
    rows = rng.permutation(nc)[:n_match] if nc else np.zeros(0, np.int64)
    n_wrong = int(round(wrong * n_match))
    planted = np.zeros(nc, bool)
    for k, c in enumerate(rows):
        q = k % n_own                                # beyond n_own several candidate rows share a current row
        flips = d_min if k == 0 else int(rng.integers(d_min, thr + 1))
        if at_thr and k == 1:
            flips = thr
        if at_thr and k == 2:
            flips = thr + 1                          # one bit too many: not kept
        desc_c[c] = _flip(rng, desc_q[q], flips)
        if k >= n_match - n_wrong:                   # a wrong match: a landmark that projects at least 50 px from the matched pixel
            while True:
                X = landmarks(1)
                p, _ = _project(T_pnp, X)
                if np.hypot(*(p[0] - uv_q[q].astype(np.float64))) >= 50.0:
                    break
            xyz_c[c] = X[0]
        else:
            xyz_c[c] = Lq[q]
            planted[c] = flips <= thr
    for c in rows[3:3 + no_lm]:                      # matched rows whose feature has no landmark
        has[c] = 0; planted[c] = False
    if mirror:                                       # the landmarks' mirror images through the camera centre: same pixels, negative depth
        pc = xyz_c @ quat_to_R(T_pnp[:4]).T + T_pnp[4:]
        xyz_c = ((-pc) @ Ri.T + Ti[4:]).astype(np.float32).astype(np.float64)
    u = rng.normal(size=6); u[3:] *= 0.05; u /= np.linalg.norm(u)       # mostly a translation: the norm of the log is the distance asked for
    T_cur = se3_mul(se3_exp(dcur * u), T_corr)
    u = rng.normal(size=6); u[3:] *= 0.05; u /= np.linalg.norm(u)
    T_cand = se3_mul(se3_inv(se3_exp(dcand * u)), T_corr)
    return dict(desc_c=desc_c, desc_q=desc_q, xyz_c=xyz_c, has_xyz=has, uv_q=uv_q, T_cur=T_cur, T_cand=T_cand,
                truth=dict(T_corr=T_corr, planted=planted))


# name -> (build arguments, parameters).  min_matches given as ("matches" | "points" | "inliers", delta) is resolved against the
# counts the reference finds with min_matches = 4: the boundary "count = min_matches - 1 / min_matches"
CASES = {
    "base_150":          (dict(seed=11, nc=150, nq=150, n_match=90, wrong=0.2, no_lm=5), {}),
    "no_candidates":     (dict(seed=12, nc=0, nq=150, n_match=0), {}),
    "no_current":        (dict(seed=13, nc=150, nq=0, n_match=0), {}),
    "one_by_one":        (dict(seed=14, nc=1, nq=1, n_match=1, at_thr=False), dict(min_matches=1)),
    "n63_65":            (dict(seed=15, nc=63, nq=65, n_match=40, wrong=0.1), {}),
    "n64_64":            (dict(seed=16, nc=64, nq=64, n_match=40, wrong=0.1), {}),
    "n65_63":            (dict(seed=17, nc=65, nq=63, n_match=64, wrong=0.1), {}),              # 64 planted rows on 62 current rows: shared rows
    "n1_150":            (dict(seed=18, nc=1, nq=150, n_match=1, at_thr=False), dict(min_matches=4)),
    "n150_1":            (dict(seed=19, nc=150, nq=1, n_match=30), {}),
    "n1024":             (dict(seed=20, nc=1024, nq=1024, n_match=300, wrong=0.3, no_lm=20), {}),
    "dmin0":             (dict(seed=21, nc=80, nq=70, n_match=50, d_min=0), {}),               # thr 30
    "dmin15":            (dict(seed=22, nc=80, nq=70, n_match=50, d_min=15), {}),              # thr 30
    "dmin16":            (dict(seed=23, nc=80, nq=70, n_match=50, d_min=16), {}),              # thr 32
    "matches_below":     (dict(seed=24, nc=70, nq=70, n_match=30), dict(min_matches=("matches", 1))),
    "matches_at":        (dict(seed=24, nc=70, nq=70, n_match=30), dict(min_matches=("matches", 0))),
    "points_below":      (dict(seed=25, nc=70, nq=70, n_match=30, no_lm=3), dict(min_matches=("points", 1))),
    "points_at":         (dict(seed=25, nc=70, nq=70, n_match=30, no_lm=3), dict(min_matches=("points", 0))),
    "inliers_below":     (dict(seed=26, nc=70, nq=70, n_match=30, wrong=0.2), dict(min_matches=("inliers", 1))),
    "inliers_at":        (dict(seed=26, nc=70, nq=70, n_match=30, wrong=0.2), dict(min_matches=("inliers", 0))),
    "half_wrong":        (dict(seed=27, nc=120, nq=120, n_match=100, wrong=0.5), {}),
    "all_behind":        (dict(seed=29, nc=60, nq=60, n_match=40, mirror=True), {}),
    "collinear_all":     (dict(seed=29, nc=60, nq=60, n_match=40, collinear="all"), {}),
    "collinear_some":    (dict(seed=30, nc=60, nq=60, n_match=45, collinear="some"), {}),
    "too_far":           (dict(seed=31, nc=60, nq=60, n_match=40, dcand=25.0), {}),
    "too_different":     (dict(seed=32, nc=60, nq=60, n_match=40, dcur=60.0), {}),
    "correction_on":     (dict(seed=33, nc=60, nq=60, n_match=40, dcur=2.0), {}),
    "correction_off":    (dict(seed=34, nc=60, nq=60, n_match=40, dcur=0.5), {}),
    "iters_1":           (dict(seed=35, nc=60, nq=60, n_match=40), dict(ransac_iters=1, seed=7)),
    "iters_1024":        (dict(seed=36, nc=60, nq=60, n_match=40, wrong=0.3), dict(ransac_iters=1024, seed=123456789)),
}
# what each case is expected to end as: a generator that drifts from its purpose fails test_ref_loop_verify.py
EXPECTED = {"no_candidates": "FEW_MATCHES", "no_current": "FEW_MATCHES", "n1_150": "FEW_MATCHES", "matches_below": "FEW_MATCHES",
            "points_below": "FEW_POINTS", "inliers_below": "FEW_INLIERS", "all_behind": "FEW_INLIERS", "collinear_all": "FEW_INLIERS",
            "too_far": "TOO_FAR", "too_different": "TOO_DIFFERENT", "one_by_one": "FEW_POINTS", "n150_1": "FEW_INLIERS"}
NOISE_FREE = [n for n in CASES if EXPECTED.get(n, "ACCEPTED") == "ACCEPTED"]


@functools.lru_cache(maxsize=None)
def _built(name):
    return build(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def params(name):
    p = dict(CASES[name][1])
    mm = p.get("min_matches")
    if isinstance(mm, tuple):
        probe = rl.loop_verify(_built(name), CAM, EXT_L, **dict(p, min_matches=4))
        p["min_matches"] = probe["n_" + mm[0]] + mm[1]
    return p


def case(name):
    return _built(name)


def _margins(name, ref, detail, p):
    p = dict(rl.DEFAULTS, **p)
    if "hyps" in detail:
        thr2 = detail["thr2"]; win = detail["winner"]
        for i, h in enumerate(detail["hyps"]):
            if h is None:
                continue
            e2, front, inl = h
            assert not np.any(np.abs(e2[front] - thr2) <= 1e-6 * thr2), (name, "a squared error at the threshold, hypothesis %d" % i)
            if win >= 0 and int(inl.sum()) == int(detail["hyps"][win][2].sum()):
                assert np.array_equal(inl, detail["hyps"][win][2]), (name, "the winner's count is tied with another inlier set (hypothesis %d)" % i)
    if "far" in detail:
        assert abs(detail["far"] - p["max_pose_distance"]) > 1e-6 * p["max_pose_distance"], name
        if ref["status"] != rl.TOO_FAR:
            for k in ("min_pose_difference", "max_pose_difference"):
                assert abs(ref["d"] - p[k]) > 1e-6 * p[k], (name, k)


@functools.lru_cache(maxsize=None)
def reference(name):
    detail = {}
    ref = rl.loop_verify(_built(name), CAM, EXT_L, detail=detail, **params(name))
    _margins(name, ref, detail, params(name))
    ref["T_pnp"] = detail.get("T_pnp")
    return ref


def compare(got, ref):
    """status, counts, the match list with its inlier flags and need_correction exactly; the poses and d at the tolerances"""
    msgs = []
    for k in ("status", "n_matches", "n_points", "n_inliers"):
        if int(got[k]) != int(ref[k]):
            msgs.append("%s %d != %d" % (k, got[k], ref[k]))
    if bool(got["need_correction"]) != bool(ref["need_correction"]):
        msgs.append("need_correction")
    if not np.array_equal(np.asarray(got["matches"], np.int64), ref["matches"]):
        msgs.append("match list")
    for k in ("T_corr", "T_rel"):
        g = np.asarray(got[k]); r = ref[k]
        dq = min(np.abs(g[:4] - r[:4]).max(), np.abs(g[:4] + r[:4]).max()); dt = np.abs(g[4:] - r[4:]).max()
        if not (dq <= TOL_Q and dt <= TOL_T):
            msgs.append("%s dq %.3g dt %.3g" % (k, dq, dt))
    if not abs(got["d"] - ref["d"]) <= TOL_D:
        msgs.append("d %.3g" % abs(got["d"] - ref["d"]))
    return not msgs, "; ".join(msgs)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in
               ("status", "n_matches", "n_points", "n_inliers", "need_correction", "matches", "T_corr", "T_rel", "d"))


# ---------------------------------------------------------------- the host emulation's ctypes side (tests/cpp/lv_host_emu)
class EmuLoopJob(C.Structure):
    _fields_ = [("c_ofs", C.c_int), ("nc", C.c_int), ("q_ofs", C.c_int), ("nq", C.c_int), ("T_cur", C.c_double * 7), ("T_cand", C.c_double * 7),
                ("status", C.c_int), ("n_matches", C.c_int), ("n_points", C.c_int), ("n_inliers", C.c_int), ("need_correction", C.c_int),
                ("reserved", C.c_int), ("T_corr", C.c_double * 7), ("T_rel", C.c_double * 7), ("d", C.c_double)]


class EmuLoopParams(C.Structure):
    _fields_ = [("cam", C.c_double * 4), ("ext_l", C.c_double * 7), ("min_matches", C.c_int), ("ransac_iters", C.c_int),
                ("reproj_px", C.c_double), ("max_pose_distance", C.c_double), ("min_pose_difference", C.c_double),
                ("max_pose_difference", C.c_double), ("seed", C.c_uint), ("reserved", C.c_int)]


def emu_run(lib, jobs, cam=CAM, ext_l=EXT_L, **prm):
    swap = prm.pop("swap_ranges", False)             # hand jobs 0 and 1 over in descending order of their ranges
    p = dict(rl.DEFAULTS); p.update(prm)
    n = len(jobs)
    arr = (EmuLoopJob * n)()
    DC, XC, HX, DQ, UV = [], [], [], [], []
    co = qo = 0
    for i, job in enumerate(jobs):
        dc = np.ascontiguousarray(job["desc_c"], np.uint8).reshape(-1, 32); dq = np.ascontiguousarray(job["desc_q"], np.uint8).reshape(-1, 32)
        arr[i].c_ofs, arr[i].nc, arr[i].q_ofs, arr[i].nq = co, len(dc), qo, len(dq)
        arr[i].T_cur = (C.c_double * 7)(*job["T_cur"]); arr[i].T_cand = (C.c_double * 7)(*job["T_cand"])
        co += len(dc); qo += len(dq)
        DC.append(dc); DQ.append(dq); XC.append(np.asarray(job["xyz_c"], np.float64).reshape(-1, 3))
        HX.append(np.asarray(job["has_xyz"], np.uint8).reshape(-1)); UV.append(np.asarray(job["uv_q"], np.float32).reshape(-1, 2))
    if swap:
        a, b = arr[0], arr[1]
        (a.c_ofs, a.nc, a.q_ofs, a.nq), (b.c_ofs, b.nc, b.q_ofs, b.nq) = (b.c_ofs, b.nc, b.q_ofs, b.nq), (a.c_ofs, a.nc, a.q_ofs, a.nq)
    cat = lambda v, shape, dt: np.ascontiguousarray(np.concatenate(v), dt) if v else np.zeros(shape, dt)
    DC = cat(DC, (0, 32), np.uint8); DQ = cat(DQ, (0, 32), np.uint8); XC = cat(XC, (0, 3), np.float64); HX = cat(HX, 0, np.uint8)
    UV = cat(UV, (0, 2), np.float32)
    P = EmuLoopParams((C.c_double * 4)(*cam), (C.c_double * 7)(*ext_l), int(p["min_matches"]), int(p["ransac_iters"]), p["reproj_px"],
                      p["max_pose_distance"], p["min_pose_difference"], p["max_pose_difference"], int(p["seed"]), 0)
    mc = np.full(co, -7, np.int32); mq = np.full(co, -7, np.int32); md = np.full(co, -7, np.int32); mi = np.full(co, 9, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.emu_lv_error.restype = C.c_char_p
    rc = lib.emu_loop_verify(n, arr, C.byref(P), co, ptr(DC), ptr(XC), ptr(HX), qo, ptr(DQ), ptr(UV), ptr(mc), ptr(mq), ptr(md), ptr(mi))
    if rc != 0:
        assert (mc == -7).all() and (mi == 9).all(), "a refused call wrote into the match lists"
        raise RuntimeError(lib.emu_lv_error().decode())
    out = []
    for j in arr:
        s = slice(j.c_ofs, j.c_ofs + j.n_matches)
        out.append(dict(status=j.status, n_matches=j.n_matches, n_points=j.n_points, n_inliers=j.n_inliers,
                        need_correction=bool(j.need_correction), T_corr=np.array(j.T_corr), T_rel=np.array(j.T_rel), d=j.d,
                        matches=np.stack([mc[s], mq[s], md[s], mi[s]], axis=1).astype(np.int64)))
    return out
