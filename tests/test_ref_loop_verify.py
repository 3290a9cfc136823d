"""tests/ref_loop_verify.py, the numeric contract of svslam_loop_verify_batch, against independent statements of its pieces: the
matcher against an np.unpackbits brute force, the P3P against its own constraints and the true pose, the planted inliers recovered,
the refined pose against the truth, the outcome each case was built for; the refinement against statements that share none of its
code: its Jacobian against central differences, its end point against the truth's cost, a zero gradient and a plain Gauss-Newton."""
import hashlib
import math

import numpy as np
import pytest

import loop_verify_cases as lc
import ref_loop_verify as rl
from ref_pose_graph import quat_to_R, se3_exp, se3_mul

# the refined pose of the converging noisy cases, measured here (DESIGN 10's convention: bounded at ten times the figure):
# the largest central-difference gradient of the cost, in px^2 per metre or radian (the reference's LM stops on rounding, not on a
# gradient test; the cost itself is 56 px^2 there), and the distance to where a plain Gauss-Newton with a numeric Jacobian ends, whose
# own steps stay near 3e-12 for the noise of that Jacobian.  All three are largest on noisy_10
MEASURED_GRAD = 1.31e-5
MEASURED_GN_T, MEASURED_GN_Q = 4.45e-12, 1.77e-13


@pytest.mark.parametrize("name", ["base_150", "n65_63", "dmin15", "dmin16", "n150_1", "n1024"])
def test_matcher_against_unpackbits_brute_force(name):
    job = lc.case(name)
    bc = np.unpackbits(job["desc_c"], axis=1).astype(np.int32); bq = np.unpackbits(job["desc_q"], axis=1).astype(np.int32)
    D = bc @ (1 - bq).T + (1 - bc) @ bq.T                       # Hamming distances, every pair
    bj, bd = rl.hamming_match(job["desc_c"], job["desc_q"])
    assert np.array_equal(bd, D.min(axis=1))
    assert np.array_equal(bj, np.array([np.nonzero(row == row.min())[0][0] for row in D]))     # the lowest index on a tie
    ref = lc.reference(name)
    thr = max(2 * int(D.min()), 30)
    keep = np.nonzero(D.min(axis=1) <= thr)[0]
    assert np.array_equal(ref["matches"][:, 0], keep) and ref["n_matches"] == len(keep)
    assert np.array_equal(ref["matches"][:, 2], D.min(axis=1)[keep])


def test_the_tie_and_the_shared_rows_are_in_the_cases():
    job = lc.case("n65_63"); ref = lc.reference("n65_63")
    nq = len(job["desc_q"])
    assert np.array_equal(job["desc_q"][nq - 1], job["desc_q"][0])                  # a Hamming tie between rows 0 and nq - 1 ...
    assert 0 in ref["matches"][:, 1] and (nq - 1) not in ref["matches"][:, 1]       # ... goes to the lowest index
    cur, cnt = np.unique(ref["matches"][:, 1], return_counts=True)
    assert cnt.max() >= 2                                                           # several candidates on one current row
    for n, thr in (("dmin0", 30), ("dmin15", 30), ("dmin16", 32)):
        d = lc.reference(n)["matches"][:, 2]
        assert d.min() == {"dmin0": 0, "dmin15": 15, "dmin16": 16}[n] and d.max() == thr      # a match exactly at thr kept, thr + 1 dropped
        bj, bd = rl.hamming_match(lc.case(n)["desc_c"], lc.case(n)["desc_q"])
        assert (bd == thr + 1).any()


def test_p3p_solutions_reproject_their_points_and_contain_the_truth():
    cam = [float(v) for v in lc.CAM]
    found = 0
    for X, uv, T_pnp in lc.p3p_triples():
        sols = rl.p3p([[float(v) for v in x] for x in X], rl.bearings(cam, uv))
        assert 1 <= len(sols) <= 4
        errs = []
        for R, t in sols:
            e2, front = rl.reproj2(cam, R, t, X, uv)
            assert front.all() and e2.max() < 1e-12                                   # squared pixels: every solution reprojects its three points
            Rm = np.array(R).reshape(3, 3)
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-9 and np.linalg.det(Rm) > 0
            errs.append(max(np.abs(Rm - quat_to_R(T_pnp[:4])).max(), np.abs(np.array(t) - T_pnp[4:]).max()))
        found += min(errs) < 1e-6
    assert found == 50


def _digest(job):
    h = hashlib.sha256()
    for k in ("desc_c", "desc_q", "xyz_c", "has_xyz", "uv_q", "T_cur", "T_cand"):
        h.update(np.ascontiguousarray(job[k]).tobytes())
    h.update(np.ascontiguousarray(job["truth"]["T_corr"]).tobytes()); h.update(np.ascontiguousarray(job["truth"]["planted"]).tobytes())
    return h.hexdigest()


def test_the_noise_free_cases_keep_their_bits():
    """the generator's newer arguments draw from a generator of their own: digests taken before they existed"""
    assert _digest(lc.case("base_150")) == "454a3591dffe3b22733370173ff88600a85bb6f9800b119f0f4d3807fa8ff747"
    assert _digest(lc.case("n1024")) == "00eade9e5b7cac501aa46e8ac46c5d6fc363d38d9d63de9e7de9ea82638e3bf2"
    assert _digest(lc.case("half_wrong")) == "1e7f8dc7c07083c15b0ab7a49c0b3525a05a0a5dcc886080e99994a64afd9190"
    assert lc.NOISE_FREE == ["base_150", "n63_65", "n64_64", "n65_63", "n1024", "dmin0", "dmin15", "dmin16", "matches_at", "points_at",
                             "inliers_at", "half_wrong", "collinear_some", "correction_on", "correction_off", "iters_1", "iters_1024",
                             "behind_8"]


def _pattern(ref):
    return "".join("A" if t[5] else "r" for t in ref["lm"])


def _counts(ref):
    return [int(h[2].sum()) for h in ref["hyps"] if h is not None]


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_outcome_each_case_was_built_for(name):
    ref = lc.reference(name)                                                           # (asserts the margins)
    assert rl.STATUS_NAMES[ref["status"]] == lc.EXPECTED.get(name, "ACCEPTED")
    p = lc.params(name)
    if name.endswith("_below") or name.endswith("_at"):
        what = "n_" + name.split("_")[0]
        assert ref[what] == p["min_matches"] - (1 if name.endswith("_below") else 0)
    if name == "correction_on":
        assert ref["need_correction"] and ref["d"] > 1.0
    if name == "correction_off":
        assert not ref["need_correction"] and 0.0 < ref["d"] < 1.0
    if name in ("collinear_all", "n150_1"):
        assert ref["n_inliers"] == 0 and not ref["matches"][:, 3].any()                # no hypothesis at all
    if name == "half_wrong":
        assert ref["n_inliers"] * 2 <= ref["n_points"] + 1
    if name in lc.COUNTS:
        assert (ref["n_points"], ref["n_inliers"]) == lc.COUNTS[name]
    if name in lc.CONVERGING:                                                          # real steps first, rounding after them
        lm = ref["lm"]
        assert _pattern(ref).startswith("AA") and min(t[3] for t in lm if t[5]) < 0.6 * lm[0][2]
        assert abs(lm[-1][4]) < 1e-6                                                   # ... and it has arrived
    if name == "noisy_220":
        assert ref["n_inliers"] > 2 * 64                                               # a third round of the 64 LM lanes
    if name in lc.DESCENT:
        assert ref["lm"][-1][0] == rl.LM_ITERS - 1, "the LM stopped before its last iteration"
        assert "rA" in _pattern(ref), "no rejection that is followed by an acceptance"
    if name.startswith("descent_wide"):
        assert 65 <= ref["n_inliers"] <= 128                                           # two rounds of the 64 LM lanes
    if name == "descent_tiny_460":
        assert _pattern(ref).startswith("rrrrA")                                       # the first decisions of the run are rejections
    if name == "descent_310":                                                          # the fourth point decides, and not for the first solution
        cam = [float(v) for v in lc.CAM]
        idx = rl.draw4(0, 0, ref["n_points"])
        sols = rl.p3p([[float(v) for v in ref["xyz"][k]] for k in idx[:3]], rl.bearings(cam, ref["uv"][idx[:3]]))
        e = [rl.reproj2(cam, R, t, ref["xyz"][idx[3]:idx[3] + 1], ref["uv"][idx[3]:idx[3] + 1]) for R, t in sols]
        e = [float(e2[0]) if front[0] else math.inf for e2, front in e]
        assert len(e) >= 2 and e[0] < math.inf and int(np.argmin(e)) != 0
    if name.startswith("ties"):
        cnt = _counts(ref); full = ref["n_points"]
        tied = [i for i, h in enumerate(ref["hyps"]) if h is not None and int(h[2].sum()) == full]
        assert ref["n_inliers"] == full and len(tied) > 100 and ref["winner"] == tied[0]
        assert min(cnt) < full                                                         # not every hypothesis ties
        if lc.params(name)["ransac_iters"] > 129:
            assert ref["winner"] + 128 in tied                                         # the winner's lane holds a second tied hypothesis
        assert (tied[0] == 0) == (name != "ties_314_low1")
    if name in lc.QUAT_BRANCH:
        assert ref["quat_branch"] == lc.QUAT_BRANCH[name]
    if name == "behind_8":
        job = lc.case(name); m = ref["matches"]
        planted = job["truth"]["planted"]
        assert np.array_equal(m[:, 3] != 0, planted[m[:, 0]]) and int(planted.sum()) == 32
        e2, front, inl = ref["hyps"][ref["winner"]]
        assert (~front).sum() == 8 and e2[~front].max() < 1e-3 * rl.DEFAULTS["reproj_px"] ** 2      # they fit, and are no inliers
    if name.startswith("small"):
        assert ref["n_points"] == int(name[-1]) and len(set(_counts(ref))) >= 2        # the count varies from hypothesis to hypothesis


def test_every_branch_of_R_to_T_is_taken_by_a_descent_case():
    assert {lc.reference(n)["quat_branch"] for n in lc.DESCENT} == {1, 2, 3, 4}


@pytest.mark.parametrize("name", lc.NOISE_FREE)
def test_planted_inliers_recovered_and_pose_against_the_truth(name):
    job = lc.case(name); ref = lc.reference(name)
    planted = job["truth"]["planted"]
    m = ref["matches"]
    assert np.array_equal(m[:, 3] != 0, planted[m[:, 0]])                              # the inlier set IS the planted set
    assert ref["n_inliers"] == int(planted.sum())
    T = job["truth"]["T_corr"]; g = ref["T_corr"]
    dq = min(np.abs(g[:4] - T[:4]).max(), np.abs(g[:4] + T[:4]).max()); dt = np.abs(g[4:] - T[4:]).max()
    print(name, "dq %.3g dt %.3g" % (dq, dt))
    assert dq <= 10 * lc.MEASURED_Q and dt <= 10 * lc.MEASURED_T


# ---------------------------------------------------------------- the refinement, against statements that share none of its code
def _residual(T, xyz, uv):
    """stacked pixel errors of world points under T (world -> camera), written here and not taken from the reference"""
    pc = xyz @ quat_to_R(T[:4]).T + T[4:]
    return np.concatenate([uv[:, 0] - (lc.CAM[0] * pc[:, 0] / pc[:, 2] + lc.CAM[2]), uv[:, 1] - (lc.CAM[1] * pc[:, 1] / pc[:, 2] + lc.CAM[3])])


def _step(T, k, h):
    d = np.zeros(6); d[k] = h
    return se3_mul(se3_exp(d), T)


# Central differences of a residual f (pixels) along exp(h e_k) T.  |f| <= 1300 px and about 8 roundings on the way give f an absolute
# error of 8 * 1.1e-16 * 1300 = 1.2e-12 px, so the quotient carries 1.2e-12 / h; the truncation is h^2 f3 / 6 with the third
# derivative f3 <= 1e5 px (fx d^3 tan / d theta^3 = fx * 2 sec^2 (sec^2 + 2 tan^2) = 9.3e4 at the image's edge, tan = 2; the
# translations' are smaller).  h = 4e-6: 2.7e-7 + 2.9e-7 = 5.6e-7, bounded at 1e-6 px per metre or radian.  A wrong sign or a wrong
# term is off by the size of the entry itself: 10 .. 3000.
FD_H, FD_BOUND = 4e-6, 1e-6


def _numeric_jacobian(T, xyz, uv, h=FD_H):
    return np.stack([(_residual(_step(T, k, h), xyz, uv) - _residual(_step(T, k, -h), xyz, uv)) / (2 * h) for k in range(6)], axis=1)


def test_the_jacobian_against_central_differences():
    ref = lc.reference("noisy_10")
    xyz, uv, T = ref["xyz"][ref["inl"]], ref["uv"][ref["inl"]], ref["T_pnp"]
    R, t = rl.T_to_Rt(T)
    J0, J1 = rl.jacobian([float(v) for v in lc.CAM], xyz @ R.reshape(3, 3).T + t)
    num = _numeric_jacobian(T, xyz, uv)
    err = np.abs(np.concatenate([J0, J1]) - num).max()
    print("jacobian: largest entry %.4g, largest deviation %.3g" % (np.abs(num).max(), err))
    assert np.abs(num).max() > 100 and err <= FD_BOUND


def _cost(T, xyz, uv):
    r = _residual(T, xyz, uv)
    return float(r @ r)


@pytest.mark.parametrize("name", lc.CONVERGING)
def test_the_refined_pose_is_the_minimum_of_the_cost(name):
    job = lc.case(name); ref = lc.reference(name)
    m = ref["matches"]
    assert np.array_equal(m[:, 3] != 0, job["truth"]["planted"][m[:, 0]])              # the planted set, exactly
    xyz, uv, T = ref["xyz"][ref["inl"]], ref["uv"][ref["inl"]], ref["T_pnp"]
    truth = se3_mul(lc.EXT_L, job["truth"]["T_corr"])
    assert _cost(T, xyz, uv) <= _cost(truth, xyz, uv)                                  # the truth is not the minimum of a noisy cost
    h = 1e-6
    grad = np.array([(_cost(_step(T, k, h), xyz, uv) - _cost(_step(T, k, -h), xyz, uv)) / (2 * h) for k in range(6)])
    G = truth                                                                          # plain Gauss-Newton from the truth, to convergence
    for it in range(20):                                                               # (the numeric Jacobian's noise keeps the steps near 3e-12)
        d = np.linalg.lstsq(_numeric_jacobian(G, xyz, uv), -_residual(G, xyz, uv), rcond=None)[0]
        G = se3_mul(se3_exp(d), G)
        if np.abs(d).max() < 1e-10:
            break
    assert it < 19
    dq = min(np.abs(G[:4] - T[:4]).max(), np.abs(G[:4] + T[:4]).max()); dt = np.abs(G[4:] - T[4:]).max()
    print(name, "cost %.6g (truth %.6g) |grad| %.3g; Gauss-Newton in %d steps: dt %.3g dq %.3g" % (
        _cost(T, xyz, uv), _cost(truth, xyz, uv), np.abs(grad).max(), it + 1, dt, dq))
    assert np.abs(grad).max() <= 10 * MEASURED_GRAD
    assert dt <= 10 * MEASURED_GN_T and dq <= 10 * MEASURED_GN_Q
