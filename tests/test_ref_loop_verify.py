"""tests/ref_loop_verify.py, the numeric contract of svslam_loop_verify_batch, against independent statements of its pieces: the
matcher against an np.unpackbits brute force, the P3P against its own constraints and the true pose, the planted inliers recovered,
the refined pose against the truth, the outcome each case was built for."""
import numpy as np
import pytest

import loop_verify_cases as lc
import ref_loop_verify as rl
from ref_pose_graph import quat_to_R, se3_mul


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
    rng = np.random.default_rng(5)
    cam = [float(v) for v in lc.CAM]
    found = 0
    for trial in range(50):
        job = lc.build(seed=100 + trial, nc=8, nq=8, n_match=8, at_thr=False)
        T_pnp = se3_mul(lc.EXT_L, job["truth"]["T_corr"])
        U = np.unique(job["xyz_c"], axis=0)                                             # (candidate rows may share a landmark)
        X = U[rng.permutation(len(U))[:3]]
        pc = X @ quat_to_R(T_pnp[:4]).T + T_pnp[4:]
        uv = np.stack([cam[0] * pc[:, 0] / pc[:, 2] + cam[2], cam[1] * pc[:, 1] / pc[:, 2] + cam[3]], axis=1)
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
