"""tests/ref_pose_graph.py (the numeric contract of svslam_pose_graph_batch) pinned by things it shares no code with: SE(3) exp / log
against scipy's matrix exponential / logarithm, the closed-form Jacobians against central differences, the converged state against
scipy.optimize.least_squares on the same residuals, its two solvers and its two summation orders against each other — and the
properties the test cases must have (pose_graph_cases.py), asserted on the reference's own run."""
import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

import pose_graph_cases as pc
import ref_pose_graph as rpg


def _mat(T):
    A = np.eye(4); A[:3, :3] = rpg.quat_to_R(T[:4]); A[:3, 3] = T[4:]
    return A


def _tw(xi):
    A = np.zeros((4, 4)); A[:3, :3] = rpg.hat(xi[3:]); A[:3, 3] = xi[:3]
    return A


def test_exp_and_log_against_the_matrix_functions():
    rng = np.random.default_rng(1)
    for scale in (1e-12, 1e-6, 1e-2, 0.3, 1.0, 2.5):
        for _ in range(5):
            xi = np.concatenate([rng.standard_normal(3), scale * rng.standard_normal(3) / np.sqrt(3)])
            T = rpg.se3_exp(xi)
            assert abs(np.linalg.norm(T[:4]) - 1) < 1e-15
            # Sophus' own formulas bound the agreement with the series: V = I + (1 - cos t) / t^2 hat + ... cancels to eps / t^2 in
            # its coefficient (eps |u| / t in the translation), and below 1e-10 rad V = R stands for I + hat / 2 (|u| t / 2)
            th = float(np.linalg.norm(xi[3:])); un = float(np.linalg.norm(xi[:3]))
            atol = 1e-13 + (un * th if th < 1e-10 else 2e-15 * un / th)
            assert np.allclose(_mat(T), scipy.linalg.expm(_tw(xi)), rtol=0, atol=atol)
            back = rpg.se3_log(T)
            assert np.allclose(back, xi, rtol=0, atol=(1e-12 if scale < 2 else 1e-10) + atol)
            lg = np.real(scipy.linalg.logm(_mat(T)))
            assert np.allclose(_tw(back), lg, rtol=0, atol=1e-9)
    A, B = rpg.se3_exp(rng.standard_normal(6)), rpg.se3_exp(rng.standard_normal(6))
    assert np.allclose(_mat(rpg.se3_mul(A, B)), _mat(A) @ _mat(B), atol=1e-14)
    assert np.allclose(_mat(rpg.se3_inv(A)), np.linalg.inv(_mat(A)), atol=1e-14)
    p = rng.standard_normal(3)
    assert np.allclose(rpg.se3_act(A, p), (_mat(A) @ np.r_[p, 1])[:3], atol=1e-14)


def test_analytic_jacobian_against_central_differences():
    rng = np.random.default_rng(2)
    for scale in (1e-4, 0.05, 0.099, 0.101, 0.3, 1.0, 2.0):          # both sides of the 0.1 rad switch to the power series
        for _ in range(3):
            Ta, Tb = rpg.se3_exp(rng.standard_normal(6)), rpg.se3_exp(rng.standard_normal(6))
            err = np.concatenate([rng.standard_normal(3), scale * rng.standard_normal(3) / np.sqrt(3)])
            M = rpg.se3_mul(rpg.se3_exp(err), rpg.se3_mul(Ta, rpg.se3_inv(Tb)))
            Ja, Jb = rpg.edge_jac_analytic(M, Ta, Tb)
            Na, Nb = rpg.edge_jac_numeric(M, Ta, Tb, delta=1e-6)      # truncation 1e-12, rounding 1e-10
            assert np.abs(Ja - Na).max() < 2e-8 and np.abs(Jb - Nb).max() < 2e-8, (scale, np.abs(Ja - Na).max(), np.abs(Jb - Nb).max())


def _least_squares(job):
    poses0 = np.asarray(job["poses"]); fixed = np.asarray(job["fixed"]).astype(bool)
    ea, eb, meas = job["edges"]
    free = np.flatnonzero(~fixed)

    def state(x):
        P = poses0.copy()
        for i, v in enumerate(free):
            P[v] = rpg.se3_mul(rpg.se3_exp(x[6 * i:6 * i + 6]), poses0[v])
        return P

    def res(x):
        P = state(x)
        return np.concatenate([rpg.edge_error(meas[k], P[ea[k]], P[eb[k]]) for k in range(len(ea))])
    sol = scipy.optimize.least_squares(res, np.zeros(6 * len(free)), method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return state(sol.x), float(res(sol.x) @ res(sol.x))


@pytest.mark.parametrize("name", ["n2", "n3_loop_to_fixed", "span2", "fixed_mid", "both_fixed_edge"])
def test_converged_state_against_scipy_least_squares(name):
    """vertex 0 is fixed: no gauge freedom, the poses compare directly.  The reference runs g2o's 22 iterations here."""
    job = pc.cases()[name]
    got = rpg.pose_graph(job, 22)
    want, chi = _least_squares(job)
    assert abs(got["chi2_after"] - chi) <= 1e-9 * max(chi, 1e-6)
    assert np.abs(got["poses"][:, 4:] - want[:, 4:]).max() < 1e-6
    sgn = np.sign(np.sum(got["poses"][:, :4] * want[:, :4], axis=1))[:, None]
    assert np.abs(got["poses"][:, :4] * sgn - want[:, :4]).max() < 1e-7


@pytest.mark.parametrize("name", [n for n in pc.cases() if n != "n257"])
def test_solvers_and_summation_orders_agree(name):
    """every LM decision identical without skipping a trial, the figures far inside the tolerances the kernel is held to"""
    ref = pc.reference(name)
    for solver, order in (("envelope", "edge"), ("dense", "reverse"), ("envelope", "reverse")):
        got = pc.reference(name, solver=solver, h_order=order)
        ok, ties, msg = pc.compare(got, ref, {k: 0.1 * v for k, v in pc.TOL_SMALL.items()})
        assert ok and ties == 0, (name, solver, order, msg)


def test_variants_of_the_reference_at_257():
    """the measurement behind pose_graph_cases.TOL_257: the four variants of the reference differ by at most a tenth of it
    (lambda: not at all)"""
    ref = pc.reference("n257")
    worst = dict(t=0.0, q=0.0, pts=0.0, lam=0.0, chi2=0.0)
    for solver, order in (("envelope", "edge"), ("dense", "reverse"), ("envelope", "reverse")):
        got = pc.reference("n257", solver=solver, h_order=order)
        ok, ties, msg = pc.compare(got, ref, pc.TOL_SMALL)
        assert ok and ties == 0, msg
        for k, v in pc.diffs(got, ref).items():
            worst[k] = max(worst[k], float(v))
    print("n257 variants differ by", worst)
    assert worst["lam"] == 0.0
    for k in ("t", "q", "pts", "chi2"):
        assert worst[k] <= 0.1 * pc.TOL_257[k] * 1.0000001, (k, worst[k])
        assert 10 * pc.TOL_257[k] <= 100 * pc.TOL_SMALL[k]           # far from "too ill-conditioned to test an implementation"


def test_the_cases_have_the_properties_the_tests_rely_on():
    c = pc.cases()
    assert set(pc.ITERS) == set(c)
    heading = 0.0
    job = c["n63"]
    for M in job["edges"][2][job["edges"][0] - job["edges"][1] == 1]:
        heading += abs(rpg.se3_log(M)[4])
    assert heading > 2 * np.pi                                       # more than a full turn along the chain
    near_pi = ("theta_3.0", "theta_pi-1e-5", "pi_plus", "pi_minus")
    for name in c:
        ref = pc.reference(name)
        if name in near_pi:                                          # the cases that are there to evaluate log near its branch cut
            assert ref["max_rot"] >= 3.0, name
        else:
            assert ref["max_rot"] < np.pi - 0.5, name                # elsewhere it never is
        tr = ref["trace"]
        if name == "overflow":
            continue                                                 # its own assertions below
        if name in ("empty", "n1", "edgeless"):
            assert ref["iters"] == 0 and ref["trials"] == 0 and ref["chi2_before"] == 0 and np.array_equal(ref["poses"], np.asarray(c[name]["poses"]).reshape(-1, 7))
        elif name in ("zero_chain", "ten_failed"):
            assert ref["chi2_before"] == 0.0 and ref["iters"] == 1 and np.array_equal(ref["poses"], c[name]["poses"])
            if name == "ten_failed":        # the 10-failed-trials stop: every trial rejected with rho < 0, lambda x 2, 4, 8, ...
                assert ref["trials"] == 10 and not tr[:, 5].any() and (tr[:, 4] < 0).all() and np.allclose(tr[1:, 1] / tr[:-1, 1], 2.0 ** np.arange(1, 10))
            else:
                assert ref["trials"] == 1 and tr[0, 4] == 0.0
        elif name == "optimum":
            assert ref["iters"] == 1 and ref["trials"] == 1 and ref["chi2_before"] == 0.0 and tr[0, 4] == 0.0
            assert np.array_equal(ref["poses"], c[name]["poses"])     # stops at the rho == 0 rule with its input bits
        else:
            assert np.abs(tr[:, 4]).min() > 1e-9, name                # no decision of the reference is rounding noise
            assert ref["chi2_after"] < ref["chi2_before"]
    tr = pc.reference("rejected")["trace"]
    assert (tr[:, 5] == 0).sum() >= 5 and (tr[:, 5] == 1).sum() >= 5 and np.abs(tr[:, 4]).min() > 1e-3
    _new_case_properties(c)
    # pieces of the ABI's bookkeeping the cases exercise
    assert (np.asarray(c["fixed_mid"]["fixed"]) != 0).sum() == 2
    assert (c["loop_full"]["anchor"] == -1).any() and (np.bincount(c["loop_full"]["anchor"][c["loop_full"]["anchor"] >= 0]) > 1).any()


def _new_case_properties(c):
    ne = lambda n: c[n]["edges"]
    b = pc.base_graph(pts="one")
    a, bb, _ = ne("reversed")
    assert (a < bb).sum() >= 6 and (a > bb).sum() >= 6 and ((a < bb) == (np.arange(len(a)) % 2 == 1)).all()
    assert (ne("reversed_all")[0] < ne("reversed_all")[1]).all()
    for k in range(len(a)):                                          # a reversed edge is the same constraint: e' = -Ad(M) e
        e = rpg.edge_error(b["edges"][2][k], b["poses"][b["edges"][0][k]], b["poses"][b["edges"][1][k]])
        r = c["reversed_all"]
        er = rpg.edge_error(r["edges"][2][k], r["poses"][r["edges"][0][k]], r["poses"][r["edges"][1][k]])
        assert np.abs(er + rpg.se3_adj(b["edges"][2][k]) @ e).max() < 1e-12
    f = c["fixed_last"]["fixed"]
    assert f[0] == 0 and f[-1] == 1 and f.sum() == 1
    f = c["fixed_two_ends"]
    assert f["fixed"][0] == 1 and f["fixed"][-1] == 1 and f["fixed"].sum() == 2 and {0, len(f["fixed"]) - 1} <= set(f["anchor"].tolist())
    key = lambda e: sorted(zip(e[0].tolist(), e[1].tolist(), [m.tobytes() for m in e[2]]))
    assert key(ne("edge_perm")) == key(b["edges"]) and not np.array_equal(ne("edge_perm")[0], b["edges"][0])
    v = c["vertex_perm"]
    first = rpg.envelope_first(int((v["fixed"] == 0).sum()), rpg.free_index(v["fixed"]), v["edges"][0], v["edges"][1])
    assert (np.diff(first) < 0).any() and (np.arange(len(first)) - first).max() >= 8 and v["fixed"][0] == 0      # non-monotone, wide
    assert sorted(map(bytes, v["poses"])) == sorted(map(bytes, b["poses"])) and len(v["anchor"]) == len(v["poses"])
    d = ne("duplicate_edge")
    assert (d[0][-1], d[1][-1]) == (8, 3) and ((d[0] == 8) & (d[1] == 3)).sum() == 2 and np.array_equal(d[2][-1], d[2][(d[0] == 8) & (d[1] == 3)][0])
    i = c["isolated_free"]
    q = i["poses"][4, :4]
    assert not ((i["edges"][0] == 4) | (i["edges"][1] == 4)).any() and i["fixed"][4] == 0 and i["anchor"][-1] == 4
    assert q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] == 1.0          # exp(0) T keeps every bit of it
    ref = pc.reference("isolated_free")
    assert np.array_equal(ref["poses"][4], i["poses"][4]) and np.abs(ref["pts"][-1] - i["pts"][-1]).max() < 1e-14
    n, m = c["neg_w"], c["nested"]
    neg = np.flatnonzero(np.sum(n["poses"][:, :4] * m["poses"][:, :4], axis=1) < 0)
    assert neg.tolist() == [0, 3, 4, 9, 13] and np.array_equal(np.abs(n["poses"]), np.abs(m["poses"])) and pc.ITERS["neg_w"] == pc.ITERS["nested"]
    rn, rm = pc.reference("neg_w"), pc.reference("nested")
    assert pc.compare(rn, rm, pc.TOL_SMALL)[0] and np.array_equal(rn["pts"], rm["pts"])
    for name, th in pc.THETAS.items():
        j = c[name]
        e = rpg.edge_error(j["edges"][2][2], j["poses"][2], j["poses"][0])
        assert (j["edges"][0].tolist(), j["edges"][1].tolist()) == ([1, 2, 2], [0, 1, 0])
        assert abs(np.linalg.norm(e[3:]) - th) <= 4e-16 * max(th, 1.0) + (1e-21 if th < 1e-10 else 0.0), (name, np.linalg.norm(e[3:]))
        assert np.linalg.norm(e[:3]) > 0.1                                          # and a translation residual with it
        if th >= 0.5:
            assert pc.reference(name)["max_rot"] == np.linalg.norm(e[3:])          # the start is the largest the run sees
    for name, sign in (("pi_plus", 1.0), ("pi_minus", -1.0)):
        j = c[name]
        E = rpg.se3_mul(rpg.se3_inv(j["edges"][2][-1]), rpg.se3_mul(j["poses"][4], rpg.se3_inv(j["poses"][1])))
        assert 0 < sign * E[3] < rpg.EPS and E[:3] @ E[:3] >= rpg.EPS ** 2           # the +-pi branch of so3_log, this sign
        om = rpg.so3_log(E[:4])
        assert abs(np.linalg.norm(om) - np.pi) < 1e-10 and np.sign(om[0]) == -sign
        t = E[4:]; ax = E[:3] / np.linalg.norm(E[:3])
        assert np.linalg.norm(t) > 0.5 and np.linalg.norm(np.cross(t, ax)) > 0.5     # neither zero nor along the axis
    # chi2_before does not see the sign of the branch (|V^-1 t| = |V^-T t|): the two cases start from the same chi2 to rounding, which
    # is why the device, held to chi2_before alone there, cannot check the sign.  The first trial does: the sign is the host's to check.
    pp, pm = pc.reference("pi_plus"), pc.reference("pi_minus")
    assert abs(pp["chi2_before"] - pm["chi2_before"]) <= 1e-14 * pp["chi2_before"]
    assert abs(pp["trace"][0, 3] - pm["trace"][0, 3]) > 1e3 * pc.TOL_SMALL["chi2"] * pp["trace"][0, 3]
    o = pc.reference("overflow"); tr = o["trace"]
    assert np.isfinite(o["chi2_before"]) and o["chi2_before"] > 1e307 and o["iters"] == 1 and o["trials"] == 1
    assert tr[0, 1] == np.inf and tr[0, 3] == rpg.DBL_MAX and tr[0, 4] == -np.inf and tr[0, 5] == 0.0
    assert np.array_equal(o["poses"], c["overflow"]["poses"]) and np.isfinite(c["overflow"]["poses"]).all()


def test_reversing_every_edge_keeps_a_zero_residual_optimum():
    """(a, b, M) and (b, a, M^-1) are the same constraint with the residual -Ad(M) e: where the measurements are consistent both
    graphs converge to the one state that satisfies them, compared at the final-state tolerances.  (Not so for reversed_all itself:
    its odometry is noisy, the optimum has non-zero residuals, and Ad(M) weighs them differently.)"""
    fwd, rev = pc.consistent_pair()
    a, b = rpg.pose_graph(fwd, 22), rpg.pose_graph(rev, 22)
    assert a["chi2_before"] > 1e-3 and b["chi2_before"] > 1e-3 and a["chi2_after"] < 1e-20 and b["chi2_after"] < 1e-20
    d = pc.diffs(dict(a, trace=np.zeros((0, 6))), dict(b, trace=np.zeros((0, 6))))
    assert d["t"] <= pc.TOL_SMALL["t"] and d["q"] <= pc.TOL_SMALL["q"], d
    ra, rb = pc.reference22("reversed_all"), rpg.pose_graph(pc.base_graph(pts="one"), 22)
    assert pc.diffs(dict(ra, trace=np.zeros((0, 6))), dict(rb, trace=np.zeros((0, 6))))["t"] > 1e-3      # the noisy pair: different optima


def test_numeric_and_analytic_jacobians_give_the_same_optimisation():
    """recorded in DESIGN 10, not a tolerance of any other test: g2o's numeric linearisation against the closed form"""
    a, n = pc.reference("n63"), pc.reference("n63", jac_mode="numeric")
    assert np.array_equal(a["trace"][:, 5], n["trace"][:, 5])
    d = pc.diffs(n, a)
    print("numeric vs analytic Jacobians, n63:", d)
    assert d["t"] < 1e-4 and d["q"] < 1e-5
