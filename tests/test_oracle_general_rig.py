"""CPU: the oracle on a general stereo rig — rotated extrinsics on both cameras, fx != fy, cam_l != cam_r
(common.GENERAL_RIG) — pinned against numpy before any kernel is held to it (tests/test_gpu_general_rig.py), and
the two quaternions of an identity rotation, which the GPU tests use to select the general-extrinsics kernels."""
import hashlib

import numpy as np
import pytest

import common as cm


def test_make_ba_problem_without_a_rig_is_unchanged():
    """rig=None draws from the RNG in the order it always did: every older test sees the problem it always saw"""
    p = cm.make_ba_problem(np.random.default_rng(33), 7, 300)
    h = hashlib.sha256()
    for k in ("poses", "pts", "poses0", "pts0", "okf", "olm", "ori", "ouv"):
        a = np.ascontiguousarray(p[k])
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    assert h.hexdigest() == "1a98248e5d8f0d3d4cb5cc3c2f1d0aa1e2bb18417730a682adeb4fef892e23c9"
    q = cm.make_ba_problem(np.random.default_rng(33), 7, 300, rig=cm.KITTI_RIG)
    assert all(np.array_equal(p[k], q[k]) for k in p)


def test_general_rig_is_general():
    cam_l, ext_l, cam_r, ext_r = cm.GENERAL_RIG
    assert cam_l[0] != cam_l[1] and cam_r[0] != cam_r[1] and tuple(cam_l) != tuple(cam_r)
    for e in (ext_l, ext_r):
        R = cm.quat_R(e[:4])
        assert e.dtype == np.float64 and abs(np.linalg.norm(e[:4]) - 1) < 1e-15
        assert (np.abs(R) > 1e-3).all() and np.abs(R - R.T).max() > 1e-2        # no zero entry, visibly not symmetric
    for e in cm.KITTI_RIG_NEG_W[1::2]:
        assert e[3] == -1.0 and np.array_equal(cm.quat_R(e[:4]), np.eye(3))


@pytest.mark.parametrize("nkf,nlm", [(7, 300), (4, 7)])
def test_local_ba_on_the_general_rig(orc, nkf, nlm):
    rng = np.random.default_rng(40 + nkf)
    # 7 landmarks carry no gross outlier, as in the low-latency tests this size comes from: with one, four keyframes hang on
    # five or six points, the poses wander by metres, and on EITHER rig the two linearisations end 2e-4 - 6e-4 apart
    p = cm.make_ba_problem(rng, nkf, nlm, rig=cm.GENERAL_RIG, **(dict(outlier_frac=0.0) if nlm < 50 else {}))
    job = cm.ba_job(p)
    assert len(job[2]) >= 2 * nlm and set(job[4]) == {0, 1}
    pa, xa, ca, ia = orc.local_ba(*cm.GENERAL_RIG, *job, jac_mode=0)
    # the per-edge chi2 is the reprojection through each edge's own camera, recomputed in numpy at the result
    assert np.allclose(cm.reproj_chi2(cm.GENERAL_RIG, pa, xa, *job[2:]), ca, rtol=1e-9, atol=1e-12)
    c0 = cm.reproj_chi2(cm.GENERAL_RIG, *job)                  # the same at the start
    # ... and not the reprojection through the other rig: the rig matters to the answer
    assert np.median(cm.reproj_chi2(cm.KITTI_RIG, pa, xa, *job[2:])) > 20 * np.median(ca)
    assert ia >= 3 and cm.huber(ca) < cm.huber(c0)
    # numeric Jacobians (g2o's linearisation): the gauge-invariant quantities at 1e-4, as on the KITTI rig
    pn, xn, cn, _ = orc.local_ba(*cm.GENERAL_RIG, *job, jac_mode=1)
    rel = lambda P: np.array([orc.se3_mul(P[k], orc.se3_inv(P[0])) for k in range(len(P))])
    assert np.allclose(rel(pa), rel(pn), atol=1e-4)
    assert abs(ca.sum() - cn.sum()) <= 1e-4 * cn.sum()


def test_triangulation_on_the_general_rig(orc):
    """noise-free points come back within the f32-pixel bound: twice what the same points give on the KITTI rig"""
    rng = np.random.default_rng(6)
    n = 200
    P = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2.5, 1.5, n), rng.uniform(4, 60, n)], 1)
    ident = cm.EXT_L
    err = {}
    for name, rig in (("kitti", cm.KITTI_RIG), ("general", cm.GENERAL_RIG)):
        cam_l, ext_l, cam_r, ext_r = rig
        uvl = cm.project(cam_l, ident, ext_l, P)[0].astype(np.float32)
        uvr = cm.project(cam_r, ident, ext_r, P)[0].astype(np.float32)
        xyz, ok = orc.triangulate(*rig, uvl, uvr)
        assert ok.all(), name
        err[name] = np.linalg.norm(xyz - P, axis=1).max()
        _, ok_sw = orc.triangulate(*rig, uvr, uvl)                 # swapped -> negative depth
        assert ok_sw.sum() == 0, name
        T = cm.random_pose(rng)
        xyz_w, ok_w = orc.triangulate(*rig, uvl, uvr, T_wc=T, zmax=30.0)
        assert np.allclose(xyz_w, xyz @ cm.quat_R(T[:4]).T + T[4:], atol=1e-10)
        assert np.array_equal(ok_w > 0, xyz[:, 2] <= 30.0)
    print("triangulation error, max over %d points: %s" % (n, err))
    assert err["general"] <= 2 * err["kitti"]


def test_pose_only_with_fx_not_fy(orc):
    cam = cm.GENERAL_RIG[0]
    rng = np.random.default_rng(21)
    for n in (230, 64, 400, 257, 512, 130):
        T_true, P, uv = cm.pose_problem(rng, n, cam)
        T, outl, ninl = orc.pose_only(cam, cm.EXT_L, P, uv)
        assert ninl == n - outl.sum() and 0.75 * n <= ninl
        assert np.linalg.norm(T[4:] - T_true[4:]) < 0.05, n
        # the same pixels read with fy = fx are another problem: the truth is not its answer
        T_k, _, ninl_k = orc.pose_only(cm.CAM, cm.EXT_L, P, uv)
        assert np.linalg.norm(T_k[4:] - T_true[4:]) > 0.05 or ninl_k < ninl, n


def test_quaternion_sign_of_an_identity_extrinsic_changes_no_bit(orc):
    """q and -q are one rotation; for the identity both give exactly the identity matrix, so the oracle's answers are equal
    bit for bit — the GPU tests pass (0,0,0,-1) to reach the general-extrinsics kernels on the reference's rig"""
    for seed, nkf, nlm in ((50, 7, 300), (51, 4, 7)):
        job = cm.ba_job(cm.make_ba_problem(np.random.default_rng(seed), nkf, nlm))
        a = orc.local_ba(*cm.KITTI_RIG, *job, jac_mode=0)
        b = orc.local_ba(*cm.KITTI_RIG_NEG_W, *job, jac_mode=0)
        assert a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
