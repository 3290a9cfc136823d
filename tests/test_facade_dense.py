"""facade::DenseReconstruction (host/slam_facade.h), the reference's second program: a 6-frame KITTI-layout sequence goes
through the SLAM facade (VisualOdometry, `facade_dense --slam`), then facade::DenseReconstruction reads its keyframes.txt and
writes dense_map.pcd (tests/cpp/facade_dense.cpp).  The file must hold exactly what Context.dense_cloud gives for the same
decimated frames and float-rounded poses, concatenated in keyframe order.  GPU only: the facade is bound to the HIP kernels (there is no C twin of the block
matcher to bind it to)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX, CX, CY, B = 718.856, 607.1928, 185.2157, 0.537166          # KITTI-00 calibration
W, H = 1241, 376


def _png_gray(path, img):
    h, w = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img], 1).tobytes()

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def _make_sequence(svs, root, seed, nframes):
    seq = os.path.join(root, "sequences", "00")
    os.makedirs(os.path.join(seq, "image_0")); os.makedirs(os.path.join(seq, "image_1"))
    P = lambda tx: "%.12e 0 %.12e %.12e 0 %.12e %.12e 0 0 0 1 0" % (FX, CX, tx, FX, CY)
    with open(os.path.join(seq, "calib.txt"), "w") as f:
        f.write("P0: " + P(0.0) + "\nP1: " + P(-FX * B) + "\nP2: " + P(0.0) + "\nP3: " + P(-FX * B) + "\n")
    frames = []
    for i in range(nframes):
        l, r = svs.synth_pair(seed, i, w=W, h=H, cam=(FX, FX, CX, CY), baseline=B)
        _png_gray(os.path.join(seq, "image_0", "%06d.png" % i), l)
        _png_gray(os.path.join(seq, "image_1", "%06d.png" % i), r)
        frames.append((l, r))
    cfg = os.path.join(root, "config.yaml")
    with open(cfg, "w") as f:
        f.write("%YAML:1.0\ndataset_dir: \"" + seq + "\"\nleft_cam_index: 0\nright_cam_index: 1\nis_color_input: 0\noutput_dir: " + root +
                "\nnum_features: 150\nnum_features_init: 50\nnum_features_tracking: 50\nnum_features_tracking_bad: 20\n"
                "num_features_needed_for_keyframe: 80\nmax_triangulation_depth: 300.0\nkeypoint_feature_detector: GFTT\n"
                "num_active_keyframes: 10\nbackend_on: 1\nchi2_th: 5.991\nloopclosure_on: 0\nvisualizer_on: 0\n")
    return cfg, seq, frames


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
    subprocess.check_call(["g++", "-O3", "-march=native", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib,
                           "-o", exe, "-lz", "-lm"])
    return exe


def _pose_from_record(vals):
    """Sophus::SE3f(T).cast<double>() as facade::se3_from_float_rows states it: the twelve numbers as floats, Eigen's
    matrix-to-quaternion branches IN FLOAT on them, the quaternion widened and normalised in double (the same + - * / sqrt
    in the same order and precision: the same bits)"""
    f = np.float32
    m = [f(v) for v in vals]
    R = [[m[0], m[1], m[2]], [m[4], m[5], m[6]], [m[8], m[9], m[10]]]
    q = [f(0)] * 4
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        t = np.sqrt(t + f(1)); q[3] = f(0.5) * t; t = f(0.5) / t
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]: i = 1
        if R[2][2] > R[i][i]: i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(R[i][i] - R[j][j] - R[k][k] + f(1)); q[i] = f(0.5) * t; t = f(0.5) / t
        q[3], q[j], q[k] = (R[k][j] - R[j][k]) * t, (R[j][i] + R[i][j]) * t, (R[k][i] + R[i][k]) * t
    assert all(type(v) is np.float32 for v in q)
    q = [np.float64(v) for v in q]
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([q[0] / n, q[1] / n, q[2] / n, q[3] / n, m[3], m[7], m[11]], np.float64)


def _read_pcd(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"DATA binary\n", 1)
    lines = head.decode().splitlines()
    assert lines[0].startswith("# .PCD v0.7") and "FIELDS x y z rgb" in lines and "SIZE 4 4 4 4" in lines and "HEIGHT 1" in lines
    n = int([l for l in lines if l.startswith("POINTS")][0].split()[1])
    assert int([l for l in lines if l.startswith("WIDTH")][0].split()[1]) == n and len(body) == 16 * n
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgb", "<u4")]))
    return rec["xyz"].copy(), rec["rgb"].copy()


@pytest.mark.gpu
def test_dense_map_of_a_slam_run_equals_the_python_binding(svs, tmp_path):
    root = str(tmp_path)
    cfg, seq, frames = _make_sequence(svs, root, 42, 6)
    exe = _build(tmp_path, "facade_dense")
    r = subprocess.run([exe, "--slam", cfg, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "slam ok" in r.stdout and "frames 6" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    kf_path = os.path.join(root, "keyframes.txt")
    recs = [l.split() for l in open(kf_path).read().splitlines()[2:]]
    assert len(recs) >= 1 and all(len(x) == 13 for x in recs)
    dcfg = os.path.join(root, "dense.yaml")
    out_dir = os.path.join(root, "dense"); os.makedirs(out_dir)
    open(dcfg, "w").write("%YAML:1.0\nslam_output_dir: \"" + kf_path + "\"\nleft_cam_index: 0\nright_cam_index: 1\noutput_dir: " + out_dir + "\n")
    r = subprocess.run([exe, dcfg], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "dense ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    printed = [l.split() for l in r.stdout.splitlines() if l.startswith("keyframe ")]
    assert [int(x[1]) for x in printed] == [int(x[0]) for x in recs]
    poses = [_pose_from_record(x[1:]) for x in recs]
    for p, x in zip(poses, printed):
        assert np.array_equal(p, np.array([float(v) for v in x[3:10]])), (p, x)
    xyz, rgb = _read_pcd(os.path.join(out_dir, "dense_map.pcd"))
    assert ("points %d " % len(xyz)) in r.stdout

    # the same through the Python binding: frames decimated as Dataset::FrameById does, Dataset::initialize's halved K and baseline
    fx = float("%.12e" % FX); tx = float("%.12e" % (-FX * B))
    cam = (0.5 * fx, 0.5 * fx, 0.5 * float("%.12e" % CX), 0.5 * float("%.12e" % CY))
    baseline = abs(tx / fx)
    c = svs.Context(620, 188, max_slots=2, max_jobs=2, max_pts=8, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
    want_xyz, want_grey = [], []
    try:
        for x, T in zip(recs, poses):
            l, r_ = frames[int(x[0])]
            # dst(x, y) = src(2x, 2y), size (cvRound(1241 / 2), cvRound(376 / 2)) = (620, 188)
            ld, rd = np.ascontiguousarray(l[::2, ::2][:188, :620]), np.ascontiguousarray(r_[::2, ::2][:188, :620])
            c.pyramid([0, 1], [ld, rd])
            (pts, pix, _), = c.dense_cloud([(0, 1, T)], cam, svs.IDENT, baseline)
            want_xyz.append(pts); want_grey.append(ld.reshape(-1)[pix])
    finally:
        c.close()
    want_xyz = np.concatenate(want_xyz); want_grey = np.concatenate(want_grey).astype(np.uint32)
    assert len(want_xyz) > 20000 * len(recs)
    assert len(xyz) == len(want_xyz) and np.array_equal(xyz, want_xyz)
    assert np.array_equal(rgb, (want_grey << 16) | (want_grey << 8) | want_grey)
