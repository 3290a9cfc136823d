"""The facade's loop-closure path on the device (tests/cpp/facade_loop.cpp): VisualOdometry::run() over a synthetic KITTI-layout
sequence with the host-resident map; the SetLoopClosure hook records, for every keyframe from the fourth on, a loop edge to keyframe
1 whose measurement is the ground-truth relative pose; run() ends with the pose-graph optimisation when
global_pose_graph_optimization >= 1, then keyframes.txt / landmarks.pcd.  The sequence is the project's synthetic drive (the
generator has one trajectory, no out-and-back leg); the loop edges do not need a revisit because their measurements come from the
ground truth.  A last run keeps the facade's default device-resident map: run() reports the refusal and writes uncorrected files."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import test_facade_kitti as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED, NFRAMES = 43, 30


def _run(exe, cfg_text, root, tmp, name, key, loop, gt_file, device_map=0):
    d = os.path.join(tmp, name); os.makedirs(d)
    cfg = os.path.join(d, "config.yaml")
    assert "output_dir: " + root + "\n" in cfg_text
    open(cfg, "w").write(cfg_text.replace("output_dir: " + root + "\n", "output_dir: " + d + "\n") +
                         "device_map: %d\nglobal_pose_graph_optimization: %d\n" % (device_map, key))
    r = subprocess.run([exe, cfg, gt_file, str(loop)], capture_output=True, text=True, timeout=300)
    if device_map:
        return r
    assert r.returncode == 0 and "facade loop ok" in r.stdout and "map: host" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("kf ")]
    frames = np.array([int(x[3]) for x in rows]); poses = np.array([[float(v) for v in x[5:12]] for x in rows])
    return frames, poses, {f: open(os.path.join(d, f)).read() for f in ("keyframes.txt", "landmarks.pcd")}


def test_loop_edge_corrects_the_outputs_and_no_loop_changes_nothing(svs, tmp_path):
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    tmp = str(tmp_path)
    cfg, seq, frames = fk._make_sequence(svs, tmp, SEED, NFRAMES)
    gt = np.array([svs.synth_gt(SEED, f) for f in range(NFRAMES)])
    gt_file = os.path.join(tmp, "gt.txt")
    np.savetxt(gt_file, gt, fmt="%.17g")
    exe = os.path.join(tmp, "facade_loop")
    lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_loop.cpp"), "-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib,
                           "-o", exe, "-lz", "-lm"])
    text = open(cfg).read()
    f0, p0, out0 = _run(exe, text, tmp, tmp, "key0", 0, 1, gt_file)            # loop edge recorded, optimisation off
    f1, p1, out1 = _run(exe, text, tmp, tmp, "key1", 1, 1, gt_file)            # ... on
    f2, p2, out2 = _run(exe, text, tmp, tmp, "noloop", 1, 0, gt_file)          # on, but no loop edge
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2) and len(f0) >= 4
    assert out1["keyframes.txt"] != out0["keyframes.txt"] and out1["landmarks.pcd"] != out0["landmarks.pcd"]
    ate0, ate1 = pl.ate_rmse(p0, gt[f0]), pl.ate_rmse(p1, gt[f1])
    print("keyframes %d, ATE of the keyframe poses: %.6f m without, %.6f m with the optimisation" % (len(f0), ate0, ate1))
    assert ate1 < ate0
    assert np.array_equal(p1[0], p0[0])                                   # keyframe 0 is fixed
    # without a loop edge every odometry edge is satisfied exactly: chi2 = 0, nothing moves, the files are the same bytes
    assert np.array_equal(p2, p0)
    assert out2 == out0
    # the facade's default, device_map = 1: the optimisation is refused, run() says so and still writes the (uncorrected) files
    r = _run(exe, text, tmp, tmp, "devmap", 1, 0, gt_file, device_map=1)
    assert r.returncode == 0 and "map: device" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "global pose-graph optimisation not run" in r.stderr and "device" in r.stderr
    assert os.path.exists(os.path.join(tmp, "devmap", "keyframes.txt"))
