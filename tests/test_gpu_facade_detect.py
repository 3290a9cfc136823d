"""The facade's loop detection on the device (tests/cpp/facade_detect.cpp): VisualOdometry::step() over a synthetic KITTI-layout sequence
with the host-resident map, and VisualOdometry::DetectLoop after every step with planted global descriptors.  With `loop_descriptors: 1`
every result agrees with the program's own books (skip rule, compared rows, candidate, verification equal to VerifyLoop's, loop edge,
store); with the key absent DetectLoop is refused and nothing else changes."""
import os
import subprocess

import pytest

import test_facade_kitti as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED, NFRAMES = 43, 30
KEYS = ("loop_min_keyframe_gap: 2\nkeyframes_to_ignore_after_loop: 1\nmin_num_acceptable_keypoint_match: 10\nloop_descriptor_dim: 64\n"
        "loop_store_capacity: 32\npotential_loop_weak_threshold: 0.93\npotential_loop_strong_threshold: 0.95\nmax_num_weak_threshold: 3\n")


def test_detect_loop_after_every_step(svs, tmp_path):
    tmp = str(tmp_path)
    cfg, seq, frames = fk._make_sequence(svs, tmp, SEED, NFRAMES)
    exe = os.path.join(tmp, "facade_detect")
    lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_detect.cpp"), "-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib,
                           "-o", exe, "-lz", "-lm"])
    text = open(cfg).read()
    assert "loop_descriptors" not in text and "output_dir: " + tmp + "\n" in text
    for name, extra, expect in (("with", "loop_descriptors: 1\n", 1), ("without", "", 0)):
        d = os.path.join(tmp, name); os.makedirs(d)
        c = os.path.join(d, "config.yaml")
        open(c, "w").write(text.replace("output_dir: " + tmp + "\n", "output_dir: " + d + "\n") + "device_map: 0\n" + KEYS + extra)
        r = subprocess.run([exe, c, str(expect)], capture_output=True, text=True, timeout=300)
        print(r.stdout[-400:])
        assert r.returncode == 0 and "facade detect ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("refused without" in r.stdout) == (expect == 0)
