"""The facade's loop-closure descriptors on the device (tests/cpp/facade_brief.cpp): VisualOdometry::run() over a synthetic KITTI-layout
sequence with the host-resident map.  With `loop_descriptors: 1` every keyframe is described and VerifyLoop(kf, cand, out) gives what
the explicit-descriptor overload gives when fed KeyframeDescriptors; with the key absent nothing is described, Frame::desc stays empty
and the overload without descriptors is refused."""
import os
import subprocess

import pytest

import test_facade_kitti as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED, NFRAMES = 43, 30


def test_verify_loop_on_stored_descriptors(svs, tmp_path):
    tmp = str(tmp_path)
    cfg, seq, frames = fk._make_sequence(svs, tmp, SEED, NFRAMES)
    exe = os.path.join(tmp, "facade_brief")
    lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_brief.cpp"), "-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib,
                           "-o", exe, "-lz", "-lm"])
    text = open(cfg).read()
    assert "loop_descriptors" not in text and "output_dir: " + tmp + "\n" in text
    for name, extra, expect in (("with", "loop_descriptors: 1\n", 1), ("without", "", 0)):
        d = os.path.join(tmp, name); os.makedirs(d)
        c = os.path.join(d, "config.yaml")
        open(c, "w").write(text.replace("output_dir: " + tmp + "\n", "output_dir: " + d + "\n") + "device_map: 0\n" + extra)
        r = subprocess.run([exe, c, str(expect)], capture_output=True, text=True, timeout=300)
        print(r.stdout[-400:])
        assert r.returncode == 0 and "facade brief ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("nothing described" in r.stdout) == (expect == 0)
