"""The facade closing the loop-detection path from the frames alone (tests/cpp/facade_gdesc.cpp): VisualOdometry::step() over a synthetic
KITTI-layout sequence with the host-resident map and `loop_global_descriptor:` pointing at a file written by gdesc.save;
VisualOdometry::DetectLoop(&out) without a vector after every step agrees with the program's books and with a twin facade that is
handed the vectors; with the key absent the overload throws and nothing else changes."""
import os
import subprocess

import pytest

import global_desc_cases as gc
import test_facade_kitti as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED, NFRAMES = 43, 30
KEYS = ("loop_min_keyframe_gap: 2\nkeyframes_to_ignore_after_loop: 1\nmin_num_acceptable_keypoint_match: 10\nloop_descriptors: 1\n"
        "loop_store_capacity: 32\npotential_loop_weak_threshold: 0.93\npotential_loop_strong_threshold: 0.95\nmax_num_weak_threshold: 3\n")


def test_detect_loop_without_a_vector_after_every_step(svs, tmp_path):
    tmp = str(tmp_path)
    cfg, seq, frames = fk._make_sequence(svs, tmp, SEED, NFRAMES)
    exe = os.path.join(tmp, "facade_gdesc")
    lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_gdesc.cpp"), "-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib,
                           "-o", exe, "-lz", "-lm"])
    layers, out_wh = gc.tiny_net()
    net = os.path.join(tmp, "net.svgd")
    gc.gdesc().save(net, layers, gc.seeded(layers, 3), gc.case_prep(out_wh))
    text = open(cfg).read()
    assert "loop_global_descriptor" not in text and "output_dir: " + tmp + "\n" in text
    for name, extra, expect in (("with", "loop_global_descriptor: %s\n" % net, 1), ("without", "", 0)):
        cs = []
        for who, more in (("a", extra), ("twin", "loop_descriptor_dim: 5\n")):
            d = os.path.join(tmp, name + "_" + who); os.makedirs(d)
            cs.append(os.path.join(d, "config.yaml"))
            open(cs[-1], "w").write(text.replace("output_dir: " + tmp + "\n", "output_dir: " + d + "\n") + "device_map: 0\n" + KEYS + more)
        r = subprocess.run([exe, cs[0], cs[1], str(expect)], capture_output=True, text=True, timeout=300)
        print(r.stdout[-400:])
        assert r.returncode == 0 and "facade gdesc ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("refused without" in r.stdout) == (expect == 0)
