"""`keypoint_feature_detector` in the facade's configuration file (host/slam_facade.h) on the CPU: with the oracle's kernel provider,
which has no ORB detector, `ORB` is refused with the provider's message at the first frame; any value other than GFTT and ORB throws as
it always did.  The device side of ORB is tests/test_gpu_facade_orb.py."""
import os
import subprocess

import test_facade_kitti as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, oracle):
    exe = str(tmp_path / ("facade_orb_" + ("cpu" if oracle else "hip")))
    cmd = ["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_orb.cpp")]
    if oracle:
        import oracle_lib
        oracle_lib.build()
        cmd += ["-DFACADE_ORACLE"] + [os.path.join(ROOT, "oracle", "_build", o) for o in ("orc_image.o", "orc_gftt.o", "orc_geom.o")]
    else:
        lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
        cmd += ["-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib]
    subprocess.check_call(cmd + ["-o", exe, "-lz", "-lm"])
    return exe


def config_with(cfg, detector, extra=""):
    """the sequence's configuration file with another detector (and further keys)"""
    txt = open(cfg).read()
    assert "keypoint_feature_detector: GFTT\n" in txt
    out = cfg[:-5] + "_" + detector + (str(abs(hash(extra)) % 1000) if extra else "") + ".yaml"
    open(out, "w").write(txt.replace("keypoint_feature_detector: GFTT\n", "keypoint_feature_detector: " + detector + "\n") + extra)
    return out


def run(exe, cfg, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    return subprocess.run([exe, cfg, out_dir], capture_output=True, text=True, timeout=600)


def test_the_twin_provider_refuses_orb_and_other_values_throw(svs, tmp_path):
    cfg, _, _ = fk._make_sequence(svs, str(tmp_path), 41, 2)
    exe = build(tmp_path, True)
    r = run(exe, config_with(cfg, "ORB"), str(tmp_path / "orb"))
    assert r.returncode == 3 and "threw: " in r.stdout and "this kernel provider has no ORB detector" in r.stdout, r.stdout + r.stderr
    r = run(exe, config_with(cfg, "FOO"), str(tmp_path / "foo"))
    assert r.returncode == 3 and "threw: Only the GFTT" in r.stdout and "on the GPU path" in r.stdout, r.stdout + r.stderr
    r = run(exe, config_with(cfg, "ORB", "loop_descriptors: 1\n"), str(tmp_path / "orbloop"))
    assert r.returncode == 3 and "ORB with loop_descriptors: 1" in r.stdout, r.stdout + r.stderr
    r = run(exe, cfg, str(tmp_path / "gftt"))                          # GFTT runs as before
    assert r.returncode == 0 and "facade orb ok" in r.stdout and "detector: 0" in r.stdout, r.stdout + r.stderr
