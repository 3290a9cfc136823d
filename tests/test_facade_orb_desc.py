"""`loop_descriptors: 2` in the facade's configuration file (host/slam_facade.h) on the CPU: with the oracle's kernel provider, which has
no oriented descriptors, the first keyframe is refused with the provider's message; without the key GFTT runs as before.  The device
side is tests/test_gpu_facade_orb_desc.py."""
import os
import subprocess

import test_facade_kitti as fk
import test_facade_orb as fo

ROOT = fo.ROOT


def build(tmp_path, oracle):
    exe = str(tmp_path / ("facade_orb_desc_" + ("cpu" if oracle else "hip")))
    cmd = ["g++", "-O2", "-march=native", "-ffp-contract=off", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_orb_desc.cpp")]
    if oracle:
        import oracle_lib
        oracle_lib.build()
        cmd += ["-DFACADE_ORACLE"] + [os.path.join(ROOT, "oracle", "_build", o) for o in ("orc_image.o", "orc_gftt.o", "orc_geom.o")]
    else:
        lib = os.path.join(ROOT, "stereovision-slam_amd", "lib")
        cmd += ["-L" + lib, "-lsvslam_hip", "-Wl,-rpath," + lib]
    subprocess.check_call(cmd + ["-o", exe, "-lz", "-lm"])
    return exe


def test_the_twin_provider_refuses_oriented_descriptors(svs, tmp_path):
    cfg, _, _ = fk._make_sequence(svs, str(tmp_path), 41, 2)
    exe = build(tmp_path, True)
    r = fo.run(exe, fo.config_with(cfg, "GFTT", "loop_descriptors: 2\n"), str(tmp_path / "two"))
    assert r.returncode == 3 and "threw: loop_descriptors: 2: this kernel provider has no oriented descriptors" in r.stdout, r.stdout + r.stderr
    r = fo.run(exe, fo.config_with(cfg, "GFTT", "loop_descriptors: 3\n"), str(tmp_path / "three"))
    assert r.returncode == 3 and "threw: loop_descriptors: the values are 0" in r.stdout, r.stdout + r.stderr
    r = fo.run(exe, cfg, str(tmp_path / "gftt"))                       # GFTT without the key runs as before: nothing is described
    assert r.returncode == 0 and "facade orb desc ok" in r.stdout and "detector: 0" in r.stdout and "kf 0 not described" in r.stdout, r.stdout + r.stderr
