"""The host glue of the loop verification (Pipeline::VerifyLoops, KeyframeFeatures, Map::ArchiveIndex, the keep-features switch) on a
scripted map: tests/cpp/loop_verify_host.cpp, a stand-alone program whose kernel provider is csrc/k_loop_verify.h compiled for the
host.  Every refusal leaves the map untouched; live and archived landmarks are both gathered and mp == -1 is dropped; one provider
call for several streams; an ACCEPTED pair is exactly one more edge of a following PoseGraphOptimization and a rejected one is not;
the device_map refusal.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_verify_host_cpp(tmp_path):
    exe = str(tmp_path / "loop_verify_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "loop_verify_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all loop-verify host tests passed" in r.stdout
