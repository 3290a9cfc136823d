"""tests/cpp/orb_desc_host.cpp: the host build of csrc/k_orb_desc.h as a stand-alone program, compiled with -fsanitize=address,undefined
and run on generated images of awkward sizes, keypoints on every level, on both borders, outside the image and not finite, two tables,
tiny and default chunk budgets.  Every read and write of the kernels' bodies, the plan, the layout and the copy-out is checked against
the buffers' bounds; what the device does with the same code is tests/test_gpu_orb_desc.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_build_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "orb_desc_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "orb_desc_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "orb desc host ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stdout[-1000:] + r.stderr[-3000:]
