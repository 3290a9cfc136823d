"""The host glue of the loop-closure descriptors (Pipeline::DescribeNewKeyframes, KeyframeDescriptors, VerifyLoopsStored, Frame::desc) on
a scripted map: tests/cpp/brief_host.cpp, a stand-alone program whose kernel provider is csrc/k_brief.h (and k_loop_verify.h) compiled
for the host.  The non-outlier features are selected in their order, desc_feat_indx names each row's own feature (also for two
features at one pixel), one provider call serves all streams with a new keyframe, a refusal stores nothing, stored descriptors survive
the keyframe leaving the window, VerifyLoopsStored refuses a keyframe that was never described but not one described with zero rows,
and an accepted stored pair is a loop edge.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brief_host_cpp(tmp_path):
    exe = str(tmp_path / "brief_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "brief_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all descriptor host tests passed" in r.stdout
