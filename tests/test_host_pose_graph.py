"""The host glue of the global pose-graph optimisation (Frame::loop_keyframe, MapPoint::anchor, Pipeline::AddLoopEdge /
PoseGraphOptimization) on a scripted map: tests/cpp/pose_graph_host.cpp with a CPU kernel provider whose pose-graph call is
csrc/k_pose_graph.h compiled for the host.  AddLoopEdge refusals, the job built, pose write-back, relative_pose_pkf refreshed,
the anchor following first_valid_obs_, archived landmarks re-anchored, the device_map refusal, the no-loop identity.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_graph_host_cpp(tmp_path):
    exe = str(tmp_path / "pose_graph_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "pose_graph_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all pose-graph host tests passed" in r.stdout
