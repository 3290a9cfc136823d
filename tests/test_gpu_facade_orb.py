"""A facade run (host/slam_facade.h, HIP kernels) of a reference-style configuration with `keypoint_feature_detector: ORB`: it selects
the host map, tracks, inserts keyframes and writes keyframes.txt and landmarks.pcd; ORB with `loop_descriptors: 1` throws."""
import os

import pytest

import test_facade_kitti as fk
import test_facade_orb as fo

pytestmark = pytest.mark.gpu
NFRAMES = 10


def test_facade_runs_an_orb_configuration(svs, tmp_path):
    cfg, seq, _ = fk._make_sequence(svs, str(tmp_path), 42, NFRAMES)
    exe = fo.build(tmp_path, False)
    out_dir = str(tmp_path / "orb")
    r = fo.run(exe, fo.config_with(cfg, "ORB", "output_dir: " + out_dir + "\n"), out_dir)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "facade orb ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "map: host detector: 1" in r.stdout
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("frame ")]
    assert len(rows) == NFRAMES and all(int(x[3]) in (1, 2) for x in rows) and int(rows[0][5]) == 1      # tracking, frame 0 a keyframe
    assert all(int(x[7]) > 0 for x in rows)
    kf = open(os.path.join(out_dir, "keyframes.txt")).read().splitlines()
    assert kf[0] == seq and len(kf) == 2 + sum(int(x[5]) for x in rows)
    assert open(os.path.join(out_dir, "landmarks.pcd")).read().startswith("# .PCD v0.7")
    r = fo.run(exe, fo.config_with(cfg, "ORB", "loop_descriptors: 1\n"), str(tmp_path / "orbloop"))
    assert r.returncode == 3 and "ORB with loop_descriptors: 1" in r.stdout, r.stdout + r.stderr
    r = fo.run(exe, fo.config_with(cfg, "FOO"), str(tmp_path / "foo"))
    assert r.returncode == 3 and "threw: Only the GFTT" in r.stdout, r.stdout + r.stderr
