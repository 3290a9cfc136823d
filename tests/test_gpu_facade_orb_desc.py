"""A facade run (host/slam_facade.h, HIP kernels) with `keypoint_feature_detector: ORB` and `loop_descriptors: 2`: ten frames, every
keyframe described at its keypoints' angles and octaves, outputs written.  With GFTT, `2` stores the rows `1` stores."""
import os

import pytest

import test_facade_kitti as fk
import test_facade_orb as fo
import test_facade_orb_desc as fd

pytestmark = pytest.mark.gpu
NFRAMES = 10


def kf_lines(out):
    return [l.split() for l in out.splitlines() if l.startswith("kf ")]


def test_facade_describes_orb_keyframes_at_their_angle_and_octave(svs, tmp_path):
    cfg, seq, _ = fk._make_sequence(svs, str(tmp_path), 42, NFRAMES)
    exe = fd.build(tmp_path, False)
    out_dir = str(tmp_path / "orb2")
    r = fo.run(exe, fo.config_with(cfg, "ORB", "loop_descriptors: 2\noutput_dir: " + out_dir + "\n"), out_dir)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "facade orb desc ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "map: host detector: 1" in r.stdout and "frames %d " % NFRAMES in r.stdout
    kfs = kf_lines(r.stdout)
    assert len(kfs) >= 1 and all(l[2] == "rows" and int(l[3]) > 0 for l in kfs)              # every keyframe described, with rows
    assert max(int(l[7]) for l in kfs) >= 1                                                  # some described feature is above level 0
    kf = open(os.path.join(out_dir, "keyframes.txt")).read().splitlines()
    assert kf[0] == seq and len(kf) == 2 + len(kfs)
    assert open(os.path.join(out_dir, "landmarks.pcd")).read().startswith("# .PCD v0.7")
    # GFTT on the host map (the descriptors need it): every feature is at -1 degree on level 0, so 2 stores the rows 1 stores
    runs = [fo.run(exe, fo.config_with(cfg, "GFTT", "device_map: 0\nloop_descriptors: %d\n" % v), str(tmp_path / ("gftt%d" % v))) for v in (1, 2)]
    assert all(x.returncode == 0 for x in runs), runs[0].stdout + runs[1].stdout
    assert kf_lines(runs[0].stdout) == kf_lines(runs[1].stdout) and len(kf_lines(runs[0].stdout)) >= 1
    assert all(int(l[7]) == 0 for l in kf_lines(runs[1].stdout))
