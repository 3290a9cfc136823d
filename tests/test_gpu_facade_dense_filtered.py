"""facade::DenseReconstruction with `cloud_filters: 1` in the dense config: the reference's whole second program — StereoBM and
back-projection per keyframe, pcl::StatisticalOutlierRemoval on every keyframe cloud, the merge, the outlier removal once more,
the 2 cm voxel grid, dense_map.pcd.  The file must hold exactly what the Python binding's chain gives (dense_cloud -> cloud_sor
per keyframe -> merge -> cloud_sor -> cloud_voxel_grid), and fewer points than the unfiltered run of tests/test_facade_dense.py's
sequence.  The driver is the unchanged tests/cpp/facade_dense.cpp."""
import os
import subprocess

import numpy as np
import pytest

from test_facade_dense import B, CX, CY, FX, _build, _make_sequence, _pose_from_record, _read_pcd


@pytest.mark.gpu
def test_filtered_dense_map_equals_the_python_chain(svs, tmp_path):
    root = str(tmp_path)
    cfg, seq, frames = _make_sequence(svs, root, 42, 6)
    exe = _build(tmp_path, "facade_dense")
    r = subprocess.run([exe, "--slam", cfg, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "slam ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    kf_path = os.path.join(root, "keyframes.txt")
    recs = [l.split() for l in open(kf_path).read().splitlines()[2:]]
    assert len(recs) >= 1
    clouds = {}
    for flag in (0, 1):
        out_dir = os.path.join(root, "dense%d" % flag); os.makedirs(out_dir)
        dcfg = os.path.join(root, "dense%d.yaml" % flag)
        open(dcfg, "w").write("%YAML:1.0\nslam_output_dir: \"" + kf_path + "\"\nleft_cam_index: 0\nright_cam_index: 1\noutput_dir: " + out_dir +
                              "\ncloud_filters: " + str(flag) + "\n")
        r = subprocess.run([exe, dcfg], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "dense ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        clouds[flag] = _read_pcd(os.path.join(out_dir, "dense_map.pcd"))
        assert ("points %d " % len(clouds[flag][0])) in r.stdout
        # a map of a few metres across is far below PCL's index guard: no warning
        assert "Leaf size is too small" not in r.stderr
    xyz, rgb = clouds[1]
    assert 0 < len(xyz) < len(clouds[0][0])

    fx = float("%.12e" % FX); tx = float("%.12e" % (-FX * B))
    cam = (0.5 * fx, 0.5 * fx, 0.5 * float("%.12e" % CX), 0.5 * float("%.12e" % CY))
    baseline = abs(tx / fx)
    c = svs.Context(620, 188, max_slots=2, max_jobs=2, max_pts=8, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
    try:
        kx, kg, raw = [], [], 0
        for x in recs:
            l, r_ = frames[int(x[0])]
            ld, rd = np.ascontiguousarray(l[::2, ::2][:188, :620]), np.ascontiguousarray(r_[::2, ::2][:188, :620])
            c.pyramid([0, 1], [ld, rd])
            (pts, pix, _), = c.dense_cloud([(0, 1, _pose_from_record(x[1:]))], cam, svs.IDENT, baseline)
            (keep, _, thr), = c.cloud_sor([pts])
            assert 0 < keep.sum() < len(keep) and thr > 0
            raw += len(pts)
            kx.append(pts[keep]); kg.append(ld.reshape(-1)[pix][keep])
        mx, mg = np.concatenate(kx), np.concatenate(kg)
        (keep, _, _), = c.cloud_sor([mx])
        assert not keep.all()
        wx, wrgb, over = c.cloud_voxel_grid(mx[keep], np.repeat(mg[keep][:, None], 3, 1), 0.02)
    finally:
        c.close()
    assert not over and raw == len(clouds[0][0])
    assert (wrgb[:, 0] == wrgb[:, 1]).all() and (wrgb[:, 0] == wrgb[:, 2]).all()
    g = wrgb[:, 0].astype(np.uint32)
    assert len(xyz) == len(wx) and np.array_equal(xyz, wx)
    assert np.array_equal(rgb, (g << 16) | (g << 8) | g)
