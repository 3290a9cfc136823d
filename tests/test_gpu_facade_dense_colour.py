"""facade::DenseReconstruction on colour input (`is_color_input: 1`, what every dense config of the reference says): a
KITTI-layout sequence of two colour PNGs per camera (image_2 / image_3) and a hand-written keyframes.txt of two keyframes 5 cm
apart go through the unchanged driver tests/cpp/facade_dense.cpp.  dense_map.pcd must hold exactly what the Python binding's chain
gives — pyramid_bgr -> dense_cloud_bgr -> cloud_sor per keyframe -> merge -> cloud_sor -> cloud_voxel_grid — coordinates bit
for bit, rgb = r << 16 | g << 8 | b of the left image's pixel.  The same files with `is_color_input: 0` give the grey chain's
file (pyramid of the numpy grey, r = g = b): the behaviour before colour existed.

The conditions on the inputs (clouds not empty, each outlier removal removes some and not all, fewer voxels than points,
colours that are not grey) are asserted on tests/ref_cloud_filters.py's numbers as well as on the device's."""
import os
import subprocess

import numpy as np
import pytest

import ref_cloud_filters as rcf
import ref_colour as rc
from colour_cases import DEC_DOWN, DEC_UP, stereo_pair, write_png
from test_facade_dense import _build, _pose_from_record, _read_pcd

B = 0.537166
RECORDS = ["0 1 0 0 0 0 1 0 0 0 0 1 0", "1 1 0 0 0.05 0 1 0 0 0 0 1 0"]         # identity, a 5 cm step


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("facade_dense_colour"), "facade_dense")


def _sequence(root, case):
    (sw, sh), (w, h), disp, _ = case
    seq = os.path.join(root, "sequences", "00")
    os.makedirs(os.path.join(seq, "image_2")); os.makedirs(os.path.join(seq, "image_3"))
    fx, cx, cy = 718.856 * w / 620.0, float(w), float(h)                          # halved by Dataset: fx 718.856 * 0.5 * w / 620, the centre
    P = lambda tx: "%.12e 0 %.12e %.12e 0 %.12e %.12e 0 0 0 1 0" % (fx, cx, tx, fx, cy)
    with open(os.path.join(seq, "calib.txt"), "w") as f:
        f.write("P0: " + P(0.0) + "\nP1: " + P(-fx * B) + "\nP2: " + P(0.0) + "\nP3: " + P(-fx * B) + "\n")
    frames = []
    for i in range(2):
        l, r = stereo_pair(31 + i, (sw, sh), disp)
        write_png(os.path.join(seq, "image_2", "%06d.png" % i), l[:, :, ::-1], (0, 1, 2, 3, 4))       # the file holds r, g, b
        write_png(os.path.join(seq, "image_3", "%06d.png" % i), r[:, :, ::-1], (4, 0))
        frames.append((l, r))
    kf = os.path.join(root, "keyframes.txt")
    with open(kf, "w") as f:
        f.write(seq + "\n2\n" + "\n".join(RECORDS) + "\n")
    fxp = float("%.12e" % fx); txp = float("%.12e" % (-fx * B))
    cam = (0.5 * fxp, 0.5 * fxp, 0.5 * float("%.12e" % cx), 0.5 * float("%.12e" % cy))
    return kf, frames, cam, abs(txp / fxp)


def _run(exe, root, kf, colour, filters):
    name = "c%d_f%d" % (colour, filters)
    out_dir = os.path.join(root, name); os.makedirs(out_dir)
    cfg = os.path.join(root, name + ".yaml")
    open(cfg, "w").write("%YAML:1.0\nslam_output_dir: \"" + kf + "\"\nleft_cam_index: 2\nright_cam_index: 3\nis_color_input: " + str(colour) +
                         "\noutput_dir: " + out_dir + "\ncloud_filters: " + str(filters) + "\n")
    r = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dense ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Leaf size is too small" not in r.stderr
    xyz, rgb = _read_pcd(os.path.join(out_dir, "dense_map.pcd"))
    assert ("points %d " % len(xyz)) in r.stdout
    return xyz, rgb


def _pack(bgr):
    b = bgr.astype(np.uint32)
    return (b[:, 2] << 16) | (b[:, 1] << 8) | b[:, 0]


def _chain(svs, case, frames, cam, baseline, colour):
    """per keyframe (xyz, bgr) of the binding, then the filtered merge; the yardstick's conditions on the way"""
    (sw, sh), (w, h), _, _ = case
    c = svs.Context(w, h, max_slots=2, max_jobs=2, max_pts=8, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
    try:
        raw, kept = [], []
        for rec, (l, r) in zip(RECORDS, frames):
            T = _pose_from_record(rec.split()[1:])
            if colour:
                c.colour_reserve(1)
                c.pyramid_bgr([0, 1], [0, -1], [l, r])
                (pts, pix, bgr, _), = c.dense_cloud_bgr([(0, 1, 0, T)], cam, svs.IDENT, baseline)
                assert np.array_equal(bgr, rc.prepare(l, w, h)[1].reshape(-1, 3)[pix])
            else:
                gl, gr = rc.decimate(rc.grey_from_bgr(l), w, h), rc.decimate(rc.grey_from_bgr(r), w, h)
                c.pyramid([0, 1], [gl, gr])
                (pts, pix, _), = c.dense_cloud([(0, 1, T)], cam, svs.IDENT, baseline)
                bgr = np.repeat(gl.reshape(-1)[pix][:, None], 3, 1)
            assert len(pts) > 500
            (keep, _, _), = c.cloud_sor([pts])
            ykeep, _, _ = rcf.sor(pts)
            assert np.array_equal(keep, ykeep) and 0 < ykeep.sum() < len(ykeep)
            raw.append((pts, bgr)); kept.append((pts[keep], bgr[keep]))
        mx, mb = np.concatenate([k[0] for k in kept]), np.concatenate([k[1] for k in kept])
        (keep, _, _), = c.cloud_sor([mx])
        ykeep, _, _ = rcf.sor(mx)
        assert np.array_equal(keep, ykeep) and 0 < ykeep.sum() < len(ykeep)
        wx, wb, over = c.cloud_voxel_grid(mx[keep], mb[keep], 0.02)
        yx, yb, _ = rcf.voxel_grid(mx[keep], mb[keep], 0.02)
        assert not over and np.array_equal(wx, yx) and np.array_equal(wb, yb) and 0 < len(yx) < int(keep.sum())
        if colour:
            assert ((yb[:, 0] != yb[:, 1]) | (yb[:, 1] != yb[:, 2])).any()
    finally:
        c.close()
    return (np.concatenate([k[0] for k in raw]), np.concatenate([k[1] for k in raw])), (wx, wb)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [DEC_DOWN, DEC_UP], ids=["401x121", "403x123"])
def test_coloured_dense_map_equals_the_python_chain(svs, exe, tmp_path, case):
    root = str(tmp_path)
    kf, frames, cam, baseline = _sequence(root, case)
    (ux, ub), (fx_, fb) = _chain(svs, case, frames, cam, baseline, True)
    for filters, (wx, wb) in ((0, (ux, ub)), (1, (fx_, fb))):
        xyz, rgb = _run(exe, root, kf, 1, filters)
        assert len(xyz) == len(wx) and xyz.tobytes() == wx.tobytes(), filters
        assert np.array_equal(rgb, _pack(wb)), filters
        r, g, b = (rgb >> 16) & 0xff, (rgb >> 8) & 0xff, rgb & 0xff
        assert ((r != g) | (g != b)).any() and (rgb >> 24 == 0).all()
    # the same files read grey: the file this program wrote before it knew colour
    (gx, gb), (gfx, gfb) = _chain(svs, case, frames, cam, baseline, False)
    for filters, (wx, wb) in ((0, (gx, gb)), (1, (gfx, gfb))):
        xyz, rgb = _run(exe, root, kf, 0, filters)
        assert len(xyz) == len(wx) and xyz.tobytes() == wx.tobytes(), filters
        assert (wb[:, 0] == wb[:, 1]).all() and (wb[:, 0] == wb[:, 2]).all()
        g = wb[:, 0].astype(np.uint32)
        assert np.array_equal(rgb, (g << 16) | (g << 8) | g), filters
