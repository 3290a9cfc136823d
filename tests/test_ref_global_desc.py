"""tests/ref_global_desc.py and stereovision-slam_amd/gdesc.py on their own, without a device: the reference's prep on hand-checked
values, MobileNetV2's table, the folding of convolution + BatchNorm against both evaluated in float64, the file round trip."""
import numpy as np
import torch
import torch.nn.functional as F

import global_desc_cases as gc
import ref_global_desc as rg

gd = gc.gdesc()


def test_blur_keeps_a_constant_image_and_sums_to_one():
    assert int(rg.TAPS.sum()) == 256
    for v in (0, 1, 127, 255):
        assert np.array_equal(rg.blur(np.full((4, 6), v, np.uint8)), np.full((4, 6), v, np.uint8))
    im = np.zeros((9, 9), np.uint8); im[4, 4] = 255
    b = rg.blur(im).astype(np.int64)
    assert b[4, 4] == (255 * 72 * 72 + 32768) >> 16 and b[4, 1] == (255 * 72 * 8 + 32768) >> 16 and b[0, 4] == 0


def test_blur_reflects_without_repeating_the_edge():
    im = np.zeros((4, 4), np.uint8); im[:, 3] = 255                       # reflect-101 at radius 3 reaches column 0 from column 3
    hs_edge = 255 * (72 + 0)                                              # column 3: taps at 0 .. 6 -> columns 0 1 2 3 2 1 0
    assert rg.blur(im)[0, 3] == (256 * hs_edge + 32768) >> 16
    hs0 = 255 * (8 + 8)                                                   # column 0: columns 3 2 1 0 1 2 3
    assert rg.blur(im)[0, 0] == (256 * hs0 + 32768) >> 16


def test_resize_axis_tables():
    s, s1, c0, c1 = rg.axis(4, 8)                                         # upsampling by 2: f = -0.25, 0.25, 0.75, ...
    assert s.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and s1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert c1.tolist() == [0, 512, 1536, 512, 1536, 512, 1536, 0] and (c0 + c1 == 2048).all()
    s, s1, c0, c1 = rg.axis(8, 4)                                         # downsampling by 2: always half way
    assert s.tolist() == [0, 2, 4, 6] and c0.tolist() == [1024] * 4 and c1.tolist() == [1024] * 4
    im = np.arange(64, dtype=np.uint8).reshape(8, 8)
    assert rg.resize(im, 8, 8).tolist() == im.tolist()
    assert rg.resize(np.full((5, 9), 200, np.uint8), 13, 7).tolist() == np.full((7, 13), 200).tolist()


def test_blob_is_the_reference_s_call():
    u8, blob = rg.prep(np.full((8, 8), 100, np.uint8), 4, 4)
    assert (u8 == 100).all()
    for c, m in enumerate((0.485, 0.456, 0.406)):
        assert blob[c, 0, 0] == np.float32(np.float32(100) - np.float32(m)) * np.float32(1.0 / 255.0)


def test_mobilenet_v2_table():
    T = gd.mobilenet_v2_layers()
    assert len(T) == 53 and sum(1 for l in T if l[0] != gd.AVGPOOL) == 52 and T[-1] == (gd.AVGPOOL, 1280, 1280, 1, 0, -1)
    assert len(gd.mobilenet_v2_names()) == 52
    assert 2.1e6 < gd.param_count(T) < 2.3e6                              # ~2.2 M folded parameters
    assert sum(1 for l in T if l[5] >= 0) == 10                           # torchvision's ten residual blocks
    x, outs = rg.forward(T, np.zeros(gd.param_count(T), np.float32), np.zeros((1, 3, 224, 224), np.float32))
    assert [tuple(o.shape[2:]) for o in outs[:-1]][-1] == (7, 7) and x.shape == (1, 1280)
    macs = 0
    for l, o in zip(T, outs):
        if l[0] != gd.AVGPOOL:
            k = {gd.CONV3: 9 * l[1], gd.DW3: 9, gd.PW: l[1]}[l[0]]
            macs += k * o.shape[1] * o.shape[2] * o.shape[3]
    assert 0.29e9 < macs < 0.32e9                                         # the ~0.3 GMAC of the network


def test_fold_state_dict_against_conv_and_batchnorm_in_float64():
    rng = np.random.default_rng(3)
    layers = [(gd.CONV3, 3, 6, 2, 1, -1), (gd.DW3, 6, 6, 1, 1, -1), (gd.PW, 6, 4, 1, 0, -1), (gd.AVGPOOL, 4, 4, 1, 0, -1)]
    names = [("a.0", "a.1"), ("b.0", "b.1"), ("c", "d")]
    sd = {}
    for l, (cn, bn) in zip(layers, names):
        sd[cn + ".weight"] = torch.from_numpy(rng.normal(0, 0.5, gd.weight_shape(l)).astype(np.float32))
        sd[bn + ".weight"] = torch.from_numpy(rng.uniform(0.5, 2.0, l[2]).astype(np.float32))
        sd[bn + ".bias"] = torch.from_numpy(rng.normal(0, 1.0, l[2]).astype(np.float32))
        sd[bn + ".running_mean"] = torch.from_numpy(rng.normal(0, 2.0, l[2]).astype(np.float32))
        sd[bn + ".running_var"] = torch.from_numpy(rng.uniform(0.1, 5.0, l[2]).astype(np.float32))
        sd[bn + ".num_batches_tracked"] = torch.tensor(7)
    prm = gd.fold_state_dict(sd, layers, names)
    assert prm.dtype == np.float32 and prm.size == gd.param_count(layers)
    x = torch.from_numpy(rng.normal(0, 1, (2, 3, 9, 8))).double()
    y = x
    for l, (cn, bn) in zip(layers, names):
        y = F.conv2d(y, sd[cn + ".weight"].double(), None, stride=l[3], padding=0 if l[0] == gd.PW else 1, groups=l[1] if l[0] == gd.DW3 else 1)
        y = F.batch_norm(y, sd[bn + ".running_mean"].double(), sd[bn + ".running_var"].double(), sd[bn + ".weight"].double(),
                         sd[bn + ".bias"].double(), False, 0.0, 1e-5)
        if l[4]:
            y = y.clamp(0, 6)
    want = y.mean((2, 3)).numpy()
    got, _ = rg.forward(layers, prm, x.numpy())
    # the folded parameters are f32 roundings of the float64 fold: relative 2^-24 each, three layers deep
    assert np.abs(got - want).max() <= 64 * 2.0 ** -24 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    assert np.abs(got - want).max() > 0                                  # and they ARE rounded


def test_fold_names_cover_torchvision_s_layout():
    names = gd.mobilenet_v2_names()
    assert names[0] == ("features.0.0", "features.0.1") and names[1] == ("features.1.conv.0.0", "features.1.conv.0.1")
    assert names[2] == ("features.1.conv.1", "features.1.conv.2") and names[3] == ("features.2.conv.0.0", "features.2.conv.0.1")
    assert names[5] == ("features.2.conv.2", "features.2.conv.3") and names[-2] == ("features.17.conv.2", "features.17.conv.3")
    assert names[-1] == ("features.18.0", "features.18.1")
    T = [l for l in gd.mobilenet_v2_layers() if l[0] != gd.AVGPOOL]
    assert [l[0] for l in T[1:3]] == [gd.DW3, gd.PW] and [l[0] for l in T[3:6]] == [gd.PW, gd.DW3, gd.PW]


def test_save_load_round_trip(tmp_path):
    layers, _ = gc.tiny_net()
    prm = gd.random_params(layers, 11)
    prep = dict(out_w=16, out_h=12, mean=(0.1, 0.2, 0.3), scale=0.5, workspace_bytes=1 << 20)
    p = str(tmp_path / "net.svgd")
    gd.save(p, layers, prm, prep)
    l2, p2, q2 = gd.load(p)
    assert l2 == layers and p2.dtype == np.float32 and np.array_equal(gc.bits(p2), gc.bits(prm))
    assert (q2["out_w"], q2["out_h"], q2["workspace_bytes"]) == (16, 12, 1 << 20)
    assert [np.float32(m) for m in q2["mean"]] == [np.float32(m) for m in prep["mean"]] and np.float32(q2["scale"]) == np.float32(0.5)
    gd.save(p, layers, prm)                                              # the defaults are the reference's call
    assert gd.load(p)[2]["out_w"] == 224 and np.float32(gd.load(p)[2]["scale"]) == np.float32(1.0 / 255.0)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:-4])
    try:
        gd.load(p)
        assert False, "a truncated file was read"
    except ValueError:
        pass


def test_random_params_are_seeded():
    T = gd.mobilenet_v2_layers()
    a, b, c = gd.random_params(T, 1), gd.random_params(T, 1), gd.random_params(T, 2)
    assert a.size == gd.param_count(T) and np.array_equal(a, b) and not np.array_equal(a, c)
