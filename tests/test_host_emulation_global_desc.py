"""csrc/k_global_desc.h itself, compiled for the host (tests/cpp/gd_host_emu, -ffp-contract=off, std::fmaf), without a device:
prep against tests/ref_global_desc.py in every byte and every f32; single layers against float64 inside the standard bound of a chain of
n roundings, gamma_n (|bias| + sum |w x|), computed per output element; MobileNetV2 on seeded weights against float64 within four times
the error a torch f32 evaluation of the same network shows; the chunking; every refusal with its accepted neighbour; the nets that
work in the subnormal range, with the bound's underflow term; the launcher's choice of k_gd_pw_mfma<NT> (gd_pw_tiles) at its edges.
Not a replacement for tests/test_gpu_global_desc.py: the compiler, the ISA, the MFMA and the launches are not in it."""
import ctypes as C

import numpy as np
import pytest
import torch

import global_desc_cases as gc
import ref_global_desc as rg
import ref_loop_candidates as rl

gd = gc.gdesc()


def test_table_is_the_python_one():
    L = gc.load_emu()
    arr = (gc.GdLayer * 64)()
    n = L.emu_gd_mobilenet_v2(arr, 64)
    assert n == 53 and L.emu_gd_mobilenet_v2(None, 0) == 53
    assert [(a.op, a.cin, a.cout, a.stride, a.relu6, a.add_from) for a in arr[:n]] == gd.mobilenet_v2_layers()


@pytest.mark.parametrize("out_wh", gc.OUT_SIZES, ids=lambda s: "out%dx%d" % s)
@pytest.mark.parametrize("wh", gc.PREP_SIZES, ids=lambda s: "%dx%d" % s)
def test_prep_equals_the_reference_exactly(wh, out_wh):
    w, h = wh
    layers = gc.dw_net(1)
    rc, msg = gc.emu_configure(w, h, layers, gc.seeded(layers, 1), gc.case_prep(out_wh))
    assert rc == 0, msg
    imgs = gc.images(w, h)
    r = gc.emu_describe(imgs, [2, 0, 1], out_wh=out_wh)
    assert r["rc"] == 0, r["msg"]
    for j, s in enumerate([2, 0, 1]):
        u8, blob = rg.prep(imgs[s], out_wh[0], out_wh[1])
        assert np.array_equal(r["u8"][j], u8), (np.abs(r["u8"][j].astype(int) - u8).max(), int((r["u8"][j] != u8).sum()))
        assert np.array_equal(gc.bits(r["blob"][j]), gc.bits(blob))
    assert len(np.unique(r["u8"])) > (2 if min(wh) < 6 else 16)


def test_prep_takes_mean_and_scale():
    layers = gc.dw_net(1)
    prep = gc.case_prep((13, 7), mean=(123.675, 116.28, 103.53), scale=1.0 / 58.0)
    assert gc.emu_configure(97, 53, layers, gc.seeded(layers, 1), prep)[0] == 0
    imgs = gc.images(97, 53)
    r = gc.emu_describe(imgs, [1], out_wh=(13, 7))
    _, blob = rg.prep(imgs[1], 13, 7, prep["mean"], prep["scale"])
    assert np.array_equal(gc.bits(r["blob"][0]), gc.bits(blob)) and np.abs(blob).max() < 3


def _layer_check(layers, li, out_wh, src=(97, 53), seed=7, prm=None, prep=None, underflow=False):
    """layer li of the net, host build against float64 on the host build's own input of that layer; per-element bound.  underflow:
    the chain may round in the subnormal range, where a rounding costs up to half of 2^-149 whatever the magnitude: + n 2^-149"""
    prm = gc.seeded(layers, seed) if prm is None else prm
    prep = dict(gc.PREP_DEFAULTS, **(gc.case_prep(out_wh) if prep is None else prep))
    assert gc.emu_configure(src[0], src[1], layers, prm, prep)[0] == 0
    imgs = gc.images(*src)
    slots = [0, 1, 2]
    x64, outs = rg.forward(layers, prm, np.stack([rg.prep(imgs[s], out_wh[0], out_wh[1], prep["mean"], prep["scale"])[1] for s in slots]))
    shp = lambda i: tuple(outs[i].shape[1:]) if i >= 0 else (3, out_wh[1], out_wh[0])

    def dumped(i):
        if i < 0:
            return gc.emu_describe(imgs, slots, out_wh=out_wh)["blob"]
        return gc.emu_describe(imgs, slots, dump=(i, int(np.prod(shp(i)))))["dump"].reshape((len(slots),) + shp(i))
    l = layers[li]
    wb = rg.split(layers, prm)[li]
    if l[0] == rg.AVGPOOL:
        got = gc.emu_describe(imgs, slots)["vecs"]
    else:
        got = dumped(li)
    x = torch.from_numpy(dumped(li - 1)).double()
    emu_outs = {l[5]: torch.from_numpy(dumped(l[5])).double()} if l[5] >= 0 else {}
    want = rg.layer(l, wb, x, emu_outs).numpy()
    mag = rg.layer(l, wb, x, emu_outs, absolute=True).numpy()
    n = rg.chain_length(l, x.shape[2] * x.shape[3])
    if l[0] == rg.AVGPOOL:
        mag = mag / float(x.shape[2] * x.shape[3])
    bound = rg.gamma(n) * mag + (n * 2.0 ** -149 if underflow else 0.0)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("layer %d %s n = %d: worst error / bound = %.3f, max error %.3g" % (li, l, n, worst, err.max()))
    assert got.shape == want.shape and (err <= bound).all(), worst
    return got, want


@pytest.mark.parametrize("name", [n for n in gc.LAYER_CASES if n != "tiny"])
def test_single_layers_against_float64(name):
    layers, out_wh = gc.LAYER_CASES[name]
    for li in range(len(layers) - 2, len(layers)):                       # the layer under test and the pool behind it
        got, want = _layer_check(layers, li, out_wh)
    assert np.abs(want).max() > 1e-3


def test_tiny_net_layer_by_layer():
    layers, out_wh = gc.tiny_net()
    for li in range(len(layers)):
        got, want = _layer_check(layers, li, out_wh)
        if layers[li][4]:
            assert got.min() >= 0 and got.max() <= 6
    assert layers[3][5] == 1


@pytest.mark.parametrize("cin", gc.PW_EDGES)
def test_pw_at_the_tile_edges_against_float64(cin):
    for cout in gc.PW_EDGES:
        _layer_check(gc.pw_net(cin, cout, relu6=cout & 1), 1, (7, 5), seed=cin * 100 + cout)


def test_relu6_clamps_both_ways_and_pins_zero():
    layers = [(gc.PW, 3, 4, 1, 1, -1), (gc.AVGPOOL, 4, 4, 1, 0, -1)]
    w = np.zeros((4, 3), np.float32); b = np.array([-1.0, 9.0, 2.5, -0.0], np.float32)
    assert gc.emu_configure(16, 16, layers, np.concatenate([w.reshape(-1), b]), gc.case_prep((2, 2)))[0] == 0
    v = gc.emu_describe(gc.images(16, 16), [0])["vecs"][0]
    assert gc.bits(v).tolist() == gc.bits(np.array([0.0, 6.0, 2.5, 0.0], np.float32)).tolist()


@pytest.mark.parametrize("regime", gc.SUBNORMAL_REGIMES)
def test_subnormal_regimes_against_float64(regime):
    """the nets the device test runs bit for bit against this build (test_gpu_global_desc_batch.py), here against float64: every layer
    inside gamma_n S + n 2^-149.  The classes are a condition: the case is about subnormals only while the host build produces them"""
    layers, prm, prep, classes = gc.subnormal_case(regime)
    for li in range(len(layers)):
        got, want = _layer_check(layers, li, gc.BATCH_WH, prm=prm, prep=prep, underflow=True)
    share = gc.float_classes(got)
    print(regime, "descriptor:", {k: round(float(v), 3) for k, v in share.items()})
    assert share["zero"] == 0 and share["nan"] == 0 and share["inf"] == 0 and all(share[c] >= 0.01 for c in classes), share
    assert (want != 0).all()


# ---- which k_gd_pw_mfma<NT> the launcher takes (gd_pw_tiles) ----------------------------------------------------------------------
PW_TILE_EDGES = {       # jobs -> NT for cout = 31, 33, 65, 128, 129, 160, 256 on a 7 x 5 map: 2047, 2048, 2049 and 4 pixel tiles
    1871: (1, 1, 2, 2, 4, 4, 4),
    1872: (4, 4, 4, 4, 4, 4, 4),
    1873: (4, 4, 4, 4, 4, 4, 4),
    3: (1, 1, 1, 1, 1, 1, 1),
}
PW_TILE_MOBILENET = {1: (0, 0, 34), 3: (0, 1, 33), 39: (6, 6, 22), 64: (9, 7, 18)}      # jobs -> PW layers on <4>, <2>, <1> at 224 x 224


def test_pw_tile_rule_at_its_edges():
    assert gc.BATCH_HW == 35
    for jobs, want in PW_TILE_EDGES.items():
        got = tuple(gc.pw_tiles(35, jobs, cout) for cout in (31, 33, 65, 128, 129, 160, 256))
        assert got == want, (jobs, got)
    assert gc.pw_tiles(1, 1, 1) == 1 and gc.pw_tiles(1, 1, 1 << 16) == 1            # one pixel tile times 2048 channel tiles: 2048 waves at <1> only
    assert gc.pw_tiles(224 * 224, 8192, 1280) == 4                                   # 12.8 M pixel tiles: the count is 64-bit


def test_pw_tile_rule_on_the_mobilenet_table():
    T = gd.mobilenet_v2_layers()
    h = w = 224
    pw = []
    for op, cin, cout, stride, relu6, add_from in T:
        if op in (gc.CONV3, gc.DW3):
            h, w = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
        if op == gc.PW:
            pw.append((h * w, cout))
    assert len(pw) == 34 and pw[0] == (112 * 112, 16) and pw[-1] == (7 * 7, 1280)
    for jobs, want in PW_TILE_MOBILENET.items():
        nt = [gc.pw_tiles(hw, jobs, cout) for hw, cout in pw]
        assert tuple(nt.count(k) for k in (4, 2, 1)) == want, (jobs, nt)
    assert gc.pw_tiles(112 * 112, 3, 96) == 2                                        # the one layer on <2> with three jobs: 16 -> 96


def test_whole_network_within_four_times_torch_f32_s_own_error():
    T = gd.mobilenet_v2_layers()
    prm = gd.random_params(T, 2024)
    w, h = 620, 188
    assert gc.emu_configure(w, h, T, prm, None)[0] == 0
    imgs = gc.images(w, h)
    slots = [0, 1]
    blob = np.stack([rg.prep(imgs[s])[1] for s in slots])
    d64, _ = rg.forward(T, prm, blob, torch.float64)
    d32, _ = rg.forward(T, prm, blob, torch.float32)
    inside = ((d64 > 0) & (d64 < 6)).sum(1)
    print("entries strictly inside (0, 6):", inside.tolist(), "of 1280")
    assert (inside >= 640).all()                                         # ReLU6 has neither killed nor saturated the net
    r = gc.emu_describe(imgs, slots)
    assert r["rc"] == 0, r["msg"]
    unit = lambda v: v / np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True))
    n64 = unit(d64)
    e_ref = float(np.abs(unit(d32.astype(np.float64)) - n64).max())
    e_host = float(np.abs(unit(r["vecs"].astype(np.float64)) - n64).max())
    print("e_ref (torch f32 against f64, normalised) = %.3e, host build = %.3e, ratio %.2f" % (e_ref, e_host, e_host / e_ref))
    assert e_ref > 0 and e_host <= 4 * e_ref
    for j in range(len(slots)):
        a, b = rl.normalise(r["vecs"][j]), rl.normalise(d64[j].astype(np.float32))
        sim = float(rl.similarity(a, b))
        print("similarity of the host build's and the float64 descriptor, job %d: 1 - %.3e" % (j, 1 - sim))
        assert sim > 1 - 1e-4
    assert float(rl.similarity(rl.normalise(r["vecs"][0]), rl.normalise(r["vecs"][1]))) < 1 - 1e-4     # two images, two descriptors


def test_chunks_and_neighbours_do_not_change_a_job():
    layers, out_wh = gc.tiny_net()
    prm = gc.seeded(layers, 3)
    imgs = gc.images(97, 53)
    L = gc.load_emu()
    assert gc.emu_configure(97, 53, layers, prm, gc.case_prep(out_wh))[0] == 0
    assert L.emu_gd_chunk(3) == 3
    one = gc.emu_describe(imgs, [2, 0, 1])["vecs"]
    assert gc.emu_configure(97, 53, layers, prm, gc.case_prep(out_wh, workspace_bytes=4 * L.emu_gd_job_floats()))[0] == 0
    assert L.emu_gd_chunk(3) == 1
    assert np.array_equal(gc.bits(gc.emu_describe(imgs, [2, 0, 1])["vecs"]), gc.bits(one))
    assert gc.emu_configure(97, 53, layers, prm, gc.case_prep(out_wh, workspace_bytes=1))[0] == 0      # below one job: one at a time
    assert L.emu_gd_chunk(3) == 1
    assert np.array_equal(gc.bits(gc.emu_describe(imgs, [0])["vecs"][0]), gc.bits(one[1]))
    assert np.array_equal(gc.bits(gc.emu_describe(imgs, [2, 0, 1])["vecs"]), gc.bits(one))


@pytest.mark.parametrize("case", gc.refusals(), ids=lambda c: c[0])
def test_refused_configurations_keep_the_old_network(case):
    name, bad, words, ok = case
    layers, out_wh = gc.tiny_net()
    prm = gc.seeded(layers, 3)
    imgs = gc.images(97, 53)
    assert gc.emu_configure(97, 53, layers, prm, gc.case_prep(out_wh))[0] == 0
    before = gc.emu_describe(imgs, [0, 1])["vecs"]
    l, p, q, n = gc.configure_args(bad)
    rc, msg = gc.emu_configure(97, 53, l, p, q, n)
    assert rc != 0 and words in msg, (rc, msg)
    assert gc.load_emu().emu_gd_dim() == 5
    assert np.array_equal(gc.bits(gc.emu_describe(imgs, [0, 1])["vecs"]), gc.bits(before))
    l, p, q, n = gc.configure_args(ok)
    rc, msg = gc.emu_configure(97, 53, l, p, q, n)
    assert rc == 0, msg


def test_refused_describe_leaves_vecs_untouched():
    layers, out_wh = gc.tiny_net()
    imgs = gc.images(97, 53)
    assert gc.emu_configure(97, 53, layers, gc.seeded(layers, 3), gc.case_prep(out_wh))[0] == 0
    for slots in ([0, 3], [-1], [1, 2, 3]):
        v = np.full((len(slots), 5), 7.5, np.float32)
        r = gc.emu_describe(imgs, slots, vecs=v)
        assert r["rc"] != 0 and "slot" in r["msg"] and (v == 7.5).all()
    assert gc.emu_describe(imgs, [])["rc"] == 0                            # njobs == 0 is a valid no-op
    for w, h, fine in ((3, 8, False), (8, 3, False), (4, 4, True)):
        assert gc.emu_configure(w, h, layers, gc.seeded(layers, 3), gc.case_prep(out_wh))[0] == 0
        v = np.full((1, 5), 7.5, np.float32)
        r = gc.emu_describe(gc.images(w, h), [0], vecs=v)
        assert (r["rc"] == 0) == fine and (fine or ("below 4 x 4" in r["msg"] and (v == 7.5).all()))
