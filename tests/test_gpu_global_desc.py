"""svslam_gdesc_* on the device against the host build of the same header (tests/cpp/gd_host_emu), bit for bit: the smallest shapes at
which the tiling can go wrong, prep, MobileNetV2's whole table once, the chunking, a job alone and among others, two calls, the refusals
with the outputs untouched, Context.gdesc_describe and the timing family.  The host build is held to float64 by
tests/test_host_emulation_global_desc.py; here only equality is asked, which is what the f32-input MFMA has to deliver."""
import ctypes as C

import numpy as np
import pytest

import global_desc_cases as gc

pytestmark = pytest.mark.gpu
gd = gc.gdesc()
SRC = (97, 53)


@pytest.fixture(scope="module")
def ctx(svs):
    c = gc.new_context(svs, SRC[0], SRC[1], max_slots=gc.NSLOTS, max_jobs=gc.NSLOTS)
    c.pyramid(list(range(gc.NSLOTS)), list(gc.images(*SRC)))
    yield c
    c.close()


def both(ctx, layers, prm, prep, slots, src=SRC):
    """(device, host build) descriptors of the same configuration"""
    ctx.gdesc_configure(layers, prm, prep)
    rc, msg = gc.emu_configure(src[0], src[1], layers, prm, prep)
    assert rc == 0, msg
    dev = ctx.gdesc_describe(slots)
    r = gc.emu_describe(gc.images(*src), slots)
    assert r["rc"] == 0, r["msg"]
    assert dev.shape == r["vecs"].shape and dev.shape[1] == ctx.gdesc_dim()
    return dev, r["vecs"]


def same(dev, host):
    d = gc.bits(dev) != gc.bits(host)
    assert not d.any(), "%d of %d floats differ, the largest difference %.3g" % (d.sum(), d.size, np.abs(dev.astype(np.float64) - host).max())
    assert np.isfinite(host).all() and np.abs(host).max() > 0


def test_slots_hold_the_images(ctx):
    for s, im in enumerate(gc.images(*SRC)):
        assert np.array_equal(ctx.pyramid_read(s, 0), im)


@pytest.mark.parametrize("name", list(gc.LAYER_CASES))
def test_small_shapes_equal_the_host_build(ctx, name):
    layers, out_wh = gc.LAYER_CASES[name]
    same(*both(ctx, layers, gc.seeded(layers, 7), gc.case_prep(out_wh), [0, 1, 2]))


@pytest.mark.parametrize("cin", gc.PW_EDGES)
def test_pw_at_the_tile_edges(ctx, cin):
    for cout in gc.PW_EDGES:
        layers = gc.pw_net(cin, cout, relu6=cout & 1)
        same(*both(ctx, layers, gc.seeded(layers, cin * 100 + cout), gc.case_prep((7, 5)), [2, 0, 1]))


def test_pw_residual_across_tiles(ctx):
    """add_from with more than one channel tile and a pixel count that is no multiple of 32"""
    layers = [(gc.PW, 3, 40, 1, 0, -1), (gc.PW, 40, 130, 1, 1, -1), (gc.PW, 130, 40, 1, 0, 0), (gc.AVGPOOL, 40, 40, 1, 0, -1)]
    same(*both(ctx, layers, gc.seeded(layers, 9), gc.case_prep((7, 5)), [0, 1, 2]))


@pytest.mark.parametrize("src", gc.DEVICE_PREP_SIZES, ids=lambda s: "%dx%d" % s)
def test_prep_equals_the_host_build(svs, ctx, src):
    """the blob through a network that copies it: DW3 with the centre tap 1 keeps each plane, the pool sums it; and through a PW that
    mixes the three planes pixel by pixel.  4 x 4 and 5 x 9 sources are below a context's 16 x 16 and stay with the host build's test"""
    c = ctx if src == SRC else gc.new_context(svs, src[0], src[1], max_slots=gc.NSLOTS, max_jobs=gc.NSLOTS)
    try:
        if c is not ctx:
            c.pyramid(list(range(gc.NSLOTS)), list(gc.images(*src)))
        for out_wh in gc.OUT_SIZES:
            layers = [(gc.DW3, 3, 3, 1, 0, -1), (gc.PW, 3, 33, 1, 0, -1), (gc.AVGPOOL, 33, 33, 1, 0, -1)]
            prm = gc.seeded(layers, 1)
            prm[:27] = 0; prm[4:27:9] = 1; prm[27:30] = 0            # the identity
            same(*both(c, layers, prm, gc.case_prep(out_wh), [2, 0, 1], src))
    finally:
        if c is not ctx:
            c.close()


def test_mobilenet_v2_whole_table_chunks_neighbours_and_two_calls(ctx):
    T = gd.mobilenet_v2_layers()
    prm = gd.random_params(T, 2024)
    dev, host = both(ctx, T, prm, None, [2, 0, 1])
    same(dev, host)
    assert dev.shape == (3, 1280)
    assert np.array_equal(gc.bits(ctx.gdesc_describe([2, 0, 1])), gc.bits(dev))                   # two calls
    assert np.array_equal(gc.bits(ctx.gdesc_describe([0])[0]), gc.bits(dev[1]))                   # a job alone
    ctx.gdesc_configure(T, prm, dict(workspace_bytes=4 * gc.load_emu().emu_gd_job_floats()))      # chunks of one job
    assert np.array_equal(gc.bits(ctx.gdesc_describe([2, 0, 1])), gc.bits(dev))


def test_chunks_of_one_job_on_the_tiny_net(ctx):
    layers, out_wh = gc.tiny_net()
    prm = gc.seeded(layers, 3)
    dev, host = both(ctx, layers, prm, gc.case_prep(out_wh), [2, 0, 1, 1, 2])
    same(dev, host)
    ctx.gdesc_configure(layers, prm, gc.case_prep(out_wh, workspace_bytes=1))
    assert np.array_equal(gc.bits(ctx.gdesc_describe([2, 0, 1, 1, 2])), gc.bits(dev))
    assert np.array_equal(gc.bits(dev[0]), gc.bits(dev[4])) and np.array_equal(gc.bits(dev[2]), gc.bits(dev[3]))


def test_the_kept_buffers_carry_nothing_over(svs):
    """on a fresh context with the tiny net (dim 5): 1 job, 20 jobs, 1 job.  The slots / vectors buffer takes 4 n rounded up to 256,
    then 20 n bytes: 276 for one job (the context then keeps 345) and 656 for 20, more than 1.25 * 276 + 256 = 601.  The workspace
    takes 4 * job_floats bytes per job of the chunk and no headroom; all 20 jobs are one chunk, and a job's share holds at least the
    3 x 16 x 16 blob, so 20 shares pass 1.25 shares + 256 bytes.  The second call replaces both buffers, the third runs in what it
    left: first and third are the same bits, the bits of a context that has seen nothing else, and the host build's."""
    layers, out_wh = gc.tiny_net()
    prm, prep = gc.seeded(layers, 3), gc.case_prep(out_wh)
    many = [i % gc.NSLOTS for i in range(20)]
    rc, msg = gc.emu_configure(SRC[0], SRC[1], layers, prm, prep)
    assert rc == 0, msg
    assert 20 * 4 * gc.load_emu().emu_gd_job_floats() <= 256 << 20 and gc.load_emu().emu_gd_job_floats() >= 3 * 16 * 16
    host = gc.emu_describe(gc.images(*SRC), many)
    assert host["rc"] == 0, host["msg"]
    a = gc.new_context(svs, SRC[0], SRC[1], max_slots=gc.NSLOTS, max_jobs=gc.NSLOTS)
    b = gc.new_context(svs, SRC[0], SRC[1], max_slots=gc.NSLOTS, max_jobs=gc.NSLOTS)
    try:
        for c in (a, b):
            c.pyramid(list(range(gc.NSLOTS)), list(gc.images(*SRC)))
            c.gdesc_configure(layers, prm, prep)
        first, big, third = a.gdesc_describe([0]), a.gdesc_describe(many), a.gdesc_describe([0])
        alone = b.gdesc_describe([0])
    finally:
        a.close(); b.close()
    same(big, host["vecs"])
    same(first, host["vecs"][:1])
    assert np.array_equal(gc.bits(third), gc.bits(first)) and np.array_equal(gc.bits(alone), gc.bits(first))


def test_unconfigured_context_refuses(svs):
    c = gc.new_context(svs, 32, 32, max_slots=2, max_jobs=2)
    try:
        assert c.gdesc_dim() == 0
        v = np.full((1, 4), 7.5, np.float32)
        sl = np.zeros(1, np.int32)
        assert c.L.svslam_gdesc_describe_batch(c.h, 1, sl.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)) != 0
        assert "no network is configured" in c.L.svslam_last_error(c.h).decode() and (v == 7.5).all()
        with pytest.raises(RuntimeError, match="no network is configured"):
            c.gdesc_describe([0])
    finally:
        c.close()


def test_refusals_leave_vecs_and_the_network_untouched(ctx):
    layers, out_wh = gc.tiny_net()
    prm = gc.seeded(layers, 3)
    ctx.gdesc_configure(layers, prm, gc.case_prep(out_wh))
    before = ctx.gdesc_describe([0, 1])
    for slots in ([0, gc.NSLOTS], [-1]):
        v = np.full((len(slots), 5), 7.5, np.float32)
        sl = np.asarray(slots, np.int32)
        assert ctx.L.svslam_gdesc_describe_batch(ctx.h, len(sl), sl.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)) != 0
        assert "slot" in ctx.L.svslam_last_error(ctx.h).decode() and (v == 7.5).all()
    assert ctx.gdesc_describe([]).shape == (0, 5)                        # njobs == 0 is a valid no-op
    for name, bad, words, ok in gc.refusals():
        l, p, q, n = gc.configure_args(bad)
        arr = gc.GdLayer * max(len(l), 1)
        arr = arr(*[gc.GdLayer(*[int(x) for x in e]) for e in l])
        P = gc.prep_struct(q)
        rc = ctx.L.svslam_gdesc_configure(ctx.h, len(l), C.cast(arr, C.c_void_p), p.ctypes.data_as(C.c_void_p), n, C.cast(C.pointer(P), C.c_void_p))
        assert rc != 0 and words in ctx.L.svslam_last_error(ctx.h).decode(), (name, ctx.L.svslam_last_error(ctx.h).decode())
        assert ctx.gdesc_dim() == 5
    assert np.array_equal(gc.bits(ctx.gdesc_describe([0, 1])), gc.bits(before))
    for name, bad, words, ok in gc.refusals():
        l, p, q, n = gc.configure_args(ok)
        ctx.gdesc_configure(l, p, q)


def test_timing_family(svs, ctx):
    layers, out_wh = gc.tiny_net()
    ctx.gdesc_configure(layers, gc.seeded(layers, 3), gc.case_prep(out_wh))
    assert svs.LOOP_FAMILIES["global_desc"] == 17 and "k_gd_pw_mfma" in svs.FAMILY_KERNELS["global_desc"]
    ctx.timing(True)
    try:
        ctx.gdesc_describe([0, 1, 2])
        ms, launches, units = ctx.timing_get("global_desc")
        assert launches == 1 and units == 3 and ms > 0
    finally:
        ctx.timing(False)
