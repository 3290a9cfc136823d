"""k_gd_pw_mfma<4> and <2>: svslam_gdesc_describe_batch at the job counts where the launcher takes more than one channel tile per wave
(gd_pw_tiles in csrc/k_global_desc.h), against the host build of the same header, bit for bit.  On a 7 x 5 map 1873 jobs are 2049 pixel
tiles (the last one holds 19 pixels), 1872 exactly 2048 and 1871 one less; njobs is bounded by neither max_jobs nor the slot count and
slots may repeat, so the host build computes three descriptors per case and job j is held to the row of slots[j].  Neighbouring jobs
read different images and every net ends in DW3 + AVGPOOL, so a pixel or a channel tile that lands in the wrong place changes the result.
What only matters for NT > 1 and is run here: tofs[t], the clamp of the last group's tile count (groups of 1, 2, 3, 4, 4 + 1 and 4 + 4
tiles under <4>, 2 + 1 and 2 + 2 under <2>), the t < nt store guard, co0 = 32 NT blockIdx.y.  Next to it: cin around the eight-channel
unrolled loop, chunks with a remainder and chunks of one call on different NT, subnormal A, B and accumulator values, overflow and NaN
through the chain, and the largest cout a table may hold.  Each case asserts through the host build that it reaches the instantiation it
is meant to reach and that the call is one chunk, so a later change of the rule or of the workspace's default fails here visibly."""
import numpy as np
import pytest

import global_desc_cases as gc

pytestmark = pytest.mark.gpu
SRC = (97, 53)
HW = gc.BATCH_HW
IMGS = gc.images(*SRC)


@pytest.fixture(scope="module")
def ctx(svs):
    c = gc.new_context(svs, SRC[0], SRC[1], max_slots=gc.NSLOTS, max_jobs=gc.NSLOTS)
    c.pyramid(list(range(gc.NSLOTS)), list(IMGS))
    yield c
    c.close()


def host_rows(layers, prm, prep, src=SRC, imgs=IMGS):
    """configures the host build and returns its descriptors of slots 0, 1, 2"""
    rc, msg = gc.emu_configure(src[0], src[1], layers, prm, prep)
    assert rc == 0, msg
    r = gc.emu_describe(imgs, [0, 1, 2])
    assert r["rc"] == 0, r["msg"]
    return r["vecs"]


def run(ctx, layers, prm, prep, njobs, nt=None, under_test=1):
    """(device [njobs, dim], expected [njobs, dim]); nt: the instantiation layer under_test is meant to reach in a call of one chunk"""
    host = host_rows(layers, prm, prep)
    if nt is not None:
        assert gc.chunks_of(njobs) == [njobs]
        assert gc.pw_tiles(HW, njobs, layers[under_test][2]) == nt
    ctx.gdesc_configure(layers, prm, prep)
    slots = gc.batch_slots(njobs)
    dev = ctx.gdesc_describe(slots)
    assert dev.shape == (njobs, host.shape[1])
    return dev, host[slots]


def same(dev, want):
    d = gc.bits(dev) != gc.bits(want)
    if d.any():
        j, c = np.argwhere(d)[0]
        raise AssertionError("%d of %d floats differ in %d of %d jobs and channels %s; the first: job %d channel %d, device %r, host build %r"
                             % (d.sum(), d.size, d.any(1).sum(), len(d), np.flatnonzero(d.any(0))[:16].tolist(), j, c, dev[j, c], want[j, c]))


def same_finite(dev, want):
    same(dev, want)
    assert np.isfinite(want).all() and np.abs(want).max() > 0


def test_job_counts_are_the_tile_counts_they_are_meant_to_be():
    tiles = lambda n: (HW * n + 31) // 32
    assert HW == 35 and [tiles(n) for n in (gc.JOBS_NT4, gc.JOBS_NT4_EXACT, gc.JOBS_NT2)] == [2049, 2048, 2047]
    assert HW * gc.JOBS_NT4 - 32 * 2048 == 19                              # the valid pixels of the last tile


@pytest.mark.parametrize("cin,cout", [(33, 31), (33, 33), (33, 65), (33, 97), (33, 128), (9, 129), (9, 160), (9, 256)], ids=lambda v: str(v))
def test_four_tiles_per_wave(ctx, cin, cout):
    """1873 jobs: <4> on the layer under test and on the PW in front of it; last groups of 1, 2, 3, 4 tiles, and 4 + 1, 4 + 1, 4 + 4"""
    layers = gc.batch_net(cin, cout)
    assert gc.pw_tiles(HW, gc.JOBS_NT4, cin) == 4
    same_finite(*run(ctx, layers, gc.seeded(layers, 1000 * cin + cout), gc.case_prep(gc.BATCH_WH), gc.JOBS_NT4, nt=4))


def test_four_tiles_per_wave_at_exactly_2048_pixel_tiles(ctx):
    layers = gc.batch_net(33, 65)
    same_finite(*run(ctx, layers, gc.seeded(layers, 21), gc.case_prep(gc.BATCH_WH), gc.JOBS_NT4_EXACT, nt=4))


def test_four_tiles_per_wave_residual_and_relu6(ctx):
    """40 -> 130 (ReLU6, groups of 4 + 1 tiles) and 130 -> 40 with the residual from layer 0 (one group of 2 tiles), both on <4>"""
    layers = gc.batch_residual_net()
    assert gc.pw_tiles(HW, gc.JOBS_NT4, 40) == 4
    same_finite(*run(ctx, layers, gc.seeded(layers, 9), gc.case_prep(gc.BATCH_WH), gc.JOBS_NT4, nt=4))


@pytest.mark.parametrize("cout", (65, 128))
def test_two_tiles_per_wave(ctx, cout):
    """1871 jobs: <2> with groups of 2 + 1 and 2 + 2 tiles"""
    layers = gc.batch_net(33, cout)
    same_finite(*run(ctx, layers, gc.seeded(layers, 3300 + cout), gc.case_prep(gc.BATCH_WH), gc.JOBS_NT2, nt=2))


@pytest.mark.parametrize("cin", (1, 2, 7, 8, 9, 15, 16, 17))
def test_cin_around_the_unrolled_loop(ctx, cin):
    """the tail loop alone (cin < 8), the eight-channel loop alone (8, 16), both, and an odd cin's last half step; on <1> and on <4>"""
    layers = gc.batch_net(cin, 65)
    prm = gc.seeded(layers, 70 + cin)
    for njobs, nt in ((3, 1), (gc.JOBS_NT4, 4)):
        same_finite(*run(ctx, layers, prm, gc.case_prep(gc.BATCH_WH), njobs, nt=nt))


def test_chunks_with_a_remainder_and_chunks_on_different_tile_counts(ctx):
    """workspace caps of 2, 1000 and 1872 jobs: 5 jobs as 2 + 2 + 1 (all <1>); 1873 as 1000 + 873, which the rule puts on <2> and <1>
    where the whole call ran <4>; 2812 as 1872 + 940 on <4> and <2>.  Each equals the call of one chunk and the host build"""
    layers = gc.batch_net(33, 65)
    prm = gc.seeded(layers, 21)
    whole, want = run(ctx, layers, prm, gc.case_prep(gc.BATCH_WH), 2812, nt=4)       # 1872 + 940 jobs below
    same_finite(whole, want)
    jf = int(gc.load_emu().emu_gd_job_floats())
    # (jobs, jobs per chunk, the chunks, the NT of the layer under test in each chunk)
    for njobs, cap, chunks, nts in ((5, 2, [2, 2, 1], [1, 1, 1]), (gc.JOBS_NT4, 1000, [1000, 873], [2, 1]), (2812, 1872, [1872, 940], [4, 2])):
        prep = gc.case_prep(gc.BATCH_WH, workspace_bytes=cap * 4 * jf)
        host_rows(layers, prm, prep)
        assert gc.chunks_of(njobs) == chunks and [gc.pw_tiles(HW, n, 65) for n in chunks] == nts
        assert gc.pw_tiles(HW, njobs, 65) == (4 if njobs > 5 else 1)                 # what the same call takes as one chunk
        ctx.gdesc_configure(layers, prm, prep)
        dev = ctx.gdesc_describe(gc.batch_slots(njobs))
        same(dev, whole[:njobs])
        same(dev, want[:njobs])


@pytest.mark.parametrize("regime", gc.SUBNORMAL_REGIMES)
def test_subnormals_are_neither_flushed_nor_rounded_differently(ctx, regime):
    """subnormal B and accumulators, subnormal A, accumulators that cross the edge of the normal range: the f32-input MFMA keeps the
    kernel's denormal mode on A and B and never flushes C and D, so the device equals std::fmaf here too (<1> and <4>)"""
    layers, prm, prep, classes = gc.subnormal_case(regime)
    share = gc.float_classes(host_rows(layers, prm, prep))
    assert share["zero"] == 0 and all(share[c] >= 0.01 for c in classes), share
    for njobs, nt in ((3, 1), (gc.JOBS_NT4, 4)):
        dev, want = run(ctx, layers, prm, prep, njobs, nt=nt)
        same(dev, want)
        assert np.isfinite(want).all()


def overflow_mid(relu6):
    """(layers, params, prep, the host build's output [3, 65, hw] of the layer under test) of gc.overflow_case"""
    layers, prm, prep = gc.overflow_case(relu6, IMGS)
    host_rows(layers, prm, prep)
    return layers, prm, prep, gc.emu_describe(IMGS, [0, 1, 2], dump=(1, 65 * HW))["dump"].reshape(3, 65, HW)


def test_overflow_and_nan_through_the_chain(ctx):
    """weights of 3e38 in the first PW: +inf and -inf enter the PW under test, inf - inf and 0 inf give NaN inside its chain.  The NaN
    masks, the infinities with their signs and every finite float are equal; a NaN's sign and payload are not part of the contract"""
    layers, prm, prep, mid = overflow_mid(0)
    hot = ~np.isfinite(mid[:, :1])                                         # [3, 1, hw]: the pixels at which the input holds infinities
    assert sorted(hot.any(2).ravel().tolist()) == [False, True, True]      # one image stays finite
    assert ((mid[:, 0::8] == np.inf) == hot).all() and ((mid[:, 1::8] == -np.inf) == hot).all()
    assert (np.isnan(mid[:, 2::8]) == hot).all() and (np.isnan(mid[:, 3::8]) == hot).all() and (np.isfinite(mid) == ~hot).all()
    for njobs, nt in ((3, 1), (gc.JOBS_NT4, 4)):
        dev, want = run(ctx, layers, prm, prep, njobs, nt=nt)
        assert np.isnan(want).any() and (want == np.inf).any() and (want == -np.inf).any() and np.isfinite(want).any()
        assert np.array_equal(np.isnan(dev), np.isnan(want))
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(dev), inf) and np.array_equal(dev[inf], want[inf])
        fin = np.isfinite(want)
        assert np.array_equal(gc.bits(dev)[fin], gc.bits(want)[fin])


def test_relu6_pins_nan_and_infinity(ctx):
    """the same parameters with ReLU6 on the layer whose chain holds them: NaN -> +0, -inf -> +0, +inf -> 6, so every float behind it is
    finite and the whole result is compared bit for bit"""
    raw = overflow_mid(0)[3]
    layers, prm, prep, mid = overflow_mid(1)
    assert np.isnan(raw).any() and np.isfinite(mid).all()
    assert (mid[raw == np.inf] == 6).all() and (gc.bits(mid[raw == -np.inf]) == 0).all() and (gc.bits(mid[np.isnan(raw)]) == 0).all()
    for njobs, nt in ((3, 1), (gc.JOBS_NT4, 4)):
        same_finite(*run(ctx, layers, prm, prep, njobs, nt=nt))


def test_the_largest_channel_count(ctx):
    """cout = 65536 is the largest a table may hold and k_gd_conv3's grid.y is cout: CONV3 3 -> 65536, PW 65536 -> 4 on a 1 x 1 map, 2
    jobs.  Observed on an MI355X: HIP takes a grid of (1, 65536, 2) workgroups, the call returns 0 and equals the host build, so the
    range stays as gd_configure has it.  Were such a launch refused the call would return an error (the launcher checks
    hipGetLastError behind its launches) and gdesc_describe would raise here"""
    layers, out_wh = gc.big_cout_net()
    prm = gc.seeded(layers, 65536)
    prep = gc.case_prep(out_wh)
    host = host_rows(layers, prm, prep)
    ctx.gdesc_configure(layers, prm, prep)
    dev = ctx.gdesc_describe([2, 0])
    same_finite(dev, host[[2, 0]])
