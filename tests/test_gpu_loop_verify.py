"""svslam_loop_verify_batch on the device (Context.loop_verify) against tests/ref_loop_verify.py on every case of loop_verify_cases.py:
status, counts, the match list with its inlier flags and need_correction exactly, T_corr / T_rel within DESIGN 3's tolerances (t 1e-6 m,
q 1e-7), d within 1e-6; the ABI's refusals; independence of the jobs of a call and determinism; the timing family."""
import numpy as np
import pytest

import global_desc_cases as gc     # new_context, settle_rotation: the contexts made here leave the stream rotation as it was
import loop_verify_cases as lc
import ref_loop_verify as rl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(svs):
    c = svs.Context(64, 32, max_slots=1, max_jobs=1)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_against_the_reference(ctx, name):
    ref = lc.reference(name)
    (got,) = ctx.loop_verify([lc.case(name)], lc.CAM, lc.EXT_L, **lc.params(name))
    ok, msg = lc.compare(got, ref)
    print(name, rl.STATUS_NAMES[ref["status"]], msg)
    assert ok, msg
    if ref["status"] in (rl.FEW_MATCHES, rl.FEW_POINTS, rl.FEW_INLIERS):          # stages not reached: identity, zero
        assert np.array_equal(got["T_corr"], rl.IDENT) and np.array_equal(got["T_rel"], rl.IDENT) and got["d"] == 0.0


def test_batch_independence_and_determinism(ctx):
    """every case that runs with the default parameters in one call (sizes 0 to 1024 side by side), the same call again, and every
    job alone: the same bits"""
    names = [n for n in lc.CASES if not lc.params(n)]
    assert len(names) >= 10 and "n1024" in names and "no_candidates" in names
    together = ctx.loop_verify([lc.case(n) for n in names], lc.CAM, lc.EXT_L)
    again = ctx.loop_verify([lc.case(n) for n in names], lc.CAM, lc.EXT_L)
    for i, n in enumerate(names):
        (alone,) = ctx.loop_verify([lc.case(n)], lc.CAM, lc.EXT_L)
        assert lc.same_bits(alone, together[i]) and lc.same_bits(again[i], together[i]), n
        ok, msg = lc.compare(together[i], lc.reference(n))
        assert ok, (n, msg)


def test_the_kept_buffer_carries_nothing_over(svs):
    """on a fresh context: small_412_5, n64_64, small_412_5 again.  lv_layout takes 272 bytes for the job and, rounded up to 16 each,
    3 * 4 nc + nc + 32 nc + 32 nq + 12 nc + 8 nq + nc: 832 bytes for 5 x 5 descriptors (the context then keeps 1040) and 6544 for
    64 x 64, more than 1.25 * 832 + 256 = 1296, so the second call replaces the buffer and the third runs in what the second left
    there.  The first and third results are the same bits, and the bits of the case on a context that has seen nothing else."""
    small, p = lc.case("small_412_5"), lc.params("small_412_5")
    a = gc.new_context(svs, 64, 32, max_slots=1, max_jobs=1)
    b = gc.new_context(svs, 64, 32, max_slots=1, max_jobs=1)
    try:
        (first,) = a.loop_verify([small], lc.CAM, lc.EXT_L, **p)
        (big,) = a.loop_verify([lc.case("n64_64")], lc.CAM, lc.EXT_L)
        (third,) = a.loop_verify([small], lc.CAM, lc.EXT_L, **p)
        (alone,) = b.loop_verify([small], lc.CAM, lc.EXT_L, **p)
    finally:
        a.close(); b.close(); gc.settle_rotation(svs)
    assert first["status"] == rl.ACCEPTED and big["status"] == rl.ACCEPTED
    assert lc.same_bits(first, third) and lc.same_bits(first, alone)
    ok, msg = lc.compare(big, lc.reference("n64_64"))
    assert ok, msg


def test_refusals_write_nothing(ctx, svs):
    import ctypes as C
    good = lc.case("n64_64")

    def refused(match, job=None, cam=lc.CAM, ext_l=lc.EXT_L, **prm):
        with pytest.raises(RuntimeError, match=match):
            ctx.loop_verify([good, job if job is not None else good], cam, ext_l, **prm)
    refused("1024", job=lc.build(seed=1, nc=1025, nq=10, n_match=0))
    refused("1024", job=lc.build(seed=1, nc=10, nq=1025, n_match=0))
    for key in ("T_cur", "T_cand"):
        T = np.array(good[key]); T[:4] *= 1 + 2e-6
        refused("unit length", job=dict(good, **{key: T}))
    e = np.array(lc.EXT_L); e[:4] *= 1 - 2e-6
    refused("ext_l", ext_l=e)
    refused("ransac_iters", ransac_iters=0)
    refused("ransac_iters", ransac_iters=1025)
    T = np.array(good["T_cur"]); T[:4] *= 1 + 2e-7                  # inside the allowance: accepted
    ctx.loop_verify([dict(good, T_cur=T)], lc.CAM, lc.EXT_L)
    # non-ascending ranges, through the ABI itself; the outputs keep their fill
    n = 64
    arr = (svs.LoopJob * 2)()
    for j, (co, qo) in enumerate(((n, n), (0, 0))):
        arr[j].c_ofs, arr[j].nc, arr[j].q_ofs, arr[j].nq = co, n, qo, n
        arr[j].T_cur = (C.c_double * 7)(*good["T_cur"]); arr[j].T_cand = (C.c_double * 7)(*good["T_cand"])
        arr[j].status = -5
    P = svs.LoopParams((C.c_double * 4)(*lc.CAM), (C.c_double * 7)(*lc.EXT_L), 20, 100, 5.991, 20.0, 1.0, 50.0, 0, 0)
    DC = np.ascontiguousarray(np.concatenate([good["desc_c"]] * 2)); DQ = np.ascontiguousarray(np.concatenate([good["desc_q"]] * 2))
    XC = np.ascontiguousarray(np.concatenate([good["xyz_c"]] * 2)); HX = np.ascontiguousarray(np.concatenate([good["has_xyz"]] * 2))
    UV = np.ascontiguousarray(np.concatenate([good["uv_q"]] * 2))
    mc = np.full(2 * n, -7, np.int32); mq = mc.copy(); md = mc.copy(); mi = np.full(2 * n, 9, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.L.svslam_loop_verify_batch(ctx.h, 2, arr, C.byref(P), 2 * n, ptr(DC), ptr(XC), ptr(HX), 2 * n, ptr(DQ), ptr(UV), ptr(mc), ptr(mq),
                                        ptr(md), ptr(mi))
    assert rc != 0 and b"ascend" in ctx.L.svslam_last_error(ctx.h)
    assert (mc == -7).all() and (mq == -7).all() and (md == -7).all() and (mi == 9).all() and arr[0].status == -5 and arr[1].status == -5
    assert ctx.loop_verify([], lc.CAM, lc.EXT_L) == []                # a valid no-op


def test_timing_family(ctx):
    ctx.timing(True)
    ctx.loop_verify([lc.case("n64_64")] * 3, lc.CAM, lc.EXT_L)
    ms, launches, units = ctx.timing_get("loop_verify")
    ctx.timing(False)
    assert launches == 1 and units == 3 and ms > 0
