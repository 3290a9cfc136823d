"""csrc/k_colour.h itself, compiled for the host (tests/cpp/colour_host_emu), against the numpy statement tests/ref_colour.py: the
grey image, the plane, the decimation, the row tails and the gather, bit for bit without a GPU.  Not a replacement for
tests/test_gpu_colour.py (the compiler, the ISA's unaligned 16-byte accesses and the launches are not in it); it is what makes a
change of the kernel's indexing visible on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

import ref_colour as rc
from colour_cases import DEC_DOWN, DEC_UP, DIRECT, KITTI, stereo_pair, strided


@pytest.fixture(scope="module")
def emu(svs):
    L = C.CDLL(svs._build.build_emu("colour"))
    L.emu_colour_bgr_per.restype = C.c_size_t
    L.emu_colour_gather.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _run(emu, img, w, h, plane, nplanes=3):
    sh, sw = img.shape[:2]
    grey = np.full((h, w), 0xEE, np.uint8)
    planes = np.full((nplanes, h, w, 3), 0xEE, np.uint8)
    assert emu.emu_bgr_prepare(C.c_void_p(img.ctypes.data), int(img.strides[0]), sw, sh, w, h, plane, _p(grey), _p(planes)) == 0
    return grey, planes


@pytest.mark.parametrize("case,extra", [(DIRECT, 0), (DIRECT, 5), (DEC_DOWN, 0), (DEC_DOWN, 7), (DEC_UP, 0), (DEC_UP, 1), (KITTI, 0)])
def test_prepare_source_on_the_host_equals_the_restatement(emu, case, extra):
    (sw, sh), (w, h), disp, _ = case
    left, _ = stereo_pair(11, (sw, sh), disp)
    img = strided(left, extra) if extra else left
    want_grey, want_plane = rc.prepare(left, w, h)
    grey, planes = _run(emu, img, w, h, 1)
    assert np.array_equal(grey, want_grey)
    assert np.array_equal(planes[1], want_plane)
    assert (planes[0] == 0xEE).all() and (planes[2] == 0xEE).all()        # nothing outside the named plane
    grey, planes = _run(emu, img, w, h, -1)
    assert np.array_equal(grey, want_grey) and (planes == 0xEE).all()      # -1: no plane is touched


@pytest.mark.parametrize("size,ctx", [((16, 16), (16, 16)), ((31, 33), (16, 16)), ((32, 31), (16, 16)), ((33, 35), (16, 18)), ((17, 19), (17, 19)),
                                      ((63, 37), (32, 18)), ((65, 41), (32, 20)), ((48, 16), (48, 16)), ((49, 17), (49, 17))])
def test_prepare_at_the_smallest_sizes_and_row_tails(emu, size, ctx):
    """the window that is moved back to end with the row, the odd source width that leaves it three bytes short, and the row
    shorter than one window (a 31-pixel source at a 16-pixel context)"""
    rng = np.random.default_rng(size[0] * 100 + size[1])
    img = rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)
    assert ctx == size or rc.halves_to(*size) == ctx
    want_grey, want_plane = rc.prepare(img, *ctx)
    grey, planes = _run(emu, img, ctx[0], ctx[1], 0, nplanes=1)
    assert np.array_equal(grey, want_grey) and np.array_equal(planes[0], want_plane)


def test_gather_source_on_the_host_equals_indexing(emu):
    rng = np.random.default_rng(3)
    w, h, nplanes = 37, 11, 4
    planes = rng.integers(0, 256, (nplanes, h, w, 3), dtype=np.uint8)
    for max_pts in (w * h, 50, 51, 1):
        counts = np.array([max_pts, max_pts - 1 if max_pts > 1 else 0, max_pts + 1, min(5, max_pts)], np.int32)     # job 2 overflowed: no list
        plane_of = np.array([2, 0, 1, 2], np.int32)
        pix = rng.integers(0, w * h, (4, max_pts)).astype(np.int32)
        out_per = emu.emu_colour_bgr_per(max_pts)                  # the size svslam_dense_cloud_bgr_batch allocates per job
        assert out_per == (3 * ((max_pts + 3) // 4) * 4 + 15) & ~15
        out = np.full((4, out_per), 0xEE, np.uint8)
        emu.emu_colour_gather(4, _p(counts), _p(plane_of), _p(pix), max_pts, _p(planes), w * h * 3, _p(out), out_per)
        for j in range(4):
            n = int(counts[j])
            if n > max_pts:
                assert (out[j] == 0xEE).all()
                continue
            want = planes[plane_of[j]].reshape(-1, 3)[pix[j, :n]]
            assert np.array_equal(out[j, :3 * n].reshape(-1, 3), want), (max_pts, j)
            assert (out[j, 3 * ((n + 3) // 4) * 4:] == 0xEE).all()
