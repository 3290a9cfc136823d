"""csrc/k_stereo_bm.h itself, compiled for the host and run with 256 threads per workgroup (tests/cpp/bm_host_emu), against the numpy
restatement: the kernel's tiling, chunk dealing, quarter scans, merge, texture word and dispatch checked bit for bit without a GPU.
Not a replacement for tests/test_gpu_stereo_bm.py (the compiler, the ISA and the launch are not in it); it is what makes a one-line
change of the kernel's logic visible on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

import ref_stereo_bm as rbm
from test_gpu_stereo_bm import EARLY_OUT, STRIPS
from test_ref_stereo_bm import band_pair, bw_pair, hand_pairs, texture_ramp_pair, tie_pair, uniqueness_ramp_pair


class BmPlan(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("x0", "x1", "y0", "y1", "th", "tiles", "strips")] + [("lds", C.c_size_t)]


@pytest.fixture(scope="module")
def lib(svs):
    L = C.CDLL(svs._build.build_emu("bm"))
    L.emu_bm_plan.restype = BmPlan
    L.emu_bm_lds_bytes.restype = C.c_longlong
    return L


@pytest.fixture(scope="module")
def emu(lib):
    def run(left, right, th=0, num_disparities=128, block_size=15, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15):
        left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
        h, w = left.shape
        out = np.zeros((h, w), np.int16)
        got_th = lib.emu_stereo_bm(left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), w, h, num_disparities, block_size,
                                   pre_filter_cap, texture_threshold, uniqueness_ratio, th, out.ctypes.data_as(C.c_void_p))
        assert th == 0 or got_th == th
        return out
    return run


def _crop(svs, w, h):
    left, right = svs.synth_pair(1, 0, w=620, h=188)
    y0, x0 = (188 - h) // 2, (620 - w) // 2
    return left[y0:y0 + h, x0:x0 + w].copy(), right[y0:y0 + h, x0:x0 + w].copy()


def _cases(svs):
    per = hand_pairs()["period8"]
    rng = np.random.default_rng(71)
    wide = rng.integers(0, 256, (16, 23), dtype=np.uint8)
    tr, ur = texture_ramp_pair(340, 59, 32), uniqueness_ramp_pair(340, 59, 32)
    p = dict(num_disparities=32, block_size=9)
    return {
        # every window-word count and both pairings of it with the bytes of the last word; five words at strips of 16, 8 and 4
        "bs5": (_crop(svs, 97, 53), dict(num_disparities=32, block_size=5), 0), "bs7": (_crop(svs, 131, 37), dict(num_disparities=16, block_size=7), 0),
        "bs9": (_crop(svs, 200, 48), dict(num_disparities=64, block_size=9), 0), "bs11": (bw_pair(130, 44), dict(num_disparities=32, block_size=11), 0),
        "bs13": (_crop(svs, 141, 39), dict(num_disparities=32, block_size=13), 0), "bs15": (_crop(svs, 150, 30), dict(num_disparities=128, block_size=15), 0),
        "bs17-16": (_crop(svs, 149, 43), dict(num_disparities=48, block_size=17), 16), "bs17-8": (_crop(svs, 149, 43), dict(num_disparities=48, block_size=17), 8),
        "bs17-4": (_crop(svs, 149, 43), dict(num_disparities=48, block_size=17), 4), "bs19-16": (_crop(svs, 157, 47), dict(num_disparities=32, block_size=19), 16),
        "bs19-4": (_crop(svs, 275, 55), dict(num_disparities=160, block_size=19), 4), "bs21": (_crop(svs, 161, 31), dict(num_disparities=16, block_size=21), 0),
        # disparity counts that deal the chunks unevenly
        "nd48": (band_pair(153, 59, 48), dict(num_disparities=48, block_size=9), 0),
        "nd240": (band_pair(312, 59, 240), dict(num_disparities=240, block_size=9), 0),
        # the parameters, on the inputs where they decide
        "cap1": (tr, dict(p, pre_filter_cap=1), 0), "tex8": (tr, dict(p, texture_threshold=8), 0),
        "tex0-uniq0": (tr, dict(p, texture_threshold=0, uniqueness_ratio=0), 0), "uniq0": (ur, dict(p, uniqueness_ratio=0), 0),
        "uniq100": (ur, dict(p, uniqueness_ratio=100), 0),
        # ties
        "period8-ratio0": ((per[0], per[1]), dict(per[2], uniqueness_ratio=0), 0),
        "ties48": (tie_pair(127, 40, 48), dict(num_disparities=48, block_size=9, texture_threshold=0, uniqueness_ratio=0), 0),
        # the smallest image with a computed pixel, and OpenCV's early-out
        "20x16": ((wide[:, :20].copy(), wide[:, 3:].copy()), dict(num_disparities=16, block_size=5), 0),
        "early-out": (_crop(svs, 140, 30), dict(num_disparities=128, block_size=15), 0),
    }


def test_kernel_source_on_the_host_equals_the_restatement(svs, emu):
    bad = []
    for name, ((left, right), prm, th) in _cases(svs).items():
        ref = rbm.stereo_bm(left, right, **prm)
        got = emu(left, right, th, **prm)
        if not np.array_equal(got, ref):
            bad.append((name, int((got != ref).sum())))
    assert not bad, bad


# tiles x strips x njobs of the STRIPS rows, by hand from the comment above them (test_gpu_stereo_bm.py): 8 x 11 x 12, 8 x 22 x 6,
# 3 x 3 x 114, 3 x 5 x 69, 2 x 2 x 256 and, where even strips of 4 stay far below 1024 workgroups, 2 x 8 x 2
WORKGROUPS = [1056, 1056, 1026, 1035, 1024, 32]


def test_plan_is_the_strip_rule_of_the_device_tests(lib):
    """bm_plan, the function svslam_stereo_bm_strip_rows and the launch take their numbers from"""
    def plan(w, h, njobs, nd, bs):
        p = lib.emu_bm_plan(w, h, njobs, nd, bs)
        return {k: getattr(p, k) for k, _ in BmPlan._fields_}
    assert [th for *_, th in STRIPS] == [16, 8, 16, 8, 16, 4]
    for (w, h, nd, bs, njobs, th), wgs in zip(STRIPS, WORKGROUPS):
        p, r = plan(w, h, njobs, nd, bs), bs // 2
        assert p["th"] == th and p["tiles"] * p["strips"] * njobs == wgs, (w, h, nd, bs, njobs, p)
        assert (p["x0"], p["x1"], p["y0"], p["y1"]) == (nd - 1 + r, w - r, r, h - r)
        assert p["tiles"] == -(-(p["x1"] - p["x0"]) // 64) and p["strips"] == -(-(p["y1"] - p["y0"]) // th)
        assert p["lds"] == lib.emu_bm_lds_bytes(nd, bs, th) and p["lds"] <= 160 * 1024
    for w, h, nd, bs in EARLY_OUT:
        p = plan(w, h, 2, nd, bs)
        assert p["th"] == 0 and p["x0"] >= p["x1"] and p["y0"] >= p["y1"], (w, h, nd, bs, p)      # k_bm_fill's window is empty
