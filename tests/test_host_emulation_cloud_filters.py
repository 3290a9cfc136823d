"""csrc/k_cloud_filter.h itself, compiled for the host (tests/cpp/cf_host_emu), against the numpy restatement: the Morton keys, the
cell ranges, the acceptance bound of the block search, the register list and the per-voxel sums checked bit for bit without a
GPU, and with them the file's host functions, the ones the C ABI calls: the segment set-up, PCL's statistics and the voxel plan.
Not a replacement for tests/test_gpu_cloud_filters.py (the compiler, the ISA, the device sorts and the launches are not in
it); it is what makes a change of the search's logic visible on a machine without a device."""
import ctypes as C

import numpy as np
import pytest

import ref_cloud_filters as rcf
from cloud_filter_cases import sor_cases, voxel_cases

f32 = np.float32


class CfSeg(C.Structure):
    _fields_ = [("ofs", C.c_int), ("n", C.c_int), ("mn", C.c_float * 3), ("inv_h", C.c_float), ("h", C.c_float), ("pad", C.c_int)]


class VgParams(C.Structure):
    _fields_ = [("inv", C.c_float), ("min_b", C.c_int * 3), ("mul", C.c_int * 3)]


@pytest.fixture(scope="module")
def emu(svs):
    L = C.CDLL(svs._build.build_emu("cf"))
    L.emu_cf_error.restype = C.c_char_p
    L.emu_cf_sor_decide.restype = C.c_double
    L.emu_cf_sor_decide.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.emu_voxel_grid.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _batch(clouds):
    cl = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in clouds]
    ofs = np.zeros(len(cl) + 1, np.int64); ofs[1:] = np.cumsum([len(x) for x in cl])
    return ofs, np.ascontiguousarray(np.concatenate(cl + [np.zeros((1, 3), np.float32)]))


def _emu_sor(emu, clouds, mean_k):
    ofs, xyz = _batch(clouds)
    md = np.zeros(int(ofs[-1]) + 1, np.float32); climbs = C.c_uint(0)
    assert emu.emu_sor_mean_dist(len(clouds), _p(ofs), _p(xyz), mean_k, _p(md), C.byref(climbs), None, None) == 0
    return [md[a:b] for a, b in zip(ofs[:-1], ofs[1:])], climbs.value


def test_knn_source_on_the_host_equals_the_restatement(svs, emu):
    cases = sor_cases(svs, depth=False)
    names = list(cases)
    for k in (50, 1, 7, 64):
        got, _ = _emu_sor(emu, [cases[n] for n in names], k)           # one batch: the segments share the sort
        bad = [n for n, g in zip(names, got) if not np.array_equal(g, rcf.sor_mean_dist(cases[n], k))]
        assert not bad, (k, bad)
    # the first block is a guess: some queries have to take a larger one (that path ran), most do not (the guess is worth making)
    for n in ("plane", "duplicates", "contrast"):
        _, climbs = _emu_sor(emu, [cases[n]], 50)
        assert 0 < climbs < len(cases[n]) // 4, (n, climbs)


def test_segment_setup_is_numpy_min_and_1024_over_the_extent(svs, emu):
    """cf_segments on the GPU tests' clouds as one call: the box corner, the cell and its inverse in f32, a segment without extent
    (inv_h = 0), an empty one between two others, and the refusal of a NaN with the message svslam_cloud_sor_batch gives"""
    cases = sor_cases(svs, depth=False)
    names = [n for n in cases if n != "n0"]
    names.insert(2, "n0")                                              # empty, between n50 and n51
    ofs, xyz = _batch([cases[n] for n in names])
    segs = (CfSeg * len(names))(); any_ = C.c_int(-1)
    assert emu.emu_sor_mean_dist(len(names), _p(ofs), _p(xyz), 50, None, None, segs, C.byref(any_)) == 0 and any_.value == 1
    for s, n in enumerate(names):
        x, g = cases[n], segs[s]
        assert (g.ofs, g.n) == (int(ofs[s]), len(x)), n
        if len(x) == 0:
            assert (list(g.mn), g.inv_h, g.h) == ([0.0] * 3, 0.0, 0.0), n
            continue
        ext = (x.max(0) - x.min(0)).max()
        assert ext.dtype == f32 and np.array_equal(np.array(list(g.mn), f32), x.min(0)), n
        inv_h = f32(1024.0) / ext if ext > 0 else f32(0.0)
        assert f32(g.inv_h) == inv_h and f32(g.h) == (f32(1.0) / inv_h if inv_h > 0 else f32(0.0)), n
    assert segs[names.index("coincident")].inv_h == 0.0 and segs[names.index("n1000")].inv_h > 0.0
    # no segment has mean_k + 1 points: nothing to search
    ofs2, xyz2 = _batch([cases["n50"], cases["n0"], cases["n1"]])
    assert emu.emu_sor_mean_dist(3, _p(ofs2), _p(xyz2), 50, None, None, segs, C.byref(any_)) == 0 and any_.value == 0
    bad = cases["n65"].copy()
    bad[17, 1] = np.nan
    ofs3, xyz3 = _batch([cases["n51"], bad])
    assert emu.emu_sor_mean_dist(2, _p(ofs3), _p(xyz3), 50, None, None, segs, C.byref(any_)) == -1
    assert emu.emu_cf_error() == b"cloud_filter: point 17 of segment 1 has a non-finite coordinate"


@pytest.mark.parametrize("mul", [1.0, 0.5])
def test_statistics_and_mask_are_the_restatements(svs, emu, mul):
    """cf_sor_decide on the reference's mean distances: the threshold's bits and the mask of ref_cloud_filters.sor; n50 is below
    mean_k + 1 (threshold NaN, everything kept)"""
    cases = sor_cases(svs, depth=False)
    for n in ("n51", "n1000", "n50"):
        want_keep, md, want_thr = rcf.sor(cases[n], 50, mul)
        keep = np.full(len(md), 0xEE, np.uint8)
        thr = emu.emu_cf_sor_decide(len(md), _p(md), 50, mul, _p(keep))
        assert np.float64(thr).tobytes() == np.float64(want_thr).tobytes() or (np.isnan(thr) and np.isnan(want_thr) and n == "n50"), n
        assert np.array_equal(keep, want_keep.astype(np.uint8)), n
        assert np.isnan(thr) == (n == "n50") and (n == "n50" or 0 < keep.sum() < len(keep)), n


def _plan(emu, xyz, leaf):
    """(0 planned, -1 refused, -2 PCL's guard; the plan)"""
    P = VgParams()
    return emu.emu_voxel_grid(len(xyz), _p(np.ascontiguousarray(xyz, f32)), None, leaf, C.byref(P), None, None), P


def test_voxel_plan_is_the_restatements_setup(emu):
    for name, (xyz, rgb, leaf) in voxel_cases().items():
        inv, min_b, mul, over = rcf._voxel_setup(xyz, leaf)
        rc, P = _plan(emu, xyz, leaf)
        assert rc == 0 and not over, name
        assert f32(P.inv) == inv and list(P.min_b) == min_b.tolist() and list(P.mul) == mul.tolist(), name
    # PCL's guard on the clouds of the GPU test: 5001 x 5001 x 251 cells of 2 cm; 46340 x 46341 cells <= INT32_MAX < 46341 x 46341
    xyz = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 5.0], [3.0, 2.0, 1.0]], f32)
    assert _plan(emu, xyz, 0.02)[0] == -2 and rcf._voxel_setup(xyz, 0.02)[3]
    for ex, want in ((46339.5, False), (46340.5, True)):
        xyz = np.array([[0.0, 0.0, 0.0], [ex, 46340.5, 0.5]], f32)
        assert _plan(emu, xyz, 1.0)[0] == (-2 if want else 0) and bool(rcf._voxel_setup(xyz, 1.0)[3]) is want, ex
    # a leaf without a float reciprocal: (float)leaf is 0 or infinite
    for leaf in (1e-46, 1e39):
        assert _plan(emu, xyz, leaf)[0] == -1
        assert emu.emu_cf_error() == b"cloud_filter: leaf %g has no float reciprocal" % leaf
    bad = xyz.copy()
    bad[1, 2] = np.inf
    assert _plan(emu, bad, 1.0)[0] == -1 and emu.emu_cf_error() == b"cloud_filter: point 1 has a non-finite coordinate"


def test_voxel_source_on_the_host_equals_the_restatement(emu):
    for name, (xyz, rgb, leaf) in voxel_cases().items():
        assert not rcf._voxel_setup(xyz, leaf)[3]
        oxyz = np.zeros((len(xyz), 3), np.float32); orgb = np.zeros((len(xyz), 3), np.uint8)
        m = emu.emu_voxel_grid(len(xyz), _p(xyz), _p(rgb), leaf, C.byref(VgParams()), _p(oxyz), _p(orgb))      # the kernels on the library's own plan
        wx, wr, _ = rcf.voxel_grid(xyz, rgb, leaf)
        assert m == len(wx) and np.array_equal(oxyz[:m], wx) and np.array_equal(orgb[:m], wr), name
