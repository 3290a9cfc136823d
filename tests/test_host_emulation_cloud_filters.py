"""csrc/k_cloud_filter.h itself, compiled for the host (tests/cpp/cf_host_emu), against the numpy restatement: the Morton keys, the
cell ranges, the acceptance bound of the block search, the register list and the per-voxel sums checked bit for bit without a
GPU.  Not a replacement for tests/test_gpu_cloud_filters.py (the compiler, the ISA, the device sorts and the launches are not in
it); it is what makes a change of the search's logic visible on a machine without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_cloud_filters as rcf
from cloud_filter_cases import sor_cases, voxel_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "cpp", "cf_host_emu")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("cf_host_emu")
    so = str(d / "libcf_host_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", os.path.join(EMU, "emu.cpp"), "-o", so])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _emu_sor(emu, clouds, mean_k):
    cl = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in clouds]
    ofs = np.zeros(len(cl) + 1, np.int64); ofs[1:] = np.cumsum([len(x) for x in cl])
    xyz = np.ascontiguousarray(np.concatenate(cl + [np.zeros((1, 3), np.float32)]))
    md = np.zeros(int(ofs[-1]) + 1, np.float32); climbs = C.c_uint(0)
    emu.emu_sor_mean_dist(len(cl), _p(ofs), _p(xyz), mean_k, _p(md), C.byref(climbs))
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


def test_voxel_source_on_the_host_equals_the_restatement(emu):
    for name, (xyz, rgb, leaf) in voxel_cases().items():
        inv, min_b, mul, over = rcf._voxel_setup(xyz, leaf)
        assert not over
        oxyz = np.zeros((len(xyz), 3), np.float32); orgb = np.zeros((len(xyz), 3), np.uint8)
        m = emu.emu_voxel_grid(len(xyz), _p(xyz), _p(rgb), C.c_float(inv), _p(min_b.astype(np.int32)), _p(mul.astype(np.int32)), _p(oxyz), _p(orgb))
        wx, wr, _ = rcf.voxel_grid(xyz, rgb, leaf)
        assert m == len(wx) and np.array_equal(oxyz[:m], wx) and np.array_equal(orgb[:m], wr), name
