"""Do the loop-candidate cases notice a wrong kernel?  For each single-edit mutation of csrc/k_loop_candidates.h below, the kernel source
is copied to a temporary directory, edited there (the anchor must occur exactly once: a source change that moves it fails this test
loudly), compiled for the host like tests/test_host_emulation_loop_candidates.py does, and run on the named cases meant to kill it: at
least one has to fail.  Nothing is written into the repository tree.  CPU only.

The tree lives in the host build's lc_wave_sum; the device build's butterfly is a second implementation of the same sum that only
tests/test_gpu_loop_candidates.py reaches."""
import os
import shutil

import pytest

import loop_candidates_cases as lc

CSRC = os.path.join("stereovision-slam_amd", "csrc")

# name: (anchor, replacement, the cases meant to kill it)
MUTANTS = {
    "a later row of the same similarity replaces the best (sim > best as >=)":
        ("if (sim > B.sim) { B.sim = sim; B.id = id; }", "if (sim >= B.sim) { B.sim = sim; B.id = id; }", ("tie_one_wave", "all_nonpositive")),
    "best < strong as <=":
        ("else if (B.sim < P.strong) st = LC_BELOW_STRONG;", "else if (B.sim <= P.strong) st = LC_BELOW_STRONG;", ("strong_at_own_bits",)),
    "n_weak > max_num_weak as >=":
        ("else if (B.n_weak > P.max_num_weak) st = LC_TOO_MANY_WEAK;", "else if (B.n_weak >= P.max_num_weak) st = LC_TOO_MANY_WEAK;",
         ("n_weak_at_max", "weak_at_own_bits")),
    "the count's sim > weak as >=":
        ("if (sim > weak) B.n_weak++;", "if (sim >= weak) B.n_weak++;", ("weak_at_own_bits",)),
    "the gap's < as <=":
        ("!(J.kf_id - id[k] < P.min_gap)", "!(J.kf_id - id[k] <= P.min_gap)", ("gap_by_id",)),
    "the tie rule between waves reversed":
        ("(b.sim == A.sim && b.id < A.id)", "(b.sim == A.sim && b.id > A.id)", ("tie_two_waves", "tie_three_groups")),
    "no tie rule between waves: the first wave keeps the best":
        ("(b.sim > A.sim || (b.sim == A.sim && b.id < A.id))", "(b.sim > A.sim)", ("tie_lower_id_in_a_later_wave",)),
    "one tree step dropped":
        ("for (int s = 32; s >= 1; s >>= 1)\n        for (int l = 0; l < s; ++l)", "for (int s = 32; s >= 2; s >>= 1)\n        for (int l = 0; l < s; ++l)",
         ("dim_63", "dim_1280", "rows_5")),
    "the tree starts at 16":
        ("for (int s = 32; s >= 1; s >>= 1)\n        for (int l = 0; l < s; ++l)", "for (int s = 16; s >= 1; s >>= 1)\n        for (int l = 0; l < s; ++l)",
         ("dim_63", "dim_1280")),
    "the terms of a lane's 16 bytes out of order":
        ("acc[k] = acc[k] + x[k].x * y.x;\n            acc[k] = acc[k] + x[k].y * y.y;", "acc[k] = acc[k] + x[k].y * y.y;\n            acc[k] = acc[k] + x[k].x * y.x;",
         ("dim_1280", "dim_4096", "rows_600_dim_4096")),
}


def _mutant(tmp_path, anchor=None, replacement=None):
    assert not os.path.realpath(str(tmp_path)).startswith(os.path.realpath(lc.ROOT) + os.sep)
    os.makedirs(tmp_path / CSRC); os.makedirs(tmp_path / os.path.dirname(lc.EMU))
    shutil.copy(os.path.join(lc.ROOT, CSRC, "k_loop_candidates.h"), tmp_path / CSRC / "k_loop_candidates.h")
    shutil.copy(os.path.join(lc.ROOT, lc.EMU), tmp_path / lc.EMU)
    if anchor is not None:
        path = tmp_path / CSRC / "k_loop_candidates.h"
        src = path.read_text()
        assert src.count(anchor) == 1, "the anchor of this mutation occurs %d times in k_loop_candidates.h" % src.count(anchor)
        path.write_text(src.replace(anchor, replacement))
    return lc.EmuDriver(lc.emu_build(tmp_path, tmp_path, opt="-O1"))


def _killed_by(drv, name):
    return not lc.compare(lc.run(name, drv), lc.reference(name))[0]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_is_killed(tmp_path, name):
    anchor, replacement, killers = MUTANTS[name]
    drv = _mutant(tmp_path, anchor, replacement)
    killed = [k for k in killers if _killed_by(drv, k)]
    print(name, "killed by", killed, "of", list(killers))
    assert killed, "no case notices: " + name


def test_the_unmutated_copy_passes_what_kills_the_mutants(tmp_path):
    """the copy, the build at -O1 and the runner are not what fails"""
    drv = _mutant(tmp_path)
    for k in sorted({k for m in MUTANTS.values() for k in m[2]}):
        assert not _killed_by(drv, k), k
