"""csrc/k_loop_verify.h itself, compiled for the host (tests/cpp/lv_host_emu, -ffp-contract=off), against tests/ref_loop_verify.py over
every case of loop_verify_cases.py: the Hamming scan, the order-keeping compaction, the hash, the P3P, the inlier counts, the winner,
the LM and the gates are checked here without a device; lv_draw4, lv_R_to_T and lv_p3p also on their own, against the reference's
function of the same name.  The cases with pixel noise are admitted only where this build stays within a tenth of the tolerances: an
unconverged LM amplifies rounding, and the device (whose sin / cos / atan differ) is compared at the whole.  Not a replacement for tests/test_gpu_loop_verify.py: the compiler, the ISA,
the barriers, LDS and the launch are not in it."""
import os

import numpy as np
import pytest

import loop_verify_cases as lc
import ref_loop_verify as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lc.emu_build(ROOT, tmp_path_factory.mktemp("lv_host_emu"))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    ref = lc.reference(name)
    (got,) = lc.emu_run(emu, [lc.case(name)], **lc.params(name))
    ok, msg = lc.compare(got, ref)
    print(name, rl.STATUS_NAMES[ref["status"]], msg)
    assert ok, msg
    if name in lc.NEW:                                          # a tenth of the tolerances; a seed that misses it is replaced
        ok, msg = lc.compare(got, ref, share=0.1)
        assert ok, msg


def test_draw4_against_the_reference(emu):
    lc.check_draw4(emu)


def test_R_to_T_against_the_reference_in_every_branch(emu):
    lc.check_R_to_T(emu)


def test_p3p_against_the_reference(emu):
    lc.check_p3p(emu)


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    by_params = {}
    for n in lc.CASES:
        by_params.setdefault(tuple(sorted(lc.params(n).items())), []).append(n)
    names = max(by_params.values(), key=len)                   # the largest group of cases that share their parameters: sizes 0 .. 1024
    assert len(names) >= 10
    p = lc.params(names[0])
    together = lc.emu_run(emu, [lc.case(n) for n in names], **p)
    again = lc.emu_run(emu, [lc.case(n) for n in names], **p)
    for i, n in enumerate(names):
        (alone,) = lc.emu_run(emu, [lc.case(n)], **p)
        assert lc.same_bits(alone, together[i]) and lc.same_bits(again[i], together[i]), n


def test_refusals_write_nothing(emu):
    good = lc.case("n64_64")

    def refused(match, job=None, **prm):
        with pytest.raises(RuntimeError, match=match):
            lc.emu_run(emu, [good, job if job is not None else good], **prm)      # (emu_run asserts that the match lists kept their fill)
    big = lc.build(seed=1, nc=1025, nq=10, n_match=0)
    refused("1024", job=big)
    big = lc.build(seed=1, nc=10, nq=1025, n_match=0)
    refused("1024", job=big)
    for key in ("T_cur", "T_cand"):
        T = np.array(good[key]); T[:4] *= 1 + 2e-6
        refused("unit length", job=dict(good, **{key: T}))
    T = np.array(good["T_cur"]); T[:4] *= 1 + 2e-7              # inside the allowance: accepted
    lc.emu_run(emu, [dict(good, T_cur=T)])
    refused("ascend", swap_ranges=True)
    refused("ransac_iters", ransac_iters=0)
    refused("ransac_iters", ransac_iters=1025)
    lc.emu_run(emu, [lc.build(seed=1, nc=1024, nq=3, n_match=0)], ransac_iters=1024)
    e = np.array(lc.EXT_L); e[:4] *= 1 - 2e-6
    with pytest.raises(RuntimeError, match="ext_l"):
        lc.emu_run(emu, [good], ext_l=e)
