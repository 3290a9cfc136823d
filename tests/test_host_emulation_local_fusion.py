"""csrc/k_local_fusion.h itself, compiled for the host (tests/cpp/lf_host_emu, -ffp-contract=off), against tests/ref_local_fusion.py bit
for bit over every call of local_fusion_cases.py: the host's rules (lf_plan), the buffer layout, the corrected table, the search for
the first valid observation and the copy-out are checked here without a device.  Not a replacement for
tests/test_gpu_local_fusion.py: the compiler, the ISA, the barrier and the launch are not in it."""
import ctypes as C
import os

import numpy as np
import pytest

import local_fusion_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return lc.emu_build(ROOT, tmp_path_factory.mktemp("lf_host_emu"))


def test_the_cases_are_cut_for_the_kernel_s_block_size(emu):
    assert emu.emu_lf_threads() == lc.THREADS


@pytest.mark.parametrize("name", list(lc.calls()))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    jobs = lc.calls()[name]
    got = lc.emu_run(emu, jobs)
    why = lc.same_bits(got, lc.reference(name))
    assert why is None, why
    for g, j in zip(got, jobs):
        assert np.array_equal(g["T_cur"], np.asarray(j["T_cur"]))         # an inactive cur is written nowhere
        if j["cur"] >= 0:
            assert np.array_equal(g["poses"][j["cur"]], np.asarray(j["T_corr"]))


def test_the_observation_lists_choose_what_the_rule_says(emu):
    (got,) = lc.emu_run(emu, lc.calls()["obs_lists_cur_outside"])
    assert list(got["pt_kf"]) == [-1, 2, -1, 1, 3, 0, 4, -1, 4, 3] and got["n_unanchored"] == 3
    (got,) = lc.emu_run(emu, lc.calls()["obs_lists"])
    assert list(got["pt_kf"]) == [-1, 2, -1, 1, 3, 0, 3, -1, 3, 3] and got["n_unanchored"] == 3


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    jobs = lc.calls()["three_jobs"]
    together = lc.emu_run(emu, jobs)
    for i, j in enumerate(jobs):
        (alone,) = lc.emu_run(emu, [j])
        assert lc.same_bits([alone], [together[i]]) is None, i
    assert lc.same_bits(lc.emu_run(emu, jobs), together) is None


def test_gaps_between_the_jobs_come_back_untouched(emu):
    jobs = lc.refusal_base()
    arr, P, X, OP, OK = lc.pack(jobs)
    # three keyframes and five landmarks (without observations) that belong to no job, between job 0 and job 1
    P2 = np.concatenate([P[:4], np.full((3, 7), 7.5), P[4:]]); X2 = np.concatenate([X[:20], np.full((5, 3), -3.25), X[20:]])
    OP2 = np.concatenate([OP[:21], np.full(5, OP[20], np.int32), OP[21:]])
    arr[1].kf_ofs += 3; arr[1].pt_ofs += 5
    K = np.full(len(X2), -7, np.int32)
    lc.emu_call(emu, arr, 2, P2, X2, OP2, OK, K)
    assert (P2[4:7] == 7.5).all() and (X2[20:25] == -3.25).all() and (K[20:25] == -7).all()
    ref = [lc.rlf.fuse(j) for j in jobs]
    assert np.array_equal(P2[:4], ref[0]["poses"]) and np.array_equal(P2[7:], ref[1]["poses"])
    assert np.array_equal(X2[:20], ref[0]["pts"]) and np.array_equal(X2[25:], ref[1]["pts"])
    assert np.array_equal(K[:20], ref[0]["pt_kf"]) and np.array_equal(K[25:], ref[1]["pt_kf"])


@pytest.mark.parametrize("name", [r[0] for r in lc.refusals()])
def test_a_refusal_writes_nothing(emu, name):
    edit, text = next((r[1], r[2]) for r in lc.refusals() if r[0] == name)
    arr, P, X, OP, OK = lc.pack(lc.refusal_base())
    K = np.full(len(X), -7, np.int32)
    lc.emu_call(emu, lc.pack(lc.refusal_base())[0], 2, P.copy(), X.copy(), OP, OK, K.copy())        # the unedited call is accepted
    edit(arr, P, X, OP, OK)
    keep = (P.copy(), X.copy(), K.copy(), bytes(arr))
    with pytest.raises(RuntimeError, match=text):
        lc.emu_call(emu, arr, 2, P, X, OP, OK, K)
    assert np.array_equal(P, keep[0]) and np.array_equal(X, keep[1]) and np.array_equal(K, keep[2]) and bytes(arr) == keep[3]


def test_null_arrays_and_negative_totals_are_refused_and_an_empty_call_is_not(emu):
    arr, P, X, OP, OK = lc.pack(lc.refusal_base())
    K = np.full(len(X), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [2, arr, len(P), p(P), len(X), p(X), p(OP), len(OK), p(OK), p(K)]
    for i in (1, 3, 5, 6, 8, 9):                                  # jobs, poses, pts, obs_ptr, obs_kf, pt_kf
        a = list(full); a[i] = None
        assert emu.emu_local_fusion(*a) == -1 and b"null" in emu.emu_lf_error(), i
    for i in (0, 2, 4, 7):                                        # njobs, total_kf, total_pts, total_obs
        a = list(full); a[i] = -1
        assert emu.emu_local_fusion(*a) == -1 and b"negative count" in emu.emu_lf_error(), i
    assert (K == -7).all()
    assert emu.emu_local_fusion(0, None, 0, None, 0, None, None, 0, None, None) == 0
    assert emu.emu_local_fusion(0, None, len(P), p(P), len(X), p(X), p(OP), len(OK), p(OK), p(K)) == 0 and (K == -7).all()
    q = np.array(lc.refusal_base()[1]["poses"]); q[2, :4] *= 1 + 2e-7          # inside the 1e-6 allowance: accepted
    lc.emu_run(emu, [dict(lc.refusal_base()[1], poses=q)])
