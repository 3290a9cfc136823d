"""csrc/k_pose_graph.h itself, compiled for the host (tests/cpp/pg_host_emu, -ffp-contract=off), against tests/ref_pose_graph.py over
every case of pose_graph_cases.py: the plan (free indices, envelope, incidence lists), the closed-form linearisation, the
block-skyline LDL^T, the two sweeps and g2o's LM decisions are checked here without a device.  Not a replacement for
tests/test_gpu_pose_graph.py: the compiler, the ISA, the barriers and the launch are not in it."""
import os

import numpy as np
import pytest

import pose_graph_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return pc.emu_build(ROOT, tmp_path_factory.mktemp("pg_host_emu"))


@pytest.mark.parametrize("name", list(pc.cases()))
def test_kernel_source_on_the_host_against_the_reference(emu, name):
    job = pc.cases()[name]
    ref = pc.reference(name)
    (got,) = pc.emu_run(emu, [job], pc.ITERS[name])
    ok, ties, msg = pc.compare(got, ref, pc.tol_of(name))
    print(name, msg)
    assert ok and ties == 0, msg
    if name == "ten_failed":
        assert got["iters"] == 1 and got["trials"] == 10 and not got["trace"][:, 5].any()       # the ten-failed-trials stop
    if name in ("empty", "n1", "edgeless", "optimum", "zero_chain", "ten_failed"):
        assert np.array_equal(got["poses"], np.asarray(job["poses"]).reshape(-1, 7))          # the input bits
    if name == "optimum":
        assert got["iters"] == 1 and got["trials"] == 1 and got["trace"][0, 4] == 0.0          # stopped by the rho == 0 rule
    if name in ("empty", "n1", "edgeless"):
        assert got["iters"] == 0 and got["trials"] == 0 and got["chi2_before"] == 0.0 and got["chi2_after"] == 0.0
    pc.check_new_case(name, job, got, lambda jobs, iters: pc.emu_run(emu, jobs, iters), same_libm=True)


@pytest.mark.parametrize("name", pc.FULL_RUN_CASES)
def test_final_state_at_the_reference_s_22_iterations(emu, name):
    (got,) = pc.emu_run(emu, [pc.cases()[name]], 22)
    ok, msg = pc.compare_final(got, pc.reference22(name), pc.tol_of(name))
    assert ok, msg


def test_a_job_does_not_depend_on_the_jobs_it_shares_a_call_with(emu):
    c = pc.cases()
    names = list(c)
    together = pc.emu_run(emu, [c[n] for n in names], 22)
    again = pc.emu_run(emu, [c[n] for n in names], 22)
    for i, n in enumerate(names):
        (alone,) = pc.emu_run(emu, [c[n]], 22)
        for k in ("poses", "pts", "trace"):
            assert np.array_equal(alone[k], together[i][k]) and np.array_equal(again[i][k], together[i][k]), (n, k)
        for k in ("iters", "trials", "chi2_before", "chi2_after"):
            assert alone[k] == together[i][k] == again[i][k], (n, k)


def test_refusals_write_nothing(emu):
    base = pc.cases()["span2"]

    def refused(**change):
        job = dict(base); job.update(change)
        job["poses"] = np.array(job["poses"]); keep = job["poses"].copy()
        with pytest.raises(RuntimeError):
            pc.emu_run(emu, [pc.cases()["n2"], job], 5)
        assert np.array_equal(job["poses"], keep)
    ea, eb, meas = base["edges"]
    bad = ea.copy(); bad[2] = 8
    refused(edges=(bad, eb, meas))                                    # index out of range
    bad = ea.copy(); bad[2] = -1
    refused(edges=(bad, eb, meas))
    bad = eb.copy(); bad[3] = ea[3]
    refused(edges=(ea, bad, meas))                                    # a == b
    refused(fixed=np.zeros(8, np.uint8))                              # no fixed vertex
    p = np.array(base["poses"]); p[4, :4] *= 1 + 2e-6
    refused(poses=p)                                                  # |q|^2 off by 4e-6
    m = meas.copy(); m[1, :4] *= 1 - 2e-6
    refused(edges=(ea, eb, m))
    with pytest.raises(RuntimeError, match="no vertices"):
        pc.emu_run(emu, [dict(poses=np.zeros((0, 7)), fixed=np.zeros(0, np.uint8), edges=(ea[:1], eb[:1], meas[:1]))], 2)
    p = np.array(base["poses"]); p[4, :4] *= 1 + 2e-7                 # inside the 1e-6 allowance: accepted
    pc.emu_run(emu, [dict(base, poses=p)], 2)
