"""pg_log, pg_exp, pg_jr_inv, pg_edge_linearise and pg_ldlt6_inv of csrc/k_pose_graph.h (compiled for the host, tests/cpp/pg_host_emu)
and the functions of tests/ref_pose_graph.py they mirror, one by one against 60-digit values that come from another formulation
(tests/pose_graph_direct.py: matrix exponential, Bernoulli series of ad, Newton's logarithm, central differences of the residual).
The kernel, its emulation and the reference share Barfoot's closed forms and their branch limits; this is the check that does not.
Bounds: pose_graph_cases.TOL_DIRECT, ten times the reference's own measured error.  CPU only."""
import os

import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_direct as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return pd.Emu(pc.emu_build(ROOT, tmp_path_factory.mktemp("pg_host_emu")))


def _report(who, m):
    for k, v in m.items():
        print("%-8s %-7s" % (who, k), " ".join("%.1e" % x for x in v))


def test_the_reference_against_the_60_digit_values():
    m = pd.measure(pd.Ref)
    _report("ref", m)
    bad = {(k, i): (v, pc.TOL_DIRECT[k][i]) for k, vs in m.items() for i, v in enumerate(vs) if not v <= pc.TOL_DIRECT[k][i]}
    assert not bad, bad
    pd.check_ldlt_flags(pd.Ref)


def test_the_kernel_s_functions_against_the_60_digit_values(emu):
    m = pd.measure(emu)
    _report("kernel", m)
    bad = {(k, i): (v, pc.TOL_DIRECT[k][i]) for k, vs in m.items() for i, v in enumerate(vs) if not v <= pc.TOL_DIRECT[k][i]}
    assert not bad, bad
    pd.check_ldlt_flags(emu)


def test_the_bounds_are_the_measurement_s():
    """every bound is at least 4 ulp and none is looser than a hundred times the reference's error now (ten times when it was
    measured): a bound that no longer follows the measurement is noticed"""
    m = pd.measure(pd.Ref)
    for k, vs in m.items():
        for i, v in enumerate(vs):
            b = pc.TOL_DIRECT[k][i]
            assert b >= 8.8e-16 and (b <= 100 * v or b <= 8.9e-16 * 2.5), (k, i, v, b)


def test_jr_inv_is_minus_j_b_and_the_samples_cover_the_branches():
    """the third block of pg_edge_linearise is Jr^-1(e), checked as -J_b by differences; the samples lie on both sides of every
    branch limit of the three functions and include w < 0"""
    th = np.array([np.linalg.norm(e[3:]) for e, _ in pd.want_jr_inv()])
    for lo, hi in ((0, 0), (1e-13, 1e-10), (1e-10, 1.2e-10), (0.09, 0.1 - 1e-9), (0.1, 0.1), (0.1 + 1e-9, 0.11), (2.9, 3.1), (3.14, np.pi)):
        assert ((th >= lo) & (th <= hi)).any(), (lo, hi)
    assert sum(T[3] < 0 for T, _, _ in pd.want_log()) >= 10
    for M, Ta, Tb, e, Ja, Jr in pd.want_linearise():
        J = pd._np(pd.mp_jl_inv([-pd.mp.mpf(float(v)) for v in e]))
        assert np.abs(J - Jr).max() < 1e-13          # e as rounded to doubles: the two 60-digit formulations agree with each other
