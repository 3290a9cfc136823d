"""Do the pose-graph cases notice a wrong kernel?  For each single-edit mutation of csrc/k_pose_graph.h below, the kernel source is
copied to a temporary directory, edited there (the anchor must occur exactly once: a source change that moves it fails this test
loudly), compiled for the host like tests/test_host_emulation_pose_graph.py does, and run on the cases, or the direct checks
against 60-digit values (tests/pose_graph_direct.py), that are meant to kill it: at least one of them has to fail, at the tolerances
the device is compared at.  Nothing is written into the repository tree.  CPU only.

ONE KNOWN SURVIVOR, with its reason (SURVIVORS below): pg_exp's small-angle `th2 / 48` as `th2 / 24` is the same function bit for
bit."""
import os
import shutil

import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_direct as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("stereovision-slam_amd", "csrc")
EMU = os.path.join("tests", "cpp", "pg_host_emu", "emu.cpp")
LM = ("loop_full", "nested", "rejected", "n17")
NEW = tuple(pc.new_cases())

# name: (anchor, replacement, the cases and direct checks meant to kill it)
MUTANTS = {
    "assembly: the other Jacobian is always Jr^-1":
        ("*Ju = isa ? o + 42 : o + 6;", "*Ju = o + 42;", ("reversed", "reversed_all", "vertex_perm")),
    "pg_jr_inv: the power series at every angle":
        ("if (theta < 0.1) {", "if (theta < 10.0) {", ("theta_3.0", "theta_pi-1e-5", "direct:jr_inv", "direct:lin_Ja")),
    "pg_jr_inv: the closed form at every angle":
        ("if (theta < 0.1) {", "if (theta < 0.0) {", ("theta_1e-11", "direct:jr_inv")),
    # no graph case notices this one (the closed form is good to 6e-11 there); the 60-digit value at 1e-3 rad does: the series is
    # good to 1e-16 at that angle and the bound follows it
    "pg_jr_inv: the series below 1e-3 only":
        ("if (theta < 0.1) {", "if (theta < 1e-3) {", ("direct:jr_inv", "direct:lin_Ja", "direct:lin_Jr")),
    "pg_log: +pi on both sides of w = 0":
        ("(w > 0 ? M_PI : -M_PI)", "M_PI", ("pi_minus",)),
    "pg_log: small-angle c = 1/6":
        ("if (fabs(theta) < EPS) c = 1.0 / 12.0;", "if (fabs(theta) < EPS) c = 1.0 / 6.0;", ("direct:log",)),
    "a failed factorisation keeps the trial's chi2":
        ("if (!ok) temp = 1.7976931348623157e308;", "", ("overflow",)),
    "a rejected trial does not restore the poses":
        ("PG_PAR { for (int i = tid; i < 7 * nkf; i += PG_THREADS) poses[i] = poses_sv[i]; } PG_SYNC", "", ("rejected",)),
    "nu is not doubled on a rejection":
        ("S.lambda *= S.nu; S.nu *= 2.0;", "S.lambda *= S.nu;", ("rejected", "ten_failed")),
    "nu is not reset on an acceptance":
        ("S.nu = 2.0; S.cur = temp;", "S.cur = temp;", ("rejected",)),
    "lambda0 = 1e-2 max diag":
        ("S.lambda = 1e-5 * md;", "S.lambda = 1e-2 * md;", LM),
    "alpha is not clamped to 2/3":
        ("if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;", "", LM),
    "nine trials per iteration":
        ("while (!stop && rho < 0 && qmax < 10);", "while (!stop && rho < 0 && qmax < 9);", ("ten_failed",)),
    "sign of the b side of the gradient":
        ("if (isa) s -= t; else s += t;", "if (isa) s -= t; else s -= t;", LM),
    "free index 0 is taken for a fixed vertex":
        ("if (fo >= 0 && fo < f) {", "if (fo > 0 && fo < f) {", LM),
    "forward sweep strides by one group too many":
        ("for (int k = fi + g; k < i; k += PG_FWD_GROUPS) {", "for (int k = fi + g; k < i; k += PG_FWD_GROUPS + 1) {", ("spans_9_10_11", "vertex_perm")),
    "backward sweep stops after 64 entries of a row":
        ("for (int w = tid; w < (i - fi) * 6; w += PG_THREADS) {", "for (int w = tid; w < (i - fi) * 6 && w < 64; w += PG_THREADS) {", ("spans_9_10_11",)),
    "lane 63's partial sum is dropped":
        ("for (int t_ = 0; t_ < PG_THREADS; ++t_) s_ += S.part[t_];", "for (int t_ = 0; t_ < PG_THREADS - 1; ++t_) s_ += S.part[t_];", ("n63", "n64")),
    "the largest diagonal entry is sought among the first 64":
        ("for (int w = tid; w < nf * 6; w += PG_THREADS) { const double d = fabs(", "for (int w = tid; w < nf * 6 && w < 64; w += PG_THREADS) { const double d = fabs(",
         ("n17", "spans_9_10_11", "nested")),
    "lambda on three of the six diagonal entries":
        ("PG_BLK(L, w / 6, w / 6)[(w % 6) * 7] += lambda;", "if (w % 6 < 3) PG_BLK(L, w / 6, w / 6)[(w % 6) * 7] += lambda;", LM),
    "Ad without its t x R block":
        ("Ad[i * 6 + j + 3] = TR[i * 3 + j];", "Ad[i * 6 + j + 3] = 0.0;", LM + ("direct:lin_Ja",)),
    "Q with -2 PRP":
        ("- 3.0 * PRP[i]", "- 2.0 * PRP[i]", ("rejected", "theta_2.0", "direct:jr_inv")),
    "H off the diagonal with row and column swapped":
        ("t += Jv[m * 6 + r] * Ju[m * 6 + c];", "t += Jv[m * 6 + c] * Ju[m * 6 + r];", LM),
    "points re-anchored from the new pose":
        ("pg_act(poses0 + 7 * (size_t)a, x, s);", "pg_act(poses + 7 * (size_t)a, x, s);", ("loop_full", "nested", "vertex_perm")),
    "rho's scale without its lambda term":
        ("s += xv[w] * (lambda * xv[w] + bv[w]);", "s += xv[w] * bv[w];", LM),
}
# name: (anchor, replacement, reason)
# the seven edits that used to pass everything, and the closed form at every angle: EVERY listed killer has to fire, so that the
# graph-level killers (reversed, theta_3.0, pi_minus, overflow, ...) are asserted by name and not only one of several
ALL_KILLERS_FIRE = ("assembly: the other Jacobian is always Jr^-1", "pg_jr_inv: the power series at every angle",
                    "pg_jr_inv: the closed form at every angle", "pg_jr_inv: the series below 1e-3 only", "pg_log: +pi on both sides of w = 0",
                    "pg_log: small-angle c = 1/6", "a failed factorisation keeps the trial's chi2")
SURVIVORS = {
    "pg_exp: small-angle th2 / 24":
        ("imag = 0.5 - th2 / 48.0 + th4 / 3840.0;", "imag = 0.5 - th2 / 24.0 + th4 / 3840.0;",
         "equivalent: the branch has th2 < 1e-20, and 0.5 - 4.2e-22 rounds to 0.5 as 0.5 - 2.1e-22 does (half an ulp of 0.5 is 2.8e-17)"),
}


def _mutant(tmp_path, anchor=None, replacement=None):
    """a copy of the kernel source and of the emulation's main file in the same relative places, edited, built at -O1 (quicker;
    without contraction and on SSE2 the optimisation level does not change a bit)"""
    assert not os.path.realpath(str(tmp_path)).startswith(os.path.realpath(ROOT) + os.sep)
    os.makedirs(tmp_path / CSRC); os.makedirs(tmp_path / os.path.dirname(EMU))
    shutil.copy(os.path.join(ROOT, CSRC, "k_pose_graph.h"), tmp_path / CSRC / "k_pose_graph.h")
    shutil.copy(os.path.join(ROOT, EMU), tmp_path / EMU)
    if anchor is not None:
        path = tmp_path / CSRC / "k_pose_graph.h"
        src = path.read_text()
        assert src.count(anchor) == 1, "the anchor of this mutation occurs %d times in k_pose_graph.h" % src.count(anchor)
        path.write_text(src.replace(anchor, replacement))
    return pc.emu_build(tmp_path, tmp_path, opt="-O1")


def _killed_by(lib, what):
    if what.startswith("direct:"):
        return bool(pd.beyond(pd.Emu(lib), pc.TOL_DIRECT, only=(what[7:],)))
    job = pc.cases()[what]
    run = lambda jobs, iters: pc.emu_run(lib, jobs, iters)
    with np.errstate(all="ignore"):
        (got,) = run([job], pc.ITERS[what])
        ok, ties, _ = pc.compare(got, pc.reference(what), pc.tol_of(what))
        if not ok or ties:
            return True
        try:
            pc.check_new_case(what, job, got, run, same_libm=True)
            if what == "ten_failed":
                assert got["iters"] == 1 and got["trials"] == 10
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_is_killed(tmp_path, name):
    anchor, replacement, killers = MUTANTS[name]
    lib = _mutant(tmp_path, anchor, replacement)
    killed = [k for k in killers if _killed_by(lib, k)]
    print(name, "killed by", killed, "of", list(killers))
    assert killed, "no case notices: " + name
    if name in ALL_KILLERS_FIRE:
        assert killed == list(killers), "%s: not noticed by %s" % (name, sorted(set(killers) - set(killed)))


def test_the_unmutated_copy_passes_what_kills_the_mutants(tmp_path):
    """the copy, the build at -O1 and the runner are not what fails"""
    lib = _mutant(tmp_path)
    for k in sorted({k for m in MUTANTS.values() for k in m[2]} | set(NEW)):
        assert not _killed_by(lib, k), k


@pytest.mark.parametrize("name", list(SURVIVORS))
def test_a_known_survivor_survives(tmp_path, name):
    """when a case or a bound is added that kills one, take it out of the survivors and into MUTANTS"""
    anchor, replacement, reason = SURVIVORS[name]
    assert reason
    lib = _mutant(tmp_path, anchor, replacement)
    assert not [n for n in NEW if _killed_by(lib, n)]
    assert not pd.beyond(pd.Emu(lib), pc.TOL_DIRECT)
