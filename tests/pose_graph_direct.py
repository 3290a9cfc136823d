"""The SE(3) functions of csrc/k_pose_graph.h (through tests/cpp/pg_host_emu) and of tests/ref_pose_graph.py one by one against values
computed with mpmath at 60 digits from ANOTHER formulation, so that a flaw the kernel, the emulation and the reference share (they
all use Barfoot's closed forms with the same branch limits) cannot hide:

  exp          mpmath's matrix exponential of the 4x4 twist (Taylor series with scaling and squaring)
  Jl^-1, Jr^-1 the Bernoulli series sum_n B_n / n! ad(xi)^n of the 6x6 adjoint, summed until the terms are below 1e-65
  log          Newton's iteration on expm(xi^) = T from the generating twist, its step taken with the Bernoulli series; the result
               is accepted on its residual |expm(xi^) - T| < 1e-50, so the starting point decides nothing
  J_a, J_b     central differences (h = 1e-25) of that logarithm through exp(d) T, the update the kernel applies
  6x6 inverse  mpmath's LU inverse

The wanted values are computed once per process and shared (test_pose_graph_se3_mpmath.py, test_host_emulation_pose_graph_mutants.py).
An error is |got - want| / scale, the scale of an entry being that of the terms it is summed from (so that an entry that is small
only by cancellation is not held to its own size): see measure() below; the bounds are pose_graph_cases.TOL_DIRECT."""
import ctypes as C
import math

import mpmath as mp
import numpy as np

import ref_pose_graph as rpg

mp.mp.dps = 60
THETAS = (0.0, 1e-12, 0.9e-10, 1.1e-10, 1e-6, 1e-3, 0.0999, 0.1, 0.1001, 0.5, 2.0, 3.0, math.pi - 1e-6)
FLOOR = 1e-30           # absolute floor of a scale: an entry that is exactly 0 is wanted as 0 + the 1e-60 noise of the mpmath value


# ---------------------------------------------------------------- mpmath side
def _hat3(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _hat4(xi):
    A = mp.zeros(4)
    A[:3, :3] = _hat3(xi[3:])
    for i in range(3):
        A[i, 3] = xi[i]
    return A


def _ad(xi):
    """adjoint of the twist, tangent ordered (translation, rotation): [[phi^, rho^], [0, phi^]]"""
    A = mp.zeros(6)
    P, R = _hat3(xi[3:]), _hat3(xi[:3])
    A[:3, :3] = P; A[3:, 3:] = P; A[:3, 3:] = R
    return A


def mp_jl_inv(xi):
    """sum_n B_n / n! ad^n (B_1 = -1/2): the inverse left Jacobian of SE(3); converges for |phi| < 2 pi"""
    A = _ad(xi)
    S = mp.eye(6); Pw = mp.eye(6); fact = mp.mpf(1)
    for n in range(1, 4000):
        Pw = Pw * A; fact *= n
        if n > 1 and n % 2:
            continue
        term = Pw * (mp.bernoulli(n) / fact)
        S += term
        if n > 2 and max(abs(v) for v in term) < mp.mpf(10) ** -65:
            return S
    raise AssertionError("the Bernoulli series did not converge")


def mp_mat(T):
    """the 4x4 matrix of a double[7] pose, exactly (the quaternion normalised in 60 digits)"""
    q = [mp.mpf(float(v)) for v in T[:4]]
    n2 = sum(v * v for v in q)
    x, y, z, w = q
    V = _hat3([x, y, z])
    R = mp.eye(3) + (2 / n2) * (w * V + V * V)
    A = mp.eye(4)
    A[:3, :3] = R
    for i in range(3):
        A[i, 3] = mp.mpf(float(T[4 + i]))
    return A


def _vee_first_order(A):
    """A = I + d^ + O(d^2) -> d"""
    return [A[0, 3], A[1, 3], A[2, 3], (A[2, 1] - A[1, 2]) / 2, (A[0, 2] - A[2, 0]) / 2, (A[1, 0] - A[0, 1]) / 2]


def mp_log(Tm, start, steps=4, Jli=None):
    """xi with expm(xi^) = Tm, by Newton from `start` (exp(d) exp(xi) = exp(xi + Jl^-1(xi) d + O(d^2))).  Jli: Jl^-1 at a point
    1e-25 away, for the differences below (the iteration then gains 25 digits a step, not twice the digits)"""
    xi = [mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in start]
    for _ in range(steps):
        d = _vee_first_order(Tm * mp.expm(_hat4([-v for v in xi])))
        if max(abs(v) for v in d) < mp.mpf(10) ** -55:
            break
        step = (mp_jl_inv(xi) if Jli is None else Jli) * mp.matrix(d)
        xi = [xi[i] + step[i] for i in range(6)]
    res = Tm - mp.expm(_hat4(xi))
    assert max(abs(v) for v in res) < mp.mpf(10) ** -50, "Newton's logarithm did not converge"
    return xi


def _np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


# ---------------------------------------------------------------- samples and wanted values (once per process)
def _axes(rng):
    a = rng.standard_normal(3)
    return [np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, -0.8]), a / np.linalg.norm(a)]


def _twists():
    """(rho, theta x axis): every theta of THETAS about three axes; translations random up to 1 m and, below 1e-9 rad, along one
    coordinate axis (where an entry of the result is the small-angle term alone)"""
    rng = np.random.default_rng(50)
    out = []
    for th in THETAS:
        for k, ax in enumerate(_axes(rng)):
            rho = rng.uniform(-1.0, 1.0, 3)
            if th < 1e-9 and k == 2:
                rho = np.array([0.0, 1.0, 0.0])
            out.append(np.concatenate([rho, th * ax]))
    return out


_WANT = {}


def _once(key, fn):
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def want_exp():
    def fn():
        out = []
        for xi in _twists():
            E = mp.expm(_hat4([mp.mpf(float(v)) for v in xi]))
            out.append((xi, _np(E[:3, :3]), np.array([float(E[i, 3]) for i in range(3)])))
        return out
    return _once("exp", fn)


def want_jr_inv():
    return _once("jr", lambda: [(e, _np(mp_jl_inv([-mp.mpf(float(v)) for v in e]))) for e in _twists()])


def want_log():
    """poses made by ref_pose_graph.se3_exp (any unit quaternion would do), every third with -q (w < 0: the same rotation); wanted
    for the pose as rounded to doubles"""
    def fn():
        out = []
        for k, xi in enumerate(_twists()):
            T = rpg.se3_exp(xi)
            if k % 3 == 1:
                T[:4] *= -1.0
            w = mp_log(mp_mat(T), xi)
            Vi = mp_jl_inv(w)[:3, :3]
            scale = [sum(abs(Vi[i, j] * mp.mpf(float(T[4 + j]))) for j in range(3)) for i in range(3)] + [abs(v) for v in w[3:]]
            out.append((T, np.array([float(v) for v in w]), np.maximum(np.array([float(v) for v in scale]), FLOOR)))
        return out
    return _once("log", fn)


LIN_THETAS = (1e-12, 1.1e-10, 1e-3, 0.0999, 0.1001, 0.5, 2.0, 3.0, math.pi - 1e-6)


def want_linearise():
    """edges (M, T_a, T_b) whose residual has a rotation of LIN_THETAS; wanted: e, J_a and -J_b = Jr^-1(e) by central differences of
    the 60-digit residual through T <- exp(d) T"""
    def fn():
        rng = np.random.default_rng(51)
        h = mp.mpf(10) ** -25
        out = []
        for th in LIN_THETAS:
            ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
            err = np.concatenate([rng.uniform(-1.0, 1.0, 3), th * ax])
            Ta = rpg.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.standard_normal(3)]))
            Tb = rpg.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.standard_normal(3)]))
            M = rpg.se3_mul(rpg.se3_exp(-err), rpg.se3_mul(Ta, rpg.se3_inv(Tb)))        # e = log(M^-1 T_a T_b^-1) ~ Ad(..) err
            Mi, A, Bi = mp_mat(M) ** -1, mp_mat(Ta), mp_mat(Tb) ** -1
            e = mp_log(Mi * A * Bi, rpg.edge_error(M, Ta, Tb))
            Jli = mp_jl_inv(e)
            Ja, Jb = mp.zeros(6), mp.zeros(6)
            for d in range(6):
                for s in (1, -1):
                    dx = [mp.mpf(0)] * 6; dx[d] = s * h
                    X = mp.expm(_hat4(dx))
                    ea = mp.matrix(mp_log(Mi * X * A * Bi, e, steps=3, Jli=Jli))
                    eb = mp.matrix(mp_log(Mi * A * (X * mp_mat(Tb)) ** -1, e, steps=3, Jli=Jli))
                    for i in range(6):
                        Ja[i, d] += s * ea[i] / (2 * h)
                        Jb[i, d] += s * eb[i] / (2 * h)
            out.append((M, Ta, Tb, np.array([float(v) for v in e]), _np(Ja), -_np(Jb)))
        return out
    return _once("lin", fn)


def want_ldlt():
    def fn():
        rng = np.random.default_rng(52)
        out = []
        for k in range(6):
            A = rng.standard_normal((12, 6)) * np.array([1, 1, 1, 5, 5, 5.0]) ** (k % 3)        # the rotation block of H is the larger
            D = A.T @ A + 1e-3 * np.eye(6)
            out.append((D, _np(mp.matrix(D.tolist()) ** -1)))
        return out
    return _once("ldlt", fn)


# ---------------------------------------------------------------- the implementations under test
class Ref:
    """tests/ref_pose_graph.py"""
    log = staticmethod(rpg.se3_log)
    exp = staticmethod(rpg.se3_exp)
    jr_inv = staticmethod(rpg.se3_jr_inv)

    @staticmethod
    def linearise(M, Ta, Tb):
        Ja, Jb = rpg.edge_jac_analytic(M, Ta, Tb)
        return rpg.edge_error(M, Ta, Tb), Ja, -Jb

    @staticmethod
    def ldlt(D):
        return rpg._ldlt6_inv(D)


class Emu:
    """csrc/k_pose_graph.h through the C functions tests/cpp/pg_host_emu/emu.cpp exports"""
    def __init__(self, lib):
        self.lib = lib
        lib.emu_pg_ldlt6_inv.restype = C.c_int

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.c_void_p)

    def _call(self, fn, nout, *ins):
        ins = [np.ascontiguousarray(a, np.float64) for a in ins]
        out = np.zeros(nout)
        rc = fn(*[self._p(a) for a in ins], self._p(out))
        return out, rc

    def log(self, T):
        return self._call(self.lib.emu_pg_log, 6, T)[0]

    def exp(self, xi):
        return self._call(self.lib.emu_pg_exp, 7, xi)[0]

    def jr_inv(self, e):
        return self._call(self.lib.emu_pg_jr_inv, 36, e)[0].reshape(6, 6)

    def linearise(self, M, Ta, Tb):
        o = self._call(self.lib.emu_pg_edge_linearise, 78, M, Ta, Tb)[0]
        return o[:6], o[6:42].reshape(6, 6), o[42:].reshape(6, 6)

    def ldlt(self, D):
        out, rc = self._call(self.lib.emu_pg_ldlt6_inv, 36, D)
        return out.reshape(6, 6), bool(rc)


# ---------------------------------------------------------------- errors, function by function
def _worst(err, scale):
    r = np.abs(np.asarray(err, np.float64)) / scale
    return float("inf") if not np.all(np.isfinite(r)) else float(r.max())       # a NaN is an error of any size


def _rot_of(q):
    return _np(mp_mat(np.concatenate([q, [0, 0, 0]]))[:3, :3])


CLASSES = ("below 1e-10", "1e-10 .. 0.01", "0.01 .. 0.2", "0.2 .. 3.1", "pi - 1e-6")


def cls(theta):
    """the reference's own error changes by orders of magnitude with the angle (Sophus' V cancels as eps / theta below 1e-3 and is
    replaced by R below 1e-10; the closed form of Jr^-1 cancels at the 0.1 rad switch and as eps / (pi - theta) near pi), so a
    bound per function would be set by its worst angle and notice nothing at the others: the bounds are per function and class"""
    return 0 if theta < 1e-10 else 1 if theta < 0.01 else 2 if theta < 0.2 else 3 if theta < 3.1 else 4


def measure(impl):
    """the largest error of each function over the samples of each angle class: {name: [5 errors]} (ldlt: one)"""
    m = {k: [0.0] * 5 for k in ("exp_R", "exp_t", "log", "jr_inv", "lin_e", "lin_Ja", "lin_Jr")}
    m["ldlt"] = [0.0]

    def put(name, c, *errs):
        m[name][c] = max(m[name][c], *errs)
    for xi, R, t in want_exp():
        T = impl.exp(xi); c = cls(np.linalg.norm(xi[3:]))
        put("exp_R", c, _worst(_rot_of(T[:4]) - R, 1.0), abs(float(T[:4] @ T[:4]) - 1.0))      # and a unit quaternion
        put("exp_t", c, _worst(T[4:] - t, max(float(np.abs(xi[:3]).max()), FLOOR)))
    for T, w, scale in want_log():
        put("log", cls(np.linalg.norm(w[3:])), _worst(impl.log(T) - w, scale))
    for e, J in want_jr_inv():
        put("jr_inv", cls(np.linalg.norm(e[3:])), _worst(impl.jr_inv(e) - J, max(1.0, float(np.abs(J).max()))))
    for M, Ta, Tb, e, Ja, Jr in want_linearise():
        ge, gJa, gJr = impl.linearise(M, Ta, Tb); c = cls(np.linalg.norm(e[3:]))
        put("lin_e", c, _worst(ge - e, max(1.0, float(np.abs(e).max()))))
        put("lin_Ja", c, _worst(gJa - Ja, max(1.0, float(np.abs(Ja).max()))))
        put("lin_Jr", c, _worst(gJr - Jr, max(1.0, float(np.abs(Jr).max()))))
    for D, inv in want_ldlt():
        got, ok = impl.ldlt(D)
        assert ok
        put("ldlt", 0, _worst(got - inv, float(np.abs(inv).max())))
    return m


def beyond(impl, tol, only=None):
    """{(function, class): (error, bound)} of what lies beyond its bound"""
    m = measure(impl)
    return {(k, i): (v, tol[k][i]) for k, vs in m.items() if only is None or k in only for i, v in enumerate(vs) if not v <= tol[k][i]}


def check(impl, tol, only=None):
    """every function (or those named) inside its bounds"""
    bad = beyond(impl, tol, only)
    assert not bad, "beyond the bound against the 60-digit value: %s" % bad


def check_ldlt_flags(impl):
    """false where a pivot is not positive and finite; the inverse of a well-conditioned block is still formed then"""
    D = np.diag([2.0, 3.0, -1.0, 4.0, 5.0, 6.0])
    assert not impl.ldlt(D)[1]
    D = np.diag([2.0, 3.0, 0.0, 4.0, 5.0, 6.0])
    with np.errstate(all="ignore"):
        assert not impl.ldlt(D)[1]
        D = np.diag([2.0, 3.0, np.inf, 4.0, 5.0, 6.0])
        assert not impl.ldlt(D)[1]
    assert impl.ldlt(np.diag([2.0, 3.0, 1e-300, 4.0, 5.0, 6.0]))[1]
