"""Global pose-graph optimisation in numpy f64: the numeric contract of svslam_pose_graph_batch.

Written from the reference's LoopClosure::PoseGraphOptimization (src/loopclosure.cpp:641-799), VertexPose / EdgePoseGraph
(include/StereoVisionSLAM/g2o_types.h:25-65, 231-267), Sophus' SE3 exp / log and g2o's OptimizationAlgorithmLevenberg:

  residual of an edge (a, b, M)   log(M^-1 T_a T_b^-1), 6-vector, translation part first
  information                     identity, no robust kernel
  update                          T <- exp(d) T
  LM                              lambda0 = 1e-5 max diag H; rho = (chi2 - chi2') / (d.(lambda d + b) + 1e-3); accepted:
                                  lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; rejected: lambda *= nu, nu *= 2; at most 10
                                  trials per iteration; stop on 10 failed trials, rho == 0 or a non-finite lambda

jac_mode "numeric" is g2o's linearisation of an edge without linearizeOplus (central differences, delta = 1e-9, through
oplus); "analytic" is the closed form J_a = Jr^-1(e) Ad((T_a T_b^-1)^-1), J_b = -Jr^-1(e) the HIP kernel uses.
solver "dense" forms the 6n x 6n system and hands it to numpy.linalg.solve (pivoted LU; the reference's LinearSolverDense);
"envelope" is a block-skyline LDL^T in plain Python, the factorisation the kernel runs.  h_order "edge" sums the blocks of H
edge by edge in ascending edge order (g2o), "reverse" in descending order.
SE(3) is double[7]: unit quaternion x, y, z, w and translation, the layout of Sophus::SE3d."""
import math

import numpy as np

EPS = 1e-10
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------- SE(3)
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def quat_rot(q, v):
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def quat_to_R(q):
    return np.stack([quat_rot(q, e) for e in np.eye(3)], axis=1)


def se3_mul(A, B):
    ax, ay, az, aw = A[:4]
    bx, by, bz, bw = B[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by,
                  aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx,
                  aw * bw - ax * bx - ay * by - az * bz])
    n2 = float(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])      # written out: the host's and the kernel's order (a BLAS dot may differ)
    if n2 != 1.0:                       # Sophus' first-order renormalisation of a quaternion product
        q = q * (2.0 / (1.0 + n2))
    return np.concatenate([q, A[4:] + quat_rot(A[:4], B[4:])])


def se3_inv(T):
    q = np.array([-T[0], -T[1], -T[2], T[3]])
    return np.concatenate([q, quat_rot(q, -T[4:])])


def se3_act(T, p):
    return quat_rot(T[:4], p) + T[4:]


def so3_log(q):
    n2 = float(q[:3] @ q[:3]); w = float(q[3])
    if n2 < EPS * EPS:
        two_atan = 2.0 / w - (2.0 / 3.0) * n2 / (w * w * w)
    else:
        n = math.sqrt(n2)
        if abs(w) < EPS:
            two_atan = (math.pi if w > 0 else -math.pi) / n
        else:
            two_atan = 2.0 * math.atan(n / w) / n
    return two_atan * q[:3]


def se3_log(T):
    om = so3_log(T[:4])
    theta = math.sqrt(float(om @ om))
    O = hat(om)
    if abs(theta) < EPS:
        c = 1.0 / 12.0
    else:
        half = 0.5 * theta
        c = (1.0 - theta * math.cos(half) / (2.0 * math.sin(half))) / (theta * theta)
    Vi = np.eye(3) - 0.5 * O + c * (O @ O)
    return np.concatenate([Vi @ T[4:], om])


def se3_exp(xi):
    u, om = xi[:3], xi[3:]
    th2 = float(om @ om)
    if th2 < EPS * EPS:
        theta = 0.0
        th4 = th2 * th2
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0
        real = 1.0 - th2 / 8.0 + th4 / 384.0
    else:
        theta = math.sqrt(th2)
        imag = math.sin(0.5 * theta) / theta
        real = math.cos(0.5 * theta)
    q = np.array([imag * om[0], imag * om[1], imag * om[2], real])
    if theta < EPS:
        V = quat_to_R(q)
    else:
        O = hat(om)
        V = np.eye(3) + (1.0 - math.cos(theta)) / th2 * O + (theta - math.sin(theta)) / (th2 * theta) * (O @ O)
    return np.concatenate([q, V @ u])


def se3_adj(T):
    R = quat_to_R(T[:4])
    A = np.zeros((6, 6))
    A[:3, :3] = R; A[3:, 3:] = R; A[:3, 3:] = hat(T[4:]) @ R
    return A


def _coeffs(theta):
    """the four scalar functions of the rotation angle in Jl^-1 of SO(3) and in Q of SE(3); power series below 0.1 rad, where the
    closed forms cancel"""
    t2 = theta * theta
    if theta < 0.1:
        c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 / 1209600.0))
        a1 = 1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 / 362880.0))
        a2 = 1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0 - t2 / 3628800.0))
        a3 = 1.0 / 120.0 - t2 * (1.0 / 2520.0 - t2 * (1.0 / 120960.0 - t2 / 9979200.0))
    else:
        s, co = math.sin(theta), math.cos(theta)
        c = 1.0 / t2 - (1.0 + co) / (2.0 * theta * s)
        a1 = (theta - s) / (t2 * theta)
        a2 = (t2 + 2.0 * co - 2.0) / (2.0 * t2 * t2)
        a3 = (2.0 * theta - 3.0 * s + theta * co) / (2.0 * t2 * t2 * theta)
    return c, a1, a2, a3


def se3_jl_inv(xi):
    """inverse left Jacobian of SE(3), tangent ordered (translation, rotation): [[J^-1, -J^-1 Q J^-1], [0, J^-1]]"""
    rho, phi = xi[:3], xi[3:]
    theta = math.sqrt(float(phi @ phi))
    c, a1, a2, a3 = _coeffs(theta)
    P, R = hat(phi), hat(rho)
    PP = P @ P
    Ji = np.eye(3) - 0.5 * P + c * PP
    PR, RP = P @ R, R @ P
    PRP = PR @ P
    Q = 0.5 * R + a1 * (PR + RP + PRP) + a2 * (P @ PR + RP @ P - 3.0 * PRP) + a3 * (PRP @ P + P @ PRP)
    J = np.zeros((6, 6))
    J[:3, :3] = Ji; J[3:, 3:] = Ji; J[:3, 3:] = -Ji @ Q @ Ji
    return J


def se3_jr_inv(xi):
    return se3_jl_inv(-np.asarray(xi))


# ---------------------------------------------------------------- the edge
def edge_error(M, Ta, Tb):
    # associated as M^-1 (T_a T_b^-1): an edge whose measurement is exactly T_a T_b^-1 as the host computes it has e = 0 exactly
    return se3_log(se3_mul(se3_inv(M), se3_mul(Ta, se3_inv(Tb))))


def edge_jac_analytic(M, Ta, Tb):
    e = edge_error(M, Ta, Tb)
    Jri = se3_jr_inv(e)
    Dinv = se3_mul(Tb, se3_inv(Ta))
    return Jri @ se3_adj(Dinv), -Jri


def edge_jac_numeric(M, Ta, Tb, delta=1e-9):
    """g2o BaseBinaryEdge::linearizeOplus: central differences through oplus, one coordinate at a time"""
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    for d in range(6):
        add = np.zeros(6); add[d] = delta
        ep = edge_error(M, se3_mul(se3_exp(add), Ta), Tb)
        em = edge_error(M, se3_mul(se3_exp(-add), Ta), Tb)
        Ja[:, d] = (1.0 / (2.0 * delta)) * (ep - em)
        ep = edge_error(M, Ta, se3_mul(se3_exp(add), Tb))
        em = edge_error(M, Ta, se3_mul(se3_exp(-add), Tb))
        Jb[:, d] = (1.0 / (2.0 * delta)) * (ep - em)
    return Ja, Jb


# ---------------------------------------------------------------- structure and solvers
def free_index(fixed):
    fidx = np.full(len(fixed), -1, np.int64)
    fidx[~np.asarray(fixed, bool)] = np.arange(int((~np.asarray(fixed, bool)).sum()))
    return fidx


def envelope_first(nfree, fidx, ea, eb):
    """first[i]: the smallest free index among row i's neighbours and i itself"""
    first = np.arange(nfree)
    for a, b in zip(ea, eb):
        fa, fb = fidx[a], fidx[b]
        if fa >= 0 and fb >= 0:
            hi, lo = max(fa, fb), min(fa, fb)
            first[hi] = min(first[hi], lo)
    return first


def _ldlt6_inv(D):
    """inverse of a symmetric 6x6 block by an unpivoted scalar LDL^T; ok = every pivot positive and finite"""
    L = np.eye(6); d = np.zeros(6); ok = True
    for i in range(6):
        for j in range(i):
            s = D[i, j]
            for k in range(j):
                s -= L[i, k] * d[k] * L[j, k]
            L[i, j] = s / d[j]
        s = D[i, i]
        for k in range(i):
            s -= L[i, k] * L[i, k] * d[k]
        d[i] = s
        if not (s > 0.0 and math.isfinite(s)):
            ok = False
    inv = np.zeros((6, 6))
    for c in range(6):
        y = np.zeros(6)
        for i in range(6):
            s = 1.0 if i == c else 0.0
            for k in range(i):
                s -= L[i, k] * y[k]
            y[i] = s
        y = y / d
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s -= L[k, i] * y[k]
            y[i] = s
        inv[:, c] = y
    return inv, ok


def solve_envelope(blocks, first, b, lam):
    """block-skyline LDL^T: blocks[(i, j)] (j <= i, lower part, 6x6) is H; rows eliminated in order, fill stays in [first[i], i]"""
    n = len(first)
    L = {}; Dinv = [None] * n; ok = True
    for i in range(n):
        Y = {}
        for j in range(first[i], i):
            acc = blocks.get((i, j), np.zeros((6, 6))).copy()
            for k in range(max(first[i], first[j]), j):
                acc -= Y[k] @ L[(j, k)].T
            Y[j] = acc
            L[(i, j)] = acc @ Dinv[j]
        D = blocks[(i, i)] + lam * np.eye(6)
        for k in range(first[i], i):
            D = D - Y[k] @ L[(i, k)].T
        Dinv[i], good = _ldlt6_inv(D)
        ok = ok and good
    if not ok:
        return None
    z = [None] * n
    for i in range(n):
        s = b[6 * i:6 * i + 6].copy()
        for k in range(first[i], i):
            s -= L[(i, k)] @ z[k]
        z[i] = s
    x = [Dinv[i] @ z[i] for i in range(n)]
    for i in range(n - 1, -1, -1):
        for k in range(first[i], i):
            x[k] = x[k] - L[(i, k)].T @ x[i]
    return np.concatenate(x) if n else np.zeros(0)


def solve_dense(blocks, n, b, lam):
    H = np.zeros((6 * n, 6 * n))
    for (i, j), B in blocks.items():
        H[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
        if i != j:
            H[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
    H += lam * np.eye(6 * n)
    if n == 0:
        return np.zeros(0)
    try:
        np.linalg.cholesky(H)           # LinearSolverDense refuses a matrix that is not positive definite
        return np.linalg.solve(H, b)
    except np.linalg.LinAlgError:
        return None


# ---------------------------------------------------------------- the optimisation
def optimize(poses, fixed, ea, eb, meas, iters=22, jac_mode="analytic", solver="dense", h_order="edge", stats=None):
    """returns (poses, info); info: iters, trials, chi2_before, chi2_after, trace [ntrials, 6] (iteration, lambda, chi2
    before, chi2 of the trial, rho, accepted), max_rot (largest residual rotation angle seen at any trial)"""
    poses = np.array(poses, np.float64).reshape(-1, 7).copy()
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    ea = np.asarray(ea, np.int64).reshape(-1); eb = np.asarray(eb, np.int64).reshape(-1)
    meas = np.asarray(meas, np.float64).reshape(-1, 7)
    ne = len(ea)
    info = dict(iters=0, trials=0, chi2_before=0.0, chi2_after=0.0, trace=np.zeros((0, 6)), max_rot=0.0)
    if len(poses) == 0 or ne == 0:
        return poses, info
    fidx = free_index(fixed); n = int((~fixed).sum())
    first = envelope_first(n, fidx, ea, eb)
    jac = edge_jac_analytic if jac_mode == "analytic" else edge_jac_numeric
    max_rot = [0.0]

    def errors(P):
        E = np.zeros((ne, 6))
        for k in range(ne):
            E[k] = edge_error(meas[k], P[ea[k]], P[eb[k]])
            max_rot[0] = max(max_rot[0], math.sqrt(float(E[k, 3:] @ E[k, 3:])))
        chi = 0.0
        for k in range(ne):
            chi += float(E[k] @ E[k])
        return E, chi

    trace = []
    lam, nu = 0.0, 2.0
    it_done = 0
    chi_first = None
    cur = 0.0
    for it in range(iters):
        E, cur = errors(poses)
        if chi_first is None:
            chi_first = cur
        blocks = {(i, i): np.zeros((6, 6)) for i in range(n)}
        b = np.zeros(6 * n)
        order = range(ne) if h_order == "edge" else range(ne - 1, -1, -1)
        for k in order:
            Ja, Jb = jac(meas[k], poses[ea[k]], poses[eb[k]])
            fa, fb = fidx[ea[k]], fidx[eb[k]]
            for f, J in ((fa, Ja), (fb, Jb)):
                if f >= 0:
                    blocks[(f, f)] += J.T @ J
                    b[6 * f:6 * f + 6] -= J.T @ E[k]
            if fa >= 0 and fb >= 0:
                if fa > fb:
                    blocks[(fa, fb)] = blocks.get((fa, fb), np.zeros((6, 6))) + Ja.T @ Jb
                else:
                    blocks[(fb, fa)] = blocks.get((fb, fa), np.zeros((6, 6))) + Jb.T @ Ja
        if it == 0:
            md = 0.0
            for i in range(n):
                md = max(md, float(np.abs(np.diag(blocks[(i, i)])).max()))
            lam, nu = 1e-5 * md, 2.0
        rho, qmax = 0.0, 0
        while True:
            backup = poses.copy()
            x = solve_envelope(blocks, first, b, lam) if solver == "envelope" else solve_dense(blocks, n, b, lam)
            ok = x is not None and bool(np.all(np.isfinite(x)))
            if ok:
                for v in range(len(poses)):
                    if fidx[v] >= 0:
                        poses[v] = se3_mul(se3_exp(x[6 * fidx[v]:6 * fidx[v] + 6]), poses[v])
            _, temp = errors(poses)
            if not ok:
                temp = DBL_MAX
            rho = cur - temp
            scale = 0.0
            if ok:
                scale = float(np.sum(x * (lam * x + b)))
            scale += 1e-3
            rho /= scale
            accepted = rho > 0 and math.isfinite(temp)
            trace.append([it, lam, cur, temp, rho, 1.0 if accepted else 0.0])
            if stats is not None:
                stats.append(dict(x=None if x is None else x.copy()))
            stop = False
            if accepted:
                alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                lam *= max(alpha, 1.0 / 3.0); nu = 2.0; cur = temp
            else:
                lam *= nu; nu *= 2.0
                poses = backup
                if not math.isfinite(lam):
                    stop = True
            if not stop:
                qmax += 1
            if stop or not (rho < 0 and qmax < 10):
                break
        it_done += 1
        if qmax == 10 or rho == 0 or not math.isfinite(lam):
            break
    info.update(iters=it_done, trials=len(trace), chi2_before=0.0 if chi_first is None else chi_first, chi2_after=cur,
                trace=np.array(trace, np.float64).reshape(-1, 6), max_rot=max_rot[0])
    return poses, info


def reanchor(poses_old, poses_new, pts, anchor):
    """src/loopclosure.cpp:760-784: a point keeps its coordinates in the frame of its anchor keyframe"""
    pts = np.array(pts, np.float64).reshape(-1, 3).copy()
    for i, k in enumerate(np.asarray(anchor, np.int64).reshape(-1)):
        if k >= 0:
            pts[i] = se3_act(se3_inv(poses_new[k]), se3_act(poses_old[k], pts[i]))
    return pts


def pose_graph(job, iters=22, jac_mode="analytic", solver="dense", h_order="edge"):
    """one job as Context.pose_graph takes it; returns the dict that call returns plus trace / max_rot"""
    poses0 = np.array(job["poses"], np.float64).reshape(-1, 7)
    edges = job.get("edges")
    ea, eb, meas = edges if edges is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 7)))
    poses, info = optimize(poses0, job["fixed"], ea, eb, meas, iters, jac_mode, solver, h_order)
    out = dict(poses=poses, iters=info["iters"], trials=info["trials"], chi2_before=info["chi2_before"],
               chi2_after=info["chi2_after"], trace=info["trace"], max_rot=info["max_rot"])
    if job.get("pts") is not None and len(job["pts"]):
        out["pts"] = reanchor(poses0, poses, job["pts"], job["anchor"])
    else:
        out["pts"] = np.zeros((0, 3))
    return out
