"""Geometric verification of a loop candidate in numpy f64: the numeric contract of svslam_loop_verify_batch.

Written from the reference's LoopClosure::KeypointMatchWithLoopCandid and LoopClosure::CalculatePose (src/loopclosure.cpp:286-437,
called at :831-862):

  match     BruteForce-Hamming match(query = candidate, train = current): every candidate row takes the nearest current row
            (popcount of the XOR over 256 bits, the lowest current index on a tie, no cross-check); thr = max(2 d_min, 30);
            matches with distance <= thr are kept, in ascending (candidate row, current row)          FEW_MATCHES below min_matches
  3-D       matches whose candidate feature has no landmark are dropped; landmarks rounded to float32 (cv::Point3f), all that
            follows in f64                                                                             FEW_POINTS below max(min_matches, 4)
  RANSAC    OpenCV is not restated: `ransac_iters` hypotheses, hypothesis i draws 4 distinct point indices from a stateless hash of
            (seed, i, draw), P3P on the first three, the fourth chooses among the solutions; inlier: depth > 0 and squared
            reprojection error <= reproj_px^2; the winner has the most inliers, the lowest i on a tie  FEW_INLIERS below min_matches
  refine    LM on exp(d) T over the winner's inliers, squared pixel error, no robust kernel, g2o's control (ref_pose_graph.py), 10 iterations
  gates     T_corr = ext_l^-1 T_pnp, T_rel = T_corr T_cand^-1; |log T_rel| > max_pose_distance: TOO_FAR;
            d = |log(T_cur T_corr^-1)| > max_pose_difference: TOO_DIFFERENT; else ACCEPTED, need_correction = d > min_pose_difference

The P3P uses + - * / sqrt only, in a written-out order: distances s_i along the unit bearings, s_2 = u s_1, s_3 = v s_1, the law of
cosines on the three sides, u = N(v) / D(v) and a quartic in v whose positive roots are bracketed between the roots of its
derivatives and bisected to adjacent doubles.  An implementation that keeps the order reproduces the hypotheses bit for bit."""
import math

import numpy as np

from ref_pose_graph import DBL_MAX, quat_to_R, se3_exp, se3_inv, se3_log, se3_mul

ACCEPTED, FEW_MATCHES, FEW_POINTS, FEW_INLIERS, TOO_FAR, TOO_DIFFERENT = range(6)
STATUS_NAMES = ("ACCEPTED", "FEW_MATCHES", "FEW_POINTS", "FEW_INLIERS", "TOO_FAR", "TOO_DIFFERENT")
MAX_DESC = 1024
MAX_DRAWS = 64
BISECT = 128
LM_ITERS = 10
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
# the reference's constants (src/loopclosure.cpp:381) and the keys of tests/golden/config-00.yaml
DEFAULTS = dict(min_matches=20, ransac_iters=100, reproj_px=5.991, max_pose_distance=20.0, min_pose_difference=1.0,
                max_pose_difference=50.0, seed=0)
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- match
def hamming_match(desc_c, desc_q):
    """per candidate row: (nearest current row, distance); uint8 [n, 32] each"""
    lut = np.array([bin(i).count("1") for i in range(256)], np.int32)
    bj = np.zeros(len(desc_c), np.int64); bd = np.zeros(len(desc_c), np.int64)
    for c in range(len(desc_c)):
        d = lut[np.bitwise_xor(desc_q, desc_c[c][None, :])].sum(axis=1)
        bj[c] = int(np.argmin(d))               # the first minimum: the lowest index on a tie
        bd[c] = int(d[bj[c]])
    return bj, bd


# ---------------------------------------------------------------- hypothesis
def lv_hash(seed, i, draw):
    h = (seed ^ ((i * 0x9E3779B1) & M32) ^ ((draw * 0x85EBCA77) & M32)) & M32
    h ^= h >> 16; h = (h * 0x7feb352d) & M32; h ^= h >> 15; h = (h * 0x846ca68b) & M32; h ^= h >> 16
    return h


def draw4(seed, i, n):
    idx = []; draw = 0
    for _ in range(4):
        while True:
            if draw >= MAX_DRAWS:
                return None
            v = (lv_hash(seed, i, draw) * n) >> 32
            draw += 1
            if v not in idx:
                idx.append(v); break
    return idx


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _frame(p1, p2, p3):
    d1 = [p2[k] - p1[k] for k in range(3)]; d2 = [p3[k] - p1[k] for k in range(3)]
    n = _cross(d1, d2)
    l1, l2, ln = _dot(d1, d1), _dot(d2, d2), _dot(n, n)
    if not (ln > 1e-12 * (l1 * l2)) or not (ln < math.inf):
        return None
    s1, sn = math.sqrt(l1), math.sqrt(ln)
    e1 = [d1[k] / s1 for k in range(3)]; e3 = [n[k] / sn for k in range(3)]
    return [e1, _cross(e3, e1), e3]


def _horner(c, v):
    s = c[-1]
    for k in range(len(c) - 2, -1, -1):
        s = s * v + c[k]
    return s


def bracket_roots(c, crit, B):
    roots = []
    lo, flo = 0.0, _horner(c, 0.0)
    for hi in list(crit) + [B]:
        fhi = _horner(c, hi)
        if (flo < 0.0 and fhi > 0.0) or (flo > 0.0 and fhi < 0.0):
            a, b = lo, hi
            for _ in range(BISECT):
                mid = 0.5 * (a + b)
                if not (mid > a and mid < b):
                    break
                fm = _horner(c, mid)
                if fm == 0.0:
                    a = b = mid; break
                if (fm < 0.0) == (flo < 0.0):
                    a = mid
                else:
                    b = mid
            roots.append(0.5 * (a + b))
        lo, flo = hi, fhi
    return roots


def p3p(X, f):
    """X, f: three world points and three unit bearings (lists of 3 lists of Python floats) -> list of (R as 9 floats row major, t)"""
    Ex = _frame(X[0], X[1], X[2])
    if Ex is None:
        return []
    c12, c13, c23 = _dot(f[0], f[1]), _dot(f[0], f[2]), _dot(f[1], f[2])
    t = [X[1][k] - X[2][k] for k in range(3)]; a = _dot(t, t)
    t = [X[0][k] - X[2][k] for k in range(3)]; b = _dot(t, t)
    t = [X[0][k] - X[1][k] for k in range(3)]; c = _dot(t, t)
    ca = c - a
    n0, n1, n2 = ca - b, -2.0 * ca * c13, ca + b
    d0, d1 = -2.0 * b * c12, 2.0 * b * c23
    e0, e1, e2 = -a, 2.0 * a * c13, b - a
    nn = [n0 * n0, 2.0 * n0 * n1, 2.0 * n0 * n2 + n1 * n1, 2.0 * n1 * n2, n2 * n2]
    nd = [0.0, n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1]
    dd = [d0 * d0, 2.0 * d0 * d1, d1 * d1]
    ed = [e0 * dd[0], e0 * dd[1] + e1 * dd[0], (e0 * dd[2] + e1 * dd[1]) + e2 * dd[0], e1 * dd[2] + e2 * dd[1], e2 * dd[2]]
    g = 2.0 * b * c23
    q = [(b * nn[k] - g * nd[k]) + ed[k] for k in range(5)]
    mx = max(abs(v) for v in q)
    if not (abs(q[4]) > 1e-12 * mx) or not (mx < math.inf):
        return []
    m = [q[k] / q[4] for k in range(4)] + [1.0]
    B = max(abs(v) for v in m[:4]) + 1.0
    p1 = [m[1], 2.0 * m[2], 3.0 * m[3], 4.0]
    p2 = [2.0 * m[2], 6.0 * m[3], 12.0]
    r2 = []
    disc = p2[1] * p2[1] - 4.0 * p2[2] * p2[0]
    if disc > 0.0:
        sq = math.sqrt(disc)
        ra, rb = (-p2[1] - sq) / (2.0 * p2[2]), (-p2[1] + sq) / (2.0 * p2[2])
        if 0.0 < ra < B:
            r2.append(ra)
        if 0.0 < rb < B and rb > ra:
            r2.append(rb)
    r3 = bracket_roots(p1, r2, B)
    r4 = bracket_roots(m, r3, B)
    out = []
    for v in r4:
        Dv = d1 * v + d0
        if Dv == 0.0:
            continue
        u = ((n2 * v + n1) * v + n0) / Dv
        Av = (1.0 + v * v) - 2.0 * c13 * v
        if not (u > 0.0) or not (v > 0.0) or not (Av > 0.0):
            continue
        s1 = math.sqrt(b / Av); s2 = u * s1; s3 = v * s1
        Y = [[s1 * f[0][k] for k in range(3)], [s2 * f[1][k] for k in range(3)], [s3 * f[2][k] for k in range(3)]]
        Ey = _frame(Y[0], Y[1], Y[2])
        if Ey is None:
            continue
        R = [(Ey[0][i] * Ex[0][j] + Ey[1][i] * Ex[1][j]) + Ey[2][i] * Ex[2][j] for i in range(3) for j in range(3)]
        tt = [Y[0][i] - ((R[3 * i] * X[0][0] + R[3 * i + 1] * X[0][1]) + R[3 * i + 2] * X[0][2]) for i in range(3)]
        if all(abs(x) < math.inf for x in R + tt):
            out.append((R, tt))
    return out


def reproj2(cam, R, t, xyz, uv):
    """squared pixel error of every point and whether it lies in front of the camera; the kernel's order of operations"""
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pc0 = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
    pc1 = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
    pc2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
    front = pc2 > 0.0
    with np.errstate(all="ignore"):
        ex = uv[:, 0] - (cam[0] * pc0 / pc2 + cam[2])
        ey = uv[:, 1] - (cam[1] * pc1 / pc2 + cam[3])
        e2 = ex * ex + ey * ey
    return e2, front


def bearings(cam, uv):
    out = []
    for p in uv:
        x = (float(p[0]) - cam[2]) / cam[0]; y = (float(p[1]) - cam[3]) / cam[1]
        n = math.sqrt((x * x + y * y) + 1.0)
        out.append([x / n, y / n, 1.0 / n])
    return out


def hypothesis(cam, xyz, uv, seed, i):
    """xyz [n, 3] (float32 values in f64), uv [n, 2] f64 -> (R, t) or None"""
    idx = draw4(seed, i, len(xyz))
    if idx is None:
        return None
    X = [[float(v) for v in xyz[k]] for k in idx[:3]]
    sols = p3p(X, bearings(cam, uv[idx[:3]]))
    best = None; be = 0.0
    for R, t in sols:
        e2, front = reproj2(cam, R, t, xyz[idx[3]:idx[3] + 1], uv[idx[3]:idx[3] + 1])
        if not front[0] or not (e2[0] < math.inf):
            continue
        if best is None or e2[0] < be:
            best, be = (R, t), float(e2[0])
    return best


def quat_branch(R):
    """which of R_to_T's four branches a rotation takes: 1 (trace > 0), 2, 3, 4 (the largest diagonal element is R[0], R[4], R[8])"""
    if (R[0] + R[4]) + R[8] > 0.0:
        return 1
    if R[0] > R[4] and R[0] > R[8]:
        return 2
    return 3 if R[4] > R[8] else 4


def R_to_T(R, t):
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0; w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0; w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = math.sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0; w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s
    else:
        s = math.sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0; w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    return np.array([x / n, y / n, z / n, w / n, t[0], t[1], t[2]])


def T_to_Rt(T):
    return quat_to_R(T[:4]).reshape(-1), T[4:]


# ---------------------------------------------------------------- refinement
def _ldlt6_solve(H, lam, b):
    L = np.zeros((6, 6)); d = np.zeros(6); ok = True
    for i in range(6):
        for j in range(i):
            s = H[i, j]
            for k in range(j):
                s -= L[i, k] * d[k] * L[j, k]
            L[i, j] = s / d[j]
        s = H[i, i] + lam
        for k in range(i):
            s -= L[i, k] * L[i, k] * d[k]
        d[i] = s
        if not (s > 0.0 and s < math.inf):
            ok = False
    y = np.zeros(6)
    for i in range(6):
        y[i] = b[i] - L[i, :i] @ y[:i]
    y = y / d
    for i in range(5, -1, -1):
        y[i] = y[i] - L[i + 1:, i] @ y[i + 1:]
    return y, ok


def _residuals(cam, T, xyz, uv):
    R, t = T_to_Rt(T)
    pc = xyz @ R.reshape(3, 3).T + t
    ex = uv[:, 0] - (cam[0] * pc[:, 0] / pc[:, 2] + cam[2]); ey = uv[:, 1] - (cam[1] * pc[:, 1] / pc[:, 2] + cam[3])
    return pc, ex, ey


def jacobian(cam, pc):
    """d(ex, ey) / d(delta) of T <- exp(delta) T at delta = 0 (delta = translation, rotation), per point in the camera frame: J0, J1 [n, 6]"""
    X, Y, Z = pc[:, 0], pc[:, 1], pc[:, 2]
    Zi = 1.0 / Z; Zi2 = Zi * Zi; fx, fy = cam[0], cam[1]; o = np.zeros_like(X)
    J0 = np.stack([-fx * Zi, o, fx * X * Zi2, fx * X * Y * Zi2, -fx - fx * X * X * Zi2, fx * Y * Zi], axis=1)
    J1 = np.stack([o, -fy * Zi, fy * Y * Zi2, fy + fy * Y * Y * Zi2, -fy * X * Y * Zi2, -fy * X * Zi], axis=1)
    return J0, J1


def refine(cam, T, xyz, uv, iters=LM_ITERS, stats=None):
    """g2o's Levenberg-Marquardt (ref_pose_graph.optimize's control flow) on the 6 parameters of T <- exp(d) T.
    stats (a list) receives one (iteration, lambda, cost before, cost of the trial, rho, accepted) per trial"""
    T = np.array(T, np.float64)
    lam = 0.0; nu = 2.0
    for it in range(iters):
        pc, ex, ey = _residuals(cam, T, xyz, uv)
        J0, J1 = jacobian(cam, pc)
        H = J0.T @ J0 + J1.T @ J1
        b = -(J0.T @ ex + J1.T @ ey)
        cur = float(np.sum(ex * ex + ey * ey))
        if it == 0:
            lam = 1e-5 * float(np.max(np.abs(np.diag(H)))); nu = 2.0
        rho = 0.0; qmax = 0; stop = False
        while True:
            x, ok = _ldlt6_solve(H, lam, b)
            Tsv = T
            if ok:
                T = se3_mul(se3_exp(x), T)
                scale = float(np.sum(x * (lam * x + b)))
            _, ex2, ey2 = _residuals(cam, T, xyz, uv)
            temp = float(np.sum(ex2 * ex2 + ey2 * ey2))
            if not ok:
                temp = DBL_MAX
            rho = (cur - temp) / ((scale if ok else 0.0) + 1e-3)
            acc = rho > 0 and math.isfinite(temp)
            if stats is not None:
                stats.append((it, lam, cur, temp, rho, acc))
            if acc:
                alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                lam *= max(alpha, 1.0 / 3.0); nu = 2.0; cur = temp
            else:
                lam *= nu; nu *= 2.0; T = Tsv
                if not math.isfinite(lam):
                    stop = True
            if not stop:
                qmax += 1
            if stop or not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0 or stop:
            break
    return T


# ---------------------------------------------------------------- the job
def _norm6(x):
    return math.sqrt(((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5])


def loop_verify(job, cam, ext_l, detail=None, **params):
    """job: dict(desc_c [nc, 32] u8, desc_q [nq, 32] u8, xyz_c [nc, 3], has_xyz [nc], uv_q [nq, 2] f32, T_cur[7], T_cand[7]).
    returns dict(status, n_matches, n_points, n_inliers, T_corr, T_rel, d, need_correction, matches [n, 4] = candidate row, current
    row, distance, inlier flag).  detail (a dict) receives what the case margins are asserted on: the hypotheses, the winner, the branch
    of R_to_T it took (quat_branch), the LM's trial list (lm) and what the LM ran on (T_start, xyz, uv, inl)."""
    p = dict(DEFAULTS); p.update(params)
    cam = [float(v) for v in cam]; ext_l = np.asarray(ext_l, np.float64)
    desc_c = np.asarray(job["desc_c"], np.uint8).reshape(-1, 32); desc_q = np.asarray(job["desc_q"], np.uint8).reshape(-1, 32)
    nc, nq = len(desc_c), len(desc_q)
    if nc > MAX_DESC or nq > MAX_DESC:
        raise ValueError("more than 1024 descriptors on one side")
    if not 1 <= p["ransac_iters"] <= 1024:
        raise ValueError("ransac_iters outside [1, 1024]")
    out = dict(status=FEW_MATCHES, n_matches=0, n_points=0, n_inliers=0, T_corr=IDENT.copy(), T_rel=IDENT.copy(), d=0.0,
               need_correction=False, matches=np.zeros((0, 4), np.int64))
    if detail is None:
        detail = {}
    if nc == 0 or nq == 0:
        return out
    bj, bd = hamming_match(desc_c, desc_q)
    dmin = int(bd.min()); thr = max(2 * dmin, 30)
    keep = np.nonzero(bd <= thr)[0]
    detail.update(best_j=bj, best_d=bd, d_min=dmin, thr=thr)
    matches = np.stack([keep, bj[keep], bd[keep], np.zeros(len(keep), np.int64)], axis=1).astype(np.int64)
    out["matches"] = matches; out["n_matches"] = len(keep)
    if len(keep) < p["min_matches"]:
        return out
    has = np.asarray(job["has_xyz"]).reshape(-1)[keep] != 0
    pm = np.nonzero(has)[0]                          # point k is match pm[k]
    out["n_points"] = len(pm); out["status"] = FEW_POINTS
    if len(pm) < max(p["min_matches"], 4):
        return out
    xyz = np.asarray(job["xyz_c"], np.float64).reshape(-1, 3)[keep[pm]].astype(np.float32).astype(np.float64)
    uv = np.asarray(job["uv_q"], np.float32).reshape(-1, 2)[bj[keep[pm]]].astype(np.float64)
    thr2 = p["reproj_px"] * p["reproj_px"]
    best = None; bc = -1; bi = -1
    hyps = []
    for i in range(p["ransac_iters"]):
        h = hypothesis(cam, xyz, uv, p["seed"], i)
        if h is None:
            hyps.append(None); continue
        e2, front = reproj2(cam, h[0], h[1], xyz, uv)
        inl = front & (e2 <= thr2)
        hyps.append((e2, front, inl))
        if int(inl.sum()) > bc:
            bc = int(inl.sum()); bi = i; best = (h, inl)
    detail.update(hyps=hyps, thr2=thr2, winner=bi)
    out["status"] = FEW_INLIERS
    if best is None:
        return out
    (R, t), inl = best
    out["n_inliers"] = bc
    matches[pm, 3] = inl
    if bc < p["min_matches"]:
        return out
    lm = []
    T = refine(cam, R_to_T(R, t), xyz[inl], uv[inl], stats=lm)
    detail.update(lm=lm, quat_branch=quat_branch(R), T_start=R_to_T(R, t), xyz=xyz, uv=uv, inl=inl)
    T_corr = se3_mul(se3_inv(ext_l), T)
    T_rel = se3_mul(T_corr, se3_inv(np.asarray(job["T_cand"], np.float64)))
    out["T_corr"] = T_corr; out["T_rel"] = T_rel
    far = _norm6(se3_log(T_rel))
    detail.update(T_pnp=T, far=far)
    if far > p["max_pose_distance"]:
        out["status"] = TOO_FAR
        return out
    d = _norm6(se3_log(se3_mul(np.asarray(job["T_cur"], np.float64), se3_inv(T_corr))))
    out["d"] = d
    if d > p["max_pose_difference"]:
        out["status"] = TOO_DIFFERENT
        return out
    out["status"] = ACCEPTED; out["need_correction"] = bool(d > p["min_pose_difference"])
    return out
