// k_loop_verify.h — geometric verification of a loop candidate (svslam_loop_verify_batch): LoopClosure::KeypointMatchWithLoopCandid
// and LoopClosure::CalculatePose of the reference (src/loopclosure.cpp:286-437, called at :831-862).  The numeric contract is
// tests/ref_loop_verify.py; DESIGN 11 has the declared deviations from OpenCV's solvePnPRansac.
//
// One job = one keyframe pair of one stream = one workgroup of LV_THREADS = 128 threads; thousands of jobs per launch.
//
//   stage       the current keyframe's descriptors (<= 1024 x 32 bytes) go to LDS
//   match       lane per candidate row: its 8 dwords stay in registers, every lane reads the SAME current row at a time (an LDS
//               broadcast, no bank conflict), XOR + popcount, strict "<" keeps the lowest current index on a tie
//   threshold   d_min over the job, thr = max(2 d_min, 30)
//   compact     thread t owns the candidate rows [t CH, (t + 1) CH): it counts what it keeps, every thread adds the counts of the
//               threads before it, the lists come out in ascending candidate row.  Two lists at once: the matches (the output) and
//               the matches with a landmark (the PnP points, staged as 5 floats each in the LDS the descriptors have left)
//   ransac      lane per hypothesis, hypotheses i = tid, tid + 128, ...: 4 indices from a stateless hash, P3P on three, the fourth
//               chooses among the solutions; the same lane then counts the inliers over all points (every lane reads the same point:
//               LDS broadcast again) and keeps its best (count, i).  A count is an integer: no order of summation to fix
//   winner      thread 0 takes the largest count (lowest i on a tie) and forms that hypothesis again — stateless, the same bits —
//               so no hypothesis is ever stored; lane per point then flags the winner's inliers
//   refine      LM over the inliers: 64 lanes accumulate the 28 sums of the normal equations over the points they own, 28 threads
//               add the 64 partial sums in lane order, thread 0 solves the 6x6 system (unpivoted LDL^T) and takes g2o's decision
//   gates       thread 0: T_corr, T_rel, the two norms of Sophus' log
//
// The shape differs from a ballot compaction and a wave-per-hypothesis inlier count on purpose: nothing here crosses lanes
// except through LDS between barriers, so (a) a count or a sum never depends on the wave size or on a DPP order, and (b) the file
// is plain C++ between the HIP qualifiers: compiled for the host with LV_HOST_EMU (tests/cpp/lv_host_emu) a phase becomes a loop
// over the 128 thread numbers and the very same code is checked against the reference on a machine without a device.
// All geometry is f64 without FMA contraction, IEEE division and sqrt; the P3P uses nothing but + - * / sqrt (its quartic is solved
// by bracketing between the roots of its derivatives and bisecting to adjacent doubles), so the hypotheses are the reference's bit
// for bit; sin / cos / atan appear only in exp (LM update) and log (gates).
#pragma once
#if defined(LV_HOST_EMU) && !defined(PG_HOST_EMU)
#define PG_HOST_EMU
#endif
#include "k_pose_graph.h"          // PG_DEV and the SE(3) functions (pg_mul, pg_inv, pg_log, pg_exp, pg_quat_to_R)
#pragma clang fp contract(off)

#define LV_THREADS 128
#define LV_MAX_DESC 1024           // rows per side: ORB is created with 400 features, num_features is 150
#define LV_MAX_ITERS 1024
#define LV_LM_LANES 64
#define LV_LM_ITERS 10
#define LV_MAX_DRAWS 64            // draws of one hypothesis before it is given up (4 distinct indices out of >= 4)
#define LV_BISECT 128

enum { LV_ACCEPTED = 0, LV_FEW_MATCHES = 1, LV_FEW_POINTS = 2, LV_FEW_INLIERS = 3, LV_TOO_FAR = 4, LV_TOO_DIFFERENT = 5 };

#ifdef PG_HOST_EMU
#define LV_PAR for (int tid = 0; tid < LV_THREADS; ++tid)
#define LV_SYNC
#else
#define LV_PAR for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define LV_SYNC __syncthreads();
#endif

struct LvJob {
    int c_ofs, nc, q_ofs, nq;
    double T_cur[7], T_cand[7];
    int status, n_matches, n_points, n_inliers, need_correction, pad;     // out
    double T_corr[7], T_rel[7], d;                                        // out
};

struct LvParams {
    double cam[4], ext_l[7];
    double reproj2, max_pose_distance, min_pose_difference, max_pose_difference;
    int min_matches, ransac_iters;
    uint32_t seed; int pad;
};

struct LvBuf {
    LvJob *jobs;
    int *m_c, *m_q, *m_d;              // [total_c]: a job's match list starts at its c_ofs
    uint8_t *m_inl;                    // [total_c]
    const uint32_t *desc_c, *desc_q;   // 8 dwords a row
    const float *xyz_c;                // [total_c][3], rounded to float like the reference's cv::Point3f
    const float *uv_q;                 // [total_q][2]
    const uint8_t *has_xyz;            // [total_c]
};

struct LvIn { int c_ofs, nc, q_ofs, nq; const double *T_cur, *T_cand; };

struct LvSizes { size_t result_bytes = 0, bytes = 0; };

static inline bool lv_unit(const double *q) { return fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 2e-6; }

// returns nullptr or the reason the call is refused (nothing has been written then)
static inline const char *lv_check(int njobs, const LvIn *in, int total_c, int total_q, const double *ext_l, int ransac_iters, int min_matches,
                                   double reproj_px)
{
    if (ransac_iters < 1 || ransac_iters > LV_MAX_ITERS) return "ransac_iters is outside [1, 1024]";
    if (min_matches < 0) return "min_matches is negative";
    if (!(reproj_px >= 0.0)) return "reproj_px is negative or not a number";
    if (!lv_unit(ext_l)) return "the quaternion of ext_l is not of unit length (1e-6)";
    for (int j = 0; j < njobs; ++j) {
        const LvIn &I = in[j];
        if (I.nc < 0 || I.nq < 0 || I.c_ofs < 0 || I.q_ofs < 0 || (long long)I.c_ofs + I.nc > total_c || (long long)I.q_ofs + I.nq > total_q)
            return "a job's ranges leave the arrays";
        if (I.nc > LV_MAX_DESC || I.nq > LV_MAX_DESC) return "a job has more than 1024 descriptors on one side";
        if (j > 0 && (I.c_ofs < in[j - 1].c_ofs + in[j - 1].nc || I.q_ofs < in[j - 1].q_ofs + in[j - 1].nq))
            return "the jobs' ranges must ascend and not overlap";
        if (!lv_unit(I.T_cur) || !lv_unit(I.T_cand)) return "a pose's quaternion is not of unit length (1e-6)";
    }
    return nullptr;
}

// one buffer: [jobs | match lists] (uploaded zeroed, read back) [descriptors, landmarks, pixels] (uploaded)
static inline LvBuf lv_layout(LvSizes &Z, int njobs, int total_c, int total_q, unsigned char *base)
{
    LvBuf B;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *p = base + o; o += (bytes + 15) & ~(size_t)15; return p; };
    B.jobs = (LvJob *)take(sizeof(LvJob) * (size_t)njobs);
    B.m_c = (int *)take(4 * (size_t)total_c); B.m_q = (int *)take(4 * (size_t)total_c); B.m_d = (int *)take(4 * (size_t)total_c);
    B.m_inl = (uint8_t *)take((size_t)total_c);
    Z.result_bytes = o;
    B.desc_c = (const uint32_t *)take(32 * (size_t)total_c); B.desc_q = (const uint32_t *)take(32 * (size_t)total_q);
    B.xyz_c = (const float *)take(12 * (size_t)total_c); B.uv_q = (const float *)take(8 * (size_t)total_q);
    B.has_xyz = (const uint8_t *)take((size_t)total_c);
    Z.bytes = o;
    return B;
}

// the buffer's content before the launch, written through a host view of the same layout
static inline void lv_fill(const LvSizes &Z, const LvBuf &Hb, int njobs, const LvIn *in, int total_c, const uint8_t *desc_c, const double *xyz_c,
                           const uint8_t *has_xyz, int total_q, const uint8_t *desc_q, const float *uv_q)
{
    memset((void *)Hb.jobs, 0, Z.result_bytes);
    for (int j = 0; j < njobs; ++j) {
        LvJob &J = Hb.jobs[j];
        J.c_ofs = in[j].c_ofs; J.nc = in[j].nc; J.q_ofs = in[j].q_ofs; J.nq = in[j].nq;
        memcpy(J.T_cur, in[j].T_cur, 56); memcpy(J.T_cand, in[j].T_cand, 56);
    }
    if (total_c) {
        memcpy((void *)Hb.desc_c, desc_c, 32 * (size_t)total_c); memcpy((void *)Hb.has_xyz, has_xyz, (size_t)total_c);
        float *x = (float *)Hb.xyz_c;
        for (size_t i = 0; i < 3 * (size_t)total_c; ++i) x[i] = (float)xyz_c[i];
    }
    if (total_q) { memcpy((void *)Hb.desc_q, desc_q, 32 * (size_t)total_q); memcpy((void *)Hb.uv_q, uv_q, 8 * (size_t)total_q); }
}

// ---- the pieces of a hypothesis ---------------------------------------------------------------------------------------------------
PG_DEV uint32_t lv_hash(uint32_t seed, uint32_t i, uint32_t draw)
{
    uint32_t h = seed ^ (i * 0x9E3779B1u) ^ (draw * 0x85EBCA77u);
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}

// 4 distinct indices below np (np >= 4); false: LV_MAX_DRAWS draws did not give them
PG_DEV bool lv_draw4(uint32_t seed, int i, int np, int *idx)
{
    uint32_t draw = 0;
    for (int k = 0; k < 4; ++k) {
        for (;;) {
            if (draw >= LV_MAX_DRAWS) return false;
            const int v = (int)(((uint64_t)lv_hash(seed, (uint32_t)i, draw++) * (uint64_t)np) >> 32);
            bool rep = false;
            for (int m = 0; m < k; ++m) rep = rep || idx[m] == v;
            if (!rep) { idx[k] = v; break; }
        }
    }
    return true;
}

// Rt = rotation (row major) and translation of world -> left camera; squared pixel error of a point, false behind the camera
PG_DEV bool lv_reproj2(const double *cam, const double *Rt, const float *p, double *e2)
{
    const double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    const double pc0 = ((Rt[0] * X + Rt[1] * Y) + Rt[2] * Z) + Rt[9];
    const double pc1 = ((Rt[3] * X + Rt[4] * Y) + Rt[5] * Z) + Rt[10];
    const double pc2 = ((Rt[6] * X + Rt[7] * Y) + Rt[8] * Z) + Rt[11];
    if (!(pc2 > 0.0)) return false;
    const double ex = (double)p[3] - (cam[0] * pc0 / pc2 + cam[2]);
    const double ey = (double)p[4] - (cam[1] * pc1 / pc2 + cam[3]);
    *e2 = ex * ex + ey * ey;
    return true;
}

PG_DEV double lv_horner(const double *c, int deg, double v)
{
    double s = c[deg];
    for (int k = deg - 1; k >= 0; --k) s = s * v + c[k];
    return s;
}

// the roots of a polynomial (ascending coefficients) inside (0, B), given the roots of its derivative inside (0, B) in ascending
// order: between two neighbours of 0, crit..., B the polynomial is monotonic, a strict change of sign is bisected to adjacent doubles
PG_DEV int lv_bracket_roots(const double *c, int deg, const double *crit, int ncrit, double B, double *roots)
{
    int n = 0;
    double lo = 0.0, flo = lv_horner(c, deg, 0.0);
    for (int k = 0; k <= ncrit; ++k) {
        const double hi = k < ncrit ? crit[k] : B, fhi = lv_horner(c, deg, hi);
        if ((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0)) {
            double a = lo, b = hi;
            for (int it = 0; it < LV_BISECT; ++it) {
                const double mid = 0.5 * (a + b);
                if (!(mid > a && mid < b)) break;
                const double fm = lv_horner(c, deg, mid);
                if (fm == 0.0) { a = mid; b = mid; break; }
                if ((fm < 0.0) == (flo < 0.0)) a = mid; else b = mid;
            }
            roots[n++] = 0.5 * (a + b);
        }
        lo = hi; flo = fhi;
    }
    return n;
}

PG_DEV double lv_dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PG_DEV void lv_cross(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// orthonormal frame of a triangle: e1 along p2 - p1, e3 along its normal; false when it has none
PG_DEV bool lv_frame(const double *p1, const double *p2, const double *p3, double *E)
{
    const double d1[3] = { p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2] }, d2[3] = { p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2] };
    double n[3];
    lv_cross(d1, d2, n);
    const double l1 = lv_dot3(d1, d1), l2 = lv_dot3(d2, d2), ln = lv_dot3(n, n);
    if (!(ln > 1e-12 * (l1 * l2)) || !(ln < INFINITY)) return false;          // collinear (sin^2 of the angle <= 1e-12), coincident
    const double s1 = sqrt(l1), sn = sqrt(ln);
    for (int k = 0; k < 3; ++k) { E[k] = d1[k] / s1; E[6 + k] = n[k] / sn; }
    lv_cross(E + 6, E, E + 3);
    return true;
}

// P3P: world points X (3 x 3), unit bearings f (3 x 3) -> up to 4 poses (Rt, 12 doubles each) in ascending order of the root.
// Distances s_i along the bearings with s_2 = u s_1, s_3 = v s_1; the law of cosines on the three sides gives
// u = N(v) / D(v) and the quartic b N^2 - 2 b c23 v N D + (b v^2 - a A) D^2 = 0, A = 1 + v^2 - 2 c13 v.
PG_DEV int lv_p3p(const double *X, const double *f, double *out)
{
    double Ex[9];
    if (!lv_frame(X, X + 3, X + 6, Ex)) return 0;
    const double c12 = lv_dot3(f, f + 3), c13 = lv_dot3(f, f + 6), c23 = lv_dot3(f + 3, f + 6);
    double t[3];
    for (int k = 0; k < 3; ++k) t[k] = X[3 + k] - X[6 + k];
    const double a = lv_dot3(t, t);
    for (int k = 0; k < 3; ++k) t[k] = X[k] - X[6 + k];
    const double b = lv_dot3(t, t);
    for (int k = 0; k < 3; ++k) t[k] = X[k] - X[3 + k];
    const double c = lv_dot3(t, t);
    const double ca = c - a;
    const double n0 = ca - b, n1 = -2.0 * ca * c13, n2 = ca + b;
    const double d0 = -2.0 * b * c12, d1 = 2.0 * b * c23;
    const double e0 = -a, e1 = 2.0 * a * c13, e2 = b - a;
    const double nn[5] = { n0 * n0, 2.0 * n0 * n1, 2.0 * n0 * n2 + n1 * n1, 2.0 * n1 * n2, n2 * n2 };
    const double nd[5] = { 0.0, n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1 };            // v N D
    const double dd[3] = { d0 * d0, 2.0 * d0 * d1, d1 * d1 };
    const double ed[5] = { e0 * dd[0], e0 * dd[1] + e1 * dd[0], (e0 * dd[2] + e1 * dd[1]) + e2 * dd[0], e1 * dd[2] + e2 * dd[1], e2 * dd[2] };
    const double g = 2.0 * b * c23;
    double q[5], mx = 0.0;
    for (int k = 0; k < 5; ++k) { q[k] = (b * nn[k] - g * nd[k]) + ed[k]; if (fabs(q[k]) > mx) mx = fabs(q[k]); }
    if (!(fabs(q[4]) > 1e-12 * mx) || !(mx < INFINITY)) return 0;             // no quartic (a root at infinity), or not finite
    double m[5], B = 0.0;
    for (int k = 0; k < 4; ++k) { m[k] = q[k] / q[4]; if (fabs(m[k]) > B) B = fabs(m[k]); }
    m[4] = 1.0; B += 1.0;                                                      // Cauchy's bound of the roots
    const double p1[4] = { m[1], 2.0 * m[2], 3.0 * m[3], 4.0 };
    const double p2[3] = { 2.0 * m[2], 6.0 * m[3], 12.0 };
    double r2[2], r3[3], r4[4];
    int k2 = 0;
    const double disc = p2[1] * p2[1] - 4.0 * p2[2] * p2[0];
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        const double ra = (-p2[1] - sq) / (2.0 * p2[2]), rb = (-p2[1] + sq) / (2.0 * p2[2]);
        if (ra > 0.0 && ra < B) r2[k2++] = ra;
        if (rb > 0.0 && rb < B && rb > ra) r2[k2++] = rb;
    }
    const int k3 = lv_bracket_roots(p1, 3, r2, k2, B, r3);
    const int k4 = lv_bracket_roots(m, 4, r3, k3, B, r4);
    int ns = 0;
    for (int r = 0; r < k4; ++r) {
        const double v = r4[r];
        const double Dv = d1 * v + d0;
        if (Dv == 0.0) continue;
        const double u = ((n2 * v + n1) * v + n0) / Dv;
        const double Av = (1.0 + v * v) - 2.0 * c13 * v;
        if (!(u > 0.0) || !(v > 0.0) || !(Av > 0.0)) continue;
        const double s1 = sqrt(b / Av), s2 = u * s1, s3 = v * s1;
        double Y[9], Ey[9];
        for (int k = 0; k < 3; ++k) { Y[k] = s1 * f[k]; Y[3 + k] = s2 * f[3 + k]; Y[6 + k] = s3 * f[6 + k]; }
        if (!lv_frame(Y, Y + 3, Y + 6, Ey)) continue;
        double *Rt = out + 12 * ns;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = (Ey[i] * Ex[j] + Ey[3 + i] * Ex[3 + j]) + Ey[6 + i] * Ex[6 + j];
        for (int i = 0; i < 3; ++i) Rt[9 + i] = Y[i] - (((Rt[3 * i] * X[0] + Rt[3 * i + 1] * X[1]) + Rt[3 * i + 2] * X[2]));
        bool fin = true;
        for (int i = 0; i < 12; ++i) fin = fin && fabs(Rt[i]) < INFINITY;
        if (fin) ++ns;
    }
    return ns;
}

// hypothesis i over the np staged points (5 floats each: landmark, pixel); false: no hypothesis
PG_DEV bool lv_hypothesis(const LvParams &P, const float *pt, int np, int i, double *Rt)
{
    int idx[4];
    if (!lv_draw4(P.seed, i, np, idx)) return false;
    double X[9], f[9], sol[48];
    for (int k = 0; k < 3; ++k) {
        const float *p = pt + 5 * idx[k];
        X[3 * k] = (double)p[0]; X[3 * k + 1] = (double)p[1]; X[3 * k + 2] = (double)p[2];
        const double x = ((double)p[3] - P.cam[2]) / P.cam[0], y = ((double)p[4] - P.cam[3]) / P.cam[1];
        const double n = sqrt((x * x + y * y) + 1.0);
        f[3 * k] = x / n; f[3 * k + 1] = y / n; f[3 * k + 2] = 1.0 / n;
    }
    const int ns = lv_p3p(X, f, sol);
    int best = -1; double be = 0.0;
    for (int s = 0; s < ns; ++s) {
        double e2;
        if (!lv_reproj2(P.cam, sol + 12 * s, pt + 5 * idx[3], &e2)) continue;
        if (!(e2 < INFINITY)) continue;
        if (best < 0 || e2 < be) { best = s; be = e2; }
    }
    if (best < 0) return false;
    for (int k = 0; k < 12; ++k) Rt[k] = sol[12 * best + k];
    return true;
}

PG_DEV void lv_R_to_T(const double *Rt, double *T)
{
    const double *R = Rt;
    double x, y, z, w;
    const double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) { const double s = sqrt(tr + 1.0) * 2.0; w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s; }
    else if (R[0] > R[4] && R[0] > R[8]) { const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0; w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
    else if (R[4] > R[8]) { const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0; w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
    else { const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0; w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    T[0] = x / n; T[1] = y / n; T[2] = z / n; T[3] = w / n; T[4] = Rt[9]; T[5] = Rt[10]; T[6] = Rt[11];
}
PG_DEV void lv_T_to_Rt(const double *T, double *Rt)
{
    pg_quat_to_R(T, Rt);
    Rt[9] = T[4]; Rt[10] = T[5]; Rt[11] = T[6];
}

// (H + lambda I) x = b by an unpivoted LDL^T, IEEE divisions; false: a pivot is not positive
PG_DEV bool lv_ldlt6_solve(const double *H, double lambda, const double *b, double *x)
{
    double L[36], d[6], y[6];
    bool ok = true;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < i; ++j) {
            double s = H[i * 6 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * d[k] * L[j * 6 + k];
            L[i * 6 + j] = s / d[j];
        }
        double s = H[i * 6 + i] + lambda;
        for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * L[i * 6 + k] * d[k];
        d[i] = s;
        if (!(s > 0.0 && s < INFINITY)) ok = false;
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
        y[i] = s;
    }
    for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * y[k];
        y[i] = s;
    }
    for (int i = 0; i < 6; ++i) x[i] = y[i];
    return ok;
}

PG_DEV double lv_norm6(const double *x)
{
    return sqrt(((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5]);
}

// ---- one job ---------------------------------------------------------------------------------------------------------------------
struct LvShared {
    union { uint32_t desc[LV_MAX_DESC * 8]; float pt[LV_MAX_DESC * 5]; } u;       // 32 KB: the current descriptors, then the PnP points
    unsigned short best_j[LV_MAX_DESC], best_d[LV_MAX_DESC], pt_match[LV_MAX_DESC];
    unsigned char inl[LV_MAX_DESC];
    double part[LV_LM_LANES * 28];
    int cnt_m[LV_THREADS], cnt_p[LV_THREADS], hb_cnt[LV_THREADS], hb_i[LV_THREADS];
    double H[36], b[6], x[6], T[7], Tsv[7], Rt[12];
    double cur, temp, lambda, nu, rho, scale;
    int ok, accepted, stop, qmax;
    int thr, n_matches, n_points, n_inl, win;
};

PG_DEV void lv_run(const LvBuf &B, const LvParams &P, LvJob &J, LvShared &S)
{
    const int nc = J.nc, nq = J.nq;
    const uint32_t *dc = B.desc_c + 8 * (size_t)J.c_ofs, *dq = B.desc_q + 8 * (size_t)J.q_ofs;
    const float *xyz = B.xyz_c + 3 * (size_t)J.c_ofs, *uv = B.uv_q + 2 * (size_t)J.q_ofs;
    const uint8_t *has = B.has_xyz + J.c_ofs;
    int *m_c = B.m_c + J.c_ofs, *m_q = B.m_q + J.c_ofs, *m_d = B.m_d + J.c_ofs;
    uint8_t *m_inl = B.m_inl + J.c_ofs;
    int status = LV_FEW_MATCHES, n_matches = 0, n_points = 0, n_inl = 0, need = 0;
    double T_corr[7] = { 0, 0, 0, 1, 0, 0, 0 }, T_rel[7] = { 0, 0, 0, 1, 0, 0, 0 }, dist = 0.0;

    if (nc > 0 && nq > 0) {
        // stage, match
        LV_PAR { for (int i = tid; i < nq * 8; i += LV_THREADS) S.u.desc[i] = dq[i]; } LV_SYNC
        LV_PAR {
            int dmin = 257;
            for (int c = tid; c < nc; c += LV_THREADS) {
                uint32_t a[8];
                for (int k = 0; k < 8; ++k) a[k] = dc[8 * (size_t)c + k];
                int best = 257, bj = 0;
                for (int j = 0; j < nq; ++j) {
                    const uint32_t *r = S.u.desc + 8 * j;
                    int d = 0;
                    for (int k = 0; k < 8; ++k) d += __builtin_popcount(a[k] ^ r[k]);
                    if (d < best) { best = d; bj = j; }
                }
                S.best_d[c] = (unsigned short)best; S.best_j[c] = (unsigned short)bj;
                if (best < dmin) dmin = best;
            }
            S.cnt_m[tid] = dmin;
        } LV_SYNC
        LV_PAR {
            if (tid == 0) {
                int dmin = 257;
                for (int t = 0; t < LV_THREADS; ++t) if (S.cnt_m[t] < dmin) dmin = S.cnt_m[t];
                S.thr = 2 * dmin > 30 ? 2 * dmin : 30;
            }
        } LV_SYNC
        // compact: the matches, and those of them that have a landmark
        const int CH = (nc + LV_THREADS - 1) / LV_THREADS, thr = S.thr;
        LV_PAR {
            int km = 0, kp = 0;
            for (int c = tid * CH; c < (tid + 1) * CH && c < nc; ++c)
                if ((int)S.best_d[c] <= thr) { ++km; if (has[c]) ++kp; }
            S.cnt_m[tid] = km; S.cnt_p[tid] = kp;
        } LV_SYNC
        LV_PAR {
            int om = 0, op = 0;
            for (int t = 0; t < tid; ++t) { om += S.cnt_m[t]; op += S.cnt_p[t]; }
            for (int c = tid * CH; c < (tid + 1) * CH && c < nc; ++c)
                if ((int)S.best_d[c] <= thr) {
                    const int j = S.best_j[c];
                    m_c[om] = c; m_q[om] = j; m_d[om] = S.best_d[c]; m_inl[om] = 0;
                    if (has[c]) {
                        float *p = S.u.pt + 5 * op;
                        p[0] = xyz[3 * c]; p[1] = xyz[3 * c + 1]; p[2] = xyz[3 * c + 2]; p[3] = uv[2 * j]; p[4] = uv[2 * j + 1];
                        S.pt_match[op] = (unsigned short)om;
                        ++op;
                    }
                    ++om;
                }
            if (tid == LV_THREADS - 1) { S.n_matches = om; S.n_points = op; }
        } LV_SYNC
        n_matches = S.n_matches;
        if (n_matches >= P.min_matches) {
            n_points = S.n_points;
            const int np = n_points;
            status = LV_FEW_POINTS;
            if (np >= (P.min_matches > 4 ? P.min_matches : 4)) {
                // RANSAC: a lane's hypotheses in ascending i, so its first best is its lowest
                LV_PAR {
                    int bc = -1, bi = -1;
                    for (int i = tid; i < P.ransac_iters; i += LV_THREADS) {
                        double Rt[12];
                        if (!lv_hypothesis(P, S.u.pt, np, i, Rt)) continue;
                        int cnt = 0;
                        for (int k = 0; k < np; ++k) {
                            double e2;
                            if (lv_reproj2(P.cam, Rt, S.u.pt + 5 * k, &e2) && e2 <= P.reproj2) ++cnt;
                        }
                        if (cnt > bc) { bc = cnt; bi = i; }
                    }
                    S.hb_cnt[tid] = bc; S.hb_i[tid] = bi;
                } LV_SYNC
                LV_PAR {
                    if (tid == 0) {
                        int bc = -1, bi = -1;
                        for (int t = 0; t < LV_THREADS; ++t)
                            if (S.hb_i[t] >= 0 && (S.hb_cnt[t] > bc || (S.hb_cnt[t] == bc && S.hb_i[t] < bi))) { bc = S.hb_cnt[t]; bi = S.hb_i[t]; }
                        S.win = bi; S.n_inl = bi >= 0 ? bc : 0;
                        if (bi >= 0) { lv_hypothesis(P, S.u.pt, np, bi, S.Rt); lv_R_to_T(S.Rt, S.T); }
                    }
                } LV_SYNC
                status = LV_FEW_INLIERS;
                if (S.win >= 0) {
                    LV_PAR {
                        for (int k = tid; k < np; k += LV_THREADS) {
                            double e2;
                            const unsigned char in = (lv_reproj2(P.cam, S.Rt, S.u.pt + 5 * k, &e2) && e2 <= P.reproj2) ? 1 : 0;
                            S.inl[k] = in; m_inl[S.pt_match[k]] = in;
                        }
                    } LV_SYNC
                    n_inl = S.n_inl;
                }
                if (S.win >= 0 && n_inl >= P.min_matches) {
                    // refinement: LM on exp(d) T over the winner's inliers, g2o's control
                    LV_PAR { if (tid == 0) { S.lambda = 0.0; S.nu = 2.0; S.cur = 0.0; S.rho = 0.0; S.qmax = 0; S.stop = 0; } } LV_SYNC
                    for (int it = 0; it < LV_LM_ITERS; ++it) {
                        LV_PAR {
                            if (tid < LV_LM_LANES) {
                                double acc[28], Rt[12];
                                for (int i = 0; i < 28; ++i) acc[i] = 0.0;
                                lv_T_to_Rt(S.T, Rt);
                                for (int k = tid; k < np; k += LV_LM_LANES) {
                                    if (!S.inl[k]) continue;
                                    const float *p = S.u.pt + 5 * k;
                                    const double Xw = (double)p[0], Yw = (double)p[1], Zw = (double)p[2];
                                    const double X = ((Rt[0] * Xw + Rt[1] * Yw) + Rt[2] * Zw) + Rt[9];
                                    const double Y = ((Rt[3] * Xw + Rt[4] * Yw) + Rt[5] * Zw) + Rt[10];
                                    const double Z = ((Rt[6] * Xw + Rt[7] * Yw) + Rt[8] * Zw) + Rt[11];
                                    const double fx = P.cam[0], fy = P.cam[1];
                                    const double ex = (double)p[3] - (fx * X / Z + P.cam[2]), ey = (double)p[4] - (fy * Y / Z + P.cam[3]);
                                    const double Zi = 1.0 / Z, Zi2 = Zi * Zi;
                                    const double J0[6] = { -fx * Zi, 0.0, fx * X * Zi2, fx * X * Y * Zi2, -fx - fx * X * X * Zi2, fx * Y * Zi };
                                    const double J1[6] = { 0.0, -fy * Zi, fy * Y * Zi2, fy + fy * Y * Y * Zi2, -fy * X * Y * Zi2, -fy * X * Zi };
                                    int m = 0;
                                    for (int a = 0; a < 6; ++a) {
                                        for (int c = a; c < 6; ++c) acc[m++] += J0[a] * J0[c] + J1[a] * J1[c];
                                        acc[21 + a] -= J0[a] * ex + J1[a] * ey;
                                    }
                                    acc[27] += ex * ex + ey * ey;
                                }
                                for (int i = 0; i < 28; ++i) S.part[28 * tid + i] = acc[i];
                            }
                        } LV_SYNC
                        LV_PAR {
                            if (tid < 28) {
                                double s = 0.0;
                                for (int t = 0; t < LV_LM_LANES; ++t) s += S.part[28 * t + tid];
                                if (tid < 21) {
                                    int a = 0, m = tid;
                                    while (m >= 6 - a) { m -= 6 - a; ++a; }
                                    S.H[a * 6 + a + m] = s; S.H[(a + m) * 6 + a] = s;
                                } else if (tid < 27) S.b[tid - 21] = s;
                                else S.cur = s;
                            }
                        } LV_SYNC
                        LV_PAR {
                            if (tid == 0) {
                                if (it == 0) {
                                    double md = 0.0;
                                    for (int a = 0; a < 6; ++a) if (fabs(S.H[a * 7]) > md) md = fabs(S.H[a * 7]);
                                    S.lambda = 1e-5 * md; S.nu = 2.0;
                                }
                                S.rho = 0.0; S.qmax = 0;
                            }
                        } LV_SYNC
                        int qmax = 0; double rho = 0.0; bool stop = false;
                        do {
                            LV_PAR {
                                if (tid == 0) {
                                    for (int i = 0; i < 7; ++i) S.Tsv[i] = S.T[i];
                                    S.ok = lv_ldlt6_solve(S.H, S.lambda, S.b, S.x) ? 1 : 0;
                                    if (S.ok) {
                                        double dT[7], Tn[7], s = 0.0;
                                        pg_exp(S.x, dT); pg_mul(dT, S.T, Tn);
                                        for (int i = 0; i < 7; ++i) S.T[i] = Tn[i];
                                        for (int a = 0; a < 6; ++a) s += S.x[a] * (S.lambda * S.x[a] + S.b[a]);
                                        S.scale = s;
                                    }
                                }
                            } LV_SYNC
                            LV_PAR {
                                if (tid < LV_LM_LANES) {
                                    double Rt[12], s = 0.0;
                                    lv_T_to_Rt(S.T, Rt);
                                    for (int k = tid; k < np; k += LV_LM_LANES) {
                                        if (!S.inl[k]) continue;
                                        const float *p = S.u.pt + 5 * k;
                                        const double Xw = (double)p[0], Yw = (double)p[1], Zw = (double)p[2];
                                        const double X = ((Rt[0] * Xw + Rt[1] * Yw) + Rt[2] * Zw) + Rt[9];
                                        const double Y = ((Rt[3] * Xw + Rt[4] * Yw) + Rt[5] * Zw) + Rt[10];
                                        const double Z = ((Rt[6] * Xw + Rt[7] * Yw) + Rt[8] * Zw) + Rt[11];
                                        const double ex = (double)p[3] - (P.cam[0] * X / Z + P.cam[2]), ey = (double)p[4] - (P.cam[1] * Y / Z + P.cam[3]);
                                        s += ex * ex + ey * ey;
                                    }
                                    S.part[tid] = s;
                                }
                            } LV_SYNC
                            LV_PAR {
                                if (tid == 0) {
                                    double temp = 0.0;
                                    for (int t = 0; t < LV_LM_LANES; ++t) temp += S.part[t];
                                    const bool ok = S.ok != 0;
                                    if (!ok) temp = 1.7976931348623157e308;
                                    double r = S.cur - temp;
                                    const double scale = (ok ? S.scale : 0.0) + 1e-3;
                                    r /= scale;
                                    const bool acc = r > 0 && temp < INFINITY && temp == temp;
                                    S.stop = 0;
                                    if (acc) {
                                        double alpha = 1.0 - (2.0 * r - 1.0) * (2.0 * r - 1.0) * (2.0 * r - 1.0);
                                        if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                                        S.lambda *= alpha < 1.0 / 3.0 ? 1.0 / 3.0 : alpha; S.nu = 2.0; S.cur = temp;
                                    } else {
                                        S.lambda *= S.nu; S.nu *= 2.0;
                                        for (int i = 0; i < 7; ++i) S.T[i] = S.Tsv[i];
                                        if (!(fabs(S.lambda) < INFINITY)) S.stop = 1;
                                    }
                                    S.accepted = acc ? 1 : 0; S.rho = r;
                                    if (!S.stop) S.qmax++;
                                }
                            } LV_SYNC
                            rho = S.rho; qmax = S.qmax; stop = S.stop != 0;
                        } while (!stop && rho < 0 && qmax < 10);
                        if (qmax == 10 || rho == 0 || stop) break;
                    }
                    // gates (src/loopclosure.cpp:400-436); every thread takes them on the same values, thread 0 writes
                    double Ei[7], Ci[7], Tci[7], A[7], xi[6];
                    pg_inv(P.ext_l, Ei); pg_mul(Ei, S.T, T_corr);
                    pg_inv(J.T_cand, Ci); pg_mul(T_corr, Ci, T_rel);
                    pg_log(T_rel, xi);
                    if (lv_norm6(xi) > P.max_pose_distance) status = LV_TOO_FAR;
                    else {
                        pg_inv(T_corr, Tci); pg_mul(J.T_cur, Tci, A);
                        pg_log(A, xi);
                        dist = lv_norm6(xi);
                        if (dist > P.max_pose_difference) status = LV_TOO_DIFFERENT;
                        else { status = LV_ACCEPTED; need = dist > P.min_pose_difference ? 1 : 0; }
                    }
                }
            }
        }
    }
    LV_PAR {
        if (tid == 0) {
            J.status = status; J.n_matches = n_matches; J.n_points = n_points; J.n_inliers = n_inl; J.need_correction = need;
            for (int i = 0; i < 7; ++i) { J.T_corr[i] = T_corr[i]; J.T_rel[i] = T_rel[i]; }
            J.d = dist;
        }
    } LV_SYNC
}

#ifndef PG_HOST_EMU
__global__ void __launch_bounds__(LV_THREADS) k_loop_verify(LvBuf B, LvParams P)
{
    __shared__ LvShared S;
    lv_run(B, P, B.jobs[blockIdx.x], S);
}
#endif
