// k_pose_graph.h — global pose-graph optimisation (svslam_pose_graph_batch): LoopClosure::PoseGraphOptimization of the reference
// (src/loopclosure.cpp:641-799) with VertexPose / EdgePoseGraph (g2o_types.h:25-65, 231-267) under g2o's Levenberg-Marquardt.
//
// One job = one pose graph = one workgroup of ONE wave (PG_THREADS = 64): a 1000-keyframe graph is a chain of dependent 6x6 block
// operations, which more waves would only wait on, and a batch of thousands of graphs fills the device with a wave each.  The
// phases of an LM trial are loops over edges / vertices / block entries strided by the 64 lanes, separated by workgroup
// barriers; the control flow reads its scalars from LDS, where lane 0 leaves them.
//
//   linearise   lane per edge: e = log(M^-1 T_a T_b^-1), J_a = Jr^-1(e) Ad((T_a T_b^-1)^-1), J_b = -Jr^-1(e) in closed form
//               (g2o differentiates this edge numerically: a declared deviation)
//   assemble    lane per entry of a block row: the row's edges in ascending edge order (no atomics: an entry has one owner)
//   factorise   block-skyline LDL^T in place, rows in order: H is block tridiagonal plus one block per loop edge, and under the
//               natural order the fill stays inside each row's envelope [first neighbour, i].  36 lanes own the 36 entries of the
//               block being formed and share its block dot products; lane 0 inverts the 6x6 pivot block (scalar LDL^T).
//               Unpivoted, like the library's other solves (Eigen's dense Cholesky in the reference: declared deviation).
//   sweeps      forward: a row's blocks dealt over PG_FWD_GROUPS groups of 6 lanes, partial sums added in group order;
//               backward: column-oriented, a lane per (row above, component)
//   update      T <- exp(d) T per free vertex; trial chi2; lane 0 takes g2o's decision (exactly orc_geom.c / k_ba.h)
// Sums over edges (chi2, the rho denominator) are 64 strided partial sums added in lane order by lane 0: fixed order, no
// floating-point atomics, nothing depends on the other jobs of the call.
//
// The file is self-contained plain C++ between the HIP qualifiers (no DPP, no fast reciprocals, no FMA contraction): compiled for
// the host with PG_HOST_EMU (tests/cpp/pg_host_emu) a "phase" becomes a loop over the 64 lane numbers, so the solver's logic is
// checked against tests/ref_pose_graph.py on a machine without a device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#define PG_THREADS 64
#define PG_FWD_GROUPS 10
#ifndef LM_TRACE_REC
#define LM_TRACE_REC 6
#define LM_TRACE_CAP 408
#define LM_TRACE_STRIDE (8 + LM_TRACE_REC * LM_TRACE_CAP)
#endif

#ifdef PG_HOST_EMU
#define PG_DEV static inline
#define PG_PAR for (int tid = 0; tid < PG_THREADS; ++tid)
#define PG_SYNC
#else
#define PG_DEV __device__ __forceinline__
#define PG_PAR for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define PG_SYNC __syncthreads();
#endif

struct PgJob {
    int nkf, nedge, npt, nfree;
    int kf_ofs, edge_ofs, pt_ofs, free_ofs;
    int inc_ofs, maxspan, trace_slot, iters;
    long long env_ofs, nblocks, y_ofs;          // in 6x6 blocks
    int iters_done, n_trials;                   // out
    double chi2_before, chi2_after;             // out
};

struct PgBuf {
    PgJob *jobs;
    double *poses, *meas, *pts;                                   // uploaded; poses / pts are also the result
    int *ea, *eb, *fidx, *free_v, *first, *rowptr, *inc_start, *inc_edge, *anchor;
    double *poses0, *poses_sv, *J, *chi_e, *b, *z, *x, *Dinv, *H, *L, *Y;     // device only
};

// ---- the plan: validation, free indices, envelope, incidence lists (host) -------------------------------------------------------
struct PgPlan {
    std::vector<PgJob> jobs;
    std::vector<int> fidx, free_v, first, rowptr, inc_start, inc_edge;
    long long total_free = 0, total_blocks = 0, total_y = 0;
    size_t front_bytes = 0, result_bytes = 0, bytes = 0;
};

struct PgIn { int kf_ofs, nkf, edge_ofs, nedge, pt_ofs, npt; };

// returns nullptr or the reason the call is refused (nothing has been written then)
static inline const char *pg_plan(int njobs, const PgIn *in, int total_kf, const double *poses, const uint8_t *fixed, int total_edges,
                                  const int *ea, const int *eb, int total_pts, const int *anchor, int iters, int trace_jobs, PgPlan &P)
{
    P.jobs.assign((size_t)njobs, PgJob());
    P.fidx.assign((size_t)total_kf, -1);
    P.inc_start.assign((size_t)total_kf + (size_t)njobs, 0);
    P.inc_edge.assign(2 * (size_t)total_edges, 0);
    P.free_v.clear(); P.first.clear(); P.rowptr.clear();
    P.total_free = P.total_blocks = P.total_y = 0;
    for (int j = 0; j < njobs; ++j) {
        const PgIn &I = in[j];
        if (I.nkf < 0 || I.nedge < 0 || I.npt < 0 || I.kf_ofs < 0 || I.edge_ofs < 0 || I.pt_ofs < 0 || (long long)I.kf_ofs + I.nkf > total_kf ||
            (long long)I.edge_ofs + I.nedge > total_edges || (long long)I.pt_ofs + I.npt > total_pts)
            return "a job's ranges leave the arrays";
        if (I.nkf == 0 && I.nedge > 0) return "a job has edges but no vertices";
        if (j > 0 && (I.kf_ofs < in[j - 1].kf_ofs + in[j - 1].nkf || I.edge_ofs < in[j - 1].edge_ofs + in[j - 1].nedge || I.pt_ofs < in[j - 1].pt_ofs + in[j - 1].npt))
            return "the jobs' ranges must ascend and not overlap";
        PgJob &J = P.jobs[(size_t)j];
        memset(&J, 0, sizeof(J));
        J.nkf = I.nkf; J.nedge = I.nedge; J.npt = I.npt; J.kf_ofs = I.kf_ofs; J.edge_ofs = I.edge_ofs; J.pt_ofs = I.pt_ofs;
        J.free_ofs = (int)P.total_free; J.inc_ofs = I.kf_ofs + j; J.trace_slot = j < trace_jobs ? j : -1; J.iters = iters;
        J.env_ofs = P.total_blocks; J.y_ofs = P.total_y;
        int nfixed = 0;
        for (int v = 0; v < I.nkf; ++v) {
            const double *q = poses + 7 * (size_t)(I.kf_ofs + v);
            const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            if (!(fabs(n2 - 1.0) <= 2e-6)) return "a pose's quaternion is not of unit length (1e-6)";
            if (fixed[I.kf_ofs + v]) ++nfixed;
            else { P.fidx[(size_t)(I.kf_ofs + v)] = J.nfree++; P.free_v.push_back(v); }
        }
        if (I.nkf > 0 && nfixed == 0) return "a job has vertices but none of them is fixed";
        if (J.nfree > 0x7fffffff / 42) return "a job has more than 2^31 / 42 free vertices";           // the kernel's int loop bounds (nfree * 42)
        for (int p = 0; p < I.npt; ++p) {
            const int a = anchor[I.pt_ofs + p];
            if (a < -1 || a >= I.nkf) return "a point's anchor is not a vertex of its job";
        }
        // envelope and incidence lists
        const size_t f0 = P.first.size();
        for (int f = 0; f < J.nfree; ++f) P.first.push_back(f);
        int *inc = P.inc_start.data() + J.inc_ofs;              // nkf + 1 entries
        for (int e = 0; e < I.nedge; ++e) {
            const int a = ea[I.edge_ofs + e], b = eb[I.edge_ofs + e];
            if (a < 0 || a >= I.nkf || b < 0 || b >= I.nkf) return "an edge's vertex index is out of its job's range";
            if (a == b) return "an edge joins a vertex to itself";
            ++inc[a + 1]; ++inc[b + 1];
            const int fa = P.fidx[(size_t)(I.kf_ofs + a)], fb = P.fidx[(size_t)(I.kf_ofs + b)];
            if (fa >= 0 && fb >= 0) {
                const int hi = fa > fb ? fa : fb, lo = fa > fb ? fb : fa;
                if (lo < P.first[f0 + (size_t)hi]) P.first[f0 + (size_t)hi] = lo;
            }
        }
        for (int v = 0; v < I.nkf; ++v) inc[v + 1] += inc[v];
        {
            std::vector<int> fill(inc, inc + I.nkf);
            int *ie = P.inc_edge.data() + 2 * (size_t)I.edge_ofs;
            for (int e = 0; e < I.nedge; ++e) {              // ascending edge order inside every list
                ie[fill[(size_t)ea[I.edge_ofs + e]]++] = e;
                ie[fill[(size_t)eb[I.edge_ofs + e]]++] = e;
            }
        }
        long long nb = 0; int maxspan = 0;
        for (int f = 0; f < J.nfree; ++f) {
            const int span = f - P.first[f0 + (size_t)f];
            if (nb > 0x7fffffffll - span - 1) return "a job's envelope has more than 2^31 blocks";
            P.rowptr.push_back((int)nb);
            nb += span + 1;
            if (span > maxspan) maxspan = span;
        }
        J.nblocks = nb; J.maxspan = maxspan;
        P.total_free += J.nfree; P.total_blocks += nb; P.total_y += maxspan;
        if (P.total_free > 0x7fffffffll / 36) return "too many free vertices in one call";
    }
    return nullptr;
}

// one buffer: [jobs | poses | meas | pts] (read back) [ints] (uploaded with them) [solver scratch]
static inline PgBuf pg_layout(PgPlan &P, int njobs, int total_kf, int total_edges, int total_pts, unsigned char *base)
{
    PgBuf B;
    size_t o = 0;
    auto takeD = [&](size_t n) { double *p = (double *)(base + o); o += 8 * n; return p; };
    auto takeI = [&](size_t n) { int *p = (int *)(base + o); o += 4 * n; return p; };
    B.jobs = (PgJob *)(base + o); o += sizeof(PgJob) * (size_t)njobs; o = (o + 7) & ~(size_t)7;
    B.poses = takeD(7 * (size_t)total_kf); B.meas = takeD(7 * (size_t)total_edges); B.pts = takeD(3 * (size_t)total_pts);
    P.result_bytes = o;
    B.ea = takeI((size_t)total_edges); B.eb = takeI((size_t)total_edges); B.fidx = takeI((size_t)total_kf);
    B.free_v = takeI((size_t)P.total_free); B.first = takeI((size_t)P.total_free); B.rowptr = takeI((size_t)P.total_free);
    B.inc_start = takeI((size_t)total_kf + (size_t)njobs); B.inc_edge = takeI(2 * (size_t)total_edges); B.anchor = takeI((size_t)total_pts);
    o = (o + 7) & ~(size_t)7;
    P.front_bytes = o;
    B.poses0 = takeD(7 * (size_t)total_kf); B.poses_sv = takeD(7 * (size_t)total_kf);
    B.J = takeD(78 * (size_t)total_edges); B.chi_e = takeD((size_t)total_edges);
    B.b = takeD(6 * (size_t)P.total_free); B.z = takeD(6 * (size_t)P.total_free); B.x = takeD(6 * (size_t)P.total_free);
    B.Dinv = takeD(36 * (size_t)P.total_free);
    B.H = takeD(36 * (size_t)P.total_blocks); B.L = takeD(36 * (size_t)P.total_blocks); B.Y = takeD(36 * (size_t)P.total_y);
    P.bytes = o;
    return B;
}

// the uploaded part of the buffer, written through a host view of the same layout
static inline void pg_fill_front(const PgPlan &P, const PgBuf &Hb, int njobs, int total_kf, const double *poses, int total_edges,
                                 const int *ea, const int *eb, const double *meas, int total_pts, const int *anchor, const double *pts)
{
    memcpy(Hb.jobs, P.jobs.data(), sizeof(PgJob) * (size_t)njobs);
    if (total_kf) memcpy(Hb.poses, poses, 56 * (size_t)total_kf);
    if (total_edges) { memcpy(Hb.meas, meas, 56 * (size_t)total_edges); memcpy(Hb.ea, ea, 4 * (size_t)total_edges); memcpy(Hb.eb, eb, 4 * (size_t)total_edges); }
    if (total_pts) { memcpy(Hb.pts, pts, 24 * (size_t)total_pts); memcpy(Hb.anchor, anchor, 4 * (size_t)total_pts); }
    if (total_kf) memcpy(Hb.fidx, P.fidx.data(), 4 * (size_t)total_kf);
    if (P.total_free) {
        memcpy(Hb.free_v, P.free_v.data(), 4 * (size_t)P.total_free); memcpy(Hb.first, P.first.data(), 4 * (size_t)P.total_free);
        memcpy(Hb.rowptr, P.rowptr.data(), 4 * (size_t)P.total_free);
    }
    memcpy(Hb.inc_start, P.inc_start.data(), 4 * P.inc_start.size());
    if (total_edges) memcpy(Hb.inc_edge, P.inc_edge.data(), 4 * P.inc_edge.size());
}

// ---- SE(3), Sophus layout qx qy qz qw tx ty tz; the operation order of tests/ref_pose_graph.py ----------------------------------
PG_DEV void pg_rot(const double *q, const double *v, double *o)
{
    double ux = q[1] * v[2] - q[2] * v[1];
    double uy = q[2] * v[0] - q[0] * v[2];
    double uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    const double o0 = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
    const double o1 = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
    const double o2 = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
    o[0] = o0; o[1] = o1; o[2] = o2;
}
PG_DEV void pg_mul(const double *A, const double *B, double *C)
{
    const double ax = A[0], ay = A[1], az = A[2], aw = A[3];
    const double bx = B[0], by = B[1], bz = B[2], bw = B[3];
    double q0 = aw * bx + ax * bw + ay * bz - az * by;
    double q1 = aw * by + ay * bw + az * bx - ax * bz;
    double q2 = aw * bz + az * bw + ax * by - ay * bx;
    double q3 = aw * bw - ax * bx - ay * by - az * bz;
    const double n2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3;
    if (n2 != 1.0) { const double s = 2.0 / (1.0 + n2); q0 *= s; q1 *= s; q2 *= s; q3 *= s; }
    double t[3];
    pg_rot(A, B + 4, t);
    C[4] = A[4] + t[0]; C[5] = A[5] + t[1]; C[6] = A[6] + t[2];
    C[0] = q0; C[1] = q1; C[2] = q2; C[3] = q3;
}
PG_DEV void pg_inv(const double *T, double *R)
{
    const double nt[3] = { -T[4], -T[5], -T[6] };
    R[0] = -T[0]; R[1] = -T[1]; R[2] = -T[2]; R[3] = T[3];
    pg_rot(R, nt, R + 4);
}
PG_DEV void pg_act(const double *T, const double *p, double *o)
{
    pg_rot(T, p, o);
    o[0] += T[4]; o[1] += T[5]; o[2] += T[6];
}
PG_DEV void pg_hat(const double *w, double *O)
{
    O[0] = 0; O[1] = -w[2]; O[2] = w[1]; O[3] = w[2]; O[4] = 0; O[5] = -w[0]; O[6] = -w[1]; O[7] = w[0]; O[8] = 0;
}
PG_DEV void pg_m3(const double *A, const double *B, double *C)        // C = A B (C distinct from A and B)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
PG_DEV void pg_quat_to_R(const double *q, double *R)                    // columns = rotated unit vectors, as the reference builds it
{
    for (int c = 0; c < 3; ++c) {
        const double e[3] = { c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0 };
        double o[3];
        pg_rot(q, e, o);
        R[c] = o[0]; R[3 + c] = o[1]; R[6 + c] = o[2];
    }
}
PG_DEV void pg_log(const double *T, double *xi)
{
    const double EPS = 1e-10;
    const double n2 = T[0] * T[0] + T[1] * T[1] + T[2] * T[2], w = T[3];
    double two_atan;
    if (n2 < EPS * EPS) two_atan = 2.0 / w - (2.0 / 3.0) * n2 / (w * w * w);
    else {
        const double n = sqrt(n2);
        if (fabs(w) < EPS) two_atan = (w > 0 ? M_PI : -M_PI) / n;
        else two_atan = 2.0 * atan(n / w) / n;
    }
    const double om[3] = { two_atan * T[0], two_atan * T[1], two_atan * T[2] };
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    double O[9], O2[9];
    pg_hat(om, O); pg_m3(O, O, O2);
    double c;
    if (fabs(theta) < EPS) c = 1.0 / 12.0;
    else { const double half = 0.5 * theta; c = (1.0 - theta * cos(half) / (2.0 * sin(half))) / (theta * theta); }
    double Vi[9];
    for (int i = 0; i < 9; ++i) Vi[i] = ((i % 4 == 0 ? 1.0 : 0.0) - 0.5 * O[i]) + c * O2[i];
    const double *t = T + 4;
    for (int i = 0; i < 3; ++i) xi[i] = (Vi[i * 3] * t[0] + Vi[i * 3 + 1] * t[1]) + Vi[i * 3 + 2] * t[2];
    xi[3] = om[0]; xi[4] = om[1]; xi[5] = om[2];
}
PG_DEV void pg_exp(const double *xi, double *T)
{
    const double EPS = 1e-10;
    const double *u = xi, *om = xi + 3;
    const double th2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double theta, imag, real;
    if (th2 < EPS * EPS) {
        theta = 0;
        const double th4 = th2 * th2;
        imag = 0.5 - th2 / 48.0 + th4 / 3840.0;
        real = 1.0 - th2 / 8.0 + th4 / 384.0;
    } else {
        theta = sqrt(th2);
        imag = sin(0.5 * theta) / theta;
        real = cos(0.5 * theta);
    }
    T[0] = imag * om[0]; T[1] = imag * om[1]; T[2] = imag * om[2]; T[3] = real;
    double V[9];
    if (theta < EPS) pg_quat_to_R(T, V);
    else {
        double O[9], O2[9];
        pg_hat(om, O); pg_m3(O, O, O2);
        const double a = (1.0 - cos(theta)) / th2, b = (theta - sin(theta)) / (th2 * theta);
        for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * O[i]) + b * O2[i];
    }
    for (int i = 0; i < 3; ++i) T[4 + i] = (V[i * 3] * u[0] + V[i * 3 + 1] * u[1]) + V[i * 3 + 2] * u[2];
}

// e = log(M^-1 (T_a T_b^-1)).  The product is associated this way, not as the reference's (M^-1 T_a) T_b^-1, on purpose: T_a T_b^-1
// is then formed by the very operations the host forms relative_pose_pkf with (host/se3.h, no contraction), so an odometry edge
// whose measurement IS that product has M^-1 M = (0, 0, 0, w; 0, 0, 0) exactly and e = 0 exactly — a graph without loop edges has
// chi2 = 0, no trial can be accepted and the poses come back with their input bits.
PG_DEV void pg_edge_error(const double *M, const double *Ta, const double *Tb, double *e)
{
    double Mi[7], Tbi[7], D[7], E[7];
    pg_inv(M, Mi); pg_inv(Tb, Tbi);
    pg_mul(Ta, Tbi, D); pg_mul(Mi, D, E);
    pg_log(E, e);
}

// inverse RIGHT Jacobian of SE(3) at e (= inverse left Jacobian at -e), tangent ordered (translation, rotation):
// [[Ji, -Ji Q Ji], [0, Ji]], Ji = I - P/2 + c P^2, Q as in Barfoot (7.86); power series of the four coefficients below 0.1 rad
PG_DEV void pg_jr_inv(const double *e, double *J)
{
    const double rho[3] = { -e[0], -e[1], -e[2] }, phi[3] = { -e[3], -e[4], -e[5] };
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    const double theta = sqrt(t2);
    double c, a1, a2, a3;
    if (theta < 0.1) {
        c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 / 1209600.0));
        a1 = 1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 / 362880.0));
        a2 = 1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0 - t2 / 3628800.0));
        a3 = 1.0 / 120.0 - t2 * (1.0 / 2520.0 - t2 * (1.0 / 120960.0 - t2 / 9979200.0));
    } else {
        const double s = sin(theta), co = cos(theta);
        c = 1.0 / t2 - (1.0 + co) / (2.0 * theta * s);
        a1 = (theta - s) / (t2 * theta);
        a2 = (t2 + 2.0 * co - 2.0) / (2.0 * t2 * t2);
        a3 = (2.0 * theta - 3.0 * s + theta * co) / (2.0 * t2 * t2 * theta);
    }
    double P[9], R[9], PP[9], Ji[9], PR[9], RP[9], PRP[9], PPR[9], RPP[9], PRPP[9], PPRP[9], Q[9], T1[9], T2[9];
    pg_hat(phi, P); pg_hat(rho, R);
    pg_m3(P, P, PP); pg_m3(P, R, PR); pg_m3(R, P, RP); pg_m3(PR, P, PRP);
    pg_m3(P, PR, PPR); pg_m3(RP, P, RPP); pg_m3(PRP, P, PRPP); pg_m3(P, PRP, PPRP);
    for (int i = 0; i < 9; ++i) {
        Ji[i] = ((i % 4 == 0 ? 1.0 : 0.0) - 0.5 * P[i]) + c * PP[i];
        Q[i] = ((0.5 * R[i] + a1 * ((PR[i] + RP[i]) + PRP[i])) + a2 * ((PPR[i] + RPP[i]) - 3.0 * PRP[i])) + a3 * (PRPP[i] + PPRP[i]);
    }
    pg_m3(Ji, Q, T1); pg_m3(T1, Ji, T2);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            J[i * 6 + j] = Ji[i * 3 + j]; J[(i + 3) * 6 + j + 3] = Ji[i * 3 + j];
            J[i * 6 + j + 3] = -T2[i * 3 + j]; J[(i + 3) * 6 + j] = 0.0;
        }
}

// out[0..5] = e, out[6..41] = J_a, out[42..77] = Jr^-1(e) (J_b is its negative)
PG_DEV void pg_edge_linearise(const double *M, const double *Ta, const double *Tb, double *out)
{
    pg_edge_error(M, Ta, Tb, out);
    double *Jr = out + 42, *Ja = out + 6;
    pg_jr_inv(out, Jr);
    double Tai[7], Di[7], Rm[9], Tx[9], TR[9], Ad[36];
    pg_inv(Ta, Tai); pg_mul(Tb, Tai, Di);                    // (T_a T_b^-1)^-1
    pg_quat_to_R(Di, Rm); pg_hat(Di + 4, Tx); pg_m3(Tx, Rm, TR);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ad[i * 6 + j] = Rm[i * 3 + j]; Ad[(i + 3) * 6 + j + 3] = Rm[i * 3 + j];
            Ad[i * 6 + j + 3] = TR[i * 3 + j]; Ad[(i + 3) * 6 + j] = 0.0;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int m = 0; m < 6; ++m) s += Jr[i * 6 + m] * Ad[m * 6 + j];
            Ja[i * 6 + j] = s;
        }
}

// inverse of a symmetric 6x6 block by an unpivoted scalar LDL^T (tests/ref_pose_graph.py: _ldlt6_inv); false: a pivot is not positive
PG_DEV bool pg_ldlt6_inv(const double *D, double *inv)
{
    double L[36], d[6];
    bool ok = true;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < i; ++j) {
            double s = D[i * 6 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * d[k] * L[j * 6 + k];
            L[i * 6 + j] = s / d[j];
        }
        double s = D[i * 6 + i];
        for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * L[i * 6 + k] * d[k];
        d[i] = s;
        if (!(s > 0.0 && s < INFINITY)) ok = false;
    }
    for (int c = 0; c < 6; ++c) {
        double y[6];
        for (int i = 0; i < 6; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
            y[i] = s;
        }
        for (int i = 0; i < 6; ++i) y[i] = y[i] / d[i];
        for (int i = 5; i >= 0; --i) {
            double s = y[i];
            for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * y[k];
            y[i] = s;
        }
        for (int i = 0; i < 6; ++i) inv[i * 6 + c] = y[i];
    }
    return ok;
}

// ---- one job ---------------------------------------------------------------------------------------------------------------------
struct PgShared {
    double part[PG_THREADS];
    double blk[36];
    double fw[PG_FWD_GROUPS * 6];
    double cur, temp, lambda, nu, rho, scale;
    int ok, accepted, stop, qmax;
};

// chi2 of the state in `poses` (and, with lin, the Jacobians) -> S.part; lane 0 adds the partial sums in lane order
#define PG_SUM_PARTS(dst)                                                                  \
    PG_PAR { if (tid == 0) { double s_ = 0.0; for (int t_ = 0; t_ < PG_THREADS; ++t_) s_ += S.part[t_]; (dst) = s_; } } PG_SYNC

PG_DEV void pg_run(const PgBuf &B, PgJob &J, PgShared &S, double *trace_all)
{
    const int nkf = J.nkf, ne = J.nedge, nf = J.nfree;
    double *poses = B.poses + 7 * (size_t)J.kf_ofs, *poses0 = B.poses0 + 7 * (size_t)J.kf_ofs, *poses_sv = B.poses_sv + 7 * (size_t)J.kf_ofs;
    const double *meas = B.meas + 7 * (size_t)J.edge_ofs;
    const int *ea = B.ea + J.edge_ofs, *eb = B.eb + J.edge_ofs, *fidx = B.fidx + J.kf_ofs;
    const int *free_v = B.free_v + J.free_ofs, *first = B.first + J.free_ofs, *rowptr = B.rowptr + J.free_ofs;
    const int *inc_start = B.inc_start + J.inc_ofs, *inc_edge = B.inc_edge + 2 * (size_t)J.edge_ofs;
    double *Jb = B.J + 78 * (size_t)J.edge_ofs, *chi_e = B.chi_e + J.edge_ofs;
    double *bv = B.b + 6 * (size_t)J.free_ofs, *zv = B.z + 6 * (size_t)J.free_ofs, *xv = B.x + 6 * (size_t)J.free_ofs;
    double *Dinv = B.Dinv + 36 * (size_t)J.free_ofs;
    double *H = B.H + 36 * (size_t)J.env_ofs, *L = B.L + 36 * (size_t)J.env_ofs, *Y = B.Y + 36 * (size_t)J.y_ofs;
    double *trace = (trace_all && J.trace_slot >= 0) ? trace_all + (size_t)J.trace_slot * LM_TRACE_STRIDE : nullptr;
    const long long nent = 36 * J.nblocks;
#define PG_BLK(base, i, j) ((base) + 36 * ((size_t)rowptr[i] + (size_t)((j) - first[i])))

    PG_PAR { for (int i = tid; i < 7 * nkf; i += PG_THREADS) poses0[i] = poses[i]; } PG_SYNC
    int it_done = 0, n_trials = 0;
    double chi_first = 0.0, chi_last = 0.0;
    if (nkf > 0 && ne > 0) {
        PG_PAR { if (tid == 0) { S.lambda = 0.0; S.nu = 2.0; S.cur = 0.0; S.rho = 0.0; S.qmax = 0; S.stop = 0; } } PG_SYNC
        for (int it = 0; it < J.iters; ++it) {
            // linearise
            PG_PAR {
                double s = 0.0;
                for (int e = tid; e < ne; e += PG_THREADS) {
                    double *o = Jb + 78 * (size_t)e;
                    pg_edge_linearise(meas + 7 * (size_t)e, poses + 7 * (size_t)ea[e], poses + 7 * (size_t)eb[e], o);
                    const double c = ((((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]) + o[4] * o[4]) + o[5] * o[5];
                    chi_e[e] = c; s += c;
                }
                S.part[tid] = s;
                for (long long i = tid; i < nent; i += PG_THREADS) H[i] = 0.0;
            } PG_SYNC
            PG_SUM_PARTS(S.cur)
            if (it == 0) chi_first = S.cur;
            // assemble: an entry of a block row has one owner, which walks the row's edges in ascending order
            PG_PAR {
                for (int w = tid; w < nf * 42; w += PG_THREADS) {
                    const int f = w / 42, l = w % 42, v = free_v[f];
                    if (l < 36) {
                        const int r = l / 6, c = l % 6;
                        double dg = 0.0;
                        for (int u = inc_start[v]; u < inc_start[v + 1]; ++u) {
                            const int e = inc_edge[u];
                            const double *o = Jb + 78 * (size_t)e;
                            const bool isa = ea[e] == v;
                            const double *Jv = isa ? o + 6 : o + 42, *Ju = isa ? o + 42 : o + 6;
                            double s = 0.0;
                            for (int m = 0; m < 6; ++m) s += Jv[m * 6 + r] * Jv[m * 6 + c];
                            dg += s;
                            const int fo = fidx[isa ? eb[e] : ea[e]];
                            if (fo >= 0 && fo < f) {
                                double t = 0.0;
                                for (int m = 0; m < 6; ++m) t += Jv[m * 6 + r] * Ju[m * 6 + c];
                                PG_BLK(H, f, fo)[l] -= t;                  // one of the two Jacobians is -Jr^-1
                            }
                        }
                        PG_BLK(H, f, f)[l] = dg;
                    } else {
                        const int r = l - 36;
                        double s = 0.0;
                        for (int u = inc_start[v]; u < inc_start[v + 1]; ++u) {
                            const int e = inc_edge[u];
                            const double *o = Jb + 78 * (size_t)e;
                            const bool isa = ea[e] == v;
                            const double *Jv = isa ? o + 6 : o + 42;
                            double t = 0.0;
                            for (int m = 0; m < 6; ++m) t += Jv[m * 6 + r] * o[m];
                            if (isa) s -= t; else s += t;
                        }
                        bv[6 * f + r] = s;
                    }
                }
            } PG_SYNC
            if (it == 0) {
                PG_PAR {
                    double md = 0.0;
                    for (int w = tid; w < nf * 6; w += PG_THREADS) { const double d = fabs(PG_BLK(H, w / 6, w / 6)[(w % 6) * 7]); if (d > md) md = d; }
                    S.part[tid] = md;
                } PG_SYNC
                PG_PAR { if (tid == 0) { double md = 0.0; for (int t = 0; t < PG_THREADS; ++t) if (S.part[t] > md) md = S.part[t]; S.lambda = 1e-5 * md; S.nu = 2.0; } } PG_SYNC
            }
            PG_PAR { if (tid == 0) { S.rho = 0.0; S.qmax = 0; } } PG_SYNC
            int qmax = 0; double rho = 0.0; bool stop = false;
            do {
                const double lambda = S.lambda;
                // save the state, copy H with lambda on the diagonal
                PG_PAR {
                    for (int i = tid; i < 7 * nkf; i += PG_THREADS) poses_sv[i] = poses[i];
                    for (long long i = tid; i < nent; i += PG_THREADS) L[i] = H[i];
                    if (tid == 0) S.ok = 1;
                } PG_SYNC
                PG_PAR { for (int w = tid; w < nf * 6; w += PG_THREADS) PG_BLK(L, w / 6, w / 6)[(w % 6) * 7] += lambda; } PG_SYNC
                // factorise, rows in order
                for (int i = 0; i < nf; ++i) {
                    const int fi = first[i];
                    for (int j = fi; j < i; ++j) {
                        PG_PAR {
                            if (tid < 36) {
                                const int r = tid / 6, c = tid % 6, fj = first[j];
                                double acc = PG_BLK(L, i, j)[tid];
                                for (int k = fi > fj ? fi : fj; k < j; ++k) {
                                    const double *Yik = Y + 36 * (size_t)(k - fi), *Ljk = PG_BLK(L, j, k);
                                    double s = 0.0;
                                    for (int m = 0; m < 6; ++m) s += Yik[r * 6 + m] * Ljk[c * 6 + m];
                                    acc -= s;
                                }
                                Y[36 * (size_t)(j - fi) + tid] = acc;
                            }
                        } PG_SYNC
                        PG_PAR {
                            if (tid < 36) {
                                const int r = tid / 6, c = tid % 6;
                                const double *Yij = Y + 36 * (size_t)(j - fi), *Dj = Dinv + 36 * (size_t)j;
                                double s = 0.0;
                                for (int m = 0; m < 6; ++m) s += Yij[r * 6 + m] * Dj[m * 6 + c];
                                PG_BLK(L, i, j)[tid] = s;
                            }
                        } PG_SYNC
                    }
                    PG_PAR {
                        if (tid < 36) {
                            const int r = tid / 6, c = tid % 6;
                            double acc = PG_BLK(L, i, i)[tid];
                            for (int k = fi; k < i; ++k) {
                                const double *Yik = Y + 36 * (size_t)(k - fi), *Lik = PG_BLK(L, i, k);
                                double s = 0.0;
                                for (int m = 0; m < 6; ++m) s += Yik[r * 6 + m] * Lik[c * 6 + m];
                                acc -= s;
                            }
                            S.blk[tid] = acc;
                        }
                    } PG_SYNC
                    PG_PAR { if (tid == 0) { if (!pg_ldlt6_inv(S.blk, Dinv + 36 * (size_t)i)) S.ok = 0; } } PG_SYNC
                }
                const bool ok = S.ok != 0;
                if (ok) {
                    // forward sweep: z_i = b_i - sum_k L(i,k) z_k
                    for (int i = 0; i < nf; ++i) {
                        const int fi = first[i];
                        PG_PAR {
                            if (tid < 6 * PG_FWD_GROUPS) {
                                const int c = tid % 6, g = tid / 6;
                                double s = 0.0;
                                for (int k = fi + g; k < i; k += PG_FWD_GROUPS) {
                                    const double *Lik = PG_BLK(L, i, k), *zk = zv + 6 * (size_t)k;
                                    double t = 0.0;
                                    for (int m = 0; m < 6; ++m) t += Lik[c * 6 + m] * zk[m];
                                    s += t;
                                }
                                S.fw[g * 6 + c] = s;
                            }
                        } PG_SYNC
                        PG_PAR {
                            if (tid < 6) {
                                double s = 0.0;
                                for (int g = 0; g < PG_FWD_GROUPS; ++g) s += S.fw[g * 6 + tid];
                                zv[6 * (size_t)i + tid] = bv[6 * (size_t)i + tid] - s;
                            }
                        } PG_SYNC
                    }
                    PG_PAR {
                        for (int w = tid; w < nf * 6; w += PG_THREADS) {
                            const double *Di = Dinv + 36 * (size_t)(w / 6), *zi = zv + 6 * (size_t)(w / 6);
                            double s = 0.0;
                            for (int m = 0; m < 6; ++m) s += Di[(w % 6) * 6 + m] * zi[m];
                            xv[w] = s;
                        }
                    } PG_SYNC
                    // backward sweep, column-oriented: x_k -= L(i,k)^T x_i for the rows k of i's envelope
                    for (int i = nf - 1; i > 0; --i) {
                        const int fi = first[i];
                        if (fi == i) continue;
                        PG_PAR {
                            for (int w = tid; w < (i - fi) * 6; w += PG_THREADS) {
                                const int k = fi + w / 6, c = w % 6;
                                const double *Lik = PG_BLK(L, i, k), *xi = xv + 6 * (size_t)i;
                                double s = 0.0;
                                for (int m = 0; m < 6; ++m) s += Lik[m * 6 + c] * xi[m];
                                xv[6 * (size_t)k + c] -= s;
                            }
                        } PG_SYNC
                    }
                    // rho's denominator and the update T <- exp(d) T
                    PG_PAR {
                        double s = 0.0;
                        for (int w = tid; w < nf * 6; w += PG_THREADS) s += xv[w] * (lambda * xv[w] + bv[w]);
                        S.part[tid] = s;
                        for (int f = tid; f < nf; f += PG_THREADS) {
                            double dT[7], Tn[7];
                            double *T = poses + 7 * (size_t)free_v[f];
                            pg_exp(xv + 6 * (size_t)f, dT);
                            pg_mul(dT, T, Tn);
                            for (int m = 0; m < 7; ++m) T[m] = Tn[m];
                        }
                    } PG_SYNC
                    PG_SUM_PARTS(S.scale)
                }
                // chi2 of the trial state
                PG_PAR {
                    double s = 0.0;
                    for (int e = tid; e < ne; e += PG_THREADS) {
                        double er[6];
                        pg_edge_error(meas + 7 * (size_t)e, poses + 7 * (size_t)ea[e], poses + 7 * (size_t)eb[e], er);
                        s += ((((er[0] * er[0] + er[1] * er[1]) + er[2] * er[2]) + er[3] * er[3]) + er[4] * er[4]) + er[5] * er[5];
                    }
                    S.part[tid] = s;
                } PG_SYNC
                PG_SUM_PARTS(S.temp)
                // g2o's decision
                PG_PAR {
                    if (tid == 0) {
                        double temp = S.temp;
                        if (!ok) temp = 1.7976931348623157e308;
                        double r = S.cur - temp;
                        const double scale = (ok ? S.scale : 0.0) + 1e-3;
                        r /= scale;
                        const bool acc = r > 0 && temp < INFINITY && temp == temp;
                        if (trace) {
                            const int n = (int)trace[0];
                            if (n < LM_TRACE_CAP) {
                                double *t = trace + 8 + LM_TRACE_REC * n;
                                t[0] = it; t[1] = S.lambda; t[2] = S.cur; t[3] = temp; t[4] = r; t[5] = acc ? 1.0 : 0.0;
                                trace[0] = (double)(n + 1);
                            }
                        }
                        S.stop = 0;
                        if (acc) {
                            double alpha = 1.0 - (2.0 * r - 1.0) * (2.0 * r - 1.0) * (2.0 * r - 1.0);
                            if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                            S.lambda *= alpha < 1.0 / 3.0 ? 1.0 / 3.0 : alpha; S.nu = 2.0; S.cur = temp;
                        } else {
                            S.lambda *= S.nu; S.nu *= 2.0;
                            if (!(fabs(S.lambda) < INFINITY)) S.stop = 1;
                        }
                        S.accepted = acc ? 1 : 0; S.rho = r;
                        if (!S.stop) S.qmax++;
                    }
                } PG_SYNC
                ++n_trials;
                const bool accepted = S.accepted != 0;
                rho = S.rho; qmax = S.qmax; stop = S.stop != 0;
                if (!accepted) {
                    PG_PAR { for (int i = tid; i < 7 * nkf; i += PG_THREADS) poses[i] = poses_sv[i]; } PG_SYNC
                }
                chi_last = S.cur;
            } while (!stop && rho < 0 && qmax < 10);
            ++it_done;
            if (qmax == 10 || rho == 0 || stop) break;
        }
    }
    // landmarks keep their coordinates in the frame of their anchor keyframe (src/loopclosure.cpp:760-784)
    PG_PAR {
        for (int p = tid; p < J.npt; p += PG_THREADS) {
            const int a = B.anchor[J.pt_ofs + p];
            if (a < 0) continue;
            double *x = B.pts + 3 * (size_t)(J.pt_ofs + p), s[3], Ti[7];
            pg_act(poses0 + 7 * (size_t)a, x, s);
            pg_inv(poses + 7 * (size_t)a, Ti);
            pg_act(Ti, s, x);
        }
        if (tid == 0) { J.iters_done = it_done; J.n_trials = n_trials; J.chi2_before = chi_first; J.chi2_after = chi_last; }
    } PG_SYNC
#undef PG_BLK
}

#ifndef PG_HOST_EMU
__global__ void __launch_bounds__(PG_THREADS) k_pose_graph(PgBuf B, double *trace_all)
{
    __shared__ PgShared S;
    pg_run(B, B.jobs[blockIdx.x], S, trace_all);
}
#endif
