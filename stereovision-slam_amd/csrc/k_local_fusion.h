// k_local_fusion.h — the arithmetic of LoopClosure::LocalFusion (svslam_local_fusion_batch): steps 1-3 of the reference's
// src/loopclosure.cpp:439-526, the corrected poses of the active window, the active landmarks moved with the keyframe that first
// saw them, and the frontend's last frame.  The numeric contract is tests/ref_local_fusion.py; DESIGN 15 has the rules and the
// declared deviation.  The map surgery that follows in the reference (:530-573) is the host's.
//
// One job = one closed loop of one stream = one workgroup of LF_THREADS = 256 threads; `cur` is the keyframe that closed the loop.
//
//   table       lane per row of the corrected table: row i < nkf is window keyframe i, row nkf is `cur` when it has left the window.
//               corrected[cur] = T_corr, corrected[i] = (T_i T_cur^-1) T_corr in that association (:462-464).  Lane 0 also moves the
//               last frame: a window keyframe takes its row, any other frame (T_f T_cur^-1) T_corr (:507, :524)
//   landmarks   lane per landmark: it walks the landmark's observation list in list order and takes the FIRST entry >= 0 (the host
//               writes -1 where the feature no longer names a live landmark or its frame has no row: the three conditions of
//               :479-488), then p' = corrected[k]^-1 (T_k p) with the OLD T_k (:498-500).  A landmark without such an entry keeps
//               its position and is counted (the reference asserts and dereferences null: declared deviation)
//   count       the lanes' counts go through LDS and lane 0 adds them: integers, no order to fix
//
// The uploaded poses are never written: the table is a buffer of its own, so "old T_k" needs no copy and no lane reads what another
// writes inside a phase.  No atomics; every floating-point result is a function of the job's inputs alone (pg_mul / pg_inv / pg_act
// of k_pose_graph.h, f64, no contraction), not of the launch.  Plain C++ between the HIP qualifiers: compiled for the host with
// LF_HOST_EMU (tests/cpp/lf_host_emu) a phase becomes a loop over the 256 thread numbers.
#pragma once
#if defined(LF_HOST_EMU) && !defined(PG_HOST_EMU)
#define PG_HOST_EMU
#endif
#include "k_pose_graph.h"          // PG_DEV and the SE(3) functions (pg_mul, pg_inv, pg_act)
#pragma clang fp contract(off)

#define LF_THREADS 256

#ifdef PG_HOST_EMU
#define LF_PAR for (int tid = 0; tid < LF_THREADS; ++tid)
#define LF_SYNC
#else
#define LF_PAR for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define LF_SYNC __syncthreads();
#endif

struct LfJob {
    int kf_ofs, nkf, pt_ofs, npt;
    int cur, last, corr_ofs;                    // corr_ofs: the job's first row of the corrected table (nkf + 1 rows)
    int n_unanchored;                           // out
    double T_cur[7], T_corr[7];
    double T_last[7];                           // in / out
};

struct LfBuf {
    LfJob *jobs;
    double *pts;                                // [total_pts][3], in place
    double *corr;                               // [total_kf + njobs][7]: the corrected table, device output
    int *pt_kf;                                 // [total_pts]: the row a landmark moved with, or -1
    const double *poses;                        // [total_kf][7], the old poses: read only
    const int *obs_ptr, *obs_kf;                // CSR over all landmarks of the call: [total_pts + 1], [total_obs]
};

struct LfIn { int kf_ofs, nkf, pt_ofs, npt, cur, last; const double *T_cur, *T_corr, *T_last; };

struct LfSizes { size_t result_bytes = 0, bytes = 0; };

static inline bool lf_unit(const double *q) { return fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 2e-6; }

// The host's rules.  Returns nullptr or the reason the call is refused (nothing has been written or launched then).
// The arrays may be null where their count is 0; obs_ptr has total_pts + 1 entries whenever total_pts > 0.
static inline const char *lf_plan(int njobs, const LfIn *in, int total_kf, const double *poses, int total_pts, const double *pts,
                                  const int *obs_ptr, int total_obs, const int *obs_kf, const int *pt_kf)
{
    if (njobs < 0 || total_kf < 0 || total_pts < 0 || total_obs < 0) return "negative count";
    if (njobs == 0) return nullptr;
    if (!in) return "null jobs";
    if ((total_kf && !poses) || (total_pts && (!pts || !obs_ptr || !pt_kf)) || (total_obs && !obs_kf)) return "null array";
    if ((long long)total_kf + njobs > 0x7fffffffll / 7) return "too many keyframes in one call";
    if (total_pts) {
        if (obs_ptr[0] < 0 || obs_ptr[total_pts] > total_obs) return "obs_ptr leaves obs_kf";
        for (int p = 0; p < total_pts; ++p)
            if (obs_ptr[p + 1] < obs_ptr[p]) return "obs_ptr descends";
    }
    for (int j = 0; j < njobs; ++j) {
        const LfIn &I = in[j];
        if (I.nkf < 0 || I.npt < 0) return "negative count";
        if (I.kf_ofs < 0 || I.pt_ofs < 0 || (long long)I.kf_ofs + I.nkf > total_kf || (long long)I.pt_ofs + I.npt > total_pts)
            return "a job's ranges leave the arrays";
        if (j > 0 && (I.kf_ofs < in[j - 1].kf_ofs + in[j - 1].nkf || I.pt_ofs < in[j - 1].pt_ofs + in[j - 1].npt))
            return "the jobs' ranges must ascend and not overlap";
        if (I.cur < -1 || I.cur >= I.nkf) return "cur is not a keyframe of its job's window (or -1)";
        if (I.last < -1 || I.last >= I.nkf) return "last is not a keyframe of its job's window (or -1)";
        if (!I.T_corr || (I.cur < 0 && !I.T_cur) || (I.last < 0 && !I.T_last)) return "null array";
        if (!lf_unit(I.T_corr) || (I.cur < 0 && !lf_unit(I.T_cur)) || (I.last < 0 && !lf_unit(I.T_last)))
            return "a pose's quaternion is not of unit length (1e-6)";
        for (int v = 0; v < I.nkf; ++v)
            if (!lf_unit(poses + 7 * (size_t)(I.kf_ofs + v))) return "a pose's quaternion is not of unit length (1e-6)";
        // row nkf of the table is `cur` outside the window: with cur inside it that row names nothing
        const int top = I.cur < 0 ? I.nkf : I.nkf - 1;
        if (I.npt)
            for (int o = obs_ptr[I.pt_ofs]; o < obs_ptr[I.pt_ofs + I.npt]; ++o)
                if (obs_kf[o] < -1 || obs_kf[o] > top) return "an obs_kf is outside [-1, nkf] (nkf only with cur outside the window)";
    }
    return nullptr;
}

// one buffer: [jobs | pts | table | pt_kf] (read back) [poses | obs_ptr | obs_kf]; all of it is uploaded
static inline LfBuf lf_layout(LfSizes &Z, int njobs, int total_kf, int total_pts, int total_obs, unsigned char *base)
{
    LfBuf B;
    size_t o = 0;
    auto take = [&](size_t bytes) { unsigned char *p = base + o; o += (bytes + 15) & ~(size_t)15; return p; };
    B.jobs = (LfJob *)take(sizeof(LfJob) * (size_t)njobs);
    B.pts = (double *)take(24 * (size_t)total_pts);
    B.corr = (double *)take(56 * ((size_t)total_kf + (size_t)njobs));
    B.pt_kf = (int *)take(4 * (size_t)total_pts);
    Z.result_bytes = o;
    B.poses = (const double *)take(56 * (size_t)total_kf);
    B.obs_ptr = (const int *)take(4 * ((size_t)total_pts + 1));
    B.obs_kf = (const int *)take(4 * (size_t)total_obs);
    Z.bytes = o;
    return B;
}

// the buffer's content before the launch, written through a host view of the same layout
static inline void lf_fill(const LfSizes &Z, const LfBuf &Hb, int njobs, const LfIn *in, int total_kf, const double *poses, int total_pts,
                           const double *pts, const int *obs_ptr, int total_obs, const int *obs_kf)
{
    memset((void *)Hb.jobs, 0, Z.bytes);
    for (int j = 0; j < njobs; ++j) {
        LfJob &J = Hb.jobs[j];
        const LfIn &I = in[j];
        J.kf_ofs = I.kf_ofs; J.nkf = I.nkf; J.pt_ofs = I.pt_ofs; J.npt = I.npt; J.cur = I.cur; J.last = I.last; J.corr_ofs = I.kf_ofs + j;
        memcpy(J.T_corr, I.T_corr, 56);
        if (I.cur < 0) memcpy(J.T_cur, I.T_cur, 56);
        if (I.last < 0) memcpy(J.T_last, I.T_last, 56);
    }
    if (total_kf) memcpy((void *)Hb.poses, poses, 56 * (size_t)total_kf);
    if (total_pts) { memcpy(Hb.pts, pts, 24 * (size_t)total_pts); memcpy((void *)Hb.obs_ptr, obs_ptr, 4 * ((size_t)total_pts + 1)); }
    if (total_obs) memcpy((void *)Hb.obs_kf, obs_kf, 4 * (size_t)total_obs);
}

// the results of job j, from a host view of the buffer after the run: the window's poses (step 4 of the reference writes the active
// keyframes and nothing else, :511-519), its landmarks and their rows, the last frame, the count
static inline void lf_copy_out(const LfBuf &Hb, int j, double *poses, double *pts, int *pt_kf, double *T_last, int *n_unanchored)
{
    const LfJob &J = Hb.jobs[j];
    if (J.nkf) memcpy(poses + 7 * (size_t)J.kf_ofs, Hb.corr + 7 * (size_t)J.corr_ofs, 56 * (size_t)J.nkf);
    if (J.npt) {
        memcpy(pts + 3 * (size_t)J.pt_ofs, Hb.pts + 3 * (size_t)J.pt_ofs, 24 * (size_t)J.npt);
        memcpy(pt_kf + J.pt_ofs, Hb.pt_kf + J.pt_ofs, 4 * (size_t)J.npt);
    }
    memcpy(T_last, J.T_last, 56);
    *n_unanchored = J.n_unanchored;
}

// ---- one job ---------------------------------------------------------------------------------------------------------------------
struct LfShared { int cnt[LF_THREADS]; };

// (T T_cur^-1) T_corr, the reference's association: T_i_c = T_i * T_cur^-1, then T_i_c * T_corr
PG_DEV void lf_corrected(const double *T, const double *Tcur_inv, const double *T_corr, double *out)
{
    double D[7];
    pg_mul(T, Tcur_inv, D);
    pg_mul(D, T_corr, out);
}

PG_DEV void lf_run(const LfBuf &B, LfJob &J, LfShared &S)
{
    const int nkf = J.nkf, npt = J.npt, cur = J.cur;
    const double *poses = B.poses + 7 * (size_t)J.kf_ofs;
    double *corr = B.corr + 7 * (size_t)J.corr_ofs;
    const double *Tcur = cur >= 0 ? poses + 7 * (size_t)cur : J.T_cur;
    LF_PAR {
        double Ci[7];
        pg_inv(Tcur, Ci);
        for (int i = tid; i <= nkf; i += LF_THREADS) {
            double *o = corr + 7 * (size_t)i;
            if (i == nkf || i == cur) { for (int m = 0; m < 7; ++m) o[m] = J.T_corr[m]; }
            else lf_corrected(poses + 7 * (size_t)i, Ci, J.T_corr, o);
        }
        if (tid == 0) {
            double L[7];
            if (J.last >= 0 && J.last == cur) { for (int m = 0; m < 7; ++m) L[m] = J.T_corr[m]; }
            else lf_corrected(J.last >= 0 ? poses + 7 * (size_t)J.last : J.T_last, Ci, J.T_corr, L);
            for (int m = 0; m < 7; ++m) J.T_last[m] = L[m];
        }
    } LF_SYNC
    LF_PAR {
        int un = 0;
        for (int p = tid; p < npt; p += LF_THREADS) {
            const size_t g = (size_t)J.pt_ofs + (size_t)p;
            int k = -1;
            for (int o = B.obs_ptr[g]; o < B.obs_ptr[g + 1]; ++o)
                if (B.obs_kf[o] >= 0) { k = B.obs_kf[o]; break; }
            B.pt_kf[g] = k;
            if (k < 0) { ++un; continue; }
            const double *Tk = k < nkf ? poses + 7 * (size_t)k : Tcur;
            double *x = B.pts + 3 * g, s[3], Ki[7];
            pg_act(Tk, x, s);
            pg_inv(corr + 7 * (size_t)k, Ki);
            pg_act(Ki, s, x);
        }
        S.cnt[tid] = un;
    } LF_SYNC
    LF_PAR {
        if (tid == 0) { int n = 0; for (int t = 0; t < LF_THREADS; ++t) n += S.cnt[t]; J.n_unanchored = n; }
    } LF_SYNC
}

#ifndef PG_HOST_EMU
__global__ void __launch_bounds__(LF_THREADS) k_local_fusion(LfBuf B)
{
    __shared__ LfShared S;
    lf_run(B, B.jobs[blockIdx.x], S);
}
#endif
