// csrc/k_loop_verify.h compiled for the host (tests/test_host_emulation_loop_verify.py): with LV_HOST_EMU the HIP qualifiers vanish and
// a phase of the kernel becomes a loop over its 128 thread numbers (the phases end at the kernel's barriers and no thread reads what
// another thread writes inside a phase, so running the threads one after the other is the same computation).  The checks, the buffer
// layout, the staging and the kernel body are the library's own code; only the launch and the copies are restated here.
#define LV_HOST_EMU
#include "../../../stereovision-slam_amd/csrc/k_loop_verify.h"
#include <string>

struct EmuLoopJob {
    int c_ofs, nc, q_ofs, nq;
    double T_cur[7], T_cand[7];
    int status, n_matches, n_points, n_inliers, need_correction, reserved;
    double T_corr[7], T_rel[7], d;
};
struct EmuLoopParams {
    double cam[4], ext_l[7];
    int min_matches, ransac_iters;
    double reproj_px, max_pose_distance, min_pose_difference, max_pose_difference;
    unsigned seed; int reserved;
};
static std::string g_lv_err;

extern "C" const char *emu_lv_error() { return g_lv_err.c_str(); }

// pieces of a hypothesis on their own, each compared with the reference's function of the same name
extern "C" int emu_lv_draw4(unsigned seed, int i, int np, int *idx) { return lv_draw4(seed, i, np, idx) ? 1 : 0; }
extern "C" void emu_lv_R_to_T(const double *Rt, double *T) { lv_R_to_T(Rt, T); }
extern "C" int emu_lv_p3p(const double *X, const double *f, double *out) { return lv_p3p(X, f, out); }

extern "C" int emu_loop_verify(int njobs, EmuLoopJob *jobs, const EmuLoopParams *prm, int total_c, const uint8_t *desc_c, const double *xyz_c,
                               const uint8_t *has_xyz, int total_q, const uint8_t *desc_q, const float *uv_q, int *match_c, int *match_q,
                               int *match_dist, uint8_t *match_inlier)
{
    std::vector<LvIn> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = LvIn{ jobs[j].c_ofs, jobs[j].nc, jobs[j].q_ofs, jobs[j].nq, jobs[j].T_cur, jobs[j].T_cand };
    const char *why = lv_check(njobs, in.data(), total_c, total_q, prm->ext_l, prm->ransac_iters, prm->min_matches, prm->reproj_px);
    if (why) { g_lv_err = why; return -1; }
    LvParams P;
    memset(&P, 0, sizeof(P));
    memcpy(P.cam, prm->cam, 32); memcpy(P.ext_l, prm->ext_l, 56);
    P.reproj2 = prm->reproj_px * prm->reproj_px; P.max_pose_distance = prm->max_pose_distance;
    P.min_pose_difference = prm->min_pose_difference; P.max_pose_difference = prm->max_pose_difference;
    P.min_matches = prm->min_matches; P.ransac_iters = prm->ransac_iters; P.seed = prm->seed;
    LvSizes Z;
    (void)lv_layout(Z, njobs, total_c, total_q, nullptr);
    std::vector<double> mem(Z.bytes / 8 + 2);
    const LvBuf B = lv_layout(Z, njobs, total_c, total_q, (unsigned char *)mem.data());
    lv_fill(Z, B, njobs, in.data(), total_c, desc_c, xyz_c, has_xyz, total_q, desc_q, uv_q);
    std::vector<LvShared> S(1);
    for (int j = 0; j < njobs; ++j) {
        memset(&S[0], 0xA5, sizeof(LvShared));              // a job must not rely on what the one before it left in LDS
        lv_run(B, P, B.jobs[j], S[0]);
        const LvJob &J = B.jobs[j];
        jobs[j].status = J.status; jobs[j].n_matches = J.n_matches; jobs[j].n_points = J.n_points; jobs[j].n_inliers = J.n_inliers;
        jobs[j].need_correction = J.need_correction;
        memcpy(jobs[j].T_corr, J.T_corr, 56); memcpy(jobs[j].T_rel, J.T_rel, 56); jobs[j].d = J.d;
    }
    if (total_c) {
        memcpy(match_c, B.m_c, 4 * (size_t)total_c); memcpy(match_q, B.m_q, 4 * (size_t)total_c); memcpy(match_dist, B.m_d, 4 * (size_t)total_c);
        memcpy(match_inlier, B.m_inl, (size_t)total_c);
    }
    return 0;
}
