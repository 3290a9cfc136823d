// csrc/k_orb_desc.h compiled for the host (tests/test_host_emulation_orb_desc.py): with OD_HOST_EMU the HIP qualifiers of it and of the
// two headers it shares code with (k_brief.h, k_orb.h) vanish and a phase of a kernel becomes a loop over its 256 thread numbers (the
// phases end at the kernel's barriers and no thread reads what another thread writes inside a phase).  The plan with its refusals, the
// buffer layout, the staging, the copy-out and every kernel body are the library's own code; only the launches and the copies are
// restated here, in the order api_orb_desc.h enqueues them.  The images are tight: slot s is imgs + s * w * h.
#define OD_HOST_EMU
#include "../../../stereovision-slam_amd/csrc/k_orb_desc.h"
#include <string>

struct EmuOdJob { int slot, pt_ofs, npts, n_desc, reserved; };
static std::string g_od_err;
static long long g_stats[4];       // of the last call: chunks, resize launches, bytes of level storage reserved, the table's reach

extern "C" const char *emu_orb_desc_error() { return g_od_err.c_str(); }
extern "C" void emu_orb_desc_stats(long long *out) { for (int i = 0; i < 4; ++i) out[i] = g_stats[i]; }
extern "C" void emu_orb_desc_rotation(float angle_deg, float *ab) { od_rotation(angle_deg, ab, ab + 1); }

extern "C" int emu_orb_desc_describe(int w, int h, int nslots, const uint8_t *imgs, int njobs, EmuOdJob *jobs, const OdParams *prm,
                                     int total_pts, const OrbKp *kps, uint8_t *desc, int *desc_pt, long long budget)
{
    std::vector<OdJob> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = OdJob{ jobs[j].slot, jobs[j].pt_ofs, jobs[j].npts, 0 };
    OdPlan P;
    const char *why = od_plan(P, w, h, nslots, njobs, in.data(), prm, total_pts, kps, budget > 0 ? (size_t)budget : ORB_BUDGET_DEFAULT);
    if (why) { g_od_err = why; return -1; }
    g_stats[0] = (long long)P.chunks.size(); g_stats[1] = 0; g_stats[2] = 0; g_stats[3] = P.G.reach;
    if (njobs == 0) return 0;
    OrbImg I;
    I.base = imgs; I.slot_bytes = (size_t)w * h; I.origin = 0; I.pitch = w; I.w = w; I.h = h;
    std::vector<int> cnt(BR_THREADS);
    std::vector<double> smem(((size_t)P.lds.wave_bytes * BR_ROWS_PER_WG) / 8 + 2);
    std::vector<double> mem;
    for (OdChunk &C : P.chunks) {
        (void)od_layout(P, C, nullptr);
        mem.assign(C.bytes / 8 + 2, 0.0);
        memset(mem.data(), 0xA5, mem.size() * 8);                  // what the device buffer holds before a call is not specified
        const OdBuf B = od_layout(P, C, (unsigned char *)mem.data());
        od_fill(P, C, B, in.data(), kps);
        const OdGeom &G = *B.geom;                                 // as the kernels get it
        g_stats[2] = std::max(g_stats[2], (long long)(G.job_bytes * (size_t)C.n));
        for (int l = 1; l <= G.lmax; ++l) {
            const int nt = ((G.L[l].w * G.L[l].h + 3) / 4 + BR_THREADS - 1) / BR_THREADS * BR_THREADS;
            for (int j = 0; j < C.n; ++j) for (int t = 0; t < nt; ++t) od_resize_task(G, I, B, l, j, t);
            ++g_stats[1];
        }
        for (int j = 0; j < C.n; ++j) {
            for (int &v : cnt) v = (int)0xA5A5A5A5;                 // a job must not rely on what the one before it left in LDS
            od_filter_run(G, B, j, cnt.data());
        }
        for (int wg = 0; wg < (C.npts + BR_ROWS_PER_WG - 1) / BR_ROWS_PER_WG; ++wg) {
            memset(smem.data(), 0xA5, smem.size() * 8);
            od_describe_run(G, I, B, P.lds, wg, (unsigned char *)smem.data());
        }
        od_copy_out(C, B, in.data(), desc, desc_pt);
    }
    for (int j = 0; j < njobs; ++j) jobs[j].n_desc = in[(size_t)j].n_desc;
    return 0;
}
