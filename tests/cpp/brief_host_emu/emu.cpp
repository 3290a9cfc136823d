// csrc/k_brief.h compiled for the host (tests/test_host_emulation_brief.py): with BR_HOST_EMU the HIP qualifiers vanish and a phase of a
// kernel becomes a loop over its 256 thread numbers (the phases end at the kernel's barriers and no thread reads what another thread
// writes inside a phase, so running the threads one after the other is the same computation).  The checks, the offsets, the buffer
// layout, the staging, the copy-out and both kernel bodies are the library's own code; only the launches and the copies are restated
// here.  The images are tight: slot s is imgs + s * w * h.
#define BR_HOST_EMU
#include "../../../stereovision-slam_amd/csrc/k_brief.h"
#include <string>

struct EmuBriefJob { int slot, pt_ofs, npts, n_desc, reserved; };
struct EmuBriefParams { const int8_t *pattern; float angle_deg; int edge; };
static std::string g_br_err;

extern "C" const char *emu_brief_error() { return g_br_err.c_str(); }

extern "C" void emu_brief_default_pattern(int8_t *out) { memcpy(out, BR_DEFAULT_PATTERN, sizeof(BR_DEFAULT_PATTERN)); }

extern "C" int emu_brief_describe(int w, int h, int nslots, const uint8_t *imgs, int njobs, EmuBriefJob *jobs, const EmuBriefParams *prm,
                                  int total_pts, const float *xy, uint8_t *desc, int *desc_pt)
{
    std::vector<BrJob> in((size_t)njobs);
    for (int j = 0; j < njobs; ++j) in[(size_t)j] = BrJob{ jobs[j].slot, jobs[j].pt_ofs, jobs[j].npts, 0 };
    int off[1024], reach = 0;
    const char *why = br_check(njobs, in.data(), total_pts, nslots, prm->pattern ? prm->pattern : BR_DEFAULT_PATTERN, prm->angle_deg,
                               prm->edge, off, &reach);
    if (why) { g_br_err = why; return -1; }
    if (njobs == 0) return 0;
    const BrPlan L = br_plan(reach);
    BrSizes Z;
    (void)br_layout(Z, njobs, total_pts, nullptr);
    std::vector<double> mem(Z.bytes / 8 + 2);
    memset(mem.data(), 0xA5, mem.size() * 8);                  // what the device buffer holds before a call is not specified
    const BrBuf B = br_layout(Z, njobs, total_pts, (unsigned char *)mem.data());
    br_fill(B, L, njobs, in.data(), total_pts, xy, off);
    BrImg I;
    I.base = imgs; I.slot_bytes = (size_t)w * h; I.origin = 0; I.pitch = w; I.w = w; I.h = h;
    std::vector<int> cnt(BR_THREADS);
    for (int j = 0; j < njobs; ++j) {
        for (int &v : cnt) v = (int)0xA5A5A5A5;                 // a job must not rely on what the one before it left in LDS
        br_filter_run(B, I, prm->edge, L.R, B.jobs[j], cnt.data());
    }
    std::vector<double> smem(((size_t)L.wave_bytes * BR_ROWS_PER_WG) / 8 + 2);
    for (int wg = 0; wg < (total_pts + BR_ROWS_PER_WG - 1) / BR_ROWS_PER_WG; ++wg) {
        memset(smem.data(), 0xA5, smem.size() * 8);
        br_describe_run(B, I, L, total_pts, wg, (unsigned char *)smem.data());
    }
    br_copy_out(B, njobs, in.data(), desc, desc_pt);
    for (int j = 0; j < njobs; ++j) jobs[j].n_desc = in[(size_t)j].n_desc;
    return 0;
}
