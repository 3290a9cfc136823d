// Host run of k_stereo_bm (csrc/k_stereo_bm.h under BM_HOST_EMU): 256 real threads per workgroup behind a barrier, workgroups one
// after another, LDS a heap block of exactly the plan's lds bytes so that a sanitizer or the allocator sees an overrun.  The window,
// the strip height, the grid and the LDS size are bm_plan's, the fill is bm_fill_one, the two images lie in slots with the stored
// border (csrc/pyr_geom.h).  One job per call; th_force names a strip height the plan would not choose for so small an image.
#include "../hip_on_host.h"
#include <pthread.h>
#include <thread>
#include <vector>
static thread_local Dim3 threadIdx, blockIdx;
static Dim3 blockDim, gridDim;          // k_bm_fill's, which is not run here: the fill below is the loop over bm_fill_one
static unsigned int *emu_lds;
static pthread_barrier_t bar;
static void emu_barrier() { pthread_barrier_wait(&bar); }
#define __syncthreads emu_barrier
// v_alignbyte_b32: bytes sh .. sh + 3 of hi:lo; v_sad_u8: acc + the four absolute byte differences
static inline unsigned int emu_alignbyte(unsigned int hi, unsigned int lo, unsigned int sh) { return (unsigned int)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3))); }
static inline unsigned int emu_sad_u8(unsigned int a, unsigned int b, unsigned int acc) { for (int i = 0; i < 4; ++i) acc += (unsigned)std::abs((int)((a >> (8 * i)) & 255) - (int)((b >> (8 * i)) & 255)); return acc; }
#define BM_HOST_EMU
#include "../../../stereovision-slam_amd/csrc/k_stereo_bm.h"

extern "C" BmPlan emu_bm_plan(int w, int h, int njobs, int nd, int bs) { return bm_plan(w, h, njobs, BmParams{nd, bs, 0, 0, 0}); }
extern "C" long long emu_bm_lds_bytes(int nd, int bs, int th) { return (long long)bm_lds_bytes(nd, bs, th); }

extern "C" int emu_stereo_bm(const uint8_t *left, const uint8_t *right, int w, int h, int nd, int bs, int cap, int tex, int uniq, int th_force, int16_t *out)
{
    const BmParams P{nd, bs, cap, tex, uniq};
    PyrGeom g; memset(&g, 0, sizeof g);
    g.w[0] = w; g.h[0] = h; g.pitch[0] = (w + 2 * SVS_BORDER + 15) & ~15; g.slot_bytes = (size_t)g.pitch[0] * (h + 2 * SVS_BORDER); g.nlevels = 1;
    std::vector<uint8_t> pyr(2 * g.slot_bytes, 0xA5);
    for (int y = 0; y < h; ++y) {
        memcpy(lvl_origin(pyr.data(), g, 0) + (size_t)y * g.pitch[0], left + (size_t)y * w, w);
        memcpy(lvl_origin(pyr.data() + g.slot_bytes, g, 0) + (size_t)y * g.pitch[0], right + (size_t)y * w, w);
    }
    const BmJob job{0, 1};
    BmPlan pl = bm_plan(w, h, 1, P);
    for (size_t i = 0; i < (size_t)w * h; ++i) { out[i] = 12345; bm_fill_one(out, i, w, h, pl.x0, pl.x1, pl.y0, pl.y1); }       // 12345: a pixel the kernel failed to write
    if (!pl.th) return 0;
    if (th_force) { pl.th = th_force; pl.strips = (pl.y1 - pl.y0 + pl.th - 1) / pl.th; pl.lds = bm_lds_bytes(nd, bs, pl.th); }
    pthread_barrier_init(&bar, nullptr, BM_THREADS);
    std::vector<std::thread> ts;
    for (int t = 0; t < BM_THREADS; ++t) ts.emplace_back([&, t]() {
        threadIdx = Dim3{(unsigned)t, 0, 0};
        for (unsigned by = 0; by < (unsigned)pl.strips; ++by) for (unsigned bx = 0; bx < (unsigned)pl.tiles; ++bx) {
            if (t == 0) { emu_lds = (unsigned int *)malloc(pl.lds); memset(emu_lds, 0xA5, pl.lds); }
            emu_barrier();
            blockIdx = Dim3{bx, by, 0};
            switch ((bs + 3) / 4) {
            case 2: k_stereo_bm<2>(&job, pyr.data(), g, P, pl.th, out); break;
            case 3: k_stereo_bm<3>(&job, pyr.data(), g, P, pl.th, out); break;
            case 4: k_stereo_bm<4>(&job, pyr.data(), g, P, pl.th, out); break;
            case 5: k_stereo_bm<5>(&job, pyr.data(), g, P, pl.th, out); break;
            default: k_stereo_bm<6>(&job, pyr.data(), g, P, pl.th, out); break;
            }
            emu_barrier();
            if (t == 0) free(emu_lds);
            emu_barrier();
        }
    });
    for (auto &t : ts) t.join();
    pthread_barrier_destroy(&bar);
    return pl.th;
}
