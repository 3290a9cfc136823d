// Host run of k_stereo_bm (a copy of csrc/k_stereo_bm.h cut before the cloud, see tests/test_host_emulation_stereo_bm.py): 256 real
// threads per workgroup behind a barrier, workgroups one after another, LDS a heap block of exactly bm_lds_bytes() so that a sanitizer
// or the allocator sees an overrun, the fill and the dispatch on ceil(bs / 4) restated from launch_stereo_bm.  One job per call.
#include "k_stereo_bm.h"
#include <pthread.h>
#include <thread>
#include <vector>
#include <cstring>
thread_local Dim3 threadIdx, blockIdx;
Dim3 blockDim, gridDim;
unsigned int *g_lds;
static pthread_barrier_t bar;
void emu_barrier() { pthread_barrier_wait(&bar); }
static int cdiv(int a, int b) { return (a + b - 1) / b; }
extern "C" int emu_stereo_bm(const uint8_t *left, const uint8_t *right, int w, int h, int nd, int bs, int cap, int tex, int uniq, int th_force, int16_t *out)
{
    BmParams P{nd, bs, cap, tex, uniq};
    PyrGeom g; memset(&g, 0, sizeof g); g.w[0] = w; g.h[0] = h; g.pitch[0] = w; g.slot_bytes = (size_t)w * h; g.nlevels = 1;
    std::vector<uint8_t> pyr((size_t)2 * w * h); memcpy(pyr.data(), left, (size_t)w * h); memcpy(pyr.data() + (size_t)w * h, right, (size_t)w * h);
    BmJob job{0, 1};
    const int r = bs / 2, x0 = nd - 1 + r, x1 = w - r, y0 = r, y1 = h - r;
    const bool none = x0 >= x1 || h < 2 * r + 1;
    for (int i = 0; i < w * h; ++i) { int y = i / w, x = i % w; out[i] = (none || !(x >= x0 && x < x1 && y >= y0 && y < y1)) ? BM_FILTERED : 12345; }   // 12345: a pixel the kernel failed to write
    if (none) return 0;
    int th = 16; const int tiles = cdiv(x1 - x0, BM_TW);
    while (th > 4 && (long long)tiles * cdiv(y1 - y0, th) < 1024) th >>= 1;
    if (th_force) th = th_force;
    gridDim = Dim3{(unsigned)tiles, (unsigned)cdiv(y1 - y0, th), 1}; blockDim = Dim3{BM_THREADS, 1, 1};
    const size_t lds = bm_lds_bytes(nd, bs, th);
    pthread_barrier_init(&bar, nullptr, BM_THREADS);
    std::vector<std::thread> ts;
    unsigned int **ldsp = &g_lds;
    for (int t = 0; t < BM_THREADS; ++t) ts.emplace_back([&, t]() {
        threadIdx = Dim3{(unsigned)t, 0, 0};
        for (unsigned by = 0; by < gridDim.y; ++by) for (unsigned bx = 0; bx < gridDim.x; ++bx) {
            if (t == 0) { *ldsp = (unsigned int *)malloc(lds); memset(*ldsp, 0xA5, lds); }
            emu_barrier();
            blockIdx = Dim3{bx, by, 0};
            int nww = (bs + 3) / 4;
            switch (nww) {
            case 2: k_stereo_bm<2>(&job, pyr.data(), g, P, th, out); break;
            case 3: k_stereo_bm<3>(&job, pyr.data(), g, P, th, out); break;
            case 4: k_stereo_bm<4>(&job, pyr.data(), g, P, th, out); break;
            case 5: k_stereo_bm<5>(&job, pyr.data(), g, P, th, out); break;
            default: k_stereo_bm<6>(&job, pyr.data(), g, P, th, out); break;
            }
            emu_barrier();
            if (t == 0) free(*ldsp);
            emu_barrier();
        }
    });
    for (auto &t : ts) t.join();
    pthread_barrier_destroy(&bar);
    return th;
}
