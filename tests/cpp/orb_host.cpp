// orb_host.cpp — a stand-alone program over the host build of csrc/k_orb.h (tests/cpp/orb_host_emu/emu.cpp, included here): the
// kernels' bodies, the plan, the layout and the copy-out on generated images of awkward sizes, with rects inside, across and outside
// the image, one level and eight, both edge limits, tiny and default chunk budgets.  tests/test_host_orb_program.py compiles it with
// -fsanitize=address,undefined and runs it: every read and write of the bodies is then checked against the buffers' bounds.
#include "orb_host_emu/emu.cpp"
#include <cstdio>

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// blocks of two sizes plus a little texture, as tests/orb_cases.py draws them
static void draw(std::vector<uint8_t> &img, int w, int h)
{
    std::vector<int> big((size_t)(w / 32 + 1) * (h / 32 + 1)), small((size_t)(w / 9 + 1) * (h / 9 + 1));
    for (int &v : big) v = (int)(rnd() % 190);
    for (int &v : small) v = (int)(rnd() % 60);
    img.resize((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int v = big[(size_t)(y / 32) * (w / 32 + 1) + x / 32] + small[(size_t)(y / 9) * (w / 9 + 1) + x / 9] + (int)(rnd() % 7) - 3;
            img[(size_t)y * w + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
}

int main()
{
    const int sizes[][2] = { { 300, 230 }, { 161, 121 }, { 63, 63 }, { 97, 53 }, { 70, 71 } };
    long long total = 0;
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], nslots = 3;
        std::vector<uint8_t> imgs, one;
        for (int s = 0; s < nslots; ++s) { draw(one, w, h); imgs.insert(imgs.end(), one.begin(), one.end()); }
        std::vector<float> rects;
        for (int i = 0; i < 24; ++i) { rects.push_back((float)(rnd() % (unsigned)(w + 40)) - 20.f); rects.push_back((float)(rnd() % (unsigned)(h + 40)) - 20.f); }
        rects.push_back(NAN); rects.push_back(5.f);
        for (int edge : { 16, 31 })
            for (int nlevels : { 1, 8 })
                for (int nfeatures : { 1, 40, 500 })
                    for (long long budget : { 1LL, 0LL }) {
                        EmuOrbJob jobs[4] = { { 2, 0, 25, 0, 0, 0 }, { 0, 3, 0, 0, 0, 0 }, { 1, 5, 20, 0, 0, 0 }, { 2, 24, 1, 0, 0, 0 } };
                        OrbParams P{ nfeatures, nlevels, nfeatures == 40 ? 5 : 20, edge };
                        const int max_out = nfeatures == 500 ? 7 : 600;
                        std::vector<OrbKp> out((size_t)4 * max_out);
                        if (emu_orb_detect(w, h, nslots, imgs.data(), 4, jobs, &P, 25, rects.data(), max_out, out.data(), budget) != 0) {
                            std::printf("refused: %s\n", emu_orb_error());
                            return 1;
                        }
                        for (int j = 0; j < 4; ++j) {
                            if (jobs[j].n_out != (jobs[j].n_found < max_out ? jobs[j].n_found : max_out)) { std::printf("counts disagree\n"); return 1; }
                            total += jobs[j].n_found;
                        }
                        std::vector<uint8_t> img((size_t)w * h), mask((size_t)w * h);
                        int lw = 0, lh = 0;
                        if (emu_orb_read_level(3, nlevels - 1, img.data(), mask.data(), &lw, &lh) != 0 || lw > w || lh > h) { std::printf("read_level\n"); return 1; }
                    }
    }
    std::printf("keypoints %lld\norb host ok\n", total);
    return total > 0 ? 0 : 1;
}
