// orb_desc_host.cpp — a stand-alone program over the host build of csrc/k_orb_desc.h (tests/cpp/orb_desc_host_emu/emu.cpp, included
// here): the kernels' bodies, the plan, the layout and the copy-out on generated images of awkward sizes, with keypoints on every level,
// on and around both borders, outside the image and not finite, the default table and one of reach 22, tiny and default chunk budgets.
// tests/test_host_orb_desc_program.py compiles it with -fsanitize=address,undefined and runs it: every read and write of the bodies is
// then checked against the buffers' bounds.
#include "orb_desc_host_emu/emu.cpp"
#include <cstdio>

static uint32_t g_seed = 4711u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

int main()
{
    const int sizes[][2] = { { 300, 240 }, { 161, 121 }, { 63, 63 }, { 97, 53 }, { 620, 188 }, { 70, 71 } };
    int8_t wide[1024];
    memcpy(wide, BR_DEFAULT_PATTERN, 1024);
    wide[0] = 15; wide[1] = 15; wide[2] = -15; wide[3] = 15;               // reach 22
    long long total = 0;
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], nslots = 3;
        std::vector<uint8_t> imgs((size_t)nslots * w * h);
        for (uint8_t &v : imgs) v = (uint8_t)(rnd() & 255u);
        for (int table = 0; table < 2; ++table) {
            const int edge = table ? 26 : 31;
            // points of four jobs with a gap: random positions around the whole image, every octave, border values on each level
            std::vector<OrbKp> kps;
            auto add = [&](float x, float y, float angle, int octave) { kps.push_back(OrbKp{ x, y, 31.f, angle, 0.f, octave }); };
            for (int i = 0; i < 300; ++i)
                add((float)(rnd() % (unsigned)(w + 20)) - 10.f + 0.25f * (float)(rnd() % 4u), (float)(rnd() % (unsigned)(h + 20)) - 10.f, (float)(rnd() % 36000u) * 0.01f,
                    (int)(rnd() % 8u));
            for (int l = 0; l < 8; ++l) {
                float scale; int lw, lh;
                orb_level_size(w, h, l, &scale, &lw, &lh);
                const int xs[4] = { edge - 1, edge, lw - edge - 1, lw - edge }, ys[4] = { edge - 1, edge, lh - edge - 1, lh - edge };
                for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) add((float)xs[a] * scale, (float)ys[b] * scale, 45.f * (float)(a + b), l);
            }
            add((float)edge - 0.01f, (float)edge, -1.f, 0); add((float)(w - edge) - 0.01f, (float)(h - edge) - 0.01f, -1.f, 0);
            add(NAN, 40.f, 1.f, 0); add(40.f, INFINITY, 1.f, 3); add(-INFINITY, -INFINITY, 1.f, 7); add(1e30f, 1e30f, 359.99f, 7);
            const int n = (int)kps.size();
            for (long long budget : { 1LL, 300000LL, 0LL }) {
                EmuOdJob jobs[5] = { { 2, 0, 150, 0, 0 }, { 0, 150, 0, 0, 0 }, { 1, 152, 148, 0, 0 }, { 2, 300, n - 300, 0, 0 }, { 0, n, 0, 0, 0 } };
                OdParams P{ table ? wide : nullptr, table ? edge : 0, 0, 0 };
                std::vector<uint8_t> desc((size_t)32 * n);
                std::vector<int> dpt((size_t)n);
                if (emu_orb_desc_describe(w, h, nslots, imgs.data(), 5, jobs, &P, n, kps.data(), desc.data(), dpt.data(), budget) != 0) {
                    std::printf("refused: %s\n", emu_orb_desc_error());
                    return 1;
                }
                for (int j = 0; j < 5; ++j) {
                    if (jobs[j].n_desc < 0 || jobs[j].n_desc > jobs[j].npts) { std::printf("n_desc out of range\n"); return 1; }
                    for (int r = 0; r < jobs[j].n_desc; ++r)
                        if (dpt[(size_t)jobs[j].pt_ofs + r] < 0 || dpt[(size_t)jobs[j].pt_ofs + r] >= jobs[j].npts) { std::printf("desc_pt out of range\n"); return 1; }
                    total += jobs[j].n_desc;
                }
            }
            // all octave 0: no level storage; one point; a refusal
            for (OrbKp &k : kps) k.octave = 0;
            EmuOdJob one[1] = { { 1, 7, 1, 0, 0 } };
            OdParams P{ nullptr, 0, 1, 0 };
            std::vector<uint8_t> desc((size_t)32 * n);
            std::vector<int> dpt((size_t)n);
            if (emu_orb_desc_describe(w, h, nslots, imgs.data(), 1, one, &P, n, kps.data(), desc.data(), dpt.data(), 0) != 0) { std::printf("refused: %s\n", emu_orb_desc_error()); return 1; }
            long long st[4];
            emu_orb_desc_stats(st);
            if (st[1] != 0 || st[2] != 0) { std::printf("levels built for octave 0\n"); return 1; }
            kps[7].octave = 1;
            if (emu_orb_desc_describe(w, h, nslots, imgs.data(), 1, one, &P, n, kps.data(), desc.data(), dpt.data(), 0) == 0) { std::printf("octave 1 of 1 level accepted\n"); return 1; }
        }
    }
    std::printf("rows %lld\norb desc host ok\n", total);
    return total > 0 ? 0 : 1;
}
