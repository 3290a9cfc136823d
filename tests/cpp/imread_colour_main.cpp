// imread_colour_main.cpp — stand-alone driver of facade::imread (host/slam_facade.h) for tests/test_imread_colour.py: no GPU, no
// library of the project; built plain and with the host sanitizers.
//   imread_colour_main dump <flags> <file> <out>       the image as "cols rows channels\n" on stdout, its bytes into <out>
//   imread_colour_main fuzz <flags> <file> <tmp>       every truncation of <file> at a stride of 7 bytes ("t <length> ...") and each of
//                                                      its first 40 bytes flipped ("f <index> ..."), written to <tmp> and read:
//                                                      one line "<kind> <n> <cols> <rows> <channels> <bytes>" each
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "../../include/svslam.h"
#include "../../stereovision-slam_amd/host/slam_facade.h"

using svs::facade::Image;
using svs::facade::imread;

static bool write_file(const std::string &path, const std::vector<uint8_t> &b, size_t n)
{
    std::ofstream o(path, std::ios::binary | std::ios::trunc);
    o.write(reinterpret_cast<const char *>(b.data()), (std::streamsize)n);
    return (bool)o;
}

int main(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: imread_colour_main dump|fuzz <flags> <file> <out>\n"); return 2; }
    const std::string mode = argv[1];
    const int flags = std::atoi(argv[2]);
    if (mode == "dump") {
        const Image img = imread(argv[3], flags);
        std::printf("%d %d %d\n", img.cols, img.rows, img.empty() ? 0 : img.channels);
        std::vector<uint8_t> d = img.data;
        return write_file(argv[4], d, d.size()) ? 0 : 1;
    }
    if (mode != "fuzz") return 2;
    std::ifstream in(argv[3], std::ios::binary);
    if (!in) return 1;
    const std::vector<uint8_t> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    auto report = [&](char kind, size_t n) {
        const Image img = imread(argv[4], flags);
        std::printf("%c %zu %d %d %d %zu\n", kind, n, img.empty() ? 0 : img.cols, img.empty() ? 0 : img.rows, img.empty() ? 0 : img.channels, img.data.size());
    };
    for (size_t n = 0; n < f.size(); n += 7) {
        if (!write_file(argv[4], f, n)) return 1;
        report('t', n);
    }
    for (size_t i = 0; i < 40 && i < f.size(); ++i) {
        std::vector<uint8_t> g = f;
        g[i] = (uint8_t)~g[i];
        if (!write_file(argv[4], g, g.size())) return 1;
        report('f', i);
    }
    return 0;
}
