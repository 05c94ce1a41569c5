// jpeg_driver.cpp -- a stand-alone program around the host side of the JPEG frames:
// opk_jpeg_encode_host and opk_jpeg_bound, built with -fsanitize=address,undefined together with
// host/jpeg.cpp (tests/test_jpeg.py).
//   jpeg_driver sweep          the edge sizes at qualities 1, 50, 75 and 100, two frames with a padded
//                              step and stride; then every capacity 0..bound of a small frame
//   jpeg_driver bad            every refused argument; prints "bad ok"
//   jpeg_driver file W H Q SEED OUT    one frame of the generator below, written to OUT
// Exit 0 on success, 1 with a message on a wrong result, 2 on a usage problem.
// Frames, destination and offsets are heap blocks of exactly their size, so a read or write past
// an end is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "opk.h"

namespace opk {
// the library's error text lives in api.cpp, which this program does without
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace opk

// the test's generator (tests/test_jpeg.py restates it): a 32-bit LCG's high bytes
static void fill(std::vector<uint8_t>& v, unsigned seed)
{
    unsigned s = seed;
    for (auto& b : v) {
        s = s * 1664525u + 1013904223u;
        b = (uint8_t)(s >> 24);
    }
}

static int fail(const char* what, int a = 0, int b = 0, int c = 0)
{
    std::printf("FAILED %s (%d, %d, %d): %s\n", what, a, b, c, opk::g_error.c_str());
    return 1;
}

static bool well_formed(const uint8_t* p, size_t n, int w, int h)
{
    return n >= 627 && p[0] == 0xFF && p[1] == 0xD8 && p[n - 2] == 0xFF && p[n - 1] == 0xD9 &&
           p[163] == (h >> 8) && p[164] == (h & 255) && p[165] == (w >> 8) && p[166] == (w & 255);
}

static int sweep()
{
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 9}, {16, 16}, {17, 23}, {8, 40}, {24, 8}, {7, 64},
                            {34, 18}, {50, 33}, {90, 160}};
    const int qualities[] = {1, 50, 75, 100};
    for (const auto& sz : sizes)
        for (int q : qualities) {
            const int w = sz[0], h = sz[1], n = 2;
            const size_t step = (size_t)w * 3 + 5, frame = step * h + 7;
            // exactly the bytes the encoder may read: the last frame ends with its last pixel
            std::vector<uint8_t> src((n - 1) * frame + step * (h - 1) + (size_t)w * 3);
            fill(src, (unsigned)(w * 131 + h * 7 + q));
            const size_t bound = opk_jpeg_bound(n, w, h);
            std::vector<uint8_t> dst(bound);
            std::vector<uint64_t> off(n + 1);
            if (opk_jpeg_encode_host(dst.data(), bound, off.data(), src.data(), step, frame, n, w,
                                     h, q) != OPK_OK)
                return fail("encode", w, h, q);
            if (off[0] != 0 || off[2] > bound) return fail("offsets", w, h, q);
            for (int f = 0; f < n; ++f)
                if (!well_formed(dst.data() + off[f], off[f + 1] - off[f], w, h))
                    return fail("file", w, h, q);
        }
    // every capacity of a small batch: the frames that fit whole are written, nothing else
    const int w = 9, h = 9, n = 2;
    std::vector<uint8_t> src((size_t)n * w * h * 3);
    fill(src, 99);
    const size_t bound = opk_jpeg_bound(n, w, h);
    std::vector<uint8_t> full(bound);
    std::vector<uint64_t> want(n + 1), off(n + 1);
    if (opk_jpeg_encode_host(full.data(), bound, want.data(), src.data(), 0, 0, n, w, h, 100) != OPK_OK)
        return fail("encode");
    for (size_t cap = 0; cap <= bound; cap += cap < want[n] + 3 ? 1 : 97) {
        std::vector<uint8_t> dst(cap ? cap : 1, 0xA5);   // a block of exactly the capacity
        if (opk_jpeg_encode_host(dst.data(), cap, off.data(), src.data(), 0, 0, n, w, h, 100) != OPK_OK)
            return fail("encode at capacity", (int)cap);
        if (off != want) return fail("offsets at capacity", (int)cap);
        size_t written = 0;
        for (int f = 0; f < n && want[f + 1] <= cap; ++f) written = want[f + 1];
        if (std::memcmp(dst.data(), full.data(), written) != 0) return fail("bytes at capacity", (int)cap);
        for (size_t i = written; i < cap; ++i)
            if (dst[i] != 0xA5) return fail("wrote past the last fitting frame", (int)cap, (int)i);
    }
    std::printf("sweep ok\n");
    return 0;
}

static int bad()
{
    std::vector<uint8_t> src(16 * 16 * 3, 7), dst(opk_jpeg_bound(1, 16, 16), 0xA5);
    uint64_t off[2] = {77, 77};
    auto enc = [&](uint8_t* d, uint64_t* o, const uint8_t* s, size_t step, size_t frame, int n,
                   int w, int h, int q) {
        return opk_jpeg_encode_host(d, dst.size(), o, s, step, frame, n, w, h, q);
    };
    int wrong = 0;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 16, 16, 0) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 16, 16, 101) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 0, 16, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 16, -1, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 65536, 1, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, 1, 1, 65536, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 0, -1, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 47, 0, 1, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, src.data(), 0, 100, 2, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(nullptr, off, src.data(), 0, 0, 1, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), nullptr, src.data(), 0, 0, 1, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(dst.data(), off, nullptr, 0, 0, 1, 16, 16, 100) != OPK_ERR_ARG;
    wrong += enc(src.data(), off, src.data(), 0, 0, 1, 16, 16, 100) != OPK_ERR_ARG;   // overlap
    if (wrong) return fail("a bad argument was accepted", wrong);
    if (off[0] != 77 || off[1] != 77) return fail("a refused call wrote offsets");
    for (uint8_t b : dst)
        if (b != 0xA5) return fail("a refused call wrote bytes");
    if (enc(nullptr, off, nullptr, 0, 0, 0, 16, 16, 100) != OPK_OK || off[0] != 0)
        return fail("n == 0");
    if (enc(nullptr, nullptr, nullptr, 0, 0, 0, 16, 16, 100) != OPK_OK) return fail("n == 0, no offsets");
    if (opk_jpeg_bound(0, 16, 16) != 0 || opk_jpeg_bound(1, 0, 16) != 0 || opk_jpeg_bound(-1, 1, 1) != 0)
        return fail("bound of nothing");
    if (opk_jpeg_bound(3, 65535, 65535) / 3 != opk_jpeg_bound(1, 65535, 65535)) return fail("bound");
    std::printf("bad ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !std::strcmp(argv[1], "bad")) return bad();
    if (argc == 7 && !std::strcmp(argv[1], "file")) {
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), q = std::atoi(argv[4]);
        if (w < 1 || h < 1 || w > 4096 || h > 4096) return 2;
        std::vector<uint8_t> src((size_t)w * h * 3);
        fill(src, (unsigned)std::atoi(argv[5]));
        std::vector<uint8_t> dst(opk_jpeg_bound(1, w, h));
        uint64_t off[2];
        if (opk_jpeg_encode_host(dst.data(), dst.size(), off, src.data(), 0, 0, 1, w, h, q) != OPK_OK)
            return fail("encode", w, h, q);
        FILE* f = std::fopen(argv[6], "wb");
        if (!f) return 2;
        std::fwrite(dst.data(), 1, off[1], f);
        std::fclose(f);
        return 0;
    }
    std::fprintf(stderr, "usage: jpeg_driver sweep | bad | file W H Q SEED OUT\n");
    return 2;
}
