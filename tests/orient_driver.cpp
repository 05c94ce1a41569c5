// orient_driver.cpp -- a stand-alone program around the host side of the rotated and flipped
// frames: opk_orient_size, opk_orient_keypoints and the argument checks of opk_orient_frames that
// need no device (make_orientation, the descriptor resolver, check_orient), built with
// -fsanitize=address,undefined together with host/orient.cpp (tests/test_orient.py).
//   orient_driver size W H ROTATE              prints "OW OH"
//   orient_driver keypoints PEOPLE PARTS W H ROTATE FLIP INVERSE
//     the array is x = 10 i + 1, y = 10 i + 2, score = i % 3 for point i; prints every value
//   orient_driver check FORMAT N W H DW DH ROTATE FLIP
//     descriptors of tight frames over fake addresses (nothing is dereferenced); prints "check ok"
// Exit 0 on success, 1 with "error CODE: TEXT" on a library error, 2 on a usage problem.
// The keypoints are a heap block of exactly their size, so a read or write past an end is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "opk.h"
#include "../openpose_amd/csrc/host/orient.h"

namespace opk {
// the library's error text lives in api.cpp, which this program does without
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace opk

static int fail(int rc)
{
    std::printf("error %d: %s\n", rc, opk::g_error.c_str());
    return 1;
}

static int run_check(char** a)
{
    const int format = std::atoi(a[0]), n = std::atoi(a[1]), w = std::atoi(a[2]), h = std::atoi(a[3]);
    const int dw = std::atoi(a[4]), dh = std::atoi(a[5]), rotate = std::atoi(a[6]), flip = std::atoi(a[7]);
    opk_frames s{};
    opk_frames_out d{};
    s.format = d.format = format;
    s.n = d.n = n;
    s.width = w;
    s.height = h;
    d.width = dw;
    d.height = dh;
    for (int i = 0; i < 3; ++i) {
        s.plane[i] = reinterpret_cast<const uint8_t*>((uintptr_t)0x10000000 * (unsigned)(i + 1));
        d.plane[i] = reinterpret_cast<uint8_t*>((uintptr_t)0x10000000 * (unsigned)(i + 5));
    }
    try {
        const opk::Orientation o = opk::make_orientation(rotate, flip);
        opk::check_orient(opk::frame_dest(d), opk::frame_source(s), o);
    } catch (const opk::Error& e) {
        opk::set_error(e.what());
        return fail(e.code);
    }
    std::printf("check ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 5 && std::strcmp(argv[1], "size") == 0) {
        int ow = -1, oh = -1;
        const int rc = opk_orient_size(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), &ow, &oh);
        if (rc != OPK_OK) return fail(rc);
        std::printf("%d %d\n", ow, oh);
        return 0;
    }
    if (argc == 9 && std::strcmp(argv[1], "keypoints") == 0) {
        const int people = std::atoi(argv[2]), parts = std::atoi(argv[3]);
        const size_t count = people > 0 && parts > 0 ? (size_t)people * (size_t)parts : 0;
        if (count > 1000000) return 2;
        std::vector<float> kp(count * 3);
        for (size_t i = 0; i < count; ++i) {
            kp[3 * i] = (float)(10 * i + 1);
            kp[3 * i + 1] = (float)(10 * i + 2);
            kp[3 * i + 2] = (float)(i % 3);
        }
        const int rc = opk_orient_keypoints(count ? kp.data() : nullptr, people, parts, std::atoi(argv[4]),
                                            std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]),
                                            std::atoi(argv[8]));
        if (rc != OPK_OK) return fail(rc);
        for (float v : kp) std::printf("%.9g ", v);
        std::printf("\nkeypoints ok\n");
        return 0;
    }
    if (argc == 10 && std::strcmp(argv[1], "check") == 0) return run_check(argv + 2);
    return 2;
}
