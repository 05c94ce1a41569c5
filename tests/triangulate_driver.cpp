// triangulate_driver.cpp -- a stand-alone program around opk_triangulate_host, built with
// -fsanitize=address,undefined together with host/triangulate.cpp (tests/test_triangulate.py).
// Reads one case from a binary file, writes the results to another:
//   in:  int32 V, min_views, steps, parts; double P[V][12]; int32 sizes[V][2];
//        float kp[steps][V][parts][3]; int32 present[steps][V]
//   out: float xyz[steps][parts][4]; int32 status[steps]; double errors[steps][parts];
//        int32 dropped[steps][parts]
// Every buffer is a heap block of exactly its size, so a read or write past an end is reported.
#include <cstdio>
#include <string>
#include <vector>

#include "opk.h"

namespace opk {
// the library's error text lives in api.cpp, which this program does without
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}  // namespace opk

template <class T>
static bool read_block(FILE* f, std::vector<T>& v)
{
    return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T>
static bool write_block(FILE* f, const std::vector<T>& v)
{
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int> head(4);
    if (!read_block(in, head)) return 2;
    const int V = head[0], min_views = head[1], steps = head[2], parts = head[3];
    if (V < 0 || V > 64 || steps < 0 || steps > 1024 || parts < 1 || parts > 1024) return 2;
    std::vector<double> P((size_t)V * 12);
    std::vector<int> sizes((size_t)V * 2);
    std::vector<float> kp((size_t)steps * V * parts * 3);
    std::vector<int> present((size_t)steps * V);
    if (!read_block(in, P) || !read_block(in, sizes) || !read_block(in, kp) ||
        !read_block(in, present))
        return 2;
    std::fclose(in);
    std::vector<float> xyz((size_t)steps * parts * 4);
    std::vector<int> status((size_t)steps), dropped((size_t)steps * parts);
    std::vector<double> errors((size_t)steps * parts);
    const opk_rig rig{V, P.data(), sizes.data(), min_views};
    const int rc = opk_triangulate_host(&rig, steps, parts, kp.data(), present.data(), xyz.data(),
                                        status.data(), errors.data(), dropped.data());
    if (rc != OPK_OK) {
        std::printf("error %d: %s\n", rc, opk::g_error.c_str());
        return 1;
    }
    // and once without the optional outputs
    std::vector<float> xyz2(xyz.size());
    std::vector<int> status2(status.size());
    if (opk_triangulate_host(&rig, steps, parts, kp.data(), present.data(), xyz2.data(),
                             status2.data(), nullptr, nullptr) != OPK_OK || xyz2 != xyz ||
        status2 != status)
        return 3;
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = write_block(out, xyz) && write_block(out, status) && write_block(out, errors) &&
                    write_block(out, dropped);
    std::fclose(out);
    std::printf("triangulate ok\n");
    return ok ? 0 : 2;
}
