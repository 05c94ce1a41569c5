// undistort_driver.cpp -- a stand-alone program around opk_undistort_maps_host and
// opk_camera_parameters_read, built with -fsanitize=address,undefined together with
// host/undistort.cpp (tests/test_undistort.py).
//   undistort_driver maps IN OUT
//     IN:  int32 V, view; double K[V][9]; double dist[V][12]; int32 ncoef[V]; int32 sizes[V][2]
//     OUT: int16 m1[h][w][2]; uint16 m2[h][w]
//   undistort_driver read DIR [SERIAL ...]
//     prints one line per camera: serial, ncoef, has_initial, then the 12 + 9 + ncoef + 12 + 12
//     numbers of extrinsics, intrinsics, distortion, extrinsics_initial, camera_matrix as %.17g
// Exit 0 on success, 1 with "error CODE: TEXT" on a library error, 2 on a usage or file problem.
// Every buffer is a heap block of exactly its size, so a read or write past an end is reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static int fail(int rc)
{
    std::printf("error %d: %s\n", rc, opk::g_error.c_str());
    return 1;
}

static int run_maps(const char* in_path, const char* out_path)
{
    FILE* in = std::fopen(in_path, "rb");
    if (!in) return 2;
    std::vector<int> head(2);
    if (!read_block(in, head)) return 2;
    const int V = head[0], view = head[1];
    if (V < 0 || V > 64) return 2;
    std::vector<double> K((size_t)V * 9), dist((size_t)V * 12);
    std::vector<int> ncoef((size_t)V), sizes((size_t)V * 2);
    if (!read_block(in, K) || !read_block(in, dist) || !read_block(in, ncoef) || !read_block(in, sizes))
        return 2;
    std::fclose(in);
    const opk_cameras cams{V, K.data(), dist.data(), ncoef.data(), sizes.data()};
    size_t w = 0, h = 0;
    if (view >= 0 && view < V && sizes[2 * view] > 0 && sizes[2 * view + 1] > 0) {
        w = (size_t)sizes[2 * view];
        h = (size_t)sizes[2 * view + 1];
        if (w > 4096 || h > 4096) return 2;
    }
    std::vector<int16_t> m1(w * h * 2);
    std::vector<uint16_t> m2(w * h);
    const int rc = opk_undistort_maps_host(&cams, view, m1.data(), m2.data());
    if (rc != OPK_OK) return fail(rc);
    FILE* out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const bool ok = write_block(out, m1) && write_block(out, m2);
    std::fclose(out);
    std::printf("maps ok\n");
    return ok ? 0 : 2;
}

static int run_read(const char* dir, int n, char** serials)
{
    int count = 0;
    std::vector<const char*> names(serials, serials + n);
    const char* const* list = n > 0 ? names.data() : nullptr;
    int rc = opk_camera_parameters_read(dir, list, n, nullptr, 0, &count);
    if (rc != OPK_OK) return fail(rc);
    std::vector<opk_camera_parameters> cams((size_t)count);
    rc = opk_camera_parameters_read(dir, list, n, cams.data(), count, &count);
    if (rc != OPK_OK) return fail(rc);
    for (const opk_camera_parameters& c : cams) {
        std::printf("%s %d %d", c.serial, c.ncoef, c.has_initial);
        for (double v : c.extrinsics) std::printf(" %.17g", v);
        for (double v : c.intrinsics) std::printf(" %.17g", v);
        for (int i = 0; i < c.ncoef; ++i) std::printf(" %.17g", c.distortion[i]);
        for (double v : c.extrinsics_initial) std::printf(" %.17g", v);
        for (double v : c.camera_matrix) std::printf(" %.17g", v);
        std::printf("\n");
    }
    std::printf("read ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "maps") == 0) return run_maps(argv[2], argv[3]);
    if (argc >= 3 && std::strcmp(argv[1], "read") == 0) return run_read(argv[2], argc - 3, argv + 3);
    return 2;
}
