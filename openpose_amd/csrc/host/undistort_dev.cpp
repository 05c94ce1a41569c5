// undistort_dev.cpp -- the device route of the undistortion (include/opk.h): the context's cache of
// uploaded maps, the per-camera launches of kernels/undistort.hip, and opk_undistort_frames.
#include <cstring>

#include "../../../include/opk.h"
#include "../common.h"
#include "context.h"
#include "frames.h"
#include "input.h"
#include "undistort.h"

namespace opk {

const Context::UndistortDev& Context::undistort_dev(const UndistortCameras& cams)
{
    const std::string key = cams.key();
    auto it = undistort_maps.find(key);
    if (it != undistort_maps.end()) return *it->second;
    const int V = cams.views();
    auto pad16 = [](size_t b) { return (b + 15) / 16 * 16; };
    // views with equal parameters share one pair of maps (the reference's rig: camera 0's for all)
    std::vector<int> same((size_t)V);
    std::vector<size_t> m1_at((size_t)V), m2_at((size_t)V);
    size_t bytes = 0;
    for (int v = 0; v < V; ++v) {
        same[(size_t)v] = v;
        for (int u = 0; u < v; ++u)
            if (std::memcmp(&cams.cam[(size_t)u], &cams.cam[(size_t)v], sizeof(UndistortCamera)) == 0) {
                same[(size_t)v] = u;
                break;
            }
        if (same[(size_t)v] != v) continue;
        const UndistortCamera& c = cams.cam[(size_t)v];
        const size_t pitch = ((size_t)c.w + 3) / 4 * 4;
        m1_at[(size_t)v] = bytes;
        bytes = pad16(bytes + (size_t)c.h * pitch * 2 * sizeof(int16_t));
        m2_at[(size_t)v] = bytes;
        bytes = pad16(bytes + (size_t)c.h * pitch * sizeof(uint16_t));
    }
    std::vector<uint8_t> host(bytes, 0);   // (the rows' padding entries are zeros, never stored from)
    for (int v = 0; v < V; ++v) {
        if (same[(size_t)v] != v) continue;
        const UndistortCamera& c = cams.cam[(size_t)v];
        const size_t pitch = ((size_t)c.w + 3) / 4 * 4;
        undistort_map(c, reinterpret_cast<int16_t*>(host.data() + m1_at[(size_t)v]), pitch,
                      reinterpret_cast<uint16_t*>(host.data() + m2_at[(size_t)v]), pitch);
    }
    auto t = std::make_unique<UndistortDev>();
    uint8_t* dev = static_cast<uint8_t*>(t->buf.get(bytes));
    OPK_HIP(hipMemcpyAsync(dev, host.data(), bytes, hipMemcpyHostToDevice, stream));
    OPK_HIP(hipStreamSynchronize(stream));
    t->view.resize((size_t)V);
    for (int v = 0; v < V; ++v) {
        const int u = same[(size_t)v];
        t->view[(size_t)v] = UndistortMap{reinterpret_cast<const short2*>(dev + m1_at[(size_t)u]),
                                          reinterpret_cast<const uint16_t*>(dev + m2_at[(size_t)u]),
                                          (int)(((size_t)cams.cam[(size_t)u].w + 3) / 4 * 4)};
    }
    auto& ref = *t;
    undistort_maps.emplace(key, std::move(t));
    return ref;
}

void undistort_frames(Context* ctx, const FrameDest& dst, const FrameSource& src,
                      const UndistortCameras& cams, hipStream_t stream)
{
    OPK_CHECK_ARG(dst.format == kFramesBgr, "the undistorted frames are BGR");
    OPK_CHECK_ARG(dst.n == src.n, "the destination's frame count differs from the source's");
    OPK_CHECK_ARG(src.w > 0 && src.h > 0, "Input images has 0 area.");
    OPK_CHECK_ARG(dst.w == src.w && dst.h == src.h,
                  "the destination's width and height differ from the source's");
    check_cameras(cams, src.n, src.w, src.h);
    if (src.n == 0) return;
    OPK_CHECK_ARG(src.plane[0] && dst.plane[0], "NULL buffer");
    check_frames(dst);
    check_frames(src);
    ctx->bind();
    const short* wtab = ctx->warp_weight_table(false);
    const Context::UndistortDev& maps = ctx->undistort_dev(cams);
    const int V = cams.views();
    for (int v = 0; v < V; ++v)   // (n is a multiple of V: every view has frames)
        launch_undistort_frames(dst, src, maps.view[(size_t)v], wtab, v, V, stream);
}

namespace {
template <class F>
int guarded_undistort(F&& f)
{
    try {
        f();
        return OPK_OK;
    } catch (const Error& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_error(e.what());
        return OPK_ERR_STATE;
    }
}
}  // namespace

}  // namespace opk

struct opk_ctx : opk::Context {};

extern "C" int opk_undistort_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* src,
                                    const opk_cameras* cams)
{
    return opk::guarded_undistort([&] {
        OPK_CHECK_ARG(ctx && dst && src, "NULL argument");
        const opk::FrameSource s = opk::frame_source(*src);
        const opk::UndistortCameras c = opk::make_cameras(cams);
        opk::undistort_frames(ctx, opk::frame_dest_for(*dst, s), s, c, ctx->stream);
    });
}
