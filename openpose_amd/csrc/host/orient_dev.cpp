// orient_dev.cpp -- the device route of the rotated and flipped frames (include/opk.h): the checks
// that come before any device work, the launches of kernels/orient.hip, and opk_orient_frames.
#include "../../../include/opk.h"
#include "../common.h"
#include "context.h"
#include "frames.h"
#include "input.h"
#include "orient.h"

namespace opk {

void orient_frames(Context* ctx, const FrameDest& dst, const FrameSource& src, const Orientation& o,
                   hipStream_t stream)
{
    check_orient(dst, src, o);
    if (src.n == 0) return;
    OPK_CHECK_ARG(src.plane[0] && dst.plane[0], "NULL buffer");
    check_frames(dst);
    check_frames(src);
    check_frames_apart(dst, src);
    ctx->bind();
    launch_orient_frames(dst, src, o.turn(), o.mx(), o.my(), stream);
}

}  // namespace opk

struct opk_ctx : opk::Context {};

extern "C" int opk_orient_frames(opk_ctx* ctx, const opk_frames_out* dst, const opk_frames* src,
                                 int rotate, int flip)
{
    try {
        OPK_CHECK_ARG(ctx && dst && src, "NULL argument");
        const opk::FrameSource s = opk::frame_source(*src);
        const opk::FrameDest d = opk::frame_dest(*dst);
        opk::orient_frames(ctx, d, s, opk::make_orientation(rotate, flip), ctx->stream);
        return OPK_OK;
    } catch (const opk::Error& e) {
        opk::set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        opk::set_error(e.what());
        return OPK_ERR_STATE;
    }
}
