// frames.h -- the one frame description (FramesT, kernels/kernels.h) on the host: how a caller's
// descriptor becomes one, what a launcher may assume of one, and when its planes take wide accesses
// (internal).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../../include/opk.h"
#include "../common.h"
#include "../kernels/kernels.h"

namespace opk {

static_assert(OPK_FRAMES_BGR == kFramesBgr && OPK_FRAMES_NV12 == kFramesNv12 &&
                  OPK_FRAMES_I420 == kFramesI420,
              "OPK_FRAMES_* are FrameFormat's values");

// The resolver: an opk_frames (B const) or opk_frames_out (B writable) descriptor checked and
// resolved, before any device work: unknown format, n < 0, a step shorter than its row, and for
// NV12 / I420 an odd width or height and (n > 0) a NULL plane are OPK_ERR_ARG; steps and frame
// strides of 0 get their tight values, NV12's V plane is U + 1.  Sizes <= 0 and a NULL BGR buffer are
// left to the callers' own checks, which the pointer-taking entry points share.  The result holds
// no pointer into the descriptor.  Callers read the texts through opk_last_error(): they name
// frame_source for either descriptor, as they did when the destinations went through it.
template <class B, class Desc>
FramesT<B> resolve_frames(const Desc& d)
{
    auto need = [](bool ok, const char* msg) {
        if (!ok) throw Error(OPK_ERR_ARG, std::string("frame_source: ") + msg);
    };
    need(d.format == OPK_FRAMES_BGR || d.format == OPK_FRAMES_NV12 || d.format == OPK_FRAMES_I420,
         "unknown frame format: OPK_FRAMES_BGR (0), OPK_FRAMES_NV12 (1) or OPK_FRAMES_I420 (2)");
    need(d.n >= 0, "negative frame count");
    FramesT<B> s{};
    s.format = d.format;
    s.n = d.n;
    s.w = d.width;
    s.h = d.height;
    const size_t w = d.width > 0 ? (size_t)d.width : 0, h = d.height > 0 ? (size_t)d.height : 0;
    if (d.format == OPK_FRAMES_BGR) {
        need(d.step[0] == 0 || d.step[0] >= w * 3, "row step shorter than the row");
        s.plane[0] = d.plane[0];
        s.step = d.step[0] ? d.step[0] : w * 3;
        s.frame[0] = d.frame_bytes[0] ? d.frame_bytes[0] : s.step * h;
        return s;
    }
    need(d.width % 2 == 0 && d.height % 2 == 0, "YUV 4:2:0 frames need an even width and height");
    const bool nv12 = d.format == OPK_FRAMES_NV12;
    const size_t crow = nv12 ? w : w / 2;   // bytes of a chroma row
    need(d.step[0] == 0 || d.step[0] >= w, "row step shorter than the row");
    need(d.step[1] == 0 || d.step[1] >= crow, "row step shorter than the row");
    need(nv12 || d.step[2] == 0 || d.step[2] >= crow, "row step shorter than the row");
    if (d.n > 0)
        need(d.plane[0] && d.plane[1] && (nv12 || d.plane[2]),
             nv12 ? "NULL plane: NV12 frames need plane[0] (Y) and plane[1] (UV)"
                  : "NULL plane: I420 frames need plane[0] (Y), plane[1] (U) and plane[2] (V)");
    s.step = d.step[0] ? d.step[0] : w;
    s.cstep = d.step[1] ? d.step[1] : crow;
    need(nv12 || (d.step[2] ? d.step[2] : crow) == s.cstep,
         "the U and V planes of I420 frames share one row step");
    s.cpix = nv12 ? 2 : 1;
    s.plane[0] = d.plane[0];
    s.plane[1] = d.plane[1];
    s.plane[2] = nv12 ? (d.plane[1] ? d.plane[1] + 1 : nullptr) : d.plane[2];
    s.frame[0] = d.frame_bytes[0] ? d.frame_bytes[0] : s.step * h;
    s.frame[1] = d.frame_bytes[1] ? d.frame_bytes[1] : s.cstep * (h / 2);
    s.frame[2] = nv12 ? s.frame[1] : (d.frame_bytes[2] ? d.frame_bytes[2] : s.cstep * (h / 2));
    return s;
}
inline FrameSource frame_source(const ::opk_frames& d) { return resolve_frames<const uint8_t>(d); }
inline FrameDest frame_dest(const ::opk_frames_out& d) { return resolve_frames<uint8_t>(d); }

// The validator: what every launcher needs of a description's layout before it reads or writes
// through it -- BGR: the row step; NV12 / I420: the format, an even size, all three planes, the
// chroma sample stride that goes with the format, both row steps.  Nothing a resolved descriptor
// can fail: these guard the launchers against descriptions built by hand.  Emptiness (n, w, h, a
// NULL plane[0]) has a site's own words and comes first there, as do a site's own limits.
template <class B>
void check_frames(const FramesT<B>& f)
{
    if (f.format == kFramesBgr) {
        OPK_CHECK_ARG(f.step >= (size_t)f.w * 3, "row step shorter than the row");
        return;
    }
    OPK_CHECK_ARG(f.format == kFramesNv12 || f.format == kFramesI420, "unknown frame format");
    OPK_CHECK_ARG(f.w % 2 == 0 && f.h % 2 == 0, "YUV 4:2:0 frames have even width and height");
    OPK_CHECK_ARG(f.plane[0] && f.plane[1] && f.plane[2], "NULL plane");
    OPK_CHECK_ARG(f.cpix == (f.format == kFramesNv12 ? 2 : 1), "chroma sample stride");
    OPK_CHECK_ARG(f.step >= (size_t)f.w && f.cstep >= (size_t)(f.w / 2) * f.cpix,
                  "row step shorter than the row");
}

// The alignment predicate: every plane base, row step and frame stride that a `bytes`-wide access
// goes through is a multiple of the access.  BGR is the one-plane case.  NV12's pairs go through
// plane[1] alone (plane[2] is plane[1] + 1 and never aligned).  bytes = 16 asks for the 16-pixel
// pieces of yuv.hip, which take I420's chroma as two 8-byte halves, so its U and V planes need 8;
// any other width (the render's 4-byte tile stores) is the same on every plane.
template <class B>
bool frames_aligned(const FramesT<B>& f, size_t bytes)
{
    auto on = [](const void* base, size_t step, size_t frame, size_t a) {
        return (uintptr_t)base % a == 0 && step % a == 0 && frame % a == 0;
    };
    if (!on(f.plane[0], f.step, f.frame[0], bytes)) return false;
    if (f.format == kFramesBgr) return true;
    if (f.format == kFramesNv12) return on(f.plane[1], f.cstep, f.frame[1], bytes);
    const size_t chroma = bytes == 16 ? 8 : bytes;
    return on(f.plane[1], f.cstep, f.frame[1], chroma) && on(f.plane[2], f.cstep, f.frame[2], chroma);
}

}  // namespace opk
