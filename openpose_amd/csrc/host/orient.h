// orient.h -- rotated and flipped frames (include/opk.h; the reference's rotateAndFlipFrame,
// utilities/openCv.cpp:236-282): the orientation, its checks and the keypoint map on the host
// (host/orient.cpp, no device code), and the device route (host/orient_dev.cpp) (internal).
#pragma once
#include "frames.h"

namespace opk {

struct Context;

// rotate in {0, 90, 180, 270} and the flip, as the table of include/opk.h reads them: the
// destination is the transpose (turn) or not, mirrored on the source's x and / or y axis
struct Orientation {
    int rotate = 0;
    bool flip = false;
    bool set() const { return rotate != 0 || flip; }
    bool turn() const { return rotate == 90 || rotate == 270; }
    bool mx() const { return flip != (rotate == 90 || rotate == 180); }
    bool my() const { return rotate == 180 || rotate == 270; }
};
// OPK_ERR_ARG with the reference's text for rotate % 360 outside {0, +-90, +-180, +-270}, and for a
// flip other than 0 or 1
Orientation make_orientation(int rotate, int flip);
// the checks of opk_orient_frames that need no device and no other frame set: format, n, sizes
void check_orient(const FrameDest& dst, const FrameSource& src, const Orientation& o);
// [people][parts][3] in place: source -> oriented coordinates (inverse: back); w, h the source's
void orient_keypoints(float* kp, int people, int parts, int w, int h, const Orientation& o,
                      bool inverse);
// check_orient, the overlap rule, then launch_orient_frames on `stream`; n == 0 returns before it
void orient_frames(Context* ctx, const FrameDest& dst, const FrameSource& src, const Orientation& o,
                   hipStream_t stream);

}  // namespace opk
