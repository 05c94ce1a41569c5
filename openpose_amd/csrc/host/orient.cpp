// orient.cpp -- the host side of the rotated and flipped frames (include/opk.h): the orientation
// and its checks, opk_orient_size and opk_orient_keypoints.  No device code: tests/orient_driver.cpp
// builds this file alone under the sanitizers.
#include "orient.h"

#include <string>

namespace opk {

Orientation make_orientation(int rotate, int flip)
{
    const int r = rotate % 360;   // (int)std::round(rotationAngle) % 360 of the reference
    OPK_CHECK_ARG(r % 90 == 0,
                  "Rotation angle = " + std::to_string(r) + " != {0, 90, 180, 270} degrees.");
    OPK_CHECK_ARG(flip == 0 || flip == 1, "flip: 0 or 1");
    Orientation o;
    o.rotate = (r + 360) % 360;   // -270, -180, -90 are 90, 180, 270
    o.flip = flip != 0;
    return o;
}

void check_orient(const FrameDest& dst, const FrameSource& src, const Orientation& o)
{
    OPK_CHECK_ARG(dst.format == src.format, "the destination's format differs from the source's");
    OPK_CHECK_ARG(dst.n == src.n, "the destination's frame count differs from the source's");
    OPK_CHECK_ARG(src.w > 0 && src.h > 0, "Input images has 0 area.");
    OPK_CHECK_ARG(dst.w == (o.turn() ? src.h : src.w) && dst.h == (o.turn() ? src.w : src.h),
                  "the destination's width and height are not opk_orient_size's");
}

void orient_keypoints(float* kp, int people, int parts, int w, int h, const Orientation& o,
                      bool inverse)
{
    OPK_CHECK_ARG(people >= 0 && parts >= 0, "negative people or parts");
    OPK_CHECK_ARG(w > 0 && h > 0, "empty frame");
    const size_t count = (size_t)people * (size_t)parts;
    if (count == 0) return;
    OPK_CHECK_ARG(kp != nullptr, "NULL keypoints");
    const float xm = (float)(w - 1), ym = (float)(h - 1);
    const bool turn = o.turn(), mx = o.mx(), my = o.my();
    for (size_t i = 0; i < count; ++i) {
        float* p = kp + 3 * i;
        if (p[2] == 0.f) continue;   // the reference's missing keypoint (0, 0, 0)
        const float x = p[0], y = p[1];
        if (!inverse) {
            // (x, y) a source position: D[Y][X] = S[y][x] for the (X, Y) stored
            const float a = mx ? xm - x : x, b = my ? ym - y : y;
            p[0] = turn ? b : a;
            p[1] = turn ? a : b;
        } else {
            // (x, y) an oriented position: its source column comes from x, or from y when turned
            const float u = turn ? y : x, v = turn ? x : y;
            p[0] = mx ? xm - u : u;
            p[1] = my ? ym - v : v;
        }
    }
}

namespace {
template <class F>
int guarded_orient(F&& f)
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

extern "C" {

int opk_orient_size(int width, int height, int rotate, int* out_w, int* out_h)
{
    return opk::guarded_orient([&] {
        OPK_CHECK_ARG(out_w && out_h, "NULL argument");
        OPK_CHECK_ARG(width >= 0 && height >= 0, "negative size");
        const opk::Orientation o = opk::make_orientation(rotate, 0);
        *out_w = o.turn() ? height : width;
        *out_h = o.turn() ? width : height;
    });
}

int opk_orient_keypoints(float* keypoints_host, int people, int parts, int width, int height,
                         int rotate, int flip, int inverse)
{
    return opk::guarded_orient([&] {
        OPK_CHECK_ARG(inverse == 0 || inverse == 1, "inverse: 0 or 1");
        const opk::Orientation o = opk::make_orientation(rotate, flip);
        opk::orient_keypoints(keypoints_host, people, parts, width, height, o, inverse != 0);
    });
}

}  // extern "C"
