// yuv_dev.h -- YUV 4:2:0 -> BGR on the device: the integer arithmetic of OpenCV's
// cvtColor(COLOR_YUV2BGR_NV12 / _I420) (BT.601 limited range, 20-bit fixed point; each 2x2 block of
// luma pixels shares one (U, V) pair, nearest chroma), as include/opk.h states it.  Shared by the
// standalone conversion and the YUV warps (yuv.hip) and by the frame -> output image kernels
// (render.hip), so every path computes the BGR bytes of opk_frames_to_bgr.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace opk {

constexpr int kYuvShift = 20;
constexpr int kYuvCY = 1220542, kYuvCUB = 2116026, kYuvCUG = -409993, kYuvCVG = -852492,
              kYuvCVR = 1673527;

// clamp(v >> 20, 0, 255) with the arithmetic shift, written as a clamp of v followed by a logical
// shift: the same value for every int, and not the shift-then-saturate pair that the compiler
// fuses, two at a time, into gfx950's v_ashr_pk_u8_i32 -- whose upper result half it then reads
// as zero although the instruction leaves it alone (seen as garbage in bytes 2 and 3 of the packed
// words of yuv.hip)
__device__ __forceinline__ int yuv_clamp(int v)
{
    constexpr int top = (256 << kYuvShift) - 1;
    v = v < 0 ? 0 : (v > top ? top : v);
    return (int)((unsigned)v >> kYuvShift);
}

// the three chroma terms of a 2x2 block, rounding included; one luma term per pixel
struct YuvChroma {
    int b, g, r;
};
__device__ __forceinline__ YuvChroma yuv_chroma(int U, int V)
{
    const int u = U - 128, v = V - 128;
    return YuvChroma{(1 << (kYuvShift - 1)) + kYuvCUB * u,
                     (1 << (kYuvShift - 1)) + kYuvCVG * v + kYuvCUG * u,
                     (1 << (kYuvShift - 1)) + kYuvCVR * v};
}
__device__ __forceinline__ void yuv_pixel(int c[3], int Y, const YuvChroma& k)
{
    const int y = max(0, Y - 16) * kYuvCY;
    c[0] = yuv_clamp(y + k.b);
    c[1] = yuv_clamp(y + k.g);
    c[2] = yuv_clamp(y + k.r);
}
// the same, packed: B | G << 8 | R << 16
__device__ __forceinline__ unsigned yuv_pixel_packed(int Y, const YuvChroma& k)
{
    int c[3];
    yuv_pixel(c, Y, k);
    return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
}

// One row of a YUV frame: the luma row yy and the chroma row yy >> 1 that goes with it -- where the
// warps read their taps (B const) and where converted samples go (B writable, yuv_out_dev.h)
template <class B>
struct YuvRowT {
    B* y;
    B* u;
    B* v;
    int cpix;
};
using YuvRow = YuvRowT<const uint8_t>;
template <class B>
__device__ __forceinline__ YuvRowT<B> yuv_row(const FramesT<B>& s, int f, int yy)
{
    const size_t c = (size_t)(yy >> 1) * s.cstep;
    return YuvRowT<B>{s.plane[0] + (size_t)f * s.frame[0] + (size_t)yy * s.step,
                      s.plane[1] + (size_t)f * s.frame[1] + c, s.plane[2] + (size_t)f * s.frame[2] + c,
                      s.cpix};
}
// pixel xx of the row as BGR (warp_pixel's tap fetch, warp_dev.h)
__device__ __forceinline__ void warp_tap(int c[3], const YuvRow& row, int xx)
{
    const int o = (xx >> 1) * row.cpix;
    yuv_pixel(c, row.y[xx], yuv_chroma(row.u[o], row.v[o]));
}

}  // namespace opk
