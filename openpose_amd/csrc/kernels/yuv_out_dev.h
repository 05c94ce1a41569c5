// yuv_out_dev.h -- BGR -> YUV 4:2:0 on the device: the integer arithmetic of OpenCV's
// cvtColor(COLOR_BGR2YUV_I420) (BT.601 limited range, 20-bit fixed point; every pixel gives a luma
// sample, the top-left pixel of each 2x2 block the block's (U, V), no averaging), as include/opk.h
// states it.  Shared by the standalone conversion (yuv.hip) and by the store epilogue of the batch
// render (render.hip), so both write the bytes of opk_bgr_to_frames.
//
// Every sum is non-negative and below 2^31 for all (B, G, R) in [0, 255]^3, and the shifted values
// lie in [16, 235] (Y) and [16, 240] (U, V): there is no clamp, and the arithmetic shift of the
// definition is written as a logical one -- the same value, and nothing the compiler could fuse
// with a saturate into gfx950's packed shift (the note in yuv_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace opk {

constexpr int kYuvOutShift = 20;
constexpr int kYuvOutRY = 269484, kYuvOutGY = 528482, kYuvOutBY = 102760;
constexpr int kYuvOutRU = -155188, kYuvOutGU = -305135, kYuvOutBU = 460324;
constexpr int kYuvOutRV = 460324, kYuvOutGV = -385875, kYuvOutBV = -74448;
constexpr int kYuvOutHalf = 1 << (kYuvOutShift - 1);

__device__ __forceinline__ unsigned bgr_to_y(int b, int g, int r)
{
    const int s = kYuvOutRY * r + kYuvOutGY * g + kYuvOutBY * b + kYuvOutHalf + (16 << kYuvOutShift);
    return (unsigned)s >> kYuvOutShift;
}
__device__ __forceinline__ unsigned bgr_to_u(int b, int g, int r)
{
    const int s = kYuvOutRU * r + kYuvOutGU * g + kYuvOutBU * b + kYuvOutHalf + (128 << kYuvOutShift);
    return (unsigned)s >> kYuvOutShift;
}
__device__ __forceinline__ unsigned bgr_to_v(int b, int g, int r)
{
    const int s = kYuvOutRV * r + kYuvOutGV * g + kYuvOutBV * b + kYuvOutHalf + (128 << kYuvOutShift);
    return (unsigned)s >> kYuvOutShift;
}

// Where the samples of row yy (luma) / chroma row yy >> 1 of frame f go
struct YuvOutRow {
    uint8_t* y;
    uint8_t* u;
    uint8_t* v;
    int cpix;
};
__device__ __forceinline__ YuvOutRow yuv_out_row(const FrameDest& d, int f, int yy)
{
    const size_t c = (size_t)(yy >> 1) * d.cstep;
    return YuvOutRow{d.plane[0] + (size_t)f * d.frame[0] + (size_t)yy * d.step,
                     d.plane[1] + (size_t)f * d.frame[1] + c, d.plane[2] + (size_t)f * d.frame[2] + c,
                     d.cpix};
}

}  // namespace opk
