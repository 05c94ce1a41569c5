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
#include "yuv_dev.h"

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

// ---- the store epilogue of the batch render (render.hip) -----------------------------------------
// A workgroup of 256 lanes holds a 32 x 8 pixel tile at (tx0, ty0), lane tid = 32 * row + column, of
// which rows x cols pixels lie inside the frame; the lane's pixel (x, y) has the cast bytes
// (cb, cg, cr).  They become samples here -- every lane its pixel's luma, the lanes at even (x, y)
// their block's (U, V); w and h are even, so a block lies inside the frame, and the tile, with its
// top-left.  `stage`: 384 bytes of LDS that nothing else uses any more.
constexpr int kYuvTileW = 32, kYuvTileH = 8;
__device__ __forceinline__ void yuv_store_tile(const RenderFramesArgs& a, int f, int x, int y,
                                               bool inside, unsigned cb, unsigned cg, unsigned cr,
                                               uint8_t* stage, unsigned tid, int tx0, int ty0,
                                               int rows, int cols)
{
    const FrameDest& out = a.out;
    const unsigned Y = bgr_to_y((int)cb, (int)cg, (int)cr);
    const bool top = ((x | y) & 1) == 0;
    const unsigned U = bgr_to_u((int)cb, (int)cg, (int)cr);
    const unsigned V = bgr_to_v((int)cb, (int)cg, (int)cr);
    const int cpix = out.cpix;
    if (!a.dst_aligned) {
        if (inside) {
            const YuvRowT<uint8_t> o = yuv_row(out, f, y);
            o.y[x] = (uint8_t)Y;
            if (top) {
                o.u[(x >> 1) * cpix] = (uint8_t)U;
                o.v[(x >> 1) * cpix] = (uint8_t)V;
            }
        }
        return;
    }
    // every plane on 4-byte boundaries (a tile starts at byte 32 * blockIdx.x of its luma and
    // NV12 chroma rows, 16 * blockIdx.x of its I420 ones): the tile's 8 x 32 luma bytes and
    // 4 x 32 chroma bytes (NV12: pairs; I420: 16 of U at 256, 16 of V at 320 per row) go through
    // LDS and leave as 4-byte stores: wave 0 the luma, 8 lanes a row; wave 1 the chroma,
    // 8 (NV12) or 4 + 4 (I420) lanes a row; what a row has left over as bytes
    const int lx = tid & (kYuvTileW - 1), ly = tid / kYuvTileW;
    stage[tid] = (uint8_t)Y;
    if (top) {
        if (cpix == 2) {
            stage[256 + (ly >> 1) * 32 + lx] = (uint8_t)U;
            stage[256 + (ly >> 1) * 32 + lx + 1] = (uint8_t)V;
        } else {
            stage[256 + (ly >> 1) * 16 + (lx >> 1)] = (uint8_t)U;
            stage[320 + (ly >> 1) * 16 + (lx >> 1)] = (uint8_t)V;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    if (wave > 1) return;
    uint8_t* d;
    const uint8_t* s;
    int left;   // bytes of the row from this lane's first
    if (wave == 0) {
        const int row = lane >> 3, o = (lane & 7) * 4;
        if (row >= rows) return;
        d = out.plane[0] + (size_t)f * out.frame[0] + (size_t)(ty0 + row) * out.step + tx0 + o;
        s = stage + row * 32 + o;
        left = cols - o;
    } else if (cpix == 2) {
        const int row = lane >> 3, o = (lane & 7) * 4;
        if (lane >= 32 || 2 * row >= rows) return;
        d = out.plane[1] + (size_t)f * out.frame[1] + (size_t)((ty0 >> 1) + row) * out.cstep + tx0 + o;
        s = stage + 256 + row * 32 + o;
        left = cols - o;
    } else {
        const int p = lane >> 4, row = (lane >> 2) & 3, o = (lane & 3) * 4;   // p: U, V
        if (lane >= 32 || 2 * row >= rows) return;
        d = out.plane[1 + p] + (size_t)f * out.frame[1 + p] +
            (size_t)((ty0 >> 1) + row) * out.cstep + (tx0 >> 1) + o;
        s = stage + 256 + p * 64 + row * 16 + o;
        left = (cols >> 1) - o;
    }
    if (left >= 4) {
        *reinterpret_cast<unsigned*>(d) = *reinterpret_cast<const unsigned*>(s);
    } else {
        for (int i = 0; i < left; ++i) d[i] = s[i];
    }
}

}  // namespace opk
