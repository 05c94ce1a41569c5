// undistort.hip -- cv::remap(INTER_LINEAR, constant border 0) of a batch of frames through one
// camera's CV_16SC2 maps (include/opk.h "THE REMAP OF ONE FRAME"; the maps: host/undistort.cpp).
//
// A gather: per destination pixel 6 map bytes, four 3-byte taps (a luma byte and a chroma pair per
// tap for NV12 / I420, converted as they are read: yuv_dev.h), one 8-byte weight set of the 8 KB
// bilinear table, 3 bytes written.  The sums are warp_pixel<2>'s (warp_dev.h) -- the frame warp's
// integers with (sx, sy) and the fraction taken from the maps instead of the axis tables -- so BGR
// and YUV sources give the bytes of the text by construction.
// Two mappings (dev switch UNDISTORT_VEC: 1 vec, 0 plain; unset: vec for BGR sources, plain for YUV
// ones, as measured):
//   vec    a lane owns 4 consecutive destination pixels of a row: its maps are one 16-byte and one
//          8-byte load (the device maps' rows are padded to 4 pixels), the weight table is staged in
//          LDS once per workgroup, which walks kUndistortIter x 256 such groups, and the 12 bytes go
//          out as three dwords -- bytes for the last group of a row when width % 4 != 0 and for
//          every group when the destination's base, row step or frame stride is not a multiple of 4;
//   plain  a lane per pixel, weights from global memory, byte stores.
// One launch covers the frames of one camera (first, first + stride, ...), so a camera's maps are
// walked by its frames back to back.
#include "kernels.h"
#include "warp_dev.h"
#include "yuv_dev.h"
#include "../common.h"
#include "../host/frames.h"
#include "../host/undistort.h"

namespace opk {

namespace {

constexpr int kUndistortIter = 4;   // groups of 4 pixels per lane of the vec mapping

// one destination pixel: taps from (s.x, s.y), weights of fraction fr = yfrac * 32 + xfrac
template <bool Yuv>
__device__ __forceinline__ void undistort_pixel(int u[3], const FrameSource& src, int f, int sx,
                                                int sy, unsigned fr, const short* wtab)
{
    const int2 yt{sy, 0}, xt{sx, 0};
    const short* w = warp_weights<2>(wtab, (int)(fr >> 5) & 31, (int)(fr & 31));
    if constexpr (Yuv) {
        warp_pixel<2>(u, yt, xt, w, src.h, src.w, [&](int, int yy) { return yuv_row(src, f, yy); });
    } else {
        const uint8_t* base = src.plane[0] + (size_t)f * src.frame[0];
        warp_pixel<2>(u, yt, xt, w, src.h, src.w,
                      [&](int, int yy) { return base + (size_t)yy * src.step; });
    }
}

// grid (column blocks, rows, the launch's frames)
template <bool Yuv>
__global__ __launch_bounds__(256) void undistort_frames_plain(FrameDest dst, FrameSource src,
                                                              UndistortMap map,
                                                              const short* __restrict__ wtab,
                                                              int first, int stride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int f = first + (int)blockIdx.z * stride;
    if (x >= src.w) return;
    const size_t at = (size_t)y * map.pitch + x;
    const short2 s = map.m1[at];
    int u[3];
    undistort_pixel<Yuv>(u, src, f, s.x, s.y, map.m2[at], wtab);
    uint8_t* d = dst.plane[0] + (size_t)f * dst.frame[0] + (size_t)y * dst.step + (size_t)x * 3;
    d[0] = (uint8_t)u[0];
    d[1] = (uint8_t)u[1];
    d[2] = (uint8_t)u[2];
}

// grid (blocks of kUndistortIter x 256 groups over the rows of a frame, 1, the launch's frames);
// groups = ceil(w / 4) per row
template <bool Yuv>
__global__ __launch_bounds__(256) void undistort_frames_vec(FrameDest dst, FrameSource src,
                                                            UndistortMap map,
                                                            const short* __restrict__ wtab,
                                                            int first, int stride, int groups,
                                                            int aligned)
{
    __shared__ __attribute__((aligned(16))) short ws[32 * 32 * 4];
    {
        const uint4* g = reinterpret_cast<const uint4*>(wtab);   // 8192 bytes: 2 x 16 per lane
        uint4* l = reinterpret_cast<uint4*>(ws);
        l[threadIdx.x] = g[threadIdx.x];
        l[256 + threadIdx.x] = g[256 + threadIdx.x];
    }
    __syncthreads();
    const int f = first + (int)blockIdx.z * stride;
    const int total = groups * src.h;
    uint8_t* fdst = dst.plane[0] + (size_t)f * dst.frame[0];
#pragma unroll 1
    for (int it = 0; it < kUndistortIter; ++it) {
        const int idx = ((int)blockIdx.x * kUndistortIter + it) * 256 + (int)threadIdx.x;
        if (idx >= total) return;
        const int y = idx / groups, x0 = 4 * (idx - y * groups);
        const size_t at = (size_t)y * map.pitch + x0;   // x0 + 3 < pitch: the rows are padded
        const uint4 a = *reinterpret_cast<const uint4*>(map.m1 + at);
        const uint2 b = *reinterpret_cast<const uint2*>(map.m2 + at);
        const unsigned xy[4] = {a.x, a.y, a.z, a.w};
        const unsigned fr[4] = {b.x & 0xffffu, b.x >> 16, b.y & 0xffffu, b.y >> 16};
        const int valid = min(4, src.w - x0);
        unsigned p[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= valid) continue;
            int u[3];
            undistort_pixel<Yuv>(u, src, f, (int)(short)(xy[i] & 0xffffu), (int)(short)(xy[i] >> 16),
                                 fr[i], ws);
            p[i] = (unsigned)u[0] | (unsigned)u[1] << 8 | (unsigned)u[2] << 16;
        }
        uint8_t* d = fdst + (size_t)y * dst.step + (size_t)x0 * 3;
        if (aligned && valid == 4) {
            unsigned* q = reinterpret_cast<unsigned*>(d);
            q[0] = p[0] | p[1] << 24;
            q[1] = p[1] >> 8 | p[2] << 16;
            q[2] = p[2] >> 16 | p[3] << 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i >= valid) continue;
                d[3 * i] = (uint8_t)(p[i] & 255u);
                d[3 * i + 1] = (uint8_t)((p[i] >> 8) & 255u);
                d[3 * i + 2] = (uint8_t)(p[i] >> 16);
            }
        }
    }
}

}  // namespace

void launch_undistort_frames(const FrameDest& dst, const FrameSource& src, const UndistortMap& map,
                             const short* wtab, int first, int stride, hipStream_t stream)
{
    OPK_CHECK_ARG(dst.format == kFramesBgr, "the destination frames are BGR");
    OPK_CHECK_ARG(src.n > 0 && src.w > 0 && src.h > 0, "empty frame");
    OPK_CHECK_ARG(dst.n == src.n && dst.w == src.w && dst.h == src.h, "frame count or size differs");
    OPK_CHECK_ARG(dst.plane[0] && src.plane[0], "NULL plane");
    check_frames(dst);
    check_frames(src);
    OPK_CHECK_ARG(map.m1 && map.m2 && wtab && map.pitch >= src.w && map.pitch % 4 == 0, "bad maps");
    OPK_CHECK_ARG(first >= 0 && stride >= 1 && first < src.n, "bad frame walk");
    const int count = (src.n - first + stride - 1) / stride;   // first + (count - 1) * stride < n
    OPK_CHECK_ARG(src.h <= 65535 && count <= 65535, "more than 65535 rows or frames");
    const bool yuv = src.format != kFramesBgr;
    // unset: the mapping measured faster for the source format -- vec for BGR
    // (0.94 against 1.00 ms on 128 frames of 1280x720), plain for NV12 / I420 (1.01 against 1.03)
    const int mapping = dev_switch("UNDISTORT_VEC", -1);
    if (mapping < 0 ? !yuv : mapping != 0) {
        const int groups = (src.w + 3) / 4;
        OPK_CHECK_ARG((long long)groups * src.h < (1LL << 31) - kUndistortIter * 256, "frame too large");
        const int per_block = kUndistortIter * 256;
        const dim3 grid((unsigned)(((long long)groups * src.h + per_block - 1) / per_block), 1,
                        (unsigned)count);
        const int aligned = frames_aligned(dst, 4) ? 1 : 0;
        note_launch(yuv ? "undistort_frames<vec,yuv>" : "undistort_frames<vec>");
        if (yuv)
            hipLaunchKernelGGL(undistort_frames_vec<true>, grid, dim3(256), 0, stream, dst, src, map,
                               wtab, first, stride, groups, aligned);
        else
            hipLaunchKernelGGL(undistort_frames_vec<false>, grid, dim3(256), 0, stream, dst, src, map,
                               wtab, first, stride, groups, aligned);
    } else {
        const dim3 grid((unsigned)((src.w + 255) / 256), (unsigned)src.h, (unsigned)count);
        note_launch(yuv ? "undistort_frames<plain,yuv>" : "undistort_frames<plain>");
        if (yuv)
            hipLaunchKernelGGL(undistort_frames_plain<true>, grid, dim3(256), 0, stream, dst, src,
                               map, wtab, first, stride);
        else
            hipLaunchKernelGGL(undistort_frames_plain<false>, grid, dim3(256), 0, stream, dst, src,
                               map, wtab, first, stride);
    }
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
