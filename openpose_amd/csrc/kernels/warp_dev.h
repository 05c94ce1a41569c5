// warp_dev.h -- one destination pixel of OpenCV's fixed-point 8-bit warpAffine(diag(scale)), shared
// by the frame -> net input kernels (input.hip) and the frame -> output image kernels (render.hip).
// The host builds the per-axis tap tables and the 2-D weight table exactly as OpenCV does
// (host/input.cpp); here the taps are gathered and the integers summed, so every caller gets the
// CPU path's bytes by construction.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace opk {

// the K*K fixed-point weights of one (row fraction, column fraction) pair of the [32][32][K*K]
// table (a caller that staged the 32 sets of one row fraction passes them with yfrac 0)
template <int K>
__device__ __forceinline__ const short* warp_weights(const short* wtab, int yfrac, int xfrac)
{
    return wtab + (yfrac * 32 + xfrac) * K * K;
}

// pixel xx of a row of packed BGR bytes (a YUV row's fetch: yuv_dev.h)
__device__ __forceinline__ void warp_tap(int c[3], const uint8_t* row, int xx)
{
    const uint8_t* p = row + (size_t)xx * 3;
    c[0] = p[0];
    c[1] = p[1];
    c[2] = p[2];
}

// u[c] = saturate_cast<uchar>((sum of taps * weights + 2^14) >> 15) of the BGR pixel whose first
// tap is (xt.x, yt.x); taps outside the sh x sw source read 0 (constant border: BGR 0 whatever the
// source format).  row_of(ky, yy) returns tap row yy as something warp_tap reads a pixel from --
// BGR bytes addressed by source column * 3, or a YuvRow -- (called for rows inside the image and,
// with yy = 0, for rows outside it, whose taps are never read).
template <int K, class RowOf>
__device__ __forceinline__ void warp_pixel(int u[3], int2 yt, int2 xt, const short* w, int sh,
                                           int sw, RowOf row_of)
{
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int yy = yt.x + ky;
        const bool yin = yy >= 0 && yy < sh;
        const auto row = row_of(ky, yin ? yy : 0);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int xx = xt.x + kx;
            const int wk = w[ky * K + kx];
            if (yin && xx >= 0 && xx < sw) {   // constant border: outside taps read 0
                int c[3];
                warp_tap(c, row, xx);
                acc[0] += c[0] * wk;
                acc[1] += c[1] * wk;
                acc[2] += c[2] * wk;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = (acc[c] + (1 << 14)) >> 15;   // FixedPtCast<int, uchar, 15>
        u[c] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
}

}  // namespace opk
