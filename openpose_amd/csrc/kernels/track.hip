// track.hip -- person identification across frames (op::PersonIdExtractor, --identification): the
// grey image + 3-level Gaussian pyramid of a batch of frames, and one pyramidal Lucas-Kanade pass
// over an array of point records (src/openpose/tracking/pyramidalLK.cpp:272-368, pyramidalLK.cu).
// include/opk.h ("Person ids across frames") is the definition every line here follows.
//
// Pyramid: three passes -- grey, level 1, level 2 -- not one fused kernel.  The grey pass moves
// 3 (BGR) or 1.5 (YUV) bytes in and 1 out per pixel; the two down-sampling passes move 1.5 and 0.75
// more, and a 130-frame 1280x720 batch of level-0 planes (120 MB) stays in the Infinity Cache
// between them.  A fused kernel would save those 2.25 bytes per pixel and pay for it with a
// (4t+12)^2 grey halo per t x t level-2 tile recomputed from BGR; with the batch's pyramid at a few
// percent of the batch's net time (profiles/tracking/README.md) that trade was not taken.
// All pyramid arithmetic is integer: level 1 holds k = 256 x value (< 2^16, uint16), level 2 the
// float k / 65536 with k < 2^24 -- exact, whatever the summation order.
//
// LK: the five sums of a level are defined as sequential row-major fp32 sums, so a lane mapping has
// to reproduce that order.  Two are built and held to the same oracle bit for bit:
//   lk_points<thread>  a thread per point, as the reference's CUDA kernel: the order holds by
//                      construction, but a point is 3 x 441 dependent iterations of uncoalesced
//                      gathers in one lane -- 0.23 ms for a launch of any size up to a few thousand
//                      points, which is what the per-frame launches for stale entries are;
//   lk_points<wave>    a wave per point (shipped; dev switch LK_WAVE=0 selects the other): the lanes
//                      stage the windows and the products in LDS, five lanes add in order.  Half
//                      the time on 16,250 and 65,000 points and 0.04 ms for a small launch
//                      (profiles/tracking/README.md).
#include "kernels.h"
#include "yuv_dev.h"
#include "../common.h"
#include "../host/frames.h"

namespace opk {

namespace {

// ---- grey: (1868 B + 9617 G + 4899 R + 8192) >> 14 of the BGR pixel ----------------------------
__device__ __forceinline__ int grey_of(int b, int g, int r)
{
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14;
}

// grid (ceil(w / 256), h, n); a lane per pixel
template <bool Yuv>
__global__ __launch_bounds__(256) void track_grey_kernel(uint8_t* __restrict__ pyr, PyramidLayout L,
                                                         FrameSource fs)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= fs.w) return;
    int c[3];
    if (Yuv) {
        warp_tap(c, yuv_row(fs, f, y), x);
    } else {
        const uint8_t* p = fs.plane[0] + (size_t)f * fs.frame[0] + (size_t)y * fs.step + (size_t)x * 3;
        c[0] = p[0];
        c[1] = p[1];
        c[2] = p[2];
    }
    pyr[(size_t)f * L.frame + L.at[0] + (size_t)y * L.w[0] + x] = (uint8_t)grey_of(c[0], c[1], c[2]);
}

// index i of an axis of n samples, reflected without repeating the edge
__device__ __forceinline__ int reflect(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// level LV (1 | 2) from level LV - 1: taps 1 4 6 4 1 in x and y around (2x, 2y), in integers.
// grid (ceil(w / 64), ceil(h / 4), n), block (64, 4)
template <int LV>
__global__ __launch_bounds__(256) void pyr_down_kernel(uint8_t* __restrict__ pyr, PyramidLayout L)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    const int w = L.w[LV], h = L.h[LV], sw = L.w[LV - 1], sh = L.h[LV - 1];
    if (x >= w || y >= h) return;
    uint8_t* frame = pyr + (size_t)f * L.frame;
    const uint8_t* src = frame + L.at[LV - 1];
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = reflect(2 * x + j - 2, sw);
    constexpr int tap[5] = {1, 4, 6, 4, 1};
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const size_t row = (size_t)reflect(2 * y + i - 2, sh) * sw;
        unsigned r = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            unsigned v;
            if (LV == 1) v = src[row + xs[j]];
            else v = reinterpret_cast<const uint16_t*>(src)[row + xs[j]];
            r += tap[j] * v;
        }
        sum += tap[i] * r;
    }
    const size_t o = (size_t)y * w + x;
    if (LV == 1) reinterpret_cast<uint16_t*>(frame + L.at[1])[o] = (uint16_t)sum;   // < 2^16
    else reinterpret_cast<float*>(frame + L.at[2])[o] = (float)sum * (1.f / 65536.f);   // sum < 2^24
}

// one level as fp32 (tests): dst [n][h][w]
template <int LV>
__global__ __launch_bounds__(256) void pyr_level_kernel(float* __restrict__ dst,
                                                        const uint8_t* __restrict__ pyr,
                                                        PyramidLayout L, size_t total)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t plane = (size_t)L.w[LV] * L.h[LV];
    const uint8_t* lv = pyr + (i / plane) * L.frame + L.at[LV];
    const size_t o = i % plane;
    float v;
    if (LV == 0) v = (float)lv[o];
    else if (LV == 1) v = (float)reinterpret_cast<const uint16_t*>(lv)[o] * (1.f / 256.f);
    else v = reinterpret_cast<const float*>(lv)[o];
    dst[i] = v;
}

// ---- Lucas-Kanade -------------------------------------------------------------------------------
// pixel (y, x) of level LV of a frame's record, as the float the definition computes with
template <int LV>
__device__ __forceinline__ float pyr_at(const uint8_t* lv, int w, int y, int x)
{
    const size_t o = (size_t)y * w + x;
    if (LV == 0) return (float)lv[o];
    if (LV == 1) return (float)reinterpret_cast<const uint16_t*>(lv)[o] * (1.f / 256.f);
    return reinterpret_cast<const float*>(lv)[o];
}

// (int) v; everything that is not inside (-2^30, 2^30) -- NaN included -- becomes -2^30, which
// fails every bounds test below before anything is read
__device__ __forceinline__ int lk_trunc(float v)
{
    return fabsf(v) < 1073741824.f ? (int)v : -(1 << 30);
}

// one level of one point: pJ moves by the Lucas-Kanade step, or stays and the status becomes 3
template <int LV>
__device__ __forceinline__ void lk_level(const uint8_t* fi, const uint8_t* fj, const PyramidLayout& L,
                                         float pix, float piy, float& pjx, float& pjy, int& status)
{
    const int w = L.w[LV], h = L.h[LV];
    const int xi = lk_trunc(pix), yi = lk_trunc(piy), xj = lk_trunc(pjx), yj = lk_trunc(pjy);
    // the gradient patch (radius 11) leaves I: every ix, iy is 0, so all five sums and the
    // determinant are 0
    if (xi - 11 < 0 || xi + 11 >= w || yi - 11 < 0 || yi + 11 >= h) {
        status = 3;
        return;
    }
    const uint8_t* I = fi + L.at[LV];
    const uint8_t* J = fj + L.at[LV];
    // (the radius-10 patch of I is inside the radius-11 one)
    const bool timed = xj - 10 >= 0 && xj + 10 < w && yj - 10 >= 0 && yj + 10 < h;
    float sxx = 0.f, syy = 0.f, sxy = 0.f, sxt = 0.f, syt = 0.f;
    for (int i = -10; i <= 10; ++i) {
        float left = pyr_at<LV>(I, w, yi + i, xi - 11), mid = pyr_at<LV>(I, w, yi + i, xi - 10);
        for (int j = -10; j <= 10; ++j) {
            const float right = pyr_at<LV>(I, w, yi + i, xi + j + 1);
            const float ix = (right - left) / 2.f;
            const float iy = (pyr_at<LV>(I, w, yi + i + 1, xi + j) - pyr_at<LV>(I, w, yi + i - 1, xi + j)) / 2.f;
            const float it = timed ? pyr_at<LV>(J, w, yj + i, xj + j) - mid : 0.f;
            sxx += ix * ix;
            syy += iy * iy;
            sxy += ix * iy;
            sxt += ix * it;
            syt += iy * it;
            left = mid;
            mid = right;
        }
    }
    const float den = sxx * syy - sxy * sxy;
    if (fabsf(den) < 1e-9f) {
        status = 3;
        return;
    }
    pjx += ((-1.f * syy) * sxt + sxy * syt) / den;
    pjy += ((-1.f * sxx) * syt + sxt * sxy) / den;
}

// a lane per point record; frame -1 is the carried-over frame
__global__ __launch_bounds__(64) void lk_points_kernel(LkPoint* __restrict__ pts, int npoints,
                                                       const uint8_t* __restrict__ pyr, int nframes,
                                                       const uint8_t* __restrict__ carry,
                                                       PyramidLayout L)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= npoints) return;
    LkPoint pt = pts[p];
    if (pt.status != 0) return;
    const int lo = carry ? -1 : 0;
    const bool ok = fabsf(pt.x) < 16777216.f && fabsf(pt.y) < 16777216.f &&   // (false for NaN)
                    pt.frame_i >= lo && pt.frame_i < nframes && pt.frame_j >= lo && pt.frame_j < nframes;
    if (!ok) {
        pts[p].status = 3;
        return;
    }
    const uint8_t* fi = pt.frame_i < 0 ? carry : pyr + (size_t)pt.frame_i * L.frame;
    const uint8_t* fj = pt.frame_j < 0 ? carry : pyr + (size_t)pt.frame_j * L.frame;
    float pix = pt.x * 0.25f, piy = pt.y * 0.25f, pjx = pix, pjy = piy;
    int status = 0;
    lk_level<2>(fi, fj, L, pix, piy, pjx, pjy, status);
    pix *= 2.f;
    piy *= 2.f;
    pjx *= 2.f;
    pjy *= 2.f;
    lk_level<1>(fi, fj, L, pix, piy, pjx, pjy, status);
    pix *= 2.f;
    piy *= 2.f;
    pjx *= 2.f;
    pjy *= 2.f;
    lk_level<0>(fi, fj, L, pix, piy, pjx, pjy, status);
    pts[p].x = pjx;
    pts[p].y = pjy;
    pts[p].status = status;
}

// ---- the same point on a whole wave (lk_points<wave>) ------------------------------------------
// A workgroup is one wave and one point.  Per level the 64 lanes stage the 23 x 23 window of I and
// the 21 x 21 window of J in LDS, each lane forms the five products of its share of the 441 patch
// pixels (every product rounded as in lk_level), and then lanes 0..4 add one product array each,
// element by element in row-major order from 0 -- the defined summation order, so the sums are the
// thread mapping's bit for bit.  The point's state lives in every lane (all lanes compute the same
// step from the broadcast sums), so every branch is wave-uniform.
constexpr int kLkI = 23 * 23, kLkP = 21 * 21;

template <int LV>
__device__ __forceinline__ void lk_level_wave(float* lds, const uint8_t* fi, const uint8_t* fj,
                                              const PyramidLayout& L, float pix, float piy,
                                              float& pjx, float& pjy, int& status)
{
    const int lane = threadIdx.x;
    const int w = L.w[LV], h = L.h[LV];
    const int xi = lk_trunc(pix), yi = lk_trunc(piy), xj = lk_trunc(pjx), yj = lk_trunc(pjy);
    if (xi - 11 < 0 || xi + 11 >= w || yi - 11 < 0 || yi + 11 >= h) {
        status = 3;
        return;
    }
    const uint8_t* I = fi + L.at[LV];
    const uint8_t* J = fj + L.at[LV];
    const bool timed = xj - 10 >= 0 && xj + 10 < w && yj - 10 >= 0 && yj + 10 < h;
    float* iw = lds;                  // [23][23]
    float* jw = lds + kLkI;           // [21][21]
    float* prod = jw + kLkP;          // [5][441]
    __syncthreads();                  // the level before has read its sums
    for (int t = lane; t < kLkI; t += 64) iw[t] = pyr_at<LV>(I, w, yi - 11 + t / 23, xi - 11 + t % 23);
    if (timed)
        for (int t = lane; t < kLkP; t += 64) jw[t] = pyr_at<LV>(J, w, yj - 10 + t / 21, xj - 10 + t % 21);
    __syncthreads();
    for (int t = lane; t < kLkP; t += 64) {
        const int i = t / 21, j = t % 21;
        const float mid = iw[(i + 1) * 23 + j + 1];
        const float ix = (iw[(i + 1) * 23 + j + 2] - iw[(i + 1) * 23 + j]) / 2.f;
        const float iy = (iw[(i + 2) * 23 + j + 1] - iw[i * 23 + j + 1]) / 2.f;
        const float it = timed ? jw[t] - mid : 0.f;
        prod[t] = ix * ix;
        prod[kLkP + t] = iy * iy;
        prod[2 * kLkP + t] = ix * iy;
        prod[3 * kLkP + t] = ix * it;
        prod[4 * kLkP + t] = iy * it;
    }
    __syncthreads();
    float s = 0.f;
    if (lane < 5) {
        const float* p = prod + lane * kLkP;
#pragma unroll 9
        for (int t = 0; t < kLkP; ++t) s += p[t];
    }
    const float sxx = __shfl(s, 0), syy = __shfl(s, 1), sxy = __shfl(s, 2), sxt = __shfl(s, 3),
                syt = __shfl(s, 4);
    const float den = sxx * syy - sxy * sxy;
    if (fabsf(den) < 1e-9f) {
        status = 3;
        return;
    }
    pjx += ((-1.f * syy) * sxt + sxy * syt) / den;
    pjy += ((-1.f * sxx) * syt + sxt * sxy) / den;
}

// grid (npoints), block 64
__global__ __launch_bounds__(64) void lk_points_wave_kernel(LkPoint* __restrict__ pts, int npoints,
                                                            const uint8_t* __restrict__ pyr,
                                                            int nframes,
                                                            const uint8_t* __restrict__ carry,
                                                            PyramidLayout L)
{
    __shared__ float lds[kLkI + kLkP + 5 * kLkP];
    const int p = blockIdx.x;
    const LkPoint pt = pts[p];
    if (pt.status != 0) return;
    const int lo = carry ? -1 : 0;
    const bool ok = fabsf(pt.x) < 16777216.f && fabsf(pt.y) < 16777216.f &&
                    pt.frame_i >= lo && pt.frame_i < nframes && pt.frame_j >= lo && pt.frame_j < nframes;
    if (!ok) {
        if (threadIdx.x == 0) pts[p].status = 3;
        return;
    }
    const uint8_t* fi = pt.frame_i < 0 ? carry : pyr + (size_t)pt.frame_i * L.frame;
    const uint8_t* fj = pt.frame_j < 0 ? carry : pyr + (size_t)pt.frame_j * L.frame;
    float pix = pt.x * 0.25f, piy = pt.y * 0.25f, pjx = pix, pjy = piy;
    int status = 0;
    lk_level_wave<2>(lds, fi, fj, L, pix, piy, pjx, pjy, status);
    pix *= 2.f;
    piy *= 2.f;
    pjx *= 2.f;
    pjy *= 2.f;
    lk_level_wave<1>(lds, fi, fj, L, pix, piy, pjx, pjy, status);
    pix *= 2.f;
    piy *= 2.f;
    pjx *= 2.f;
    pjy *= 2.f;
    lk_level_wave<0>(lds, fi, fj, L, pix, piy, pjx, pjy, status);
    if (threadIdx.x == 0) {
        pts[p].x = pjx;
        pts[p].y = pjy;
        pts[p].status = status;
    }
}

}  // namespace

PyramidLayout pyramid_layout(int width, int height, int levels)
{
    OPK_CHECK_ARG(width > 0 && height > 0, "empty frame");
    OPK_CHECK_ARG(levels >= 1 && levels <= kPyramidLevels,
                  "1..3 pyramid levels (a fourth level is not exact in fp32)");
    PyramidLayout L{};
    L.levels = levels;
    size_t at = 0;
    for (int l = 0; l < levels; ++l) {
        L.w[l] = l ? (L.w[l - 1] + 1) / 2 : width;
        L.h[l] = l ? (L.h[l - 1] + 1) / 2 : height;
        L.at[l] = at;
        at += ((size_t)L.w[l] * L.h[l] * (l == 0 ? 1 : (l == 1 ? 2 : 4)) + 15) & ~(size_t)15;
    }
    L.frame = at;
    return L;
}

void launch_pyramid(uint8_t* pyr, const PyramidLayout& L, const FrameSource& fs, hipStream_t stream)
{
    OPK_CHECK_ARG(pyr != nullptr, "NULL pyramid buffer");
    OPK_CHECK_ARG(fs.n > 0 && fs.w == L.w[0] && fs.h == L.h[0], "frames of another size than the layout");
    OPK_CHECK_ARG(fs.plane[0] != nullptr, "NULL frames");
    OPK_CHECK_ARG(fs.h <= 65535 && fs.n <= 65535, "more than 65535 rows or frames");
    const bool yuv = fs.format != kFramesBgr;
    check_frames(fs);
    const dim3 g0((unsigned)((fs.w + 255) / 256), (unsigned)fs.h, (unsigned)fs.n);
    if (yuv) {
        note_launch("track_grey<yuv>");
        hipLaunchKernelGGL(track_grey_kernel<true>, g0, dim3(256), 0, stream, pyr, L, fs);
    } else {
        note_launch("track_grey<bgr>");
        hipLaunchKernelGGL(track_grey_kernel<false>, g0, dim3(256), 0, stream, pyr, L, fs);
    }
    OPK_LAUNCH_CHECK();
    for (int l = 1; l < L.levels; ++l) {
        const dim3 g((unsigned)((L.w[l] + 63) / 64), (unsigned)((L.h[l] + 3) / 4), (unsigned)fs.n);
        note_launch("pyr_down<%d>", l);
        if (l == 1) hipLaunchKernelGGL(pyr_down_kernel<1>, g, dim3(64, 4), 0, stream, pyr, L);
        else hipLaunchKernelGGL(pyr_down_kernel<2>, g, dim3(64, 4), 0, stream, pyr, L);
        OPK_LAUNCH_CHECK();
    }
}

void launch_pyramid_level(float* dst, const uint8_t* pyr, const PyramidLayout& L, int n, int level,
                          hipStream_t stream)
{
    OPK_CHECK_ARG(dst && pyr && n > 0, "NULL buffer or no frames");
    OPK_CHECK_ARG(level >= 0 && level < L.levels, "no such pyramid level");
    const size_t total = (size_t)n * L.w[level] * L.h[level];
    const dim3 g((unsigned)((total + 255) / 256));
    note_launch("pyr_level<%d>", level);
    if (level == 0) hipLaunchKernelGGL(pyr_level_kernel<0>, g, dim3(256), 0, stream, dst, pyr, L, total);
    else if (level == 1) hipLaunchKernelGGL(pyr_level_kernel<1>, g, dim3(256), 0, stream, dst, pyr, L, total);
    else hipLaunchKernelGGL(pyr_level_kernel<2>, g, dim3(256), 0, stream, dst, pyr, L, total);
    OPK_LAUNCH_CHECK();
}

void launch_lk_points(LkPoint* points, int npoints, const uint8_t* pyr, int nframes,
                      const uint8_t* carry, const PyramidLayout& L, hipStream_t stream)
{
    OPK_CHECK_ARG(npoints >= 0 && nframes >= 0, "negative count");
    OPK_CHECK_ARG(L.levels == kPyramidLevels, "Lucas-Kanade runs on 3-level pyramids");
    if (npoints == 0) return;
    OPK_CHECK_ARG(points != nullptr, "NULL points");
    OPK_CHECK_ARG(nframes == 0 || pyr != nullptr, "NULL pyramid buffer");
    if (dev_switch("LK_WAVE", 1) != 0) {
        note_launch("lk_points<wave>");
        hipLaunchKernelGGL(lk_points_wave_kernel, dim3((unsigned)npoints), dim3(64), 0, stream, points,
                           npoints, pyr, nframes, carry, L);
    } else {
        note_launch("lk_points<thread>");
        hipLaunchKernelGGL(lk_points_kernel, dim3((unsigned)((npoints + 63) / 64)), dim3(64), 0,
                           stream, points, npoints, pyr, nframes, carry, L);
    }
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
