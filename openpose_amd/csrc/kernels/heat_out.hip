// heat_out.hip -- getHeatMapsCopy of a batch straight from its lazy HeatMap (kernels.h): the
// resize / merge of resize.hip (heat_at's operations in heat_at's order, heat_dev.h), the channel
// selection and the ScaleMode epilogue of heat_copy_kernel (misc.hip) in one pass.  Every
// destination value is written once and only net-output values are read, so the full-resolution
// stack (75 MB per 656x368 frame) is neither written nor read back.
//
// The only HBM traffic is the destination, but the kernel is issue-bound, not write-bound: measured
// at 53 % (float) and 12 % (uint8) of the streaming write rate, about 0.5 T values/s either way
// (DESIGN.md §4.13).  One workgroup = HT output rows x HX output columns of one destination plane.
// Stage: lane t evaluates the horizontal pass of column t once per source row of the tile's
// footprint (<= 7 rows at x8) into the LDS window; one barrier; then lane (g, wv) = (t & 63, t >> 6)
// owns the columns 4g .. 4g + 3 of the rows wv, wv + 4, ...: it reads the four staged rows as
// float4, forms the vertical combinations, applies the epilogue and stores 16 bytes (float) or
// 4 bytes (uint8) -- a wave's store instruction covers one whole 1 KiB / 256 B row segment.
// Several sources repeat stage + combine per source (two barriers each); a footprint taller than
// the window (downsampling ratios) and CUDA map semantics evaluate every pixel on its own.
// Compiled with -ffp-contract=off like every user of heat_dev.h.
#include <algorithm>

#include "kernels.h"
#include "heat_dev.h"
#include "../common.h"

namespace opk {

namespace {

constexpr int HX = 256;     // output columns per workgroup
constexpr int HT = 32;      // output rows per workgroup
constexpr int HROWS = 16;   // footprint rows the LDS window holds
constexpr int HJ = HT / 4;  // rows per lane (4 waves)

// ScaleMode values (include/openpose/core/enumClasses.hpp:6-17), as misc.hip
constexpr int kZeroToOne = 3, kZeroToOneFixed = 4, kPlusMinusOne = 5, kPlusMinusOneFixed = 6,
              kUnsignedChar = 7, kNoScale = 8;

__device__ __forceinline__ float out_trunc01(float v, float lo)   // fastTruncate(v, lo, 1)
{
    const float m = lo > v ? lo : v;
    return 1.f < m ? 1.f : m;
}

// heat_copy_kernel's epilogue (poseExtractorNet.cpp:106-244), unchanged
__device__ __forceinline__ float out_scale(float v, int paf, int mode)
{
    if (mode == kNoScale) return v;
    if (!paf) {
        const float t = out_trunc01(v, 0.f);
        if (mode == kPlusMinusOne || mode == kPlusMinusOneFixed) return t * 2.f - 1.f;
        if (mode == kUnsignedChar) return (float)(int)(t * 255.f + 0.5f);
        return t;
    }
    const float t = out_trunc01(v, -1.f);
    if (mode == kZeroToOne || mode == kZeroToOneFixed) return t * 0.5f + 0.5f;
    if (mode == kUnsignedChar) return (float)(int)(t * 128.5f + 128.5f + 0.5f);
    return t;
}

// the float values are non-negative integers here (UnsignedChar mode); 256 and 257 saturate
__device__ __forceinline__ uint8_t out_u8(float v) { return (uint8_t)(int)(v < 255.f ? v : 255.f); }

__device__ __forceinline__ void store4(float* p, const float v[4])
{
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store4(uint8_t* p, const float v[4])
{
    *reinterpret_cast<uchar4*>(p) = make_uchar4(out_u8(v[0]), out_u8(v[1]), out_u8(v[2]), out_u8(v[3]));
}
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(uint8_t* p, float v) { *p = out_u8(v); }

struct HeatOutArgs {
    HeatMap map;
    HeatSelection sel;
    int frame0, mode;
    int vec;   // set by the launcher: rows of 4-column groups are aligned for 4-element stores
};

template <typename T>
__global__ __launch_bounds__(HX) void heat_copy_lazy_kernel(T* __restrict__ dst, const HeatOutArgs a)
{
    __shared__ float hbuf[HROWS * HX];
    const HeatMap& M = a.map;
    const int t = threadIdx.x;
    const int g = t & 63, wv = t >> 6;
    const int xb = blockIdx.x * HX;
    const int y0 = blockIdx.y * HT;
    const int y1 = min(y0 + HT, M.h);
    const int f = blockIdx.z / a.sel.nsel, c = blockIdx.z % a.sel.nsel;
    int src_c = 0, paf = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (c >= a.sel.dst0[s] && c < a.sel.dst0[s] + a.sel.count[s]) {
            src_c = a.sel.src0[s] + (c - a.sel.dst0[s]);
            paf = a.sel.paf[s];
        }
    const int plane = (a.frame0 + f) * M.channels + src_c;
    T* out = dst + (size_t)blockIdx.z * M.h * M.w;

    float acc[HJ][4];
    if (M.cuda) {
#pragma unroll
        for (int j = 0; j < HJ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int x = xb + 4 * g + i, y = y0 + wv + 4 * j;
                acc[j][i] = (x < M.w && y < y1) ? heat_at_cuda(M, plane, x, y) : 0.f;
            }
    } else {
        for (int n = 0; n < M.nsrc; ++n) {
            const ResizeSource& S = M.src[n];
            const float* src = S.src + (size_t)plane * S.sh * S.sw;
            const int r_lo = heat_clampi(S.yofs[y0] - 1, 0, S.sh - 1);
            const int r_hi = heat_clampi(S.yofs[y1 - 1] + 2, 0, S.sh - 1);
            const int nrows = r_hi - r_lo + 1;
            const bool tiled = nrows <= HROWS;   // block-uniform
            if (tiled) {
                if (n > 0) __syncthreads();   // the previous source's window was read
                const int x = xb + t;
                if (x < M.w) {
                    const int x0 = S.xofs[x];
                    const float4 cf = *reinterpret_cast<const float4*>(S.xcoef + 4 * x);
                    const float ca[4] = {cf.x, cf.y, cf.z, cf.w};
                    for (int r = 0; r < nrows; ++r)
                        hbuf[r * HX + t] = cubic_hpass(src + (size_t)(r_lo + r) * S.sw, S.sw, x0, ca);
                }
                __syncthreads();
            }
#pragma unroll
            for (int j = 0; j < HJ; ++j) {
                const int y = y0 + wv + 4 * j;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (y < y1 && xb + 4 * g < M.w) {
                    const float4 b = *reinterpret_cast<const float4*>(S.ycoef + 4 * y);
                    const int yb = S.yofs[y] - 1;
                    float h[4][4];   // [tap row][column]
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = heat_clampi(yb + k, 0, S.sh - 1);
                        if (tiled) {
                            // (M.w % 4 != 0: the group's columns past M.w were never staged;
                            // their values are computed from stale LDS and never stored)
                            const float4 q = *reinterpret_cast<const float4*>(&hbuf[(r - r_lo) * HX + 4 * g]);
                            h[k][0] = q.x; h[k][1] = q.y; h[k][2] = q.z; h[k][3] = q.w;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const int x = xb + 4 * g + i;
                                h[k][i] = 0.f;
                                if (x < M.w) {
                                    const float4 cf = *reinterpret_cast<const float4*>(S.xcoef + 4 * x);
                                    const float ca[4] = {cf.x, cf.y, cf.z, cf.w};
                                    h[k][i] = cubic_hpass(src + (size_t)r * S.sw, S.sw, S.xofs[x], ca);
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float hc[4] = {h[0][i], h[1][i], h[2][i], h[3][i]};
                        v[i] = cubic_vpass(hc, b.x, b.y, b.z, b.w,
                                           cubic_simd_column(xb + 4 * g + i, M.w));
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = (n == 0) ? v[i] : v[i] + acc[j][i];
            }
        }
        if (M.nsrc > 1)
#pragma unroll
            for (int j = 0; j < HJ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = acc[j][i] * M.inv_n;
    }

#pragma unroll
    for (int j = 0; j < HJ; ++j) {
        const int y = y0 + wv + 4 * j;
        const int x = xb + 4 * g;
        if (y >= y1 || x >= M.w) continue;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = out_scale(acc[j][i], paf, a.mode);
        T* p = out + (size_t)y * M.w + x;
        if (a.vec) {   // M.w % 4 == 0: the four columns are inside the row
            store4(p, v);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < M.w) store1(p + i, v[i]);
        }
    }
}

}  // namespace

void launch_heat_copy_lazy(void* dst, bool u8, const HeatMap& M, const HeatSelection& sel,
                           int frame0, int nframes, int scale_mode, hipStream_t stream)
{
    OPK_CHECK_ARG(dst != nullptr, "NULL destination");
    OPK_CHECK_ARG(!M.heat && M.nsrc >= 1 && M.nsrc <= kMaxResizeSources, "heat copy: 1..8 lazy sources");
    OPK_CHECK_ARG(M.h > 0 && M.w > 0 && frame0 >= 0 && nframes > 0, "empty target");
    OPK_CHECK_ARG(!u8 || scale_mode == kUnsignedChar, "uint8 heat maps need ScaleMode::UnsignedChar");
    int nsel = 0;
    for (int s = 0; s < 3; ++s) {
        OPK_CHECK_ARG(sel.count[s] >= 0 && sel.dst0[s] == nsel && sel.src0[s] >= 0 &&
                          sel.src0[s] + sel.count[s] <= M.channels,
                      "heat copy: channel selection outside the map");
        nsel += sel.count[s];
    }
    OPK_CHECK_ARG(nsel == sel.nsel && nsel > 0, "heat copy: empty channel selection");
    const unsigned gy = (unsigned)((M.h + HT - 1) / HT);
    OPK_CHECK_ARG(nsel <= 65535 && gy <= 65535, "heat copy: map too large for one launch");
    HeatOutArgs a{};
    a.map = M;
    a.sel = sel;
    a.mode = scale_mode;
    const size_t elem = u8 ? 1 : 4;
    a.vec = M.w % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % (4 * elem) == 0;
    // grid.z = planes of as many frames as fit its 65535 limit
    const int per = 65535 / nsel;
    const size_t frame_bytes = (size_t)nsel * M.h * M.w * elem;
    for (int f = 0; f < nframes; f += per) {
        const int nf = std::min(per, nframes - f);
        a.frame0 = frame0 + f;
        dim3 grid((unsigned)((M.w + HX - 1) / HX), gy, (unsigned)(nf * nsel));
        char* d = static_cast<char*>(dst) + (size_t)f * frame_bytes;
        if (u8)
            hipLaunchKernelGGL(heat_copy_lazy_kernel<uint8_t>, grid, dim3(HX), 0, stream,
                               reinterpret_cast<uint8_t*>(d), a);
        else
            hipLaunchKernelGGL(heat_copy_lazy_kernel<float>, grid, dim3(HX), 0, stream,
                               reinterpret_cast<float*>(d), a);
        OPK_LAUNCH_CHECK();
    }
}

}  // namespace opk
