// orient.hip -- the reference's rotateAndFlipFrame (--frame_rotate / --frame_flip) on a batch of
// frames (include/opk.h "ROTATED AND FLIPPED FRAMES"; the checks and the plane walk: host/orient.cpp,
// host/orient_dev.cpp).
//
// A pure permutation of samples of S = 1 (Y, U, V), 2 (NV12's UV pair) or 3 (BGR) bytes.  One plane
// of all frames per launch (the frame is grid axis z).  With the source plane S of h rows and w
// samples, mx / my the mirror of the source's x / y axis:
//   rows    D[y][x] = S[my ? h-1-y : y][mx ? w-1-x : x]            (0 and 180 degrees)
//   turn    D[y][x] = S[my ? h-1-x : x][mx ? w-1-y : y]            (90 and 270; D has w rows, h columns)
// Three kernels (dev switch ORIENT_TILE: 0 plain, 1 the dword kernels; unset: the dword kernels,
// measured faster everywhere), the dword ones only where every base, row step and
// frame stride of both sides is a multiple of 4 (frames_aligned):
//   plain        a lane per destination sample, byte loads and stores; either family.
//   orient_rows  a lane owns 4 destination samples of a row = S aligned dwords.  Mirrored, their
//                source bytes start at (w - 4g - 4) * S, which is dword aligned only when w * S is:
//                the lane loads the S + 1 aligned dwords around them, funnel-shifts by the uniform
//                byte offset and reverses the four samples in registers.  The last, partial group of
//                a row goes by bytes.
//   orient_turn  a workgroup moves a tile of 64 source columns x 64 destination columns through
//                LDS.  Tiles are cut on the source's x axis and on the destination's x axis, both at
//                multiples of 64 samples, so a tile's rows start dword aligned on both sides
//                whatever the mirrors are (a mirror only changes which rows they are).  Source rows
//                come in as dwords (consecutive lanes, consecutive dwords of a row) into LDS rows of
//                64 * S + 4 bytes; every destination dword is gathered from LDS by bytes and stored
//                whole (consecutive lanes, consecutive dwords of a destination row).  A dword that
//                holds the row's end is stored by bytes.
// A dword load may read up to 3 bytes past a row's last sample; they lie in the same aligned dword
// as a sample, so inside the row step or, for the very last row, inside the page of its last byte.
// Nothing is stored outside the samples.
#include "kernels.h"
#include "../common.h"
#include "../host/frames.h"

namespace opk {

namespace {

constexpr int kTurnTile = 64;   // samples per tile side of orient_turn

template <int S>
__device__ __forceinline__ void copy_sample(uint8_t* d, const uint8_t* s)
{
#pragma unroll
    for (int i = 0; i < S; ++i) d[i] = s[i];
}

// grid (column blocks of the destination, destination rows, frames)
template <int S, bool Turn>
__global__ __launch_bounds__(256) void orient_plain(OrientPlane p)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= (Turn ? p.h : p.w)) return;
    int sx = Turn ? y : x, sy = Turn ? x : y;
    if (p.mx) sx = p.w - 1 - sx;
    if (p.my) sy = p.h - 1 - sy;
    copy_sample<S>(p.dst + (size_t)f * p.dframe + (size_t)y * p.dstep + (size_t)x * S,
                   p.src + (size_t)f * p.sframe + (size_t)sy * p.sstep + (size_t)sx * S);
}

// the four samples held in S dwords, in reverse order
template <int S>
__device__ __forceinline__ void reverse4(unsigned (&u)[S])
{
    if constexpr (S == 1) {
        u[0] = __builtin_bswap32(u[0]);
    } else if constexpr (S == 2) {
        const unsigned a = u[0], b = u[1];
        u[0] = b >> 16 | b << 16;
        u[1] = a >> 16 | a << 16;
    } else {
        const unsigned p0 = u[0] & 0xffffffu, p1 = u[0] >> 24 | (u[1] & 0xffffu) << 8;
        const unsigned p2 = u[1] >> 16 | (u[2] & 0xffu) << 16, p3 = u[2] >> 8;
        u[0] = p3 | p2 << 24;
        u[1] = p2 >> 8 | p1 << 16;
        u[2] = p1 >> 16 | p0 << 8;
    }
}

// grid (blocks of 256 groups of 4 samples, rows, frames); both sides 4-byte aligned
template <int S>
__global__ __launch_bounds__(256) void orient_rows(OrientPlane p)
{
    const int g = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    const int x0 = 4 * g;
    if (x0 >= p.w) return;
    const int sy = p.my ? p.h - 1 - y : y;
    const uint8_t* srow = p.src + (size_t)f * p.sframe + (size_t)sy * p.sstep;
    uint8_t* d = p.dst + (size_t)f * p.dframe + (size_t)y * p.dstep + (size_t)x0 * S;
    if (p.w - x0 < 4) {   // the row's tail: by bytes
        for (int i = 0; i < p.w - x0; ++i) {
            const int sx = p.mx ? p.w - 1 - (x0 + i) : x0 + i;
            copy_sample<S>(d + i * S, srow + (size_t)sx * S);
        }
        return;
    }
    // the group's 4 * S source bytes start at b0 >= 0; dword k of the row holds a sample while
    // 4 * k < w * S
    const int row_bytes = p.w * S;
    const int b0 = (p.mx ? p.w - x0 - 4 : x0) * S;
    const int k0 = b0 >> 2;
    const unsigned sh = (unsigned)(b0 & 3) * 8u;
    const unsigned* s4 = reinterpret_cast<const unsigned*>(srow);
    unsigned v[S + 1];
#pragma unroll
    for (int i = 0; i <= S; ++i) v[i] = 4 * (k0 + i) < row_bytes ? s4[k0 + i] : 0u;
    unsigned u[S];
#pragma unroll
    for (int i = 0; i < S; ++i)
        u[i] = (unsigned)((((unsigned long long)v[i + 1] << 32) | v[i]) >> sh);
    if (p.mx) reverse4<S>(u);
    unsigned* d4 = reinterpret_cast<unsigned*>(d);
#pragma unroll
    for (int i = 0; i < S; ++i) d4[i] = u[i];
}

// grid (tiles over the source's x, tiles over the destination's x = the source's y, frames); both
// sides 4-byte aligned
template <int S>
__global__ __launch_bounds__(256) void orient_turn(OrientPlane p)
{
    constexpr int T = kTurnTile;
    constexpr int DW = T * S / 4;      // dwords of a tile row, on either side
    constexpr int P = T * S + 4;       // bytes of an LDS row
    __shared__ __attribute__((aligned(16))) uint8_t tile[T * P];
    const int x0 = blockIdx.x * T;     // first source column
    const int X0 = blockIdx.y * T;     // first destination column
    const int f = blockIdx.z;
    const uint8_t* fsrc = p.src + (size_t)f * p.sframe;
    uint8_t* fdst = p.dst + (size_t)f * p.dframe;
    const int src_bytes = p.w * S, dst_bytes = p.h * S;

    // LDS row r = destination column X0 + r = source row (my ? h-1-X : X), its bytes from x0 * S
#pragma unroll 4
    for (int idx = threadIdx.x; idx < T * DW; idx += 256) {
        const int r = idx / DW, k = idx - r * DW;
        const int X = X0 + r, at = x0 * S + 4 * k;
        if (X >= p.h || at >= src_bytes) continue;
        const int sy = p.my ? p.h - 1 - X : X;
        *reinterpret_cast<unsigned*>(tile + r * P + 4 * k) =
            *reinterpret_cast<const unsigned*>(fsrc + (size_t)sy * p.sstep + at);
    }
    __syncthreads();
    // destination row of source column x0 + c: (mx ? w-1-sx : sx), its bytes from X0 * S; byte b of
    // them is component b % S of LDS row b / S
#pragma unroll 4
    for (int idx = threadIdx.x; idx < T * DW; idx += 256) {
        const int c = idx / DW, j = idx - c * DW;
        const int sx = x0 + c, at = X0 * S + 4 * j;
        if (sx >= p.w || at >= dst_bytes) continue;
        const int Y = p.mx ? p.w - 1 - sx : sx;
        uint8_t* d = fdst + (size_t)Y * p.dstep + at;
        const uint8_t* col = tile + c * S;
        const int valid = min(4, dst_bytes - at);
        unsigned q = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = 4 * j + e;
            if (e < valid) q |= (unsigned)col[(b / S) * P + b % S] << (8 * e);
        }
        if (valid == 4) {
            *reinterpret_cast<unsigned*>(d) = q;
        } else {
            for (int e = 0; e < valid; ++e) d[e] = (uint8_t)(q >> (8 * e));
        }
    }
}

template <int S>
void launch_plane(const OrientPlane& p, bool turn, bool tiled, int n, hipStream_t stream)
{
    const int dw = turn ? p.h : p.w, dh = turn ? p.w : p.h;
    if (!tiled) {
        const dim3 grid((unsigned)((dw + 255) / 256), (unsigned)dh, (unsigned)n);
        note_launch("orient_plain<%d,%s>", S, turn ? "turn" : "rows");
        if (turn) hipLaunchKernelGGL((orient_plain<S, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((orient_plain<S, false>), grid, dim3(256), 0, stream, p);
    } else if (turn) {
        const dim3 grid((unsigned)((p.w + kTurnTile - 1) / kTurnTile),
                        (unsigned)((p.h + kTurnTile - 1) / kTurnTile), (unsigned)n);
        note_launch("orient_turn<%d>", S);
        hipLaunchKernelGGL(orient_turn<S>, grid, dim3(256), 0, stream, p);
    } else {
        const dim3 grid((unsigned)(((p.w + 3) / 4 + 255) / 256), (unsigned)p.h, (unsigned)n);
        note_launch("orient_rows<%d>", S);
        hipLaunchKernelGGL(orient_rows<S>, grid, dim3(256), 0, stream, p);
    }
    OPK_LAUNCH_CHECK();
}

}  // namespace

bool orient_tiled(const FrameDest& dst, const FrameSource& src)
{
    if (!frames_aligned(dst, 4) || !frames_aligned(src, 4)) return false;
    // unset: the dword kernels, measured faster for every sample size and both families (DESIGN.md
    // 4.19: 2.0 to 2.3 times the plain kernel on rows, 6 to 7 times on turns)
    return dev_switch("ORIENT_TILE", 1) != 0;
}

void launch_orient_frames(const FrameDest& dst, const FrameSource& src, bool turn, bool mx, bool my,
                          hipStream_t stream)
{
    OPK_CHECK_ARG(src.n > 0 && src.w > 0 && src.h > 0, "empty frame");
    OPK_CHECK_ARG(dst.format == src.format && dst.n == src.n, "format or frame count differs");
    OPK_CHECK_ARG(dst.w == (turn ? src.h : src.w) && dst.h == (turn ? src.w : src.h),
                  "the destination's size is not the oriented size");
    OPK_CHECK_ARG(dst.plane[0] && src.plane[0], "NULL plane");
    check_frames(dst);
    check_frames(src);
    // grid axes y and z: rows (plain, rows: of the destination) and frames
    OPK_CHECK_ARG(src.w <= 65535 && src.h <= 65535 && src.n <= 65535,
                  "more than 65535 rows, columns or frames");
    const bool tiled = orient_tiled(dst, src);
    auto plane = [&](int i, size_t sstep, size_t dstep, int w, int h) {
        OrientPlane p{};
        p.src = src.plane[i];
        p.dst = dst.plane[i];
        p.sstep = sstep;
        p.sframe = src.frame[i];
        p.dstep = dstep;
        p.dframe = dst.frame[i];
        p.w = w;
        p.h = h;
        p.mx = mx ? 1 : 0;
        p.my = my ? 1 : 0;
        return p;
    };
    if (src.format == kFramesBgr) {
        launch_plane<3>(plane(0, src.step, dst.step, src.w, src.h), turn, tiled, src.n, stream);
        return;
    }
    launch_plane<1>(plane(0, src.step, dst.step, src.w, src.h), turn, tiled, src.n, stream);
    if (src.format == kFramesNv12) {
        launch_plane<2>(plane(1, src.cstep, dst.cstep, src.w / 2, src.h / 2), turn, tiled, src.n, stream);
    } else {
        launch_plane<1>(plane(1, src.cstep, dst.cstep, src.w / 2, src.h / 2), turn, tiled, src.n, stream);
        launch_plane<1>(plane(2, src.cstep, dst.cstep, src.w / 2, src.h / 2), turn, tiled, src.n, stream);
    }
}

}  // namespace opk
