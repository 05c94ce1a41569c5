// yuv.hip -- YUV 4:2:0 frames (NV12, I420) as the decoders leave them: the standalone conversion to
// BGR (opk_frames_to_bgr), the frame -> net input warp of input.hip reading YUV directly, and the
// standalone conversion back for the encoders (opk_bgr_to_frames; the arithmetic: yuv_out_dev.h).
//
// The conversion is the integer arithmetic of yuv_dev.h; the warps convert what they read with it
// and then sum exactly the integers input.hip sums, so the net input is bit for bit the warp of the
// converted frames without the 3 byte/pixel write and read of a BGR copy: 1.5 bytes per source
// pixel instead of 3.  Taps outside the image contribute BGR 0, as in input.hip -- not YUV 0.
#include "kernels.h"
#include "warp_dev.h"
#include "yuv_dev.h"
#include "yuv_out_dev.h"
#include "../common.h"
#include "../host/frames.h"

namespace opk {

namespace {

// byte j of a 16-byte load
__device__ __forceinline__ int byte_of(const uint4& q, int j)
{
    const unsigned w = j < 4 ? q.x : (j < 8 ? q.y : (j < 12 ? q.z : q.w));
    return (int)((w >> (8 * (j & 3))) & 255u);
}

// the chroma terms of the 8 sample pairs that go with 16 luma pixels from column x (a multiple of
// 16) of a row: one 16-byte load of interleaved pairs (NV12) or two 8-byte loads (I420)
__device__ __forceinline__ void chroma16(YuvChroma k[8], const YuvRow& r, int x)
{
    if (r.cpix == 2) {
        const uint4 q = *reinterpret_cast<const uint4*>(r.u + x);
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = yuv_chroma(byte_of(q, 2 * i), byte_of(q, 2 * i + 1));
    } else {
        const uint2 a = *reinterpret_cast<const uint2*>(r.u + (x >> 1));
        const uint2 b = *reinterpret_cast<const uint2*>(r.v + (x >> 1));
        const uint4 q{a.x, a.y, b.x, b.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) k[i] = yuv_chroma(byte_of(q, i), byte_of(q, 8 + i));
    }
}

// 16 luma pixels with their chroma terms -> 48 BGR bytes
__device__ __forceinline__ void bgr16(uint4 out[3], const uint4& luma, const YuvChroma k[8])
{
    unsigned w[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) {   // four pixels -> three words
        unsigned p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = yuv_pixel_packed(byte_of(luma, 4 * g + i), k[2 * g + (i >> 1)]);
        w[3 * g] = p[0] | p[1] << 24;
        w[3 * g + 1] = p[1] >> 8 | p[2] << 16;
        w[3 * g + 2] = p[2] >> 16 | p[3] << 8;
    }
    out[0] = uint4{w[0], w[1], w[2], w[3]};
    out[1] = uint4{w[4], w[5], w[6], w[7]};
    out[2] = uint4{w[8], w[9], w[10], w[11]};
}

// the 2 x 1 pixels from even column x of a row -> 6 BGR bytes at d, byte loads and stores
__device__ __forceinline__ void bgr2(uint8_t* d, const YuvRow& r, int x)
{
    const int o = (x >> 1) * r.cpix;
    const YuvChroma k = yuv_chroma(r.u[o], r.v[o]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int c[3];
        yuv_pixel(c, r.y[x + i], k);
        d[3 * i] = (uint8_t)c[0];
        d[3 * i + 1] = (uint8_t)c[1];
        d[3 * i + 2] = (uint8_t)c[2];
    }
}

// ---- the standalone conversion -------------------------------------------------------------------
// grid (column groups, row pairs, frames).  A lane converts two rows of 16 pixels (V: source rows,
// chroma rows, destination rows and all frame strides on 16-byte boundaries): three 16-byte loads
// (four for I420), one set of chroma terms for both rows, six 16-byte stores; the columns past the
// last whole group -- and everything when V is off -- go as 2 x 2 blocks with byte accesses.
template <bool V>
__global__ __launch_bounds__(256) void yuv420_to_bgr_kernel(uint8_t* __restrict__ dst,
                                                            size_t dst_step, FrameSource fs)
{
    const int f = blockIdx.z, y0 = 2 * blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const YuvRow r0 = yuv_row(fs, f, y0), r1 = yuv_row(fs, f, y0 + 1);
    uint8_t* d0 = dst + ((size_t)f * fs.h + y0) * dst_step;
    uint8_t* d1 = d0 + dst_step;
    int x = V ? 16 * i : 2 * i;
    if (x >= fs.w) return;
    if (V && x + 16 <= fs.w) {
        YuvChroma k[8];
        chroma16(k, r0, x);
        uint4 o[3];
        bgr16(o, *reinterpret_cast<const uint4*>(r0.y + x), k);
        uint4* q = reinterpret_cast<uint4*>(d0 + (size_t)x * 3);
        q[0] = o[0];
        q[1] = o[1];
        q[2] = o[2];
        bgr16(o, *reinterpret_cast<const uint4*>(r1.y + x), k);
        q = reinterpret_cast<uint4*>(d1 + (size_t)x * 3);
        q[0] = o[0];
        q[1] = o[1];
        q[2] = o[2];
        return;
    }
    const int end = V ? fs.w : x + 2;   // (w is even)
    for (; x < end; x += 2) {
        bgr2(d0 + (size_t)x * 3, r0, x);
        bgr2(d1 + (size_t)x * 3, r1, x);
    }
}

// ---- the standalone conversion back: BGR -> NV12 / I420 (yuv_out_dev.h) ---------------------------
// The same grid and the same two routes.  V: a lane converts two rows of 16 pixels -- six 16-byte
// loads, 32 luma samples, and the (U, V) of the eight top-left pixels of its blocks -- and stores
// two 16-byte luma pieces and one 16-byte piece of interleaved pairs (NV12) or two 8-byte pieces
// (I420); source rows, every destination row and all frame strides lie on such boundaries.  The
// columns past the last whole group -- and everything when V is off -- go as 2 x 2 blocks, bytes.

// the 16 pixels of 48 BGR bytes: luma words, and (top) the chroma samples of pixels 0, 2, .. 14
template <bool Top>
__device__ __forceinline__ uint4 yuv16(const uint4 q[3], unsigned u[8], unsigned v[8])
{
    const uint4 all[3] = {q[0], q[1], q[2]};
    unsigned y[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int b = byte_of(all[(3 * p) >> 4], (3 * p) & 15);
        const int g = byte_of(all[(3 * p + 1) >> 4], (3 * p + 1) & 15);
        const int r = byte_of(all[(3 * p + 2) >> 4], (3 * p + 2) & 15);
        y[p >> 2] |= bgr_to_y(b, g, r) << (8 * (p & 3));
        if (Top && (p & 1) == 0) {
            u[p >> 1] = bgr_to_u(b, g, r);
            v[p >> 1] = bgr_to_v(b, g, r);
        }
    }
    return uint4{y[0], y[1], y[2], y[3]};
}

// the 2 x 2 block at even column x of rows s0 / s1 (BGR bytes) -> four luma bytes, one (U, V)
__device__ __forceinline__ void yuv_block(const YuvRowT<uint8_t>& r0, const YuvRowT<uint8_t>& r1,
                                          const uint8_t* s0, const uint8_t* s1, int x)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint8_t* a = s0 + 3 * (x + i);
        const uint8_t* b = s1 + 3 * (x + i);
        r0.y[x + i] = (uint8_t)bgr_to_y(a[0], a[1], a[2]);
        r1.y[x + i] = (uint8_t)bgr_to_y(b[0], b[1], b[2]);
    }
    const uint8_t* a = s0 + 3 * x;
    const int o = (x >> 1) * r0.cpix;
    r0.u[o] = (uint8_t)bgr_to_u(a[0], a[1], a[2]);
    r0.v[o] = (uint8_t)bgr_to_v(a[0], a[1], a[2]);
}

template <bool V>
__global__ __launch_bounds__(256) void bgr_to_yuv420_kernel(FrameDest dst, FrameSource fs)
{
    const int f = blockIdx.z, y0 = 2 * blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint8_t* s0 = fs.plane[0] + (size_t)f * fs.frame[0] + (size_t)y0 * fs.step;
    const uint8_t* s1 = s0 + fs.step;
    const YuvRowT<uint8_t> r0 = yuv_row(dst, f, y0), r1 = yuv_row(dst, f, y0 + 1);
    int x = V ? 16 * i : 2 * i;
    if (x >= fs.w) return;
    if (V && x + 16 <= fs.w) {
        unsigned u[8], v[8];
        const uint4* q0 = reinterpret_cast<const uint4*>(s0 + (size_t)x * 3);
        const uint4* q1 = reinterpret_cast<const uint4*>(s1 + (size_t)x * 3);
        const uint4 a[3] = {q0[0], q0[1], q0[2]}, b[3] = {q1[0], q1[1], q1[2]};
        *reinterpret_cast<uint4*>(r0.y + x) = yuv16<true>(a, u, v);
        *reinterpret_cast<uint4*>(r1.y + x) = yuv16<false>(b, u, v);
        if (dst.cpix == 2) {
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = u[2 * k] | v[2 * k] << 8 | u[2 * k + 1] << 16 | v[2 * k + 1] << 24;
            *reinterpret_cast<uint4*>(r0.u + x) = uint4{w[0], w[1], w[2], w[3]};
        } else {
            unsigned wu[2], wv[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                wu[k] = u[4 * k] | u[4 * k + 1] << 8 | u[4 * k + 2] << 16 | u[4 * k + 3] << 24;
                wv[k] = v[4 * k] | v[4 * k + 1] << 8 | v[4 * k + 2] << 16 | v[4 * k + 3] << 24;
            }
            *reinterpret_cast<uint2*>(r0.u + (x >> 1)) = uint2{wu[0], wu[1]};
            *reinterpret_cast<uint2*>(r0.v + (x >> 1)) = uint2{wv[0], wv[1]};
        }
        return;
    }
    const int end = V ? fs.w : x + 2;   // (w is even)
    for (; x < end; x += 2) yuv_block(r0, r1, s0, s1, x);
}

// ---- the warp, direct: input.hip's cvmat_to_input_kernel converting every tap it reads -----------
template <int K>
__global__ __launch_bounds__(256) void cvmat_to_input_yuv_kernel(
    float* __restrict__ dst, FrameSource fs, int dh, int dw, const int2* __restrict__ xtab,
    const int2* __restrict__ ytab, const short* __restrict__ wtab, int normalize,
    const int* __restrict__ frame_of, int tab_stride)
{
    const int y = blockIdx.x % dh;
    const int f = blockIdx.x / dh;
    xtab += (size_t)f * tab_stride;
    ytab += (size_t)f * tab_stride;
    const int2 yt = ytab[y];
    const int sf = frame_of ? frame_of[f] : f;
    const size_t plane = (size_t)dh * dw;
    float* out = dst + (size_t)f * 3 * plane + (size_t)y * dw;
    for (int x = threadIdx.x; x < dw; x += blockDim.x) {
        const int2 xt = xtab[x];
        int u[3];
        warp_pixel<K>(u, yt, xt, warp_weights<K>(wtab, yt.y, xt.y), fs.h, fs.w,
                      [&](int, int yy) { return yuv_row(fs, sf, yy); });
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)u[c];
            if (normalize) v = v * (1.f / 256.f) - 0.5f;   // exact for u in [0, 255]
            out[(size_t)c * plane + x] = v;
        }
    }
}

// ---- the warp, staged: input.hip's cvmat_to_input_lds_kernel with the same LDS layout -- the x
// table, the 32 weight sets, K rows of BGR bytes -- whose rows are converted on the way in: a lane
// loads luma and chroma of a run of pixels (A16: 16 pixels, 16-byte loads, three 16-byte LDS
// stores; else 2 pixels, bytes), converts each pixel once and stores BGR, all behind the one
// barrier; tap row yy takes chroma row yy >> 1.  The tap loop is input.hip's, on the same bytes.
// Staged columns [c0, c1) are whole chroma pairs (the width is even) inside the image, so a row
// needs at most 3 * sw bytes: input.hip's lds_row and 64 KB gate hold unchanged.
template <int K, bool A16>
__global__ __launch_bounds__(256) void cvmat_to_input_lds_yuv_kernel(
    float* __restrict__ dst, FrameSource fs, int dh, int dw, const int2* __restrict__ xtab,
    const int2* __restrict__ ytab, const short* __restrict__ wtab, int normalize,
    const int* __restrict__ frame_of, int tab_stride, int lds_row, int rows_at)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int2* xs = reinterpret_cast<int2*>(smem);                      // [dw]
    short* ws = reinterpret_cast<short*>(smem + (size_t)dw * 8);   // [32][K][K]
    uint8_t* rows = smem + rows_at;                                // [K][lds_row]
    const int sh = fs.h, sw = fs.w;
    const int y = blockIdx.x % dh;
    const int f = blockIdx.x / dh;
    xtab += (size_t)f * tab_stride;
    ytab += (size_t)f * tab_stride;
    const int2 yt = ytab[y];
    const int x_a = xtab[0].x, x_b = xtab[dw - 1].x;
    for (int x = threadIdx.x; x < dw; x += blockDim.x) xs[x] = xtab[x];
    for (int i = threadIdx.x; i < 32 * K * K; i += blockDim.x) ws[i] = wtab[yt.y * 32 * K * K + i];
    const int lo = max(min(x_a, x_b), 0), hi = min(max(x_a, x_b) + K, sw);   // source columns
    const int sf = frame_of ? frame_of[f] : f;
    const int c0 = A16 ? lo & ~15 : lo & ~1;        // first staged column of a row
    const int c1 = hi > lo ? (hi + 1) & ~1 : c0;    // one past the last (<= sw)
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const int yy = yt.x + ky;
        if (yy < 0 || yy >= sh) continue;   // never read: the taps test the row below
        uint8_t* l = rows + ky * lds_row;
        const YuvRow r = yuv_row(fs, sf, yy);
        int tail = c0;
        if (A16) {
            const int full = (c1 - c0) >> 4;   // whole 16-pixel pieces (c1 <= sw: inside the row)
            for (int i = threadIdx.x; i < full; i += blockDim.x) {
                const int x = c0 + 16 * i;
                YuvChroma k[8];
                chroma16(k, r, x);
                uint4 o[3];
                bgr16(o, *reinterpret_cast<const uint4*>(r.y + x), k);
                uint4* d = reinterpret_cast<uint4*>(l + i * 48);
                d[0] = o[0];
                d[1] = o[1];
                d[2] = o[2];
            }
            tail += full * 16;
        }
        for (int x = tail + 2 * threadIdx.x; x < c1; x += 2 * blockDim.x) bgr2(l + (x - c0) * 3, r, x);
    }
    __syncthreads();
    const size_t plane = (size_t)dh * dw;
    float* out = dst + (size_t)f * 3 * plane + (size_t)y * dw;
    for (int x = threadIdx.x; x < dw; x += blockDim.x) {
        const int2 xt = xs[x];
        int u[3];
        warp_pixel<K>(u, yt, xt, warp_weights<K>(ws, 0, xt.y), sh, sw, [&](int ky, int) {
            return static_cast<const uint8_t*>(rows + ky * lds_row - c0 * 3);
        });
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)u[c];
            if (normalize) v = v * (1.f / 256.f) - 0.5f;   // exact for u in [0, 255]
            out[(size_t)c * plane + x] = v;
        }
    }
}

// a YUV source of a launcher here: not BGR, not empty, and check_frames' layout (host/frames.h)
void check_yuv(const FrameSource& fs)
{
    OPK_CHECK_ARG(fs.format != kFramesBgr, "unknown frame format");
    OPK_CHECK_ARG(fs.n > 0 && fs.w > 0 && fs.h > 0, "empty frame");
    check_frames(fs);
}

}  // namespace

void launch_frames_to_bgr(uint8_t* dst, size_t dst_step, const FrameSource& fs, hipStream_t stream)
{
    check_yuv(fs);
    OPK_CHECK_ARG(dst != nullptr, "NULL buffer");
    OPK_CHECK_ARG(dst_step >= (size_t)fs.w * 3, "row step shorter than the row");
    OPK_CHECK_ARG(fs.h / 2 <= 65535 && fs.n <= 65535, "more than 65535 row pairs or frames");
    const bool vec = frames_aligned(fs, 16) && (uintptr_t)dst % 16 == 0 && dst_step % 16 == 0;
    const int lanes = vec ? (fs.w + 15) / 16 : fs.w / 2;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)(fs.h / 2), (unsigned)fs.n);
    if (vec) {
        note_launch("yuv420_to_bgr<v16>");
        hipLaunchKernelGGL(yuv420_to_bgr_kernel<true>, grid, dim3(256), 0, stream, dst, dst_step, fs);
    } else {
        note_launch("yuv420_to_bgr");
        hipLaunchKernelGGL(yuv420_to_bgr_kernel<false>, grid, dim3(256), 0, stream, dst, dst_step,
                           fs);
    }
    OPK_LAUNCH_CHECK();
}

void launch_bgr_to_frames(const FrameDest& dst, const FrameSource& fs, hipStream_t stream)
{
    // this site's own checks first and in the order they always had (a BGR destination before an
    // empty batch, both before a size mismatch); check_frames' layout checks come after them
    OPK_CHECK_ARG(fs.format == kFramesBgr, "the source frames are BGR");
    OPK_CHECK_ARG(dst.format != kFramesBgr, "unknown frame format");
    OPK_CHECK_ARG(fs.n > 0 && fs.w > 0 && fs.h > 0, "empty frame");
    OPK_CHECK_ARG(dst.n == fs.n && dst.w == fs.w && dst.h == fs.h, "frame count or size differs");
    OPK_CHECK_ARG(fs.plane[0] != nullptr, "NULL plane");
    check_frames(dst);
    check_frames(fs);
    OPK_CHECK_ARG(fs.h / 2 <= 65535 && fs.n <= 65535, "more than 65535 row pairs or frames");
    // both sides move as 16-pixel pieces: 48 source bytes, 16 of luma, 16 (NV12) or 8 + 8 of chroma
    const bool vec = frames_aligned(dst, 16) && frames_aligned(fs, 16);
    const int lanes = vec ? (fs.w + 15) / 16 : fs.w / 2;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)(fs.h / 2), (unsigned)fs.n);
    if (vec) {
        note_launch("bgr_to_yuv420<v16>");
        hipLaunchKernelGGL(bgr_to_yuv420_kernel<true>, grid, dim3(256), 0, stream, dst, fs);
    } else {
        note_launch("bgr_to_yuv420");
        hipLaunchKernelGGL(bgr_to_yuv420_kernel<false>, grid, dim3(256), 0, stream, dst, fs);
    }
    OPK_LAUNCH_CHECK();
}

void launch_cvmat_to_input_yuv(float* dst, const FrameSource& fs, int n, int dh, int dw,
                               const int* xtab, const int* ytab, const short* wtab, int ksize,
                               int normalize, hipStream_t stream, const int* frame_of,
                               int tab_stride)
{
    check_yuv(fs);
    const int sw = fs.w;
    const dim3 grid((unsigned)(n * dh));
    const int threads = dw >= 256 ? 256 : (dw >= 128 ? 128 : 64);
    const auto* xt = reinterpret_cast<const int2*>(xtab);
    const auto* yt = reinterpret_cast<const int2*>(ytab);
    // input.hip's layout and gate: the staged rows hold BGR bytes
    const int lds_row = ((sw * 3 + 32) + 15) & ~15;
    const size_t rows_at = ((size_t)dw * 8 + 64 * ksize * ksize + 15) & ~(size_t)15;
    const size_t lds = rows_at + (size_t)ksize * lds_row;
    if (lds <= 64 * 1024) {
        const bool a16 = frames_aligned(fs, 16);
#define OPK_WARP_LDS(K_, A_)                                                                      \
    hipLaunchKernelGGL((cvmat_to_input_lds_yuv_kernel<K_, A_>), grid, dim3(threads), lds, stream, \
                       dst, fs, dh, dw, xt, yt, wtab, normalize, frame_of, tab_stride, lds_row,    \
                       (int)rows_at)
        if (ksize == 2) {
            if (a16) { note_launch("cvmat_to_input_lds<2,a16,yuv>"); OPK_WARP_LDS(2, true); }
            else { note_launch("cvmat_to_input_lds<2,yuv>"); OPK_WARP_LDS(2, false); }
        } else {
            if (a16) { note_launch("cvmat_to_input_lds<4,a16,yuv>"); OPK_WARP_LDS(4, true); }
            else { note_launch("cvmat_to_input_lds<4,yuv>"); OPK_WARP_LDS(4, false); }
        }
#undef OPK_WARP_LDS
        OPK_LAUNCH_CHECK();
        return;
    }
    if (ksize == 2) {
        note_launch("cvmat_to_input<2,yuv>");
        hipLaunchKernelGGL(cvmat_to_input_yuv_kernel<2>, grid, dim3(threads), 0, stream, dst, fs, dh,
                           dw, xt, yt, wtab, normalize, frame_of, tab_stride);
    } else {
        note_launch("cvmat_to_input<4,yuv>");
        hipLaunchKernelGGL(cvmat_to_input_yuv_kernel<4>, grid, dim3(threads), 0, stream, dst, fs, dh,
                           dw, xt, yt, wtab, normalize, frame_of, tab_stride);
    }
    OPK_LAUNCH_CHECK();
}

}  // namespace opk
