// jpeg_dev.cpp -- the device route of the JPEG frames (include/opk.h): the checks that come before
// any device work, the tables' device copy, the chunk walk with its scratch, and opk_jpeg_encode.
#include <algorithm>
#include <memory>

#include "../../../include/opk.h"
#include "../common.h"
#include "context.h"
#include "frames.h"
#include "jpeg.h"

namespace opk {

namespace {

// The scratch of one chunk.  Per frame of M = ceil(w / 16) * ceil(h / 16) MCUs: 768 M bytes of
// coefficients, 12 M of block bit counts, the bit stream at its bound (1245 M bytes, rounded up to
// kJpegPackBytes) and a few bytes per segment and piece -- 7.3 MB for 1280 x 720 (2.8 MB of them
// coefficients).  A chunk is as many frames as fit kJpegScratchBytes, 16 at the most and one at the
// least: 16 frames and 117 MB at 1280 x 720.
constexpr size_t kJpegScratchBytes = (size_t)256 << 20;
constexpr int kJpegChunkFrames = 16;

struct Layout {
    size_t coef, blockbits, segbits, segstart, raw, rawbytes, ffcount, ffstart, fits, total;
};
size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
Layout layout(int frames, int mcus, int segs, int pieces, size_t rawcap)
{
    Layout l{};
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at = up(at + bytes, 256);
        return here;
    };
    const size_t n = (size_t)frames;
    l.coef = take(n * (size_t)mcus * 768);
    l.blockbits = take(n * (size_t)mcus * 12);
    l.segbits = take(n * (size_t)segs * 4);
    l.segstart = take(n * ((size_t)segs + 1) * 8);
    l.raw = take(n * rawcap);
    l.rawbytes = take(n * 8);
    l.ffcount = take(n * (size_t)pieces * 4);
    l.ffstart = take(n * (size_t)pieces * 8);
    l.fits = take(n * 4);
    l.total = at;
    return l;
}

const JpegTables* device_tables(Context* ctx, int w, int h, int quality, hipStream_t stream)
{
    const bool have = ctx->jpeg_tables.ptr && ctx->jpeg_key[0] == w && ctx->jpeg_key[1] == h &&
                      ctx->jpeg_key[2] == quality;
    if (!have) {   // once per (w, h, quality); the copy is waited for, so `host` may go
        auto host = std::make_unique<JpegTables>();
        make_jpeg_tables(*host, w, h, quality);
        void* dev = ctx->jpeg_tables.get(sizeof(JpegTables));
        OPK_HIP(hipMemcpyAsync(dev, host.get(), sizeof(JpegTables), hipMemcpyHostToDevice, stream));
        OPK_HIP(hipStreamSynchronize(stream));
        ctx->jpeg_key[0] = w;
        ctx->jpeg_key[1] = h;
        ctx->jpeg_key[2] = quality;
    }
    return static_cast<const JpegTables*>(ctx->jpeg_tables.ptr);
}

// the bytes from the first sample of the first frame to one past the last sample of the last frame
void source_extent(const FrameSource& s, int plane, size_t step, size_t rows, size_t row,
                   const uint8_t** lo, size_t* bytes)
{
    *lo = s.plane[plane];
    *bytes = (size_t)(s.n - 1) * s.frame[plane] + (rows - 1) * step + row;
}

}  // namespace

void jpeg_encode(Context* ctx, uint8_t* dst, size_t capacity, uint64_t* offsets,
                 const FrameSource& src, int quality, hipStream_t stream)
{
    check_jpeg(src.w, src.h, quality);
    if (src.n == 0) return;
    OPK_CHECK_ARG(dst && offsets && src.plane[0], "NULL buffer");
    OPK_CHECK_ARG((uintptr_t)offsets % 8 == 0, "offsets must be 8-byte aligned");
    check_frames(src);
    {
        const size_t w = (size_t)src.w, h = (size_t)src.h;
        const uint8_t* lo;
        size_t bytes;
        if (src.format == kFramesBgr) {
            source_extent(src, 0, src.step, h, w * 3, &lo, &bytes);
            check_jpeg_apart(dst, capacity, lo, bytes);
        } else {
            source_extent(src, 0, src.step, h, w, &lo, &bytes);
            check_jpeg_apart(dst, capacity, lo, bytes);
            const bool nv12 = src.format == kFramesNv12;
            source_extent(src, 1, src.cstep, h / 2, nv12 ? w : w / 2, &lo, &bytes);
            check_jpeg_apart(dst, capacity, lo, bytes);
            if (!nv12) {
                source_extent(src, 2, src.cstep, h / 2, w / 2, &lo, &bytes);
                check_jpeg_apart(dst, capacity, lo, bytes);
            }
        }
    }
    ctx->bind();

    const JpegGeom g = jpeg_geom(src.w, src.h);
    const size_t mcus64 = (size_t)g.mw * (size_t)g.mh;
    OPK_CHECK_ARG(mcus64 * 6 < ((size_t)1 << 31), "frame too large for the block index");
    const int mcus = (int)mcus64;
    const int segs = (mcus + kJpegSegMcus - 1) / kJpegSegMcus;
    const size_t rawcap = up((mcus64 * 6 * kJpegMaxBlockBits + 7) / 8 + 4, kJpegPackBytes);
    OPK_CHECK_ARG(rawcap / kJpegPackBytes < ((size_t)1 << 31), "frame too large for the piece index");
    const int pieces = (int)(rawcap / kJpegPackBytes);
    const size_t per_frame = layout(1, mcus, segs, pieces, rawcap).total;
    const int chunk = (int)std::min<size_t>(
        (size_t)std::min(src.n, kJpegChunkFrames), std::max<size_t>(1, kJpegScratchBytes / per_frame));
    const Layout l = layout(chunk, mcus, segs, pieces, rawcap);
    uint8_t* scratch = static_cast<uint8_t*>(ctx->jpeg_scratch.get(l.total));
    const bool yuv = src.format != kFramesBgr;
    uint8_t* bgr = nullptr;
    const size_t bgr_step = up((size_t)src.w * 3, 4), bgr_frame = bgr_step * (size_t)src.h;
    if (yuv) bgr = static_cast<uint8_t*>(ctx->jpeg_bgr.get(bgr_frame * (size_t)chunk));
    const JpegTables* tab = device_tables(ctx, src.w, src.h, quality, stream);

    for (int first = 0; first < src.n; first += chunk) {
        JpegJob j{};
        j.frames = std::min(chunk, src.n - first);
        if (yuv) {   // the file of opk_frames_to_bgr(frames)
            FrameSource part = src;
            part.n = j.frames;
            for (int p = 0; p < 3; ++p) part.plane[p] = src.plane[p] + (size_t)first * src.frame[p];
            launch_frames_to_bgr(bgr, bgr_step, part, stream);
            j.bgr = bgr;
            j.step = bgr_step;
            j.frame = bgr_frame;
        } else {
            j.bgr = src.plane[0] + (size_t)first * src.frame[0];
            j.step = src.step;
            j.frame = src.frame[0];
        }
        j.w = src.w;
        j.h = src.h;
        j.first = first;
        j.mcus = mcus;
        j.segs = segs;
        j.pieces = pieces;
        j.rawcap = rawcap;
        j.tab = tab;
        j.coef = reinterpret_cast<short*>(scratch + l.coef);
        j.blockbits = reinterpret_cast<unsigned short*>(scratch + l.blockbits);
        j.segbits = reinterpret_cast<unsigned*>(scratch + l.segbits);
        j.segstart = reinterpret_cast<unsigned long long*>(scratch + l.segstart);
        j.raw = scratch + l.raw;
        j.rawbytes = reinterpret_cast<unsigned long long*>(scratch + l.rawbytes);
        j.ffcount = reinterpret_cast<unsigned*>(scratch + l.ffcount);
        j.ffstart = reinterpret_cast<unsigned long long*>(scratch + l.ffstart);
        j.fits = reinterpret_cast<int*>(scratch + l.fits);
        j.dst = dst;
        j.capacity = capacity;
        j.offsets = reinterpret_cast<unsigned long long*>(offsets);
        const bool dwords = (uintptr_t)j.bgr % 4 == 0 && j.step % 4 == 0 && j.frame % 4 == 0;
        launch_jpeg_chunk(j, dwords, stream);
    }
}

}  // namespace opk

struct opk_ctx : opk::Context {};

extern "C" int opk_jpeg_encode(opk_ctx* ctx, uint8_t* dst_dev, size_t capacity,
                               uint64_t* offsets_dev, const opk_frames* frames, int quality)
{
    try {
        OPK_CHECK_ARG(ctx && frames, "NULL argument");
        const opk::FrameSource s = opk::frame_source(*frames);
        opk::jpeg_encode(ctx, dst_dev, capacity, offsets_dev, s, quality, ctx->stream);
        return OPK_OK;
    } catch (const opk::Error& e) {
        opk::set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        opk::set_error(e.what());
        return OPK_ERR_STATE;
    }
}
