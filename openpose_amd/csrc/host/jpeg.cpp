// jpeg.cpp -- the host side of the JPEG frames (include/opk.h): the header and the code tables, the
// bound, the argument checks and opk_jpeg_encode_host, the plain-C++ encoder.  The arithmetic is
// kernels/jpeg_dev.h, which the kernels run too.  No device code: tests/jpeg_driver.cpp builds this
// file alone under the sanitizers.
#include "jpeg.h"

#include <cstring>
#include <string>
#include <vector>

#include "../../../include/opk.h"
#include "../common.h"
#include "../kernels/jpeg_tables.inc"

namespace opk {

namespace {

void huff_table(JpegHuff& hf, int t, const unsigned char* bits, const unsigned char* vals)
{
    // T.81 Annex C: codes of each length count upwards, doubled from one length to the next
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k, ++code) {
            hf.code[t][vals[k]] = (uint16_t)code;
            hf.len[t][vals[k]] = (uint8_t)len;
        }
        code <<= 1;
    }
}

struct Bytes {
    uint8_t* p;
    void u8(int v) { *p++ = (uint8_t)v; }
    void u16(int v)
    {
        u8(v >> 8);
        u8(v & 255);
    }
    void put(const void* s, size_t n)
    {
        std::memcpy(p, s, n);
        p += n;
    }
};

void dht(Bytes& b, int tc, const unsigned char* bits, const unsigned char* vals, int nvals)
{
    b.u16(0xFFC4);
    b.u16(2 + 1 + 16 + nvals);
    b.u8(tc);
    b.put(bits, 16);
    b.put(vals, (size_t)nvals);
}

}  // namespace

void make_jpeg_tables(JpegTables& t, int w, int h, int quality)
{
    std::memset(&t, 0, sizeof t);
    uint8_t q[2][64];
    for (int k = 0; k < 64; ++k) {
        q[0][k] = (uint8_t)jpeg_quant_value(kJpegBaseLuma[k], quality);
        q[1][k] = (uint8_t)jpeg_quant_value(kJpegBaseChroma[k], quality);
        t.qv[0][k] = (uint16_t)(8 * q[0][k]);
        t.qv[1][k] = (uint16_t)(8 * q[1][k]);
        t.zigzag[k] = kJpegZigzag[k];
    }
    huff_table(t.huff, 0, kJpegBits_DC_LUMA, kJpegVals_DC_LUMA);
    huff_table(t.huff, 1, kJpegBits_AC_LUMA, kJpegVals_AC_LUMA);
    huff_table(t.huff, 2, kJpegBits_DC_CHROMA, kJpegVals_DC_CHROMA);
    huff_table(t.huff, 3, kJpegBits_AC_CHROMA, kJpegVals_AC_CHROMA);

    Bytes b{t.header};
    b.u16(0xFFD8);
    b.u16(0xFFE0);   // APP0: JFIF 1.01, no units, density 1 x 1, no thumbnail
    b.u16(16);
    b.put("JFIF", 5);
    b.u16(0x0101);
    b.u8(0);
    b.u16(1);
    b.u16(1);
    b.u16(0);
    for (int id = 0; id < 2; ++id) {
        b.u16(0xFFDB);
        b.u16(67);
        b.u8(id);
        for (int k = 0; k < 64; ++k) b.u8(q[id][kJpegZigzag[k]]);
    }
    b.u16(0xFFC0);   // SOF0
    b.u16(17);
    b.u8(8);
    b.u16(h);
    b.u16(w);
    b.u8(3);
    const uint8_t comps[9] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    b.put(comps, 9);
    dht(b, 0x00, kJpegBits_DC_LUMA, kJpegVals_DC_LUMA, (int)sizeof kJpegVals_DC_LUMA);
    dht(b, 0x10, kJpegBits_AC_LUMA, kJpegVals_AC_LUMA, (int)sizeof kJpegVals_AC_LUMA);
    dht(b, 0x01, kJpegBits_DC_CHROMA, kJpegVals_DC_CHROMA, (int)sizeof kJpegVals_DC_CHROMA);
    dht(b, 0x11, kJpegBits_AC_CHROMA, kJpegVals_AC_CHROMA, (int)sizeof kJpegVals_AC_CHROMA);
    b.u16(0xFFDA);   // SOS
    b.u16(12);
    const uint8_t scan[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    b.put(scan, 10);
    if (b.p - t.header != kJpegHeaderBytes) throw Error(OPK_ERR_STATE, "JPEG header size");
}

// The bound.  A frame has 6 * ceil(w / 16) * ceil(h / 16) blocks.  A block's longest DC is an
// 11-bit code (K.4) with 11 extra bits; each of its 63 ACs at most a 16-bit code with 10 extra bits
// -- a ZRL stands for 16 zero coefficients in 11 bits, less than one coded coefficient each -- so a
// block has at most kJpegMaxBlockBits = 22 + 63 * 26 = 1660 bits.  The stream is those bits rounded
// up to bytes by the fill, and stuffing can at most double it (every byte 0xFF).  Around it the
// 623 header bytes and FFD9.
size_t jpeg_bound(int n, int w, int h)
{
    if (n <= 0 || w <= 0 || h <= 0) return 0;
    const JpegGeom g = jpeg_geom(w, h);
    const size_t blocks = (size_t)6 * (size_t)g.mw * (size_t)g.mh;
    const size_t stream = (blocks * kJpegMaxBlockBits + 7) / 8;
    return (size_t)n * (kJpegHeaderBytes + 2 * stream + 2);
}

void check_jpeg(int w, int h, int quality)
{
    OPK_CHECK_ARG(w >= 1 && w <= 65535 && h >= 1 && h <= 65535,
                  "a JPEG frame's width and height lie in 1..65535");
    OPK_CHECK_ARG(quality >= 1 && quality <= 100, "quality: 1..100");
}

void check_jpeg_apart(const uint8_t* dst, size_t capacity, const uint8_t* src, size_t src_bytes)
{
    const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)src;
    OPK_CHECK_ARG(d0 + capacity <= s0 || s0 + src_bytes <= d0, "dst overlaps the source frames");
}

namespace {

// the stream of one frame: bits MSB first, a 0x00 after every 0xFF byte
struct BitWriter {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int held = 0;   // bits of acc not yet written, < 8 between calls
    void byte(unsigned v)
    {
        out.push_back((uint8_t)v);
        if (v == 0xFF) out.push_back(0);
    }
    void put(const JpegCode& c)
    {
        // up to 59 bits on top of up to 7: in two pieces
        int len = c.len;
        while (len > 0) {
            const int take = len > 32 ? len - 32 : len;
            acc = (acc << take) | ((c.bits >> (len - take)) & ((1ull << take) - 1ull));
            held += take;
            len -= take;
            while (held >= 8) {
                held -= 8;
                byte((unsigned)(acc >> held) & 0xFFu);
            }
        }
    }
    void fill()
    {
        if (held) byte(((unsigned)(acc << (8 - held)) | ((1u << (8 - held)) - 1u)) & 0xFFu);
        held = 0;
    }
};

// the six blocks of MCU (mx, my) of one frame: quantised coefficients in zigzag order
void mcu_coefficients(int16_t (&coef)[6][64], const uint8_t* frame, size_t step, const JpegGeom& g,
                      const JpegTables& t, int mx, int my)
{
    int samples[6][8][8];
    for (int qy = 0; qy < 8; ++qy)
        for (int qx = 0; qx < 8; ++qx) {
            const int r = 8 * my + qy, c = 8 * mx + qx;
            int cb[4], cr[4];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const int x = jpeg_col(g, 2 * c + j);
                    const uint8_t* p = frame + (size_t)jpeg_luma_row(g, r, i) * step + (size_t)x * 3;
                    const int ly = 2 * qy + i, lx = 2 * qx + j;
                    samples[2 * (ly >> 3) + (lx >> 3)][ly & 7][lx & 7] = jpeg_y(p[2], p[1], p[0]);
                    const uint8_t* q = frame + (size_t)jpeg_chroma_row(g, r, i) * step + (size_t)x * 3;
                    cb[2 * i + j] = jpeg_cb(q[2], q[1], q[0]);
                    cr[2 * i + j] = jpeg_cr(q[2], q[1], q[0]);
                }
            samples[4][qy][qx] = jpeg_downsample(cb[0], cb[1], cb[2], cb[3], c);
            samples[5][qy][qx] = jpeg_downsample(cr[0], cr[1], cr[2], cr[3], c);
        }
    for (int b = 0; b < 6; ++b) {
        if (b < 4 && jpeg_dummy(g, mx, my, b)) {   // not transformed: the DC of the block before it
            std::memset(coef[b], 0, sizeof coef[b]);
            coef[b][0] = coef[b - 1][0];
            continue;
        }
        int f[8][8];
        for (int y = 0; y < 8; ++y) {
            int d[8];
            for (int x = 0; x < 8; ++x) d[x] = samples[b][y][x] - 128;
            jpeg_fdct_pass<true>(d);
            for (int x = 0; x < 8; ++x) f[y][x] = d[x];
        }
        for (int x = 0; x < 8; ++x) {
            int d[8];
            for (int y = 0; y < 8; ++y) d[y] = f[y][x];
            jpeg_fdct_pass<false>(d);
            for (int y = 0; y < 8; ++y) f[y][x] = d[y];
        }
        const uint16_t* qv = t.qv[b < 4 ? 0 : 1];
        for (int k = 0; k < 64; ++k) {
            const int nat = t.zigzag[k];
            coef[b][k] = (int16_t)jpeg_quantise(f[nat >> 3][nat & 7], qv[nat]);
        }
    }
}

void encode_frame(std::vector<uint8_t>& out, const uint8_t* frame, size_t step, const JpegGeom& g,
                  const JpegTables& t)
{
    out.clear();
    out.insert(out.end(), t.header, t.header + kJpegHeaderBytes);
    BitWriter bw{out};
    int last_dc[3] = {0, 0, 0};
    int16_t coef[6][64];
    for (int my = 0; my < g.mh; ++my)
        for (int mx = 0; mx < g.mw; ++mx) {
            mcu_coefficients(coef, frame, step, g, t, mx, my);
            for (int b = 0; b < 6; ++b) {
                const int comp = b < 4 ? 0 : b - 3;
                uint64_t nz = 0;
                for (int k = 1; k < 64; ++k)
                    if (coef[b][k]) nz |= 1ull << k;
                bw.put(jpeg_code(t.huff, comp != 0, 0, coef[b][0] - last_dc[comp], nz));
                last_dc[comp] = coef[b][0];
                for (int k = 1; k <= 64; ++k)
                    if (k == 64 || coef[b][k])
                        bw.put(jpeg_code(t.huff, comp != 0, k, k < 64 ? coef[b][k] : 0, nz));
            }
        }
    bw.fill();
    out.push_back(0xFF);
    out.push_back(0xD9);
}

template <class F>
int guarded_jpeg(F&& f)
{
    try {
        f();
        return OPK_OK;
    } catch (const Error& e) {
        set_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_error(e.what());
        return OPK_ERR_STATE;
    }
}

}  // namespace

void jpeg_encode_host(uint8_t* dst, size_t capacity, uint64_t* offsets, const uint8_t* bgr,
                      size_t step, size_t frame_bytes, int n, int w, int h, int quality)
{
    JpegTables t;
    make_jpeg_tables(t, w, h, quality);
    const JpegGeom g = jpeg_geom(w, h);
    std::vector<uint8_t> file;
    uint64_t at = 0;
    bool room = true;   // a frame that does not fit is not written, nor is any after it
    offsets[0] = 0;
    for (int f = 0; f < n; ++f) {
        encode_frame(file, bgr + (size_t)f * frame_bytes, step, g, t);
        room = room && at + file.size() <= capacity;
        if (room) std::memcpy(dst + at, file.data(), file.size());
        at += file.size();
        offsets[f + 1] = at;
    }
}

}  // namespace opk

extern "C" {

size_t opk_jpeg_bound(int n, int w, int h) { return opk::jpeg_bound(n, w, h); }

int opk_jpeg_encode_host(uint8_t* dst, size_t capacity, uint64_t* offsets, const uint8_t* bgr,
                         size_t step, size_t frame_bytes, int n, int w, int h, int quality)
{
    return opk::guarded_jpeg([&] {
        OPK_CHECK_ARG(n >= 0, "negative frame count");
        opk::check_jpeg(w, h, quality);
        OPK_CHECK_ARG(step == 0 || step >= (size_t)w * 3, "row step shorter than the row");
        if (step == 0) step = (size_t)w * 3;
        OPK_CHECK_ARG(frame_bytes == 0 || frame_bytes >= step * (size_t)(h - 1) + (size_t)w * 3,
                      "frame stride shorter than the frame");
        if (frame_bytes == 0) frame_bytes = step * (size_t)h;
        if (n == 0) {
            if (offsets) offsets[0] = 0;
            return;
        }
        OPK_CHECK_ARG(dst && offsets && bgr, "NULL argument");
        opk::check_jpeg_apart(dst, capacity, bgr,
                              (size_t)(n - 1) * frame_bytes + step * (size_t)(h - 1) + (size_t)w * 3);
        opk::jpeg_encode_host(dst, capacity, offsets, bgr, step, frame_bytes, n, w, h, quality);
    });
}

}  // extern "C"
