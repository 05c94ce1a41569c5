// jpeg_dev.h -- the arithmetic of the baseline JPEG encoder as include/opk.h states it ("JPEG
// FRAMES"): colour conversion, the 2 x 2 chroma downsample, the two passes of the integer FDCT,
// quantisation, a value's size and extra bits, one block's codes, and the block layout of a frame.
// Compiles for host and device: opk_jpeg_encode_host (host/jpeg.cpp) and the kernels (jpeg.hip) run
// this very text.  All of it is int32 arithmetic with an arithmetic >>.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__)
#define OPK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define OPK_HD inline
#endif

namespace opk {

constexpr int kJpegHeaderBytes = 623;
// the longest a block can get: DC code (<= 11 bits, K.4) + 11 extra bits, and for each of the 63
// ACs a 16-bit code + 10 extra bits (a ZRL only ever stands for zero coefficients, which cost less)
constexpr int kJpegMaxBlockBits = 22 + 63 * 26;

// ---- the codes (built once on the host: host/jpeg.cpp make_jpeg_tables) -------------------------
// table t: 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma; code[t][symbol] in the low len bits
struct JpegHuff {
    uint16_t code[4][256];
    uint8_t len[4][256];
};
// what the kernels read besides the frames: the file header, qv = 8 * Q in natural order (0 luma,
// 1 chroma), the zigzag scan and the codes.  One device blob per (w, h, quality).
struct JpegTables {
    uint8_t header[640];     // kJpegHeaderBytes of them used
    uint16_t qv[2][64];
    uint8_t zigzag[64];      // zigzag position -> natural index
    JpegHuff huff;
};

// ---- the block layout -----------------------------------------------------------------------------
struct JpegGeom {
    int w, h;
    int mw, mh;          // MCUs per row and per column: ceil(w / 16), ceil(h / 16)
    int bw, bh;          // real luma blocks: ceil(w / 8), ceil(h / 8)
    int hc;              // real chroma rows: ceil(h / 2)
};
OPK_HD JpegGeom jpeg_geom(int w, int h)
{
    JpegGeom g;
    g.w = w;
    g.h = h;
    g.mw = (w + 15) / 16;
    g.mh = (h + 15) / 16;
    g.bw = (w + 7) / 8;
    g.bh = (h + 7) / 8;
    g.hc = (h + 1) / 2;
    return g;
}
// luma block j (0..3: (0,0), (0,1), (1,0), (1,1)) of MCU (mx, my) lies outside the real blocks
OPK_HD bool jpeg_dummy(const JpegGeom& g, int mx, int my, int j)
{
    return 2 * mx + (j & 1) >= g.bw || 2 * my + (j >> 1) >= g.bh;
}

// ---- colour ---------------------------------------------------------------------------------------
OPK_HD int jpeg_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
OPK_HD int jpeg_cb(int r, int g, int b)
{
    return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
OPK_HD int jpeg_cr(int r, int g, int b)
{
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// the four full-resolution samples under chroma column `col`: bias 1 in even columns, 2 in odd ones
OPK_HD int jpeg_downsample(int a, int b, int c, int d, int col)
{
    return (a + b + c + d + 1 + (col & 1)) >> 2;
}
// Source rows of the 2 x 2 pixels of luma rows (2r, 2r + 1), r a chroma row of the padded frame:
// the luma takes rows min(2r + i, h - 1); the chroma first replicates its last real row
// (r -> min(r, hc - 1)) and then takes min(2r + i, h - 1) of that.
OPK_HD int jpeg_luma_row(const JpegGeom& g, int r, int i)
{
    const int y = 2 * r + i;
    return y < g.h ? y : g.h - 1;
}
OPK_HD int jpeg_chroma_row(const JpegGeom& g, int r, int i)
{
    return jpeg_luma_row(g, r < g.hc ? r : g.hc - 1, i);
}
OPK_HD int jpeg_col(const JpegGeom& g, int x) { return x < g.w ? x : g.w - 1; }

// ---- FDCT: jfdctint.c, CONST_BITS 13, PASS1_BITS 2 ----------------------------------------------------
OPK_HD int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass over 8 values in place.  First: the row pass on samples - 128, outputs scaled by 4;
// otherwise the column pass, which removes that scale.
template <bool First>
OPK_HD void jpeg_fdct_pass(int (&d)[8])
{
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373,
                  F1_175 = 9633, F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819,
                  F2_562 = 20995, F3_072 = 25172;
    constexpr int N = First ? 13 - 2 : 13 + 2;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (First) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = jpeg_descale(t10 + t11, 2);
        d[4] = jpeg_descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * F0_541;
    d[2] = jpeg_descale(z1 + t13 * F0_765, N);
    d[6] = jpeg_descale(z1 - t12 * F1_847, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1_175;
    t4 *= F0_298;
    t5 *= F2_053;
    t6 *= F3_072;
    t7 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 = z3 * -F1_961 + z5;
    z4 = z4 * -F0_390 + z5;
    d[7] = jpeg_descale(t4 + z1 + z3, N);
    d[5] = jpeg_descale(t5 + z2 + z4, N);
    d[3] = jpeg_descale(t6 + z2 + z3, N);
    d[1] = jpeg_descale(t7 + z1 + z4, N);
}

// ---- quantisation ---------------------------------------------------------------------------------
OPK_HD int jpeg_quantise(int f, int qv)
{
    const int a = ((f < 0 ? -f : f) + (qv >> 1)) / qv;
    return f < 0 ? -a : a;
}
// libjpeg's jpeg_quality_scaling and jpeg_add_quant_table with force_baseline
OPK_HD int jpeg_quant_value(int base, int quality)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * s + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// ---- entropy coding -------------------------------------------------------------------------------
OPK_HD int jpeg_bit_length(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}
OPK_HD unsigned jpeg_extra_bits(int v, int n) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// What position k (0..63, zigzag) of a block puts into the stream, and slot 64 its EOB: `len` bits,
// the low ones of `bits`, MSB first.  v: the value at k (k = 0: the DC difference); nz: the mask of
// the block's non-zero ACs (bit k; bit 0 clear); chroma: which pair of tables.  At most
// 3 * 11 + 16 + 10 = 59 bits.
struct JpegCode {
    uint64_t bits;
    int len;
};
OPK_HD JpegCode jpeg_code(const JpegHuff& hf, int chroma, int k, int v, uint64_t nz)
{
    JpegCode c{0, 0};
    const int dc = 2 * chroma, ac = dc + 1;
    if (k == 0) {
        const int n = jpeg_bit_length(v);
        c.bits = ((uint64_t)hf.code[dc][n] << n) | jpeg_extra_bits(v, n);
        c.len = hf.len[dc][n] + n;
        return c;
    }
    if (k == 64) {   // EOB: the block ends in zeros
        if (!(nz >> 63)) {
            c.bits = hf.code[ac][0];
            c.len = hf.len[ac][0];
        }
        return c;
    }
    if (v == 0) return c;
    const uint64_t before = nz & ((1ull << k) - 1ull);
    // the last non-zero AC before k, or the DC's position
    const int prev = before ? 63 - __builtin_clzll(before) : 0;
    int run = k - prev - 1;
    for (; run >= 16; run -= 16) {   // ZRL
        c.bits = (c.bits << hf.len[ac][0xF0]) | hf.code[ac][0xF0];
        c.len += hf.len[ac][0xF0];
    }
    const int n = jpeg_bit_length(v), sym = (run << 4) | n;
    c.bits = (((c.bits << hf.len[ac][sym]) | hf.code[ac][sym]) << n) | jpeg_extra_bits(v, n);
    c.len += hf.len[ac][sym] + n;
    return c;
}

}  // namespace opk
