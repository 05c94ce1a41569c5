"""The JPEG frames of include/opk.h ("JPEG FRAMES") restated in numpy, whole frames at a time: the
header, colour conversion, the two edge rules, the 2 x 2 downsample, jfdctint's two passes,
quantisation, zigzag, dummy blocks, the codes and the byte stuffing.  encode(bgr, quality) is the
file.  tests/test_jpeg_cases.py holds it to Pillow (libjpeg-turbo) and to committed files byte for
byte; the host and device routes are then held to it.  cases() builds the inputs and asserts what
they cover."""
import numpy as np

ZIGZAG = [
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
]
BASE_LUMA = [   # Annex K.1, natural order
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99,
]
BASE_CHROMA = [   # Annex K.2
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
]
BITS_DC_LUMA = [   # Annex K.3
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
]
VALS_DC_LUMA = [
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b,
]
BITS_AC_LUMA = [   # Annex K.5
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
]
VALS_AC_LUMA = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa,
]
BITS_DC_CHROMA = [   # Annex K.4
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
]
VALS_DC_CHROMA = [
    0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b,
]
BITS_AC_CHROMA = [   # Annex K.6
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
]
VALS_AC_CHROMA = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa,
]


# ---- the definition ---------------------------------------------------------------------------------
FIX = {c: int(round(c * 8192)) for c in (0.298631336, 0.390180644, 0.541196100, 0.765366865,
                                         0.899976223, 1.175875602, 1.501321110, 1.847759065,
                                         1.961570560, 2.053119869, 2.562915447, 3.072711026)}
HEADER_BYTES = 623


def quant_table(base, quality):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): 64 values, natural order."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a BITS / HUFFVAL table (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(w, h, quality):
    """The 623 bytes before the entropy-coded data."""
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid, q in ((0, ql), (1, qc)):
        b += b"\xff\xdb\x00\x43" + bytes([tid]) + bytes(q[ZIGZAG[k]] for k in range(64))
    b += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3,
                                          1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, bits, vals in ((0x00, BITS_DC_LUMA, VALS_DC_LUMA), (0x10, BITS_AC_LUMA, VALS_AC_LUMA),
                           (0x01, BITS_DC_CHROMA, VALS_DC_CHROMA), (0x11, BITS_AC_CHROMA, VALS_AC_CHROMA)):
        n = 2 + 1 + 16 + len(vals)
        b += b"\xff\xc4" + bytes([n >> 8, n & 255, tc]) + bytes(bits) + bytes(vals)
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def planes(bgr):
    """(Y [16 * mcu rows, 16 * mcu columns], Cb, Cr [8 * mcu rows, 8 * mcu columns]) int32 of one
    BGR frame [h, w, 3]: colour conversion, the two edge rules, the 2 x 2 downsample."""
    h, w, _ = bgr.shape
    b, g, r = (bgr[..., i].astype(np.int32) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    mw, mh = -(-w // 16), -(-h // 16)
    full = lambda p: np.pad(p, ((0, h % 2), (0, 16 * mw - w)), mode="edge")   # even height, MCU width
    bias = np.tile(np.array([1, 2], np.int32), 4 * mw)
    down = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    rows = lambda p, n: np.pad(p, ((0, n - p.shape[0]), (0, 0)), mode="edge")
    return (rows(full(y), 16 * mh), rows(down(full(cb)), 8 * mh), rows(down(full(cr)), 8 * mh))


def _dct_pass(d, first):
    """One pass of jfdctint.c over the last axis of d [..., 8] (int64; every value fits int32)."""
    C = FIX
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    ds = lambda x, k: (x + (1 << (k - 1))) >> k
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
    z1 = (t12 + t13) * C[0.541196100]
    o[2] = ds(z1 + t13 * C[0.765366865], n)
    o[6] = ds(z1 - t12 * C[1.847759065], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C[1.175875602]
    t4, t5, t6, t7 = t4 * C[0.298631336], t5 * C[2.053119869], t6 * C[3.072711026], t7 * C[1.501321110]
    z1, z2 = -z1 * C[0.899976223], -z2 * C[2.562915447]
    z3, z4 = -z3 * C[1.961570560] + z5, -z4 * C[0.390180644] + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    out = np.stack(o, -1)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out


def fdct_quant(blocks, q):
    """blocks [..., 8, 8] samples -> quantised coefficients [..., 64] in zigzag order."""
    d = _dct_pass(blocks.astype(np.int64) - 128, True)                      # rows
    f = np.swapaxes(_dct_pass(np.swapaxes(d, -1, -2), False), -1, -2)      # columns
    qv = 8 * np.asarray(q, np.int64).reshape(8, 8)
    c = np.sign(f) * ((np.abs(f) + (qv >> 1)) // qv)
    return c.reshape(c.shape[:-2] + (64,))[..., ZIGZAG]


def coefficients(bgr, quality):
    """[MCUs, 6, 64] int64: every block of the stream in order, dummy luma blocks included."""
    h, w, _ = bgr.shape
    y, cb, cr = planes(bgr)
    mh, mw = y.shape[0] // 16, y.shape[1] // 16
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    yb = y.reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh, mw, 4, 8, 8)
    out = np.zeros((mh, mw, 6, 64), np.int64)
    out[:, :, :4] = fdct_quant(yb, ql)
    out[:, :, 4] = fdct_quant(cb.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3), qc)
    out[:, :, 5] = fdct_quant(cr.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3), qc)
    by = 2 * np.arange(mh)[:, None, None] + np.array([0, 0, 1, 1])[None, None, :]
    bx = 2 * np.arange(mw)[None, :, None] + np.array([0, 1, 0, 1])[None, None, :]
    dummy = (by >= -(-h // 8)) | (bx >= -(-w // 8)) | np.zeros((mh, mw, 4), bool)
    for j in range(1, 4):   # block 0 of an MCU is always real
        d = dummy[:, :, j]
        out[:, :, j][d] = 0
        out[:, :, j, 0][d] = out[:, :, j - 1, 0][d]
    return out.reshape(mh * mw, 6, 64), dummy.reshape(mh * mw, 4)


def _bit_length(v):
    a, n = np.abs(v), np.zeros(v.shape, np.int64)
    for k in range(12):
        n += a >= (1 << k)
    return n


def _table(codes):
    code, length = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    for s, (c, l) in codes.items():
        code[s], length[s] = c, l
    return code, length


def tokens(coef):
    """Every code of the stream in order as (value uint64, bit count) per (block, position 0..63 and
    the EOB slot 64), [MCUs * 6, 65] each: a slot holds its ZRLs, its symbol and its extra bits."""
    m = coef.shape[0]
    dc = coef[:, :, 0]
    diff = np.empty_like(dc)
    luma = dc[:, :4].reshape(-1)
    diff[:, :4] = (luma - np.concatenate([[0], luma[:-1]])).reshape(m, 4)
    for j in (4, 5):
        diff[:, j] = dc[:, j] - np.concatenate([[0], dc[:-1, j]])
    v = coef.copy()
    v[:, :, 0] = diff
    size = _bit_length(v)
    extra = np.where(v >= 0, v, (v - 1) & ((1 << size) - 1)).astype(np.uint64)
    k = np.arange(64)
    nz = (v != 0) & (k > 0)
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=-1)       # last non-zero AC up to k
    prev = np.concatenate([np.zeros_like(last[..., :1]), last[..., :-1]], -1)
    run = k - prev - 1
    val = np.zeros((m, 6, 65), np.uint64)
    length = np.zeros((m, 6, 65), np.int64)
    for sel, dc_t, ac_t in ((slice(0, 4), huff_codes(BITS_DC_LUMA, VALS_DC_LUMA), huff_codes(BITS_AC_LUMA, VALS_AC_LUMA)),
                            (slice(4, 6), huff_codes(BITS_DC_CHROMA, VALS_DC_CHROMA), huff_codes(BITS_AC_CHROMA, VALS_AC_CHROMA))):
        dcc, dcl = _table(dc_t)
        acc, acl = _table(ac_t)
        s = size[:, sel]
        assert s[..., 0].max() <= 11 and s[..., 1:].max(initial=0) <= 10
        # DC
        val[:, sel, 0] = (dcc[s[..., 0]] << s[..., 0].astype(np.uint64)) | extra[:, sel, 0]
        length[:, sel, 0] = dcl[s[..., 0]] + s[..., 0]
        # AC
        r = run[:, sel]
        sym = ((r & 15) << 4) | s
        zrl = r >> 4
        zc, zl = ac_t[0xF0]
        zval = np.zeros(r.shape, np.uint64)
        for t in (1, 2, 3):
            rep = np.uint64(sum(zc << (zl * i) for i in range(t)))
            zval = np.where(zrl == t, rep, zval)
        a_val = (((zval << acl[sym].astype(np.uint64)) | acc[sym]) << s.astype(np.uint64)) | extra[:, sel]
        a_len = zrl * zl + acl[sym] + s
        on = nz[:, sel]
        val[:, sel, 1:64] = np.where(on, a_val, 0)[..., 1:]
        length[:, sel, 1:64] = np.where(on, a_len, 0)[..., 1:]
        eob = last[:, sel, 63] < 63
        val[:, sel, 64] = np.where(eob, ac_t[0][0], 0)
        length[:, sel, 64] = np.where(eob, ac_t[0][1], 0)
    return val.reshape(m * 6, 65), length.reshape(m * 6, 65)


def pack(val, length):
    """(the stream's bytes before stuffing, the 1-bits filled in) of the codes in order."""
    l = length.reshape(-1)
    keep = l > 0
    v, l = val.reshape(-1)[keep], l[keep]
    total = int(l.sum())
    start = np.cumsum(l) - l
    at = np.arange(total) - np.repeat(start, l)
    shift = (np.repeat(l, l) - 1 - at).astype(np.uint64)
    bits = ((np.repeat(v, l) >> shift) & np.uint64(1)).astype(np.uint8)
    fill = -total % 8
    return np.packbits(np.concatenate([bits, np.ones(fill, np.uint8)])), fill


def stuff(raw):
    ff = raw == 0xFF
    out = np.zeros(raw.size + int(ff.sum()), np.uint8)
    out[np.arange(raw.size) + np.cumsum(ff) - ff] = raw
    return out


def encode(bgr, quality=100):
    """The file of one BGR frame [h, w, 3] uint8."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    h, w, _ = bgr.shape
    assert 1 <= w <= 65535 and 1 <= h <= 65535
    coef, _ = coefficients(bgr, quality)
    raw, _ = pack(*tokens(coef))
    return header(w, h, quality) + stuff(raw).tobytes() + b"\xff\xd9"


def stats(bgr, quality=100):
    """What the coverage conditions of the cases are read from."""
    h, w, _ = bgr.shape
    coef, dummy = coefficients(bgr, quality)
    val, length = tokens(coef)
    raw, fill = pack(val, length)
    k = np.arange(64)
    nz = (coef != 0) & (k > 0)
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=-1)
    prev = np.concatenate([np.zeros_like(last[..., :1]), last[..., :-1]], -1)
    zrl = np.where(nz, (k - prev - 1) >> 4, 0).sum(-1)
    luma = coef[:, :4, 0].reshape(-1)
    diffs = np.concatenate([luma - np.concatenate([[0], luma[:-1]]),
                            np.diff(coef[:, 4, 0], prepend=0), np.diff(coef[:, 5, 0], prepend=0)])
    mw = -(-w // 16)
    d = dummy.reshape(-1, mw, 4)
    return {
        "stuffed": int((raw == 0xFF).sum()),
        "max_zrl_in_block": int(zrl.max()),
        "all_eob": bool(not nz.any()),
        "fill": fill,
        "last_byte_ff_by_fill": bool(fill > 0 and raw[-1] == 0xFF),
        "dc_sizes_pos": set(_bit_length(diffs[diffs > 0]).tolist()),
        "dc_sizes_neg": set(_bit_length(diffs[diffs < 0]).tolist()),
        "dummy_right": bool(d[:, :, 1].any() and w % 16 and w % 16 <= 8),
        "dummy_bottom": bool(d[:, :, 2].any() and h % 16 and h % 16 <= 8),
    }


# ---- the cases ------------------------------------------------------------------------------------------
# (width, height) of the Pillow comparison; odd sizes, one block, dummy blocks on either side, a
# height that is even and no multiple of 16 (8, 24 -> 40, 18, 160 -> 90 x 160)
SIZES = [(1, 1), (8, 8), (9, 9), (16, 16), (17, 23), (8, 40), (24, 8), (7, 64), (34, 18), (50, 33),
         (90, 160)]
QUALITIES_50x33 = [1, 25, 49, 50, 51, 75, 95]


def noise(w, h, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(w, h, value):
    return np.full((h, w, 3), value, np.uint8)


def gradient(w, h):
    y, x, c = np.mgrid[0:h, 0:w, 0:3]
    return ((3 * y + 2 * x + 40 * c) % 256).astype(np.uint8)


def zrl_image(w, h):
    """128 + 100 cos cos at frequency (7, 7) in every 8 x 8 block of every component's plane: grey,
    so Y alone carries it; below quality 100 the rounding of the pixels quantises away and only
    coefficient 63 is left: three ZRLs in every luma block."""
    k = np.arange(8)
    c = np.cos((2 * k + 1) * 7 * np.pi / 16)
    tile = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    plane = np.tile(tile, (-(-h // 8), -(-w // 8)))[:h, :w]
    return np.repeat(plane[:, :, None], 3, axis=2)


def dc_swing(w, h):
    """Black and white 8 x 8 luma blocks side by side: DC differences of both signs and size 11."""
    y, x = np.mgrid[0:h, 0:w]
    plane = np.where(((x // 8) + (y // 8)) % 2 == 0, 0, 255).astype(np.uint8)
    return np.repeat(plane[:, :, None], 3, axis=2)


def fill_ff_case():
    """A frame whose stream's last byte is made 0xFF by the fill: found by walking seeds."""
    for seed in range(4000):
        im = noise(8, 8, 1000 + seed)
        if stats(im, 100)["last_byte_ff_by_fill"]:
            return im
    raise AssertionError("no seed gives a filled 0xFF")


def max_code_frame(w=64, h=64):
    """A frame built to make the codes long: full-swing noise at quality 100 (Q = 1 everywhere)."""
    rng = np.random.default_rng(7)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def cases():
    """[(name, bgr uint8 [h, w, 3], quality)] -- the inputs every route is held to -- with the
    coverage conditions asserted on the restatement's own streams."""
    out = [
        ("noise_48x64_q100", noise(48, 64, 1), 100),
        ("noise_50x33_q75", noise(50, 33, 2), 75),
        ("noise_17x23_q100", noise(17, 23, 3), 100),
        ("noise_24x8_q100", noise(24, 8, 4), 100),
        ("noise_8x40_q100", noise(8, 40, 5), 100),
        ("noise_7x64_q25", noise(7, 64, 6), 25),
        ("noise_1x1_q100", noise(1, 1, 7), 100),
        ("flat0_34x18_q100", flat(34, 18, 0), 100),
        ("flat255_16x16_q75", flat(16, 16, 255), 75),
        ("gradient_50x33_q100", gradient(50, 33), 100),
        ("gradient_90x160_q75", gradient(90, 160), 75),
        ("zrl_24x24_q75", zrl_image(24, 24), 75),
        ("dc_swing_40x24_q100", dc_swing(40, 24), 100),
        ("fill_ff_8x8_q100", fill_ff_case(), 100),
    ]
    st = {name: stats(im, q) for name, im, q in out}
    assert st["noise_48x64_q100"]["stuffed"] >= 10
    assert st["zrl_24x24_q75"]["max_zrl_in_block"] >= 2
    assert st["flat0_34x18_q100"]["all_eob"] and st["flat255_16x16_q75"]["all_eob"]
    assert st["fill_ff_8x8_q100"]["last_byte_ff_by_fill"]
    assert 11 in st["dc_swing_40x24_q100"]["dc_sizes_pos"] and 11 in st["dc_swing_40x24_q100"]["dc_sizes_neg"]
    assert any(s["dummy_right"] for s in st.values()) and any(s["dummy_bottom"] for s in st.values())
    return out


# the committed fixtures: tests/golden/jpeg/<name>.npy (BGR) and <name>.jpg (what Pillow wrote)
GOLDEN = ["noise_48x64_q100", "noise_50x33_q75", "zrl_24x24_q75", "dc_swing_40x24_q100",
          "flat0_34x18_q100", "fill_ff_8x8_q100"]
