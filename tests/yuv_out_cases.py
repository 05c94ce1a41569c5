"""BGR -> YUV 4:2:0 as include/opk.h defines it (OpenCV's cvtColor COLOR_BGR2YUV_I420 arithmetic:
BT.601 limited range, 20-bit fixed point, the chroma of a 2 x 2 block from its top-left pixel
alone), restated in vectorised numpy int32, and the layouts the frames-out tests share.  With an
NV12 / I420 destination the library must write, bit for bit, bgr_to_yuv420 of the bytes its BGR
call writes."""
import numpy as np

RY, GY, BY = 269484, 528482, 102760
RU, GU, BU = -155188, -305135, 460324
RV, GV, BV = 460324, -385875, -74448
HALF, SHIFT = 1 << 19, 20

# (B, G, R) -> (Y, U, V): the five of the header, then odd ones -- the extremes of U and V, greys
# around the rounding, and mixed colours
KNOWN = [
    ((0, 0, 0), (16, 128, 128)),
    ((255, 255, 255), (235, 128, 128)),
    ((255, 0, 0), (41, 240, 110)),
    ((0, 255, 0), (145, 54, 34)),
    ((0, 0, 255), (82, 90, 240)),
    ((255, 255, 0), (170, 166, 16)),
    ((0, 255, 255), (210, 16, 146)),
    ((255, 0, 255), (107, 202, 222)),
    ((128, 128, 128), (126, 128, 128)),
    ((1, 1, 1), (17, 128, 128)),
    ((254, 254, 254), (234, 128, 128)),
    ((17, 130, 201), (135, 68, 167)),
    ((200, 3, 77), (57, 204, 146)),
]


def sums(b, g, r, dtype=np.int32):
    """The three sums of the definition before the shift, in `dtype`."""
    b, g, r = (np.asarray(c).astype(dtype) for c in (b, g, r))
    t = dtype
    y = t(RY) * r + t(GY) * g + t(BY) * b + t(HALF) + t(16 << SHIFT)
    u = t(RU) * r + t(GU) * g + t(BU) * b + t(HALF) + t(128 << SHIFT)
    v = t(RV) * r + t(GV) * g + t(BV) * b + t(HALF) + t(128 << SHIFT)
    return y, u, v


def bgr_to_yuv(b, g, r):
    """Per-pixel (Y, U, V) of equally shaped integer arrays, int32 with the arithmetic shift and
    no clamp; the values as int32."""
    y, u, v = sums(b, g, r)
    assert y.dtype == u.dtype == v.dtype == np.int32
    return y >> SHIFT, u >> SHIFT, v >> SHIFT   # numpy's >> on signed integers is arithmetic


def bgr_to_yuv420(bgr):
    """bgr uint8 [n, h, w, 3] (h, w even) -> (y [n, h, w], u, v [n, h / 2, w / 2]) uint8: a luma
    sample per pixel, the chroma of each 2 x 2 block from its top-left pixel."""
    n, h, w, c = bgr.shape
    assert c == 3 and bgr.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    y = (sums(b, g, r)[0] >> SHIFT)
    top = bgr[:, 0::2, 0::2]
    _, u, v = bgr_to_yuv(top[..., 0], top[..., 1], top[..., 2])
    for p in (y, u, v):
        assert p.min() >= 0 and p.max() <= 255
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def to_nv12(y, u, v):
    """(y, uv): the interleaved pair plane [n, h / 2, w], U first."""
    uv = np.empty(u.shape[:2] + (2 * u.shape[2],), np.uint8)
    uv[:, :, 0::2] = u
    uv[:, :, 1::2] = v
    return y, uv


def exhaustive_bgr():
    """64 frames of 1024 x 1024 BGR in which every (B, G, R) of the 2^24 is the top-left pixel of
    exactly one 2 x 2 block, the block's three other pixels being other colours (the top-left's
    with 85, 170 and 255 added to every channel, modulo 256)."""
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(64, 512, 512)
    top = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], -1).astype(np.uint8)
    out = np.empty((64, 1024, 1024, 3), np.uint8)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx::2] = top + np.uint8(85 * k)   # uint8 arithmetic wraps
    return out


def random_bgr(n, h, w, seed):
    """Random frames with the extremes: the first pixels of frame 0 are black and white."""
    bgr = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    bgr[0, 0, 0] = 0
    bgr[0, -1, -1] = 255
    return bgr
