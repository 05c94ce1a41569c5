"""YUV 4:2:0 -> BGR as include/opk.h defines it (OpenCV's cvtColor COLOR_YUV2BGR_NV12 / _I420
arithmetic: BT.601 limited range, 20-bit fixed point, nearest chroma), restated in vectorised numpy
int32, and the frame layouts the YUV tests share.  The library must give, for YUV frames, bit for
bit what it gives for yuv420_to_bgr(frames)."""
import numpy as np

CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527

# (Y, U, V) -> (B, G, R)
KNOWN = [
    ((16, 128, 128), (0, 0, 0)),
    ((235, 128, 128), (255, 255, 255)),
    ((126, 128, 128), (128, 128, 128)),
    ((255, 128, 128), (255, 255, 255)),
    ((0, 0, 0), (0, 154, 0)),
    ((255, 255, 255), (255, 125, 255)),
    ((255, 0, 0), (20, 255, 74)),
    ((0, 255, 255), (255, 0, 203)),
    ((81, 90, 240), (0, 0, 254)),
    ((145, 54, 34), (1, 255, 0)),
    ((41, 240, 110), (255, 0, 0)),
    ((16, 255, 0), (255, 54, 0)),
    ((200, 0, 255), (0, 161, 255)),
]


def yuv_to_bgr(y, u, v):
    """Per-pixel conversion of equally shaped integer arrays -> uint8 [..., 3] (B, G, R)."""
    y = np.maximum(0, np.asarray(y, np.int32) - 16) * np.int32(CY) + np.int32(1 << 19)
    u = np.asarray(u, np.int32) - 128
    v = np.asarray(v, np.int32) - 128
    b = (y + CUB * u) >> 20   # numpy's >> on signed integers is arithmetic
    g = (y + CVG * v + CUG * u) >> 20
    r = (y + CVR * v) >> 20
    assert b.dtype == g.dtype == r.dtype == np.int32
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def yuv420_to_bgr(y, u, v):
    """y [n, h, w], u and v [n, h / 2, w / 2] uint8 -> BGR uint8 [n, h, w, 3]: each 2 x 2 block of
    luma pixels takes one (U, V) pair."""
    n, h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (n, h // 2, w // 2)
    up = u.repeat(2, axis=1).repeat(2, axis=2)
    vp = v.repeat(2, axis=1).repeat(2, axis=2)
    return yuv_to_bgr(y, up, vp)


def nv12_to_bgr(y, uv):
    """y [n, h, w], uv [n, h / 2, w] (U first) -> BGR uint8 [n, h, w, 3]."""
    return yuv420_to_bgr(y, uv[:, :, 0::2], uv[:, :, 1::2])


def interleave(u, v):
    """The NV12 UV plane [n, h / 2, w] of I420's u and v planes [n, h / 2, w / 2]."""
    uv = np.empty(u.shape[:2] + (2 * u.shape[2],), np.uint8)
    uv[:, :, 0::2] = u
    uv[:, :, 1::2] = v
    return uv


def random_planes(n, h, w, seed):
    """(y, u, v) uint8 planes with every value range used, the extremes included."""
    g = np.random.default_rng(seed)
    y = g.integers(0, 256, (n, h, w), dtype=np.uint8)
    u = g.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8)
    v = g.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8)
    return y, u, v


def exhaustive_planes():
    """64 frames of 512 x 512 in which every (Y, U, V) of the 2^24 occurs: the 256 x 256 chroma
    planes enumerate all (U, V) in every frame, and the four luma pixels of a block over the 64
    frames enumerate all Y."""
    vv, uu = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    u = np.broadcast_to(uu, (64, 256, 256)).copy()
    v = np.broadcast_to(vv, (64, 256, 256)).copy()
    y = np.empty((64, 512, 512), np.uint8)
    for f in range(64):
        for dy in range(2):
            for dx in range(2):
                y[f, dy::2, dx::2] = 4 * f + 2 * dy + dx
    return y, u, v
