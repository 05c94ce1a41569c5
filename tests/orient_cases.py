"""The rotated and flipped frames of include/opk.h ("ROTATED AND FLIPPED FRAMES") restated in numpy
as index arithmetic: the table, entry by entry, on planes of samples, and how BGR, NV12 and I420
frames move through it.  Held to np.rot90 / np.flip / np.transpose and to hand-worked frames in
tests/test_orient_cases.py; the reference for the host and GPU tests."""
import numpy as np

ANGLES = (0, 90, 180, 270)
CASES = [(r, f) for r in ANGLES for f in (0, 1)]   # the 8 orientations


def normalize(rotate):
    """rotate % 360 as C computes it, -270 / -180 / -90 as 90 / 180 / 270; None: not accepted."""
    r = int(np.fmod(rotate, 360))
    return (r + 360) % 360 if r % 90 == 0 else None


def size(w, h, rotate):
    return (h, w) if normalize(rotate) in (90, 270) else (w, h)


def source_index(x, y, w, h, rotate, flip):
    """(sx, sy) with D[y][x] = S[sy][sx]: the table's entry for (rotate, flip); x, y may be arrays."""
    r = normalize(rotate)
    if r == 0:
        return (w - 1 - x, y) if flip else (x, y)
    if r == 90:
        return (y, x) if flip else (w - 1 - y, x)
    if r == 180:
        return (x, h - 1 - y) if flip else (w - 1 - x, h - 1 - y)
    return (w - 1 - y, h - 1 - x) if flip else (y, h - 1 - x)


def oriented_index(sx, sy, w, h, rotate, flip):
    """The inverse of source_index: where source sample (sx, sy) lands, by search over the table."""
    ow, oh = size(w, h, rotate)
    ys, xs = np.mgrid[0:oh, 0:ow]
    qx, qy = source_index(xs, ys, w, h, rotate, flip)
    hit = np.argwhere((qx == sx) & (qy == sy))
    assert hit.shape == (1, 2)
    return int(hit[0, 1]), int(hit[0, 0])


def plane(s, rotate, flip):
    """s [..., h, w, channels] -> [..., oh, ow, channels], sample by sample."""
    h, w = s.shape[-3], s.shape[-2]
    ow, oh = size(w, h, rotate)
    ys, xs = np.mgrid[0:oh, 0:ow]
    sx, sy = source_index(xs, ys, w, h, rotate, flip)
    return np.ascontiguousarray(s[..., sy, sx, :])


def bgr(frames, rotate, flip):
    """uint8 [n, h, w, 3] -> [n, oh, ow, 3]"""
    return plane(frames, rotate, flip)


def nv12(y, uv, rotate, flip):
    """y [n, h, w], uv [n, h/2, w] (U, V interleaved): the pair is one sample."""
    n, h, w = y.shape
    oy = plane(y[..., None], rotate, flip)[..., 0]
    ouv = plane(uv.reshape(n, h // 2, w // 2, 2), rotate, flip)
    return oy, ouv.reshape(n, ouv.shape[1], -1)


def i420(y, u, v, rotate, flip):
    """y [n, h, w], u and v [n, h/2, w/2]"""
    return tuple(plane(p[..., None], rotate, flip)[..., 0] for p in (y, u, v))


def yuv_planes(seed, n, h, w):
    """Random (y, u, v) planes of n frames."""
    r = np.random.default_rng(seed)
    return (r.integers(0, 256, (n, h, w), dtype=np.uint8),
            r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8),
            r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8))


def frames_bgr(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
