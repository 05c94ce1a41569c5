"""The numpy restatement of the include/opk.h text "Undistorted rig frames": the map of one camera
(cv::initUndistortRectifyMap's scalar path, CV_16SC2, R = I, new camera matrix = K) and the remap of
one frame (cv::remap, INTER_LINEAR, constant border 0), plus the seeded cameras and frames of the
tests.  Every operation of the map is one fp64 numpy operation, rounded on its own; the accumulation
along a row is a loop over the columns (vectorised over the rows, which are independent)."""
import numpy as np

import oracle

INT_MIN = -2 ** 31

# models/cameraParameters/flir/17012332.xml.example of the reference (tests/golden/camera_parameters)
K_EXAMPLE = np.array([[8.1793481631740565e+02, 0., 6.0070689997785121e+02],
                      [0., 8.1651774059837908e+02, 5.1784529566329593e+02],
                      [0., 0., 1.]])
D8_EXAMPLE = np.array([-1.8102158829399091e+00, 9.1966147162623262e+00, -4.4293900343777355e-04,
                       1.3638377686816653e-03, 1.3303863414979364e+00, -1.4189051636354870e+00,
                       8.4725535468475819e+00, 4.7911023525901033e+00])
D5_BARREL = np.array([-0.28, 0.09, 1e-3, -5e-4, -0.01])
D4_PINCUSHION = np.array([0.3, 0., 0., 0.])
D5_K3_HUGE = np.array([0., 0., 0., 0., 1e12])
# (k1 = -0.21 puts one u*32 of the 160 x 90 image 6e-8 from a rounding tie: the cases' precondition,
# asserted in tests/test_undistort_cases.py, is 1e-7, so the case camera stands a little beside it)
D12 = np.array([-0.2103, 0.05, 7e-4, -3e-4, 0.012, 0.02, -0.01, 0.003, 2e-3, -1e-3, 1.5e-3, 5e-4])


def small_k(w, h, skew=0.0):
    """Intrinsics of a w x h image with the example's proportions (a lens whose corners see
    |x|, |y| up to ~0.8): inexact values so that no product is exact."""
    s = w / 1280.0
    return np.array([[K_EXAMPLE[0, 0] * s, skew, K_EXAMPLE[0, 2] * s + 0.137],
                     [0., K_EXAMPLE[1, 1] * s, h * 0.5057],
                     [0., 0., 1.]])


def inverse3(K):
    """ir[9]: the 3x3 closed form of the text."""
    K = np.asarray(K, np.float64)
    K00, K01, K02, K10, K11, K12, K20, K21, K22 = [np.float64(v) for v in K.reshape(-1)]
    det = K00 * (K11 * K22 - K12 * K21) - K01 * (K10 * K22 - K12 * K20) + K02 * (K10 * K21 - K11 * K20)
    d = np.float64(1.) / det
    return [(K11 * K22 - K12 * K21) * d, (K02 * K21 - K01 * K22) * d, (K01 * K12 - K02 * K11) * d,
            (K12 * K20 - K10 * K22) * d, (K00 * K22 - K02 * K20) * d, (K02 * K10 - K00 * K12) * d,
            (K10 * K21 - K11 * K20) * d, (K01 * K20 - K00 * K21) * d, (K00 * K11 - K01 * K10) * d], det


def coefficients(dist):
    k = np.zeros(12, np.float64)
    k[:len(dist)] = dist
    return k


def distort(x, y, k, fx, fy, u0, v0):
    """Step 4 of the text from (x, y) on; works on any float type the arguments share."""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
    return fx * xd + u0, fy * yd + v0


def uv(K, dist, w, h):
    """(u, v) float64 [h, w] of the text, the row accumulation included."""
    K = np.asarray(K, np.float64)
    ir, _ = inverse3(K)
    k = [np.float64(c) for c in coefficients(dist)]
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    i = np.arange(h, dtype=np.float64)
    _x = i * ir[1] + ir[2]
    _y = i * ir[4] + ir[5]
    _w = i * ir[7] + ir[8]
    u = np.empty((h, w), np.float64)
    v = np.empty((h, w), np.float64)
    with np.errstate(all="ignore"):
        for j in range(w):
            wi = 1. / _w
            u[:, j], v[:, j] = distort(_x * wi, _y * wi, k, fx, fy, u0, v0)
            _x = _x + ir[0]
            _y = _y + ir[3]
            _w = _w + ir[6]
    return u, v


def round_to_int(t):
    """round_half_even as int32; NaN and what rounds outside the int32 range give INT_MIN."""
    with np.errstate(all="ignore"):
        r = np.rint(t)
        ok = (r >= -2147483648.) & (r <= 2147483647.)
        return np.where(ok, np.where(ok, r, 0.).astype(np.int64), INT_MIN)


def fixed_maps(u, v):
    with np.errstate(all="ignore"):
        iu, iv = round_to_int(u * 32), round_to_int(v * 32)
    m1 = np.stack([((iu >> 5) & 0xffff), ((iv >> 5) & 0xffff)], -1).astype(np.uint16).view(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return m1, m2


def maps(K, dist, w, h):
    """(m1 int16 [h, w, 2], m2 uint16 [h, w]) of one camera."""
    return fixed_maps(*uv(K, dist, w, h))


_T = None


def weight_table():
    global _T
    if _T is None:
        _T = oracle.warp_weight_table(False).astype(np.int64)   # [32][32][2][2]
    return _T


def remap(frame, m1, m2):
    """The remap of one BGR uint8 frame [h, w, 3] through (m1, m2)."""
    frame = np.asarray(frame, np.uint8)
    h, w, _ = frame.shape
    sx = m1[..., 0].astype(np.int64)
    sy = m1[..., 1].astype(np.int64)
    f = m2.astype(np.int64)
    wt = weight_table()[f >> 5, f & 31]          # [h, w, 2, 2]
    src = frame.astype(np.int64)
    acc = np.zeros((h, w, 3), np.int64)
    for ky in range(2):
        for kx in range(2):
            yy, xx = sy + ky, sx + kx
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            tap = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * inside[..., None]
            acc += tap * wt[..., ky, kx][..., None]
    return ((acc + 16384) >> 15).astype(np.uint8)


def undistort(frames, cameras):
    """frames uint8 [n, h, w, 3]; cameras: a list of V (K, dist); frame f uses view f % V."""
    n, h, w, _ = frames.shape
    ms = [maps(K, d, w, h) for K, d in cameras]
    return np.stack([remap(frames[f], *ms[f % len(ms)]) for f in range(n)])


def independent_uv(K, dist, w, h):
    """(u, v) without the accumulation, in np.longdouble, and written apart from distort(): x and y
    from the closed-form inverse of an upper-triangular K with last row (0, 0, 1) -- y = (i - v0)/fy,
    x = (j - u0 - skew*y)/fx -- and the lens model from OpenCV's documentation of the rational,
    tangential and thin-prism terms, with the radial polynomials expanded in powers of r^2."""
    L = np.longdouble
    K = np.asarray(K, np.float64)
    assert K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1
    fx, skew, u0, fy, v0 = L(K[0, 0]), L(K[0, 1]), L(K[0, 2]), L(K[1, 1]), L(K[1, 2])
    y = ((np.arange(h).astype(L) - v0) / fy)[:, None] * np.ones((1, w), L)
    x = (np.arange(w).astype(L)[None, :] - u0 - skew * y) / fx
    c = dict(zip("k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4".split(), [L(v) for v in coefficients(dist)]))
    rr = x ** 2 + y ** 2
    radial = (1 + c["k1"] * rr + c["k2"] * rr ** 2 + c["k3"] * rr ** 3) \
        / (1 + c["k4"] * rr + c["k5"] * rr ** 2 + c["k6"] * rr ** 3)
    tangential_x = 2 * c["p1"] * x * y + c["p2"] * (rr + 2 * x ** 2)
    tangential_y = c["p1"] * (rr + 2 * y ** 2) + 2 * c["p2"] * x * y
    prism_x = c["s1"] * rr + c["s2"] * rr ** 2
    prism_y = c["s3"] * rr + c["s4"] * rr ** 2
    return (fx * (x * radial + tangential_x + prism_x) + u0,
            fy * (y * radial + tangential_y + prism_y) + v0)


def tie_distance(t):
    """Distance of every value to the nearest k + 0.5."""
    fr = t - np.floor(t)
    return np.abs(fr - 0.5)


# ---- the tests' cameras and frames -----------------------------------------------------------------
def frames_bgr(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def frames_yuv(seed, n, h, w):
    """(y [n, h, w], u [n, h/2, w/2], v [n, h/2, w/2]) full-range random samples."""
    r = np.random.default_rng(seed)
    return (r.integers(0, 256, (n, h, w), dtype=np.uint8),
            r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8),
            r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8))


def rig_two(w, h):
    """Two different cameras: the example's 8-coefficient barrel and a pincushion."""
    return [(small_k(w, h), D8_EXAMPLE), (small_k(w, h), D4_PINCUSHION)]


# (name, K of (w, h), distortion): the cameras held to the independent evaluation
def checked_cameras(w, h):
    return [("barrel8", small_k(w, h), D8_EXAMPLE), ("barrel5", small_k(w, h), D5_BARREL),
            ("pincushion4", small_k(w, h), D4_PINCUSHION), ("twelve", small_k(w, h), D12),
            ("skew5", small_k(w, h, skew=0.37), D5_BARREL)]
