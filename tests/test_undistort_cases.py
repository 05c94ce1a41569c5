"""CPU: the numpy restatement of the undistortion text (tests/undistort_cases.py) held to things it
was not derived from -- an evaluation of (u, v) without the row accumulation in np.longdouble, and
answers worked out from the include/opk.h text by hand."""
import numpy as np
import pytest

from tests import undistort_cases as uc

# the sizes the GPU tests use, plus the reference's own frame size for its example lens
SIZES = [(50, 37), (200, 120), (52, 38), (160, 90)]


def _held_to_independent(name, K, dist, w, h):
    u, v = uc.uv(K, dist, w, h)
    iu, iv = uc.independent_uv(K, dist, w, h)
    # the precondition: no product within 1e-7 of a rounding tie, so 1e-9 px cannot flip an integer
    tie = min(uc.tie_distance(u * 32).min(), uc.tie_distance(v * 32).min())
    err = max(np.abs(u - iu).max(), np.abs(v - iv).max())
    print("%s %dx%d: |restatement - independent| %.2e px, nearest tie %.2e" % (name, w, h, err, tie))
    assert tie >= 1e-7, (name, w, h, tie)
    assert err <= 1e-9, (name, w, h, err)
    m1, m2 = uc.fixed_maps(u, v)
    n1, n2 = uc.fixed_maps(iu.astype(np.float64), iv.astype(np.float64))
    assert np.array_equal(m1, n1) and np.array_equal(m2, n2), (name, w, h)


@pytest.mark.parametrize("size", SIZES)
def test_case_cameras_equal_the_independent_evaluation(size):
    w, h = size
    for name, K, dist in uc.checked_cameras(w, h):
        _held_to_independent(name, K, dist, w, h)


@pytest.mark.parametrize("name,dist", [("example8", uc.D8_EXAMPLE), ("barrel5", uc.D5_BARREL)])
def test_the_example_lens_at_its_own_size(name, dist):
    _held_to_independent(name, uc.K_EXAMPLE, dist, 1280, 1024)


# ---- known answers from the text ---------------------------------------------------------------------
@pytest.mark.parametrize("K", [uc.K_EXAMPLE, uc.small_k(50, 37)])
def test_zero_coefficients_are_the_identity(K):
    w, h = 50, 37
    m1, m2 = uc.maps(K, np.zeros(4), w, h)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    assert np.array_equal(m1[..., 0], jj) and np.array_equal(m1[..., 1], ii)
    assert not m2.any()
    frame = uc.frames_bgr(3, 1, h, w)[0]
    assert np.array_equal(uc.remap(frame, m1, m2), frame)   # last row and column included


def test_one_pixel_by_hand():
    """K = diag(100, 100) with centre (50, 40), k1 = 0.5, pixel (j, i) = (70, 60): x = y = 0.2,
    r2 = 0.08, kr = 1.04, xd = yd = 0.208, u = 70.8, v = 60.8; u*32 = 2265.6 -> 2266 = 70*32 + 26,
    v*32 = 1945.6 -> 1946 = 60*32 + 26."""
    K = np.array([[100., 0., 50.], [0., 100., 40.], [0., 0., 1.]])
    u, v = uc.uv(K, [0.5, 0, 0, 0], 80, 64)
    assert abs(u[60, 70] - 70.8) < 1e-12 and abs(v[60, 70] - 60.8) < 1e-12
    m1, m2 = uc.fixed_maps(u, v)
    assert m1[60, 70].tolist() == [70, 60] and m2[60, 70] == 26 * 32 + 26
    # and the remap there: weights of fraction (26, 26) on the four taps
    frame = uc.frames_bgr(4, 1, 64, 80)[0]
    wt = uc.weight_table()[26, 26]
    want = (frame[60, 70].astype(np.int64) * wt[0, 0] + frame[60, 71].astype(np.int64) * wt[0, 1]
            + frame[61, 70].astype(np.int64) * wt[1, 0] + frame[61, 71].astype(np.int64) * wt[1, 1]
            + 16384) >> 15
    assert wt.sum() == 32768
    assert np.array_equal(uc.remap(frame, m1, m2)[60, 70], want)


def test_one_pixel_by_hand_every_term():
    """K = diag(100, 100) with centre (50, 40), pixel (j, i) = (100, 90): x = y = 0.5, r2 = 0.5,
    2xy = 0.5.  k1 k2 k3 = 0.2 0.4 0.8: numerator 1 + 0.1 + 0.1 + 0.1 = 1.3; k4 k5 k6 = 0.4 0.8 1.6:
    denominator 1 + 0.2 + 0.2 + 0.2 = 1.6; kr = 0.8125.  p1 p2 = 0.02 0.04, s1 .. s4 = 0.01 0.04
    0.03 0.08:
      xd = 0.40625 + 0.02*0.5 + 0.04*(0.5 + 0.5) + 0.01*0.5 + 0.04*0.25 = 0.47125
      yd = 0.40625 + 0.02*(0.5 + 0.5) + 0.04*0.5 + 0.03*0.5 + 0.08*0.25 = 0.48125
    u = 97.125, v = 88.125; u*32 = 3108 = 97*32 + 4, v*32 = 2820 = 88*32 + 4.  Every coefficient
    carries its own weight: swapping any two of them changes xd or yd."""
    K = np.array([[100., 0., 50.], [0., 100., 40.], [0., 0., 1.]])
    dist = [0.2, 0.4, 0.02, 0.04, 0.8, 0.4, 0.8, 1.6, 0.01, 0.04, 0.03, 0.08]
    u, v = uc.uv(K, dist, 104, 92)
    assert abs(u[90, 100] - 97.125) < 1e-12 and abs(v[90, 100] - 88.125) < 1e-12
    m1, m2 = uc.fixed_maps(u, v)
    assert m1[90, 100].tolist() == [97, 88] and m2[90, 100] == 4 * 32 + 4
    iu, iv = uc.independent_uv(K, dist, 104, 92)
    assert abs(float(iu[90, 100]) - 97.125) < 1e-12 and abs(float(iv[90, 100]) - 88.125) < 1e-12


def test_pincushion_corners_read_the_border():
    w, h = 50, 37
    m1, m2 = uc.maps(uc.small_k(w, h), uc.D4_PINCUSHION, w, h)
    sx, sy = m1[..., 0].astype(int), m1[..., 1].astype(int)
    inside = np.zeros((h, w, 2, 2), bool)
    for ky in range(2):
        for kx in range(2):
            inside[..., ky, kx] = (sy + ky >= 0) & (sy + ky < h) & (sx + kx >= 0) & (sx + kx < w)
    none = ~inside.any((2, 3))
    some = inside.any((2, 3)) & ~inside.all((2, 3))
    assert none[0, 0] and none[h - 1, w - 1] and none.sum() > 8 and some.sum() > 8
    white = np.full((h, w, 3), 255, np.uint8)
    out = uc.remap(white, m1, m2)
    assert not out[none].any()
    # partial sums: 255 times the weights of the taps inside, by the text's formula
    wt = uc.weight_table()[m2 >> 5, m2 & 31]
    want = ((255 * (wt * inside).sum((2, 3)) + 16384) >> 15).astype(np.uint8)
    assert np.array_equal(out[..., 0], want) and np.array_equal(out[..., 2], want)
    assert ((want[some] > 0) & (want[some] < 255)).any()
    assert (out[inside.all((2, 3))] == 255).all()


def test_huge_k3_overflows_int32_then_wraps_the_short():
    w, h = 50, 37
    K = uc.small_k(w, h)
    u, v = uc.uv(K, uc.D5_K3_HUGE, w, h)
    m1, m2 = uc.fixed_maps(u, v)
    # the corners: u*32 is past int32 -> INT_MIN -> INT_MIN >> 5 = -2^26, low 16 bits 0, fraction 0
    for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert abs(u[i, j] * 32) > 2 ** 31 and abs(v[i, j] * 32) > 2 ** 31
        assert m1[i, j].tolist() == [0, 0] and m2[i, j] == 0
    # further in: the product fits int32 but the pixel index does not fit the short
    fits = (np.abs(u * 32) < 2 ** 31 - 1) & (np.abs(v * 32) < 2 ** 31 - 1)
    iu = np.where(fits, np.rint(np.where(fits, u, 0) * 32), 0).astype(np.int64)
    wraps = fits & (np.abs(iu >> 5) > 32767)
    assert wraps.sum() > 20
    low = ((iu >> 5) & 0xffff).astype(np.uint16).view(np.int16)
    assert np.array_equal(m1[..., 0][wraps], low[wraps])
    assert (m1[..., 0][wraps].astype(np.int64) != (iu >> 5)[wraps]).all()
    # the remap of such a map still reads only what is inside the frame
    out = uc.remap(uc.frames_bgr(5, 1, h, w)[0], m1, m2)
    assert out.shape == (h, w, 3)
