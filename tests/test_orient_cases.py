"""CPU: the numpy restatement of the rotated and flipped frames (tests/orient_cases.py) held to
numpy's own rot90 / flip / transpose, to one hand-worked 2 x 3 frame per orientation, and to the
statement of include/opk.h that the YUV -> BGR conversion commutes with it (tests/yuv_cases.py is
the numpy statement of that conversion)."""
import numpy as np
import pytest

from tests import orient_cases as oc
from tests import yuv_cases as yc


def by_numpy(a, rotate, flip):
    """a [h, w, c] as the reference's calls leave it: cv::transpose = np.transpose of the two image
    axes, cv::flip(0) = flip of the rows, (1) of the columns, (-1) of both."""
    t = lambda m: np.transpose(m, (1, 0, 2))
    if rotate == 0:
        return np.flip(a, 1) if flip else a
    if rotate == 90:
        return t(a) if flip else np.flip(t(a), 0)
    if rotate == 180:
        return np.flip(a, 0) if flip else np.flip(a, (0, 1))
    return np.flip(t(a), (0, 1)) if flip else np.flip(t(a), 1)


@pytest.mark.parametrize("rotate,flip", oc.CASES)
def test_restatement_equals_numpy_compositions(rotate, flip):
    a = oc.frames_bgr(3, 2, 5, 7)
    got = oc.bgr(a, rotate, flip)
    assert got.shape[1:3] == oc.size(7, 5, rotate)[::-1]
    for f in range(2):
        assert np.array_equal(got[f], by_numpy(a[f], rotate, flip))
    # without the flip the table is a rotation, counterclockwise by `rotate` degrees as np.rot90
    # counts them; the flip is the mirror of the source's columns ahead of it
    turned = np.rot90(np.flip(a[0], 1) if flip else a[0], rotate // 90, axes=(0, 1))
    assert np.array_equal(got[0], turned)


# S = [[a b c], [d e f]] (h = 2, w = 3), worked from the table of include/opk.h by hand
HAND = {
    (0, 0): ["abc", "def"],
    (0, 1): ["cba", "fed"],
    (90, 0): ["cf", "be", "ad"],
    (90, 1): ["ad", "be", "cf"],
    (180, 0): ["fed", "cba"],
    (180, 1): ["def", "abc"],
    (270, 0): ["da", "eb", "fc"],
    (270, 1): ["fc", "eb", "da"],
}


@pytest.mark.parametrize("rotate,flip", oc.CASES)
def test_hand_worked_frame(rotate, flip):
    s = np.frombuffer(b"abcdef", np.uint8).reshape(1, 2, 3, 1)
    got = oc.plane(s, rotate, flip)[0, :, :, 0]
    assert [bytes(row).decode() for row in got] == HAND[(rotate, flip)]


def test_angles_the_reference_accepts():
    for rotate in range(-720, 721):
        want = {0: 0, 90: 90, 180: 180, 270: 270, -90: 270, -180: 180, -270: 90}.get(
            int(np.fmod(rotate, 360)))
        assert oc.normalize(rotate) == want, rotate


def test_index_maps_invert_each_other():
    w, h = 5, 3
    for rotate, flip in oc.CASES:
        ow, oh = oc.size(w, h, rotate)
        for sy in range(h):
            for sx in range(w):
                x, y = oc.oriented_index(sx, sy, w, h, rotate, flip)
                assert 0 <= x < ow and 0 <= y < oh
                assert oc.source_index(x, y, w, h, rotate, flip) == (sx, sy)


@pytest.mark.parametrize("rotate,flip", oc.CASES)
def test_yuv_to_bgr_commutes(rotate, flip):
    """Width and height are even: 2 x 2 blocks go to 2 x 2 blocks, so converting the oriented YUV
    frames gives the oriented conversion, for NV12 and I420 alike."""
    y, u, v = oc.yuv_planes(5, 2, 6, 10)
    want = oc.bgr(yc.yuv420_to_bgr(y, u, v), rotate, flip)
    assert np.array_equal(yc.yuv420_to_bgr(*oc.i420(y, u, v, rotate, flip)), want)
    oy, ouv = oc.nv12(y, yc.interleave(u, v), rotate, flip)
    assert np.array_equal(yc.nv12_to_bgr(oy, ouv), want)
