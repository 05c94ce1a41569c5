"""CPU: the numpy restatement of the person-id definition (tests/lk_cases.py) against itself --
the pyramid's exactness claim, hand-checkable Lucas-Kanade cases, and the property the GPU tracker
test inherits: on the committed synthetic sequence the oracle alone keeps every person's id."""
import numpy as np
import pytest

from tests import lk_cases as lk

SIZES = [(1, 1), (3, 2), (4, 5), (197, 131), (192, 128)]   # (w, h)


def test_grey_known_answers():
    px = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]],
                  np.uint8)
    # 1868 + 9617 + 4899 = 16384: white is exactly 255; the others by hand
    want = [0, 255, (1868 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14, (4899 * 255 + 8192) >> 14,
            (1868 + 2 * 9617 + 3 * 4899 + 8192) >> 14]
    np.testing.assert_array_equal(lk.grey(px), np.array(want, np.float32))


def test_reflect():
    assert [lk.reflect(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [lk.reflect(i, 2) for i in (-2, -1, 2, 3)] == [0, 1, 0, 1]
    assert [lk.reflect(i, 1) for i in (-2, 0, 2)] == [0, 0, 0]


@pytest.mark.parametrize("w,h", SIZES)
def test_pyramid_is_exact_in_any_order(w, h):
    g = lk.grey(np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8))
    a, b = lk.pyramid(g, 3, order=0), lk.pyramid(g, 3, order=1)
    for lv in range(3):
        assert a[lv].shape == b[lv].shape
        np.testing.assert_array_equal(a[lv].view(np.uint32), b[lv].view(np.uint32))
    assert a[1].shape == ((h + 1) // 2, (w + 1) // 2)
    assert a[2].shape == ((a[1].shape[0] + 1) // 2, (a[1].shape[1] + 1) // 2)
    k1, k2 = a[1].astype(np.float64) * 256, a[2].astype(np.float64) * 65536
    assert np.array_equal(k1, np.round(k1)) and k1.max(initial=0) < 2 ** 16
    assert np.array_equal(k2, np.round(k2)) and k2.max(initial=0) < 2 ** 24
    # a constant image stays constant: the taps sum to 256 with the reflected border
    c = lk.pyramid(np.full((h, w), 200, np.float32), 3)
    assert all((lv == 200).all() for lv in c)


def _pyrs(frames):
    return {f: lk.pyramid(lk.grey(frames[f]), 3) for f in range(frames.shape[0])}


def test_lk_follows_a_shift_and_flags_the_rest():
    frames = lk.lk_frames()
    pyr = _pyrs(frames)
    pts = lk.lk_grid()
    out = lk.lk_points(pyr, pts)
    # interior points on the shifted pair move by about (+2, +1)
    mid = np.nonzero((pts["frame_j"] == 1) & (pts["frame_i"] == 0) & (pts["status"] == 0) &
                     (np.abs(pts["x"] - 96) < 30) & (np.abs(pts["y"] - 64) < 14))[0]
    assert mid.size >= 4 and (out["status"][mid] == 0).all()
    assert np.abs(out["x"][mid] - pts["x"][mid] - 2).max() < 0.75
    assert np.abs(out["y"][mid] - pts["y"][mid] - 1).max() < 0.75
    # level 2 is 48 x 32: x < 44 or y < 44 leaves its radius-11 patch -> status 3
    edge = (pts["status"] == 0) & ((pts["x"] < 44) | (pts["y"] < 44)) & np.isfinite(pts["x"])
    assert (out["status"][edge] == 3).all()
    # untouched: status-in, non-finite, huge, unknown frames
    keep = pts["status"] != 0
    assert np.array_equal(out[keep].tobytes(), pts[keep].tobytes())
    for i in range(len(pts)):
        big = not (abs(pts["x"][i]) < 2 ** 24 and abs(pts["y"][i]) < 2 ** 24)
        if pts["status"][i] == 0 and (big or pts["frame_j"][i] == 3 or pts["frame_i"][i] == -1):
            assert out["status"][i] == 3
            assert out["x"][i].tobytes() == pts["x"][i].tobytes() and out["y"][i].tobytes() == pts["y"][i].tobytes()
    # a flat I has no gradient: the determinant is 0
    flat = (pts["frame_i"] == 2)
    assert (out["status"][flat] == 3).all()
    # 2^24 - 1 is still a coordinate (far outside: status 3 by the bounds test, not by the range test)
    assert out["status"][pts["x"] == 16777215][0] == 3


def test_lk_point_by_hand():
    """One interior point computed with plain Python loops, as the definition words it."""
    frames = lk.lk_frames()
    pyr = _pyrs(frames)
    F = np.float32
    x, y = F(77.25), F(70.75)
    pI, pJ, status = [x * F(0.25), y * F(0.25)], [x * F(0.25), y * F(0.25)], 0
    for lv in (2, 1, 0):
        I, J = pyr[0][lv], pyr[1][lv]
        h, w = I.shape
        xi, yi, xj, yj = int(pI[0]), int(pI[1]), int(pJ[0]), int(pJ[1])
        assert 11 <= xi < w - 11 and 11 <= yi < h - 11 and 10 <= xj < w - 10 and 10 <= yj < h - 10
        s = [F(0)] * 5
        for i in range(-10, 11):
            for j in range(-10, 11):
                ix = (I[yi + i, xi + j + 1] - I[yi + i, xi + j - 1]) / F(2)
                iy = (I[yi + i + 1, xi + j] - I[yi + i - 1, xi + j]) / F(2)
                it = J[yj + i, xj + j] - I[yi + i, xi + j]
                for k, v in enumerate((ix * ix, iy * iy, ix * iy, ix * it, iy * it)):
                    s[k] = F(s[k] + F(v))
        sxx, syy, sxy, sxt, syt = s
        den = F(F(sxx * syy) - F(sxy * sxy))
        if abs(den) < F(1e-9):
            status = 3
        else:
            pJ[0] = F(pJ[0] + F(F(F(F(-1) * syy) * sxt + F(sxy * syt)) / den))
            pJ[1] = F(pJ[1] + F(F(F(F(-1) * sxx) * syt + F(sxt * sxy)) / den))
        if lv:
            pI, pJ = [pI[0] * F(2), pI[1] * F(2)], [pJ[0] * F(2), pJ[1] * F(2)]
    got = lk.lk_points(pyr, np.array([(0, 1, x, y, 0)], lk.LK_POINT))[0]
    assert (got["x"].tobytes(), got["y"].tobytes(), int(got["status"])) == (
        F(pJ[0]).tobytes(), F(pJ[1]).tobytes(), status)


@pytest.fixture(scope="module")
def sequence():
    frames, kps, truth = lk.synthetic_sequence()
    greys = [lk.grey(f) for f in frames]
    return frames, kps, truth, greys


def test_oracle_keeps_every_id_on_the_synthetic_sequence(sequence):
    frames, kps, truth, greys = sequence
    assert frames.shape == (10, 240, 320, 3)
    assert [len(t) for t in truth] == [3, 3, 3, 2, 2, 2, 3, 3, 3, 3]
    assert all((k[:, :, 2] < lk.CONFIDENCE).sum() == 3 * len(k) for k in kps)
    t = lk.Tracker()
    ids = t.run(greys, kps)
    seen = lk.stable_ids(ids, truth)
    print("ids per rectangle:", seen, "entries:", sorted(t.entries))
    assert all(len(v) == 1 for v in seen.values()), seen
    assert sorted(next(iter(v)) for v in seen.values()) == [0, 1, 2]
    assert sorted(t.entries) == [0, 1, 2] and t.next_id == 3


def test_oracle_forgets_after_frames_to_delete(sequence):
    """frames_to_delete = 2: a person gone for 4 frames comes back with a new id, gone for 2 with
    the old one (the counter test is `counter++ > frames_to_delete`)."""
    frames, _, _, _ = sequence
    for gone, same in (((3, 4), True), ((3, 4, 5, 6), False)):
        fr, kps, truth = lk.synthetic_sequence(dropout=(1, gone))
        ids = lk.Tracker(frames_to_delete=2).run([lk.grey(f) for f in fr], kps)
        seen = lk.stable_ids(ids, truth)
        assert len(seen[0]) == 1 and len(seen[2]) == 1
        assert (len(seen[1]) == 1) == same, (gone, seen)


def test_oracle_frame_without_people_still_propagates(sequence):
    _, kps, truth, greys = sequence
    empty = np.zeros((0, 25, 3), np.float32)
    kps2 = [k if f != 4 else empty for f, k in enumerate(kps)]
    truth2 = [t if f != 4 else [] for f, t in enumerate(truth)]
    ids = lk.Tracker().run(greys, kps2)
    assert ids[4].shape == (0,)
    seen = lk.stable_ids(ids, truth2)
    assert all(len(v) == 1 for v in seen.values()), seen
