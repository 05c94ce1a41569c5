"""The keypoint-render edge cases (tests/render_edge_cases.py) test what they claim, judged by the CPU
oracle alone: the off-frame person's box really is not grown, draw order across the 256-person round
of the compaction really is observable, the threshold ties really draw nothing / everything, and no
case leans on the 1e-4 ambiguity rule for more than the existing 1 % cap."""
import time

import numpy as np
import pytest

import oracle
from openpose_amd.api import LAYER_FACE, LAYER_HAND, LAYER_POSE
from tests import render_edge_cases as rc


def _changed(name, blend=True):
    out, _ = rc.oracle_render(name, blend)
    return np.any(out != rc.frame_of(name), axis=2)


@pytest.mark.parametrize("name", rc.CASES)
def test_case_shape_cost_and_ambiguity(name):
    (w, h), kind, kp, opts = rc.case(name)
    assert kp.dtype == np.float32 and kp.shape[1:] == (rc.PARTS[kind], 3)
    # seeded: the same arrays on every call (NaN == NaN here)
    np.testing.assert_array_equal(kp, rc.case(name)[2])
    frame = rc.frame_of(name)
    oracle.lib()       # built and loaded before the clock starts
    oracle.render_tables()
    dt = np.inf
    for _ in range(2):     # the better of two on a busy host; one run when the first is quick
        t0 = time.perf_counter()
        out, amb = oracle.render_keypoints(frame, kp, **rc.oracle_kwargs(kind, opts))
        dt = min(dt, time.perf_counter() - t0)
        if dt < 2.0:
            break
    print("%s: %d px, %d ambiguous, oracle %.2f s" % (name, amb.size, int(amb.sum()), dt))
    assert dt < 2.0
    assert amb.mean() <= 0.01
    if name in rc.EXACT:
        assert not amb.any()
    assert not np.isnan(out).any()


@pytest.mark.parametrize("name,axis", [("left", 0), ("top", 1), ("touch0", 0)])
def test_off_edge_box_is_not_grown(name, axis):
    (w, h), kind, kp, _ = rc.case(name)
    drawn = kp[0, :, 2] > rc.THRESHOLD[kind]
    assert drawn.all()
    assert kp[0, :, axis].min() >= -30.0
    assert kp[0, :, axis].max() == 0.0 if name == "touch0" else kp[0, :, axis].max() <= -0.5
    span = [kp[0, :, a].max() - kp[0, :, a].min() for a in (0, 1)]
    span[axis] = 0.0 - kp[0, :, axis].min()           # the maximum stays 0
    assert (span[0] + span[1]) / 400.0 >= 1.0         # scale clamps to 1
    changed = _changed(name)
    if axis == 1:
        changed = changed.T                           # [column][row] for `top`: line = row
    assert changed[:, 0].any()
    assert not changed[:, 1].any() and not changed[:, 1:].any()
    # ... although the outside part's circle reaches line 1: the oracle's dist2 <= maxr2 with
    # scale 1 and BODY_25's part scale 1
    radius = np.float32(min(w, h)) / np.float32(100.0)
    maxr2 = np.float32(1) * np.float32(1) * (radius * radius * np.float32(1))
    lx, ly = kp[0, rc.OUTSIDE_PART, :2]
    x, y = (np.float32(1), np.float32(rc.OUTSIDE_AT)) if axis == 0 else (np.float32(rc.OUTSIDE_AT),
                                                                          np.float32(1))
    dist2 = (x - lx) * (x - lx) + (y - ly) * (y - ly)
    assert np.float32(0) <= dist2 <= maxr2
    # and the box alone keeps it from drawing there.  Three parts that no limb joins (0, the
    # outside part, 23), so only circles are drawn, the other two more than 150 px along the edge
    # from the outside part; scale 1 as before.  Part 0 at -0.5 leaves the maximum at 0: line 1
    # stays.  Part 0 at +0.5 -- nothing else differs -- grows the box and the outside part's
    # circle draws on line 1.
    pairs = np.asarray(oracle.render_tables()["BODY_25"]["pairs"]).reshape(-1, 2)
    trio = [0, rc.OUTSIDE_PART, 23]
    assert not any(a in trio and b in trio for a, b in pairs)
    along = (h, w)[axis]
    at = (int(rc.OUTSIDE_AT), 1) if axis == 0 else (1, int(rc.OUTSIDE_AT))    # [row, column]
    hit = {}
    for edge in (-0.5, 0.5):
        lone = np.zeros_like(kp)
        lone[0, trio] = kp[0, trio]
        lone[0, 0, axis], lone[0, 0, 1 - axis] = edge, 20.0
        lone[0, 23, axis], lone[0, 23, 1 - axis] = -5.0, along - 20.0
        out, amb = oracle.render_keypoints(rc.frame_of(name), lone, **rc.oracle_kwargs(kind, {}))
        assert not amb.any()
        hit[edge] = bool(np.any(out[at] != rc.frame_of(name)[at]))
    assert hit == {-0.5: False, 0.5: True}
    if name == "touch0":   # the part at x == 0.0 leaves the maximum at 0 and is drawn
        assert kp[0, rc.TOUCH_PART, 0] == 0.0 and changed[int(rc.TOUCH_AT), 0]


def test_straddle_has_people_inside_across_and_outside():
    (w, h), kind, kp, _ = rc.case("straddle")
    drawn = kp[..., 2] > rc.THRESHOLD[kind]
    inside = (kp[..., 0] >= 0) & (kp[..., 0] <= w - 1) & (kp[..., 1] >= 0) & (kp[..., 1] <= h - 1)
    n_in = (inside & drawn).sum(axis=1)
    n = drawn.sum(axis=1)
    assert (n_in == 0).any()                 # every drawn part outside the frame
    assert ((n_in > 0) & (n_in < n)).any()   # across the edge
    assert (n_in == n).any()
    # centres off each of the four edges
    cx, cy = kp[..., 0].mean(axis=1), kp[..., 1].mean(axis=1)
    assert (cx < 0).any() and (cx > w).any() and (cy < 0).any() and (cy > h).any()
    assert _changed("straddle").any()


def test_people_restates_people_on():
    """_people() with its default centre range is tests/test_render.py's people_on(), draw for draw."""
    from tests.test_render import people_on
    for n, parts, seed, spread in ((6, 25, 3, 0.15), (5, 70, 4, 0.08)):
        np.testing.assert_array_equal(rc._people(200, 150, n, parts, seed, spread),
                                      people_on(200, 150, n, parts, seed, spread))


def test_far_draws_nothing():
    (w, h), _, kp, _ = rc.case("far")
    assert np.abs(kp[:3, :, 0]).min() > 9e5 and np.abs(kp[3, :, :2]).min() > 9e3
    assert not _changed("far").any()
    out, _ = rc.oracle_render("far", False)
    assert not out.any()


@pytest.mark.parametrize("name", ["coincident-on", "coincident-off"])
def test_coincident_draws_its_circles_only(name):
    _, _, kp, _ = rc.case(name)
    assert (kp[0, :, :2] == kp[0, 0, :2]).all()
    out, amb = rc.oracle_render(name)
    assert _changed(name).any() and not np.isnan(out).any()


def test_axis_limbs_are_axis_parallel():
    _, _, kp, _ = rc.case("axis")
    pairs = np.asarray(oracle.render_tables()["BODY_25"]["pairs"]).reshape(-1, 2)
    d = kp[:, pairs[:, 1], :2] - kp[:, pairs[:, 0], :2]
    assert ((d[..., 0] == 0) ^ (d[..., 1] == 0)).all()
    assert (kp[..., :2] == np.rint(kp[..., :2])).all()
    assert (d[..., 0] > 0).any() and (d[..., 0] < 0).any()     # angle 0 and pi
    assert (d[..., 1] > 0).any() and (d[..., 1] < 0).any()     # +-pi/2
    assert _changed("axis").any()


def test_nonfinite_values_sit_on_drawn_parts():
    (w, h), kind, kp, _ = rc.case("nonfinite")
    base = rc.case("straddle")[2]
    th = rc.THRESHOLD[kind]
    xy = ~np.isfinite(kp[..., :2]).all(axis=2)
    assert xy.sum() == 12 and (kp[..., 2][xy] > th).all()
    for v in (np.inf, -np.inf):
        assert (kp[..., 0] == v).any() and (kp[..., 1] == v).any()
    assert np.isnan(kp[..., 0]).any() and np.isnan(kp[..., 1]).any()
    nan_score = np.isnan(kp[..., 2])
    assert nan_score.sum() == 5 and (base[..., 2][nan_score] > th).all()
    # the branch the case is named for: limbs with a non-finite end and both scores above the
    # threshold (render.hip's limb bound is then NaN or inf), each value among them, on people
    # whose box -- the oracle's, which skips NaN and lets inf through -- meets the frame
    pairs = np.asarray(oracle.render_tables()["BODY_25"]["pairs"]).reshape(-1, 2)
    seen = set()
    for p in range(len(kp)):
        ok = kp[p, :, 2] > th
        with np.errstate(invalid="ignore"):
            x, y = kp[p, ok, 0], kp[p, ok, 1]
            minx, maxx = min([w] + list(x[x < w])), max([0] + list(x[x > 0]))
            miny, maxy = min([h] + list(y[y < h])), max([0] + list(y[y > 0]))
        grow = 50.0 if maxx != 0 and maxy != 0 else 0.0
        meets = maxx + grow >= 0 and minx - grow <= w - 1 and maxy + grow >= 0 and miny - grow <= h - 1
        for a, b in pairs:
            ends = kp[p, [a, b], :2]
            if ok[a] and ok[b] and meets and not np.isfinite(ends).all():
                seen |= {"nan" if np.isnan(v) else str(v) for v in ends.ravel() if not np.isfinite(v)}
    assert seen == {"nan", "inf", "-inf"}
    out, _ = rc.oracle_render("nonfinite")
    assert not np.isnan(out).any() and not np.isinf(out).any()
    assert _changed("nonfinite").any()
    # the non-finite values matter: the drawing differs from straddle's on the same frame
    plain, _ = oracle.render_keypoints(rc.frame_of("nonfinite"), base,
                                       **rc.oracle_kwargs(kind, {"googly": True}))
    assert np.any(plain != out)


def test_ties():
    th = np.float32(rc.THRESHOLD[LAYER_POSE])
    at, above = rc.case("ties-at")[2], rc.case("ties-above")[2]
    assert at.dtype == np.float32 and (at[..., 2] == th).all()
    assert (above[..., 2] == np.nextafter(th, np.float32(1))).all() and (above[..., 2] > th).all()
    np.testing.assert_array_equal(at[..., :2], above[..., :2])
    assert not _changed("ties-at").any()
    assert not rc.oracle_render("ties-at", False)[0].any()
    assert _changed("ties-above").any()


def _cover(name, lo, hi):
    """pixels that people lo .. hi - 1 of the case draw on."""
    (w, h), kind, kp, opts = rc.case(name)
    frame = rc.frame_of(name)
    out, _ = oracle.render_keypoints(frame, kp[lo:hi], **rc.oracle_kwargs(kind, opts))
    return np.any(out != frame, axis=2)


@pytest.mark.parametrize("name", ["hands300", "faces300"])
def test_crowd_crosses_the_round_boundary(name):
    """People of the second round of 256 draw over people of the first.  For hands the order of
    the two is observable (a part's color depends on the part, and addColorWeighted does not
    commute).  FACE has one color, so a pixel's value depends only on how often it is drawn: there
    what is observable is a person of the second round going missing."""
    (w, h), kind, kp, opts = rc.case(name)
    assert len(kp) == 300
    drawn = (kp[..., 2] > rc.THRESHOLD[kind]).sum(axis=1)
    assert (drawn == (5 if kind == LAYER_HAND else 6)).all()
    both = _cover(name, 0, 256) & _cover(name, 256, 300)
    assert both.any()
    out, _ = rc.oracle_render(name)
    frame = rc.frame_of(name)
    kw = rc.oracle_kwargs(kind, opts)
    first, _ = oracle.render_keypoints(frame, kp[:256], **kw)
    assert np.any(first != out)                                   # the second round is seen
    swapped, _ = oracle.render_keypoints(frame, np.concatenate([kp[256:], kp[:256]]), **kw)
    reverse, _ = oracle.render_keypoints(frame, kp[::-1], **kw)
    if kind == LAYER_HAND:
        assert np.any(reverse != out)
        assert np.any(swapped[both] != out[both])                 # ... and so is its place in the order
    else:
        assert len(oracle.render_tables()["FACE"]["colors"]) == 3    # one color
        np.testing.assert_array_equal(reverse, out)


@pytest.mark.parametrize("name,n", [("hands256", 256), ("hands257", 257), ("hands1024", 1024)])
def test_crowd_boundary_counts(name, n):
    (w, h), kind, kp, _ = rc.case(name)
    assert (w, h) == rc.CROWD_SIZE and kind == LAYER_HAND and len(kp) == n
    assert _cover(name, n - 1, n).any()               # the last person is seen
    assert _cover(name, 255, 256).any()               # and the first round's last


@pytest.mark.parametrize("name", sorted(rc.TINY))
def test_tiny_frames_are_drawn_on(name):
    (w, h), _, kp, _ = rc.case(name)
    assert (w, h) == rc.TINY[name]
    assert kp[..., 0].min() >= -3 and kp[..., 0].max() <= w + 3
    assert kp[..., 1].min() >= -3 and kp[..., 1].max() <= h + 3
    changed = _changed(name)
    assert changed[0, 0] and changed[h - 1, w - 1]
    assert w * h == 1 or not changed.all()
