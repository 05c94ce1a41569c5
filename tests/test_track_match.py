"""CPU: opk_match_people (host/track_match.cpp) against the numpy restatement of the matcher in
tests/lk_cases.py -- random people and entries, masked statuses, exact ties, thresholds at equality,
empty sides -- and the host-only argument checks of the person-id entry points."""
import ctypes

import numpy as np
import pytest

from openpose_amd import _lib, api
from tests import lk_cases as lk

OPK_ERR_ARG, OPK_ERR_STATE = 1, 3   # include/opk.h
SIZE = (320, 240)                    # threshold max(10, 30 * sqrt(320 * 240) / 960) = 10


def _both(entries, ids, people, size=SIZE, next_id=None, **kw):
    next_id = (max(ids) + 1 if len(ids) else 0) if next_id is None else next_id
    got = api.match_people(entries, ids, people, size, next_id, **kw)
    want = lk.match_people(entries, ids, people, size, next_id, **kw)
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1] == want[1]
    return got


def _people(rng, m, parts=25, spread=200.0):
    p = np.zeros((m, parts, 3), np.float32)
    centre = rng.uniform(40, spread, (m, 1, 2))
    p[:, :, :2] = centre + rng.uniform(-20, 20, (m, parts, 2))
    p[:, :, 2] = rng.random((m, parts)) < 0.15
    return p


@pytest.mark.parametrize("seed", range(12))
def test_random_people_and_entries(seed):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 7)), int(rng.integers(1, 9))
    people = _people(rng, m)
    # entries: some are people moved by a few pixels (matches), some strangers, some far jitter
    entries = _people(rng, n)
    for e in range(n):
        if rng.random() < 0.7:
            src = people[int(rng.integers(m))]
            entries[e, :, :2] = src[:, :2] + rng.uniform(-1, 1, (25, 2)) * rng.choice([2.0, 9.0, 14.0])
            entries[e, :, 2] = rng.choice([0, 0, 0, 1, 3], 25)
    ids = np.sort(rng.choice(40, n, replace=False))
    got, nid = _both(entries, ids, people)
    assert len(set(got.tolist())) == m, "ids are unique"
    # a wider and a narrower frame move the distance threshold
    _both(entries, ids, people, size=(1280, 720))
    _both(entries, ids, people, size=(64, 48), inlier_ratio=0.9)


def test_all_statuses_masked():
    rng = np.random.default_rng(1)
    people, entries = _people(rng, 3), _people(rng, 4)
    masked = people.copy()
    masked[:, :, 2] = 1
    ids, nid = _both(entries, [2, 5, 6, 9], masked)
    assert ids.tolist() == [10, 11, 12] and nid == 13     # nobody is active: all new
    e = entries.copy()
    e[:, :, 2] = 3
    ids, nid = _both(e, [2, 5, 6, 9], people)
    assert ids.tolist() == [10, 11, 12]
    # one person masked, its twin not: only the twin can match
    people[1] = people[0]
    people[1, :, 2] = 1
    e = np.stack([people[0]])
    e[0, :, 2] = 0
    ids, _ = _both(e, [7], people)
    assert ids[0] == 7 and ids[1] != 7


def test_exact_ties():
    rng = np.random.default_rng(2)
    one = _people(rng, 1)
    one[:, :, 2] = 0
    # two identical entries: the lower id wins ... and then, as the rounds are written, the person
    # is taken again by the second candidate of the same round
    ids, nid = _both(np.concatenate([one, one]), [3, 8], one)
    assert ids.tolist() == [8] and nid == 9
    # two identical people, one entry: the lower person index gets it
    ids, nid = _both(one, [4], np.concatenate([one, one]))
    assert ids.tolist() == [4, 5] and nid == 6
    # two identical people and two identical entries (the first frame of a tracker with twins)
    ids, nid = _both(np.concatenate([one, one]), [0, 1], np.concatenate([one, one]), next_id=2)
    assert ids.tolist() == [1, 2] and nid == 3
    # equal totals between different pairs: lower entry id first
    a, b = one.copy(), one.copy()
    a[0, :, 0] += 3
    b[0, :, 0] -= 3
    ids, _ = _both(np.concatenate([a, b]), [1, 2], one)
    assert ids.tolist() == [2]


def test_thresholds_at_equality():
    p = np.zeros((1, 4, 3), np.float32)
    p[0, :, :2] = [[50, 50], [60, 50], [50, 60], [60, 60]]
    e = p.copy()
    e[0, :2, 0] += 10          # two parts exactly at the threshold 10: `<` makes them outliers
    ids, _ = _both(e, [0], p)  # 2 of 4 inliers: score 0.5 >= 0.5
    assert ids.tolist() == [0]
    ids, _ = _both(e, [0], p, inlier_ratio=0.5000001)
    assert ids.tolist() == [1]
    e[0, 2, 0] += 10           # 1 of 4
    ids, _ = _both(e, [0], p)
    assert ids.tolist() == [1]
    # the frame size at which distance * sqrt(w * h) / 960 passes 10: 320 x 320 gives exactly 10
    assert lk.match_threshold(30, 320, 320) == np.float32(10)
    e = p.copy()
    e[0, :, 0] += 10.5
    assert _both(e, [0], p, size=(320, 320))[0].tolist() == [1]
    assert _both(e, [0], p, size=(352, 320))[0].tolist() == [1]   # threshold 10.488
    assert _both(e, [0], p, size=(384, 320))[0].tolist() == [0]   # threshold 10.954
    # inlier ratio 0: a pair with no inlier ties the initial best score 0 and is a candidate
    e[0, :, 0] += 100
    assert _both(e, [0], p, inlier_ratio=0.0)[0].tolist() == [0]


def test_empty_sides():
    rng = np.random.default_rng(3)
    people = _people(rng, 3)
    ids, nid = _both(np.zeros((0, 25, 3), np.float32), [], people, next_id=5)
    assert ids.tolist() == [5, 6, 7] and nid == 8
    ids, nid = _both(_people(rng, 2), [1, 2], np.zeros((0, 25, 3), np.float32))
    assert ids.shape == (0,) and nid == 3


def test_argument_errors():
    L = _lib.load()
    nid = ctypes.c_longlong(0)
    p = np.zeros((1, 2, 3), np.float32)
    ids = np.zeros(2, np.int64)
    out = np.zeros(1, np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    e2 = np.zeros((2, 2, 3), np.float32)
    assert L.opk_match_people(ptr(e2), ptr(ids), 2, ptr(p), 1, 2, 0.5, 30.0, 64, 48,
                              ctypes.byref(nid), ptr(out)) == OPK_ERR_ARG   # ids not ascending
    assert L.opk_match_people(None, None, 0, ptr(p), 1, 2, 0.5, 30.0, 0, 48, ctypes.byref(nid),
                              ptr(out)) == OPK_ERR_ARG
    assert L.opk_match_people(None, None, 0, ptr(p), 1, 2, 0.5, 30.0, 64, 48, None,
                              ptr(out)) == OPK_ERR_ARG
    assert L.opk_match_people(None, None, 0, ptr(p), 1, 2, 0.5, 30.0, 64, 48, ctypes.byref(nid),
                              ptr(out)) == 0 and out[0] == 0 and nid.value == 1


def test_pyramid_layout_and_levels():
    lay = api.pyramid_layout(1280, 720, 3)
    assert lay["sizes"] == [(1280, 720), (640, 360), (320, 180)]
    assert lay["offsets"] == [0, 1280 * 720, 1280 * 720 + 2 * 640 * 360]
    assert lay["frame_bytes"] == 1280 * 720 + 2 * 640 * 360 + 4 * 320 * 180   # 1.61 MB
    lay = api.pyramid_layout(197, 131, 3)
    assert lay["sizes"] == [(197, 131), (99, 66), (50, 33)]
    assert all(o % 16 == 0 for o in lay["offsets"]) and lay["frame_bytes"] % 16 == 0
    assert api.pyramid_layout(1, 1, 1)["sizes"] == [(1, 1)]
    for levels in (0, 4):
        with pytest.raises(api.OpkError, match="opk error 1"):
            api.pyramid_layout(64, 48, levels)


def test_tracker_attach_rules_host_only():
    """The state and argument checks of opk_pose_attach_tracker need no device."""
    ctx, other = api.Context.host_only(), api.Context.host_only()
    L = ctx.L
    pose = api.PoseExtractor(ctx, None)
    t, t2, foreign = api.Tracker(ctx), api.Tracker(ctx), api.Tracker(other)
    assert L.opk_pose_attach_tracker(pose.h, None) == OPK_ERR_ARG
    assert L.opk_pose_attach_tracker(pose.h, foreign.h) == OPK_ERR_ARG
    assert L.opk_pose_person_ids(pose.h, 0, None) == OPK_ERR_STATE      # no tracker
    pose.attach(tracker=t)
    assert L.opk_pose_attach_tracker(pose.h, t2.h) == OPK_ERR_STATE     # a second one
    assert L.opk_pose_person_ids(pose.h, 0, None) == OPK_ERR_STATE      # nothing collected
    # a submit without frames is refused before any device work
    fake = ctypes.c_void_p(0x1000)
    assert L.opk_pose_submit_net_output(pose.h, fake, 1, 8, 8, 64, 64, 64, 64) == OPK_ERR_STATE
    assert b"tracker" in L.opk_last_error()
    pose.detach_tracker()
    t.close()                      # destroyed while attached counts as detached
    pose.attach(tracker=t2)
    t2.close()
    assert L.opk_pose_person_ids(pose.h, 0, None) == OPK_ERR_STATE
    assert b"no tracker" in L.opk_last_error()
    pose.close()
    foreign.close()
