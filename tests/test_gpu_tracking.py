"""GPU: person ids across frames -- the grey + pyramid kernels, the Lucas-Kanade launch, the tracker
and its stage in the pose pipeline -- against the numpy restatement in tests/lk_cases.py.  Every
comparison is exact (bit patterns for floats)."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd import api, synth
from openpose_amd.api import Frames, Net, PoseExtractor, Tracker
from tests import lk_cases as lk

pytestmark = pytest.mark.gpu

OPK_ERR_ARG, OPK_ERR_STATE = 1, 3   # include/opk.h
CANARY = 0xA5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle_levels(bgr, levels):
    """[level][n, h, w] of uint8 BGR frames [n, h, w, 3]."""
    per = [lk.pyramid(lk.grey(f), levels) for f in bgr]
    return [np.stack([p[lv] for p in per]) for lv in range(levels)]


def _padded(planes, pad):
    """Each uint8 [n, rows, bytes] plane inside a canary buffer with `pad` more bytes per row."""
    out = []
    for p in planes:
        big = torch.full((p.shape[0], p.shape[1], p.shape[2] + pad), CANARY, dtype=torch.uint8,
                         device="cuda")
        big[:, :, :p.shape[2]] = p
        out.append(big)
    return out


def _build(ctx, fr, levels):
    """ctx.pyramid into the middle of a canary buffer; the bytes around the records must stay."""
    pyr = api.Pyramid(ctx, fr.n, fr.width, fr.height, levels)
    total = fr.n * pyr.layout["frame_bytes"]
    big = torch.full((total + 512,), CANARY, dtype=torch.uint8, device="cuda")
    pyr.buffer = big[256:256 + total]
    s = fr.struct()
    api.check(ctx.L.opk_pyramid_build(ctx.h, api._ptr(pyr.buffer), ctypes.byref(s), levels))
    ctx.sync()
    edge = torch.cat([big[:256], big[256 + total:]]).cpu().numpy()
    assert (edge == CANARY).all(), "bytes outside the pyramid records were written"
    return pyr


def _check_levels(pyr, want):
    for lv, w in enumerate(want):
        got = pyr.level(lv)
        assert got.shape == w.shape, (lv, got.shape, w.shape)
        np.testing.assert_array_equal(_bits(got), _bits(w), err_msg="level %d" % lv)


# ---- pyramid ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (4, 5), (197, 131)])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_pyramid_bgr(ctx, w, h, levels):
    bgr = np.random.default_rng(w * 131 + h).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    want = _oracle_levels(bgr, levels)
    t = torch.from_numpy(bgr).cuda()
    _check_levels(_build(ctx, Frames.bgr(t), levels), want)
    # an odd step inside a canary buffer (rows of w * 3 + 5 bytes)
    (big,) = _padded([t.reshape(3, h, w * 3)], 5)
    _check_levels(_build(ctx, Frames.bgr(big, width=w), levels), want)
    assert (big[:, :, w * 3:] == CANARY).all()
    # the convenience form gives the same records
    _check_levels(ctx.pyramid(t, levels), want)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("w,h", [(2, 2), (192, 128)])
@pytest.mark.parametrize("levels", [1, 3])
def test_pyramid_yuv_equals_pyramid_of_to_bgr(ctx, fmt, w, h, levels):
    rng = np.random.default_rng(w + h + len(fmt))
    bgr = torch.from_numpy(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)).cuda()
    fr = Frames.from_bgr(ctx, bgr, fmt)
    # full-range samples too, not only those a BGR frame converts to
    for p in fr.planes:
        p.copy_(torch.from_numpy(rng.integers(0, 256, tuple(p.shape), dtype=np.uint8)).cuda())
    back = fr.to_bgr(ctx)
    want = _oracle_levels(back.cpu().numpy(), levels)
    _check_levels(_build(ctx, fr, levels), want)
    _check_levels(ctx.pyramid(back, levels), want)
    # odd steps inside canary buffers
    big = _padded(fr.planes, 3)
    odd = Frames.nv12(*big, width=w) if fmt == "nv12" else Frames.i420(*big, width=w)
    _check_levels(_build(ctx, odd, levels), want)


def test_pyramid_argument_errors(ctx):
    t = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    s = Frames.bgr(t).struct()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for levels in (0, 4):
        assert ctx.L.opk_pyramid_build(ctx.h, api._ptr(buf), ctypes.byref(s), levels) == OPK_ERR_ARG
        with pytest.raises(api.OpkError, match="opk error 1"):
            ctx.pyramid(t, levels)
    assert ctx.L.opk_pyramid_build(ctx.h, api._ptr(buf), None, 3) == OPK_ERR_ARG
    assert ctx.L.opk_pyramid_level(ctx.h, api._ptr(buf), api._ptr(buf), 1, 8, 8, 3, 3) == OPK_ERR_ARG
    assert ctx.L.opk_pyramid_level(ctx.h, api._ptr(buf), api._ptr(buf), 1, 8, 8, 4, 0) == OPK_ERR_ARG


# ---- Lucas-Kanade -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lk_scene(ctx):
    frames = lk.lk_frames()
    oracle = {f: lk.pyramid(lk.grey(frames[f]), 3) for f in range(3)}
    pyr = ctx.pyramid(torch.from_numpy(frames).cuda())
    pts = lk.lk_grid()
    return frames, oracle, pyr, pts, lk.lk_points(oracle, pts)


def test_lk_scene_pyramid(lk_scene):
    _, oracle, pyr, _, _ = lk_scene
    assert pyr.layout["sizes"] == [(192, 128), (96, 64), (48, 32)]
    _check_levels(pyr, [np.stack([oracle[f][lv] for f in range(3)]) for lv in range(3)])


MAPPINGS = {"wave": 1, "thread": 0}   # the LK_WAVE switch: a wave per point (shipped) or a thread


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("count", [None, 1, 64, 65])
def test_lk_points_equal_the_oracle(ctx, lk_scene, count, mapping):
    _, _, pyr, pts, want = lk_scene
    with api.dev_switches(LK_WAVE=MAPPINGS[mapping]), api.launch_log() as log:
        got = ctx.lk_points(pyr, pts[:count])
    assert [k for _, k in log] == ["lk_points<%s>" % mapping]
    want = want[:count]
    assert len(got) % 64 != 0 or count == 64
    for name in ("frame_i", "frame_j", "status"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for name in ("x", "y"):
        bad = np.nonzero(got[name].view(np.uint32) != want[name].view(np.uint32))[0]
        assert bad.size == 0, (name, pts[bad[:5]], got[bad[:5]], want[bad[:5]])
    if count is None:
        moved = (want["status"] == 0) & (pts["status"] == 0)
        print("points followed: %d of %d, status 3: %d" % (moved.sum(), len(pts),
                                                           (want["status"] == 3).sum()))
        assert moved.sum() >= 20 and (want["status"] == 3).sum() >= 100


def test_lk_carry_frame_and_mixed_pairs(ctx, lk_scene):
    """Frame -1 is the carry record; one launch serves any mix of frame pairs."""
    frames, oracle, pyr, _, _ = lk_scene
    rng = np.random.default_rng(5)
    n = 1000
    pts = np.zeros(n, lk.LK_POINT)
    pts["frame_i"] = rng.choice([-1, 0, 1], n)
    pts["frame_j"] = rng.choice([-1, 0, 1, 2], n)
    pts["x"], pts["y"] = rng.uniform(40, 150, n), rng.uniform(40, 90, n)
    carry = ctx.pyramid(torch.from_numpy(frames[1:2]).cuda())
    want = lk.lk_points({-1: oracle[1], 0: oracle[0], 1: oracle[1], 2: oracle[2]}, pts)
    for switch in MAPPINGS.values():
        with api.dev_switches(LK_WAVE=switch):
            got = ctx.lk_points(pyr, pts, carry=carry)
        assert got.tobytes() == want.tobytes()
    assert (want["status"] == 0).sum() >= 300
    # a record of the batch buffer serves as the carry of another launch
    assert ctx.lk_points(pyr, pts, carry=pyr.frame(1)).tobytes() == want.tobytes()
    # no points: nothing to do
    assert len(ctx.lk_points(pyr, pts[:0])) == 0


# ---- tracker ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequence(ctx):
    frames, kps, truth = lk.synthetic_sequence()
    want = lk.Tracker().run([lk.grey(f) for f in frames], kps)
    return torch.from_numpy(frames).cuda(), kps, truth, want


def _same_ids(got, want):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg="frame %d" % f)


def test_tracker_batchings_equal_the_oracle(ctx, sequence):
    frames, kps, truth, want = sequence
    seen = lk.stable_ids(want, truth)
    assert all(len(v) == 1 for v in seen.values()), seen     # the oracle's own property
    t = Tracker(ctx)
    try:
        with api.launch_log() as log:
            _same_ids(t.update(frames, kps), want)
        # one LK launch for the fresh points of the batch, then one per frame with a stale entry:
        # the rectangle undetected in frames 3..5 is still fresh going into frame 3 (frame 2
        # detected it) and stale going into frames 4, 5 and 6
        assert [k for _, k in log].count("lk_points<wave>") == 1 + 3
        t.reset()
        with api.dev_switches(LK_WAVE=0):
            _same_ids(t.update(frames, kps), want)
        t.reset()
        _same_ids(t.update(frames[:4], kps[:4]) + t.update(frames[4:], kps[4:]), want)
        t.reset()
        _same_ids([t.update(frames[f:f + 1], kps[f:f + 1])[0] for f in range(10)], want)
        # without reset the state carries on: the same frames again keep the ids
        again = t.update(frames[9:], kps[9:])
        np.testing.assert_array_equal(again[0], want[9])
        assert t.update(frames[:0], []) == []
    finally:
        t.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_tracker_on_yuv_equals_tracker_on_to_bgr(ctx, sequence, fmt):
    frames, kps, truth, _ = sequence
    fr = Frames.from_bgr(ctx, frames, fmt)
    a, b = Tracker(ctx), Tracker(ctx)
    try:
        got = a.update(fr, kps)
        _same_ids(got, b.update(fr.to_bgr(ctx), kps))
        seen = lk.stable_ids(got, truth)
        assert all(len(v) == 1 for v in seen.values()), seen
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("gone,same", [((3, 4), True), ((3, 4, 5, 6), False)])
def test_tracker_frames_to_delete(ctx, gone, same):
    frames, kps, truth = lk.synthetic_sequence(dropout=(1, gone))
    want = lk.Tracker(frames_to_delete=2).run([lk.grey(f) for f in frames], kps)
    t = Tracker(ctx, frames_to_delete=2)
    try:
        dev = torch.from_numpy(frames).cuda()
        got = t.update(dev[:5], kps[:5]) + t.update(dev[5:], kps[5:])
        _same_ids(got, want)
        seen = lk.stable_ids(got, truth)
        assert (len(seen[1]) == 1) == same and len(seen[0]) == 1 and len(seen[2]) == 1, seen
    finally:
        t.close()


def test_tracker_frame_without_people_and_state_errors(ctx, sequence):
    frames, kps, truth, _ = sequence
    empty = np.zeros((0, 25, 3), np.float32)
    kps2 = [k if f not in (4, 9) else empty for f, k in enumerate(kps)]
    want = lk.Tracker().run([lk.grey(f) for f in frames.cpu().numpy()], kps2)
    t = Tracker(ctx)
    try:
        t.set_timing(True)
        got = t.update(frames, kps2)
        _same_ids(got, want)
        assert got[4].shape == (0,) and got[9].shape == (0,)
        times = t.read_times()
        print(times)
        lay = api.pyramid_layout(320, 240)
        # two batch buffers at most, the carried frame, the point records
        assert times["batches"] == 1 and times["device_bytes"] >= 11 * lay["frame_bytes"]
        assert times["pyramid_ms"] > 0 and times["lk_ms"] > 0 and times["host_ms"] > 0
        # frames of another size, people of another part count: refused until reset
        small = torch.zeros((1, 120, 160, 3), dtype=torch.uint8, device="cuda")
        with pytest.raises(api.OpkError, match="opk error 3"):
            t.update(small, [empty])
        with pytest.raises(api.OpkError, match="opk error 3"):
            t.update(frames[:1], [np.zeros((1, 18, 3), np.float32)])
        t.reset()
        two = np.ones((2, 18, 3), np.float32)
        two[1, :, :2] = 100
        assert t.update(small, [two])[0].tolist() == [0, 1]
    finally:
        t.close()


# ---- the stage in the pose pipeline -------------------------------------------------------------
SIZE = (640, 360)


@pytest.fixture(scope="module")
def rig(ctx):
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    pose = PoseExtractor(ctx, net)
    pose.set_input((-1, 176))
    people = synth.people(2, 22, 40, 8, min_height=0.6, max_height=0.7)
    field = synth.render_field(people, 22, 40, sigma=1.0, paf_width=1.0)
    overlay = torch.from_numpy(np.stack([field, field])).cuda()   # the same two people in every frame
    pose.set_overlay(overlay)
    x = lk.texture(SIZE[1], SIZE[0], seed=21)
    y = lk.texture(SIZE[1], SIZE[0], seed=22)
    frames_a = torch.from_numpy(np.stack([x, x])).cuda()
    frames_b = torch.from_numpy(np.stack([x, y])).cuda()
    yield ctx, pose, frames_a, frames_b
    pose.close()
    net.close()


def _collected(pose, n=2):
    return [pose.keypoints(f)[0] for f in range(n)]


def test_pipeline_ids_equal_the_tracker_by_hand(rig):
    ctx, pose, frames_a, frames_b = rig
    t, manual = Tracker(ctx), Tracker(ctx)
    try:
        pose.attach(tracker=t)
        pose.submit_frames(frames_a)
        pose.submit_frames(frames_b)
        with pytest.raises(api.OpkError, match="opk error 3"):   # batches in flight
            pose.detach_tracker()
        assert pose.collect() == 2
        kps_a, ids_a = _collected(pose), [pose.person_ids(f) for f in range(2)]
        datum = pose.datum(1)
        assert pose.collect() == 2
        kps_b, ids_b = _collected(pose), [pose.person_ids(f) for f in range(2)]
        assert all(k.shape[0] >= 2 for k in kps_a + kps_b)
        _same_ids(ids_a, manual.update(frames_a, kps_a))
        _same_ids(ids_b, manual.update(frames_b, kps_b))
        # the same frame three times: the people keep their ids
        assert sorted(ids_a[0].tolist()) == list(range(len(ids_a[0])))
        np.testing.assert_array_equal(ids_a[1], ids_a[0])
        np.testing.assert_array_equal(ids_b[0], ids_a[0])
        # datum and the JSON text carry the ids
        assert datum[0][1] == "person_id"
        np.testing.assert_array_equal(datum[0][0], ids_a[1].astype(np.float32))
        text = api.people_json(datum)
        people = json.loads(text)["people"]
        assert [p["person_id"] for p in people] == [[int(i)] for i in ids_a[1]]
        times = pose.read_track_times()
        assert times["batches"] == 2
        # raw frames only while attached
        net_in = torch.zeros((1, 3, 176, 320), device="cuda")
        with pytest.raises(api.OpkError, match="opk error 3"):
            pose.submit(net_in, SIZE)
        assert pose.pending() == 0
        # the synchronous form, as NV12: the ids of the tracker on to_bgr of it
        t.reset()
        manual.reset()
        fr = Frames.from_bgr(ctx, frames_b, "nv12")
        pose.forward_frames(fr)
        _same_ids([pose.person_ids(f) for f in range(2)], manual.update(fr.to_bgr(ctx), _collected(pose)))
    finally:
        if pose.pending() == 0:
            pose.detach_tracker()
        t.close()
        manual.close()
    # no tracker attached: everything as before
    pose.forward_frames(frames_a)
    with pytest.raises(api.OpkError, match="opk error 3"):
        pose.person_ids(0)
    people = json.loads(api.people_json(pose.datum(0)))["people"]
    assert len(people) >= 2 and all(p["person_id"] == [-1] for p in people)
    pose.submit(torch.zeros((1, 3, 176, 320), device="cuda"), SIZE)   # accepted again
    assert pose.collect() == 1
