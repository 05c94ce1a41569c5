"""GPU: opk_undistort_frames (kernels/undistort.hip) bit for bit against the numpy restatement of
the include/opk.h text (tests/undistort_cases.py), both lane mappings (UNDISTORT_VEC), at the sizes
where the vector mapping changes route -- width % 4 != 0, rows that do not take dword stores, more
than one workgroup per frame -- on BGR, NV12 and I420 sources; the argument errors, none of which
launches; and the stage in the pose pipeline (PoseExtractor.set_undistort) against the same
pipeline on frames undistorted by the stand-alone call.  Nothing here reads outside the tree."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd import api, synth
from openpose_amd.api import Frames, Net, PoseExtractor, Tracker, Triangulator
from tests import triangulate_cases as tc
from tests import undistort_cases as uc
from tests.test_gpu_whole_body import SIZE as WB_SIZE
from tests.test_gpu_whole_body import Rig as WholeBodyRig
from tests.test_gpu_whole_body import _frames as _wb_frames

pytestmark = pytest.mark.gpu

# the UNDISTORT_VEC switch: 4 pixels per lane, or one (unset: vec for BGR sources, plain for YUV)
MAPPINGS = {"vec": 1, "plain": 0}
POISON = 0xA5


def cameras(rig, w, h):
    return api.Cameras([K for K, _ in rig], [d for _, d in rig], [(w, h)] * len(rig))


def padded(frames, step, gap_rows=0, seed=9):
    """frames uint8 [n, h, w, 3] on the device as rows of `step` bytes (random padding), the frames
    gap_rows rows apart: (the view [n, h, step], the whole block)."""
    n, h, w, _ = frames.shape
    block = torch.from_numpy(np.random.default_rng(seed).integers(
        0, 256, (n, h + gap_rows, step), dtype=np.uint8)).cuda()
    view = block[:, :h, :]
    view[:, :, :w * 3] = torch.from_numpy(frames.reshape(n, h, w * 3)).cuda()
    return view, block


def run_mappings(ctx, src, cams, n, h, w, dst_step, yuv=False, gap_rows=1):
    """Both mappings into poisoned destinations of dst_step-byte rows: the bytes [n, h, w, 3] (equal
    between the two), with padding and gaps checked untouched and the launches named."""
    outs = []
    for name, switch in MAPPINGS.items():
        block = torch.full((n, h + gap_rows, dst_step), POISON, dtype=torch.uint8, device="cuda")
        dst = Frames.bgr(block[:, :h, :], w)
        with api.dev_switches(UNDISTORT_VEC=switch), api.launch_log() as log:
            ctx.undistort_frames(src, cams, out=dst)
        ctx.sync()
        kernel = "undistort_frames<%s%s>" % (name, ",yuv" if yuv else "")
        assert [k for _, k in log] == [kernel] * cams.views, log
        got = block.cpu().numpy()
        assert (got[:, h:, :] == POISON).all() and (got[:, :h, w * 3:] == POISON).all(), name
        outs.append(got[:, :h, :w * 3].reshape(n, h, w, 3))
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


# ---- the kernel against the restatement ------------------------------------------------------------
@pytest.mark.parametrize("dst_step", [152, 151, 153])
def test_odd_width_padded_rows(ctx, dst_step):
    """50 x 37, V = 2, n = 4; source rows of 157 bytes.  Width % 4 = 2: the last group of every row
    is the tail.  Destination rows of 152 bytes take the dword stores, 151 and 153 the byte route."""
    w, h, n = 50, 37, 4
    rig = uc.rig_two(w, h)
    frames = uc.frames_bgr(11, n, h, w)
    view, _ = padded(frames, 157, gap_rows=2)
    got = run_mappings(ctx, Frames.bgr(view, w), cameras(rig, w, h), n, h, w, dst_step)
    want = uc.undistort(frames, rig)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got, frames)


def test_more_than_one_workgroup(ctx):
    """200 x 120 tight: 6000 groups of 4 pixels per frame (six workgroups of the vec mapping, one
    partly idle), 120 x 1 workgroups of the plain one; destination tight too (600-byte rows)."""
    w, h, n = 200, 120, 4
    rig = uc.rig_two(w, h)
    frames = uc.frames_bgr(12, n, h, w)
    got = run_mappings(ctx, torch.from_numpy(frames).cuda(), cameras(rig, w, h), n, h, w, w * 3,
                       gap_rows=0)
    assert np.array_equal(got, uc.undistort(frames, rig))
    # wider than one workgroup's columns of the plain mapping, width % 4 = 1, one camera for all
    w, h, n = 261, 9, 2
    rig = [(uc.small_k(w, h), uc.D5_BARREL)]
    frames = uc.frames_bgr(13, n, h, w)
    got = run_mappings(ctx, torch.from_numpy(frames).cuda(), cameras(rig, w, h), n, h, w, w * 3 + 1)
    assert np.array_equal(got, uc.undistort(frames, rig))


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_sources(ctx, fmt):
    """52 x 38 with padded luma and chroma rows: bit for bit undistort_frames(to_bgr(frames)), and
    the restatement on those BGR bytes."""
    w, h, n = 52, 38, 4
    rig = uc.rig_two(w, h)
    y, u, v = uc.frames_yuv(14, n, h, w)

    def plane(a, step, seed):
        t = torch.from_numpy(np.random.default_rng(seed).integers(
            0, 256, (n, a.shape[1], step), dtype=np.uint8)).cuda()
        t[:, :, :a.shape[2]] = torch.from_numpy(a).cuda()
        return t

    if fmt == "nv12":
        uv = np.stack([u, v], -1).reshape(n, h // 2, w)
        src = Frames.nv12(plane(y, 61, 1), plane(uv, 59, 2), w)
    else:
        src = Frames.i420(plane(y, 61, 1), plane(u, 31, 2), plane(v, 31, 3), w)
    cams = cameras(rig, w, h)
    bgr = src.to_bgr(ctx)
    got = run_mappings(ctx, src, cams, n, h, w, 160, yuv=True)
    via_bgr = run_mappings(ctx, bgr, cams, n, h, w, 160)
    assert np.array_equal(got, via_bgr)
    assert np.array_equal(got, uc.undistort(bgr.cpu().numpy(), rig))


def test_one_view_identity_and_huge_k3(ctx):
    w, h, n = 50, 37, 3
    frames = uc.frames_bgr(15, n, h, w)
    dev = torch.from_numpy(frames).cuda()
    K = uc.small_k(w, h)
    same = run_mappings(ctx, dev, cameras([(K, np.zeros(4))], w, h), n, h, w, 150, gap_rows=0)
    assert np.array_equal(same, frames)                       # zero distortion: the input bytes
    rig = [(K, uc.D5_K3_HUGE)]
    got = run_mappings(ctx, dev, cameras(rig, w, h), n, h, w, 152)
    assert np.array_equal(got, uc.undistort(frames, rig))
    rig = [(K, uc.D4_PINCUSHION)]
    got = run_mappings(ctx, dev, cameras(rig, w, h), n, h, w, 152)
    assert np.array_equal(got, uc.undistort(frames, rig)) and not got[:, 0, 0].any()
    # views with equal parameters share maps: the reference's rig, camera 0's for every view
    rig = [(K, uc.D8_EXAMPLE)] * 3
    got = run_mappings(ctx, dev, cameras(rig, w, h), n, h, w, 152)
    assert np.array_equal(got, uc.undistort(frames, rig))


def test_shipped_mapping_per_source_format(ctx):
    """With the switch unset: the mapping measured faster for the format."""
    w, h, n = 52, 38, 2
    cams = cameras(uc.rig_two(w, h), w, h)
    bgr = torch.from_numpy(uc.frames_bgr(19, n, h, w)).cuda()
    with api.launch_log() as log:
        ctx.undistort_frames(bgr, cams)
        ctx.undistort_frames(Frames.from_bgr(ctx, bgr, "i420"), cams)
    names = [k for _, k in log if k.startswith("undistort")]
    assert names == ["undistort_frames<vec>"] * 2 + ["undistort_frames<plain,yuv>"] * 2, names


def test_empty_batch_succeeds_without_a_launch(ctx):
    w, h = 50, 37
    cams = cameras(uc.rig_two(w, h), w, h)
    empty = torch.empty((0, h, w, 3), dtype=torch.uint8, device="cuda")
    with api.launch_log() as log:
        out = ctx.undistort_frames(empty, cams)
    assert out.shape == (0, h, w, 3) and log == []


def test_argument_errors_launch_nothing(ctx):
    w, h, n = 50, 37, 4
    rig = uc.rig_two(w, h)
    cams = cameras(rig, w, h)
    src = torch.from_numpy(uc.frames_bgr(16, n, h, w)).cuda()
    dst = torch.full((n, h, w, 3), POISON, dtype=torch.uint8, device="cuda")
    L = ctx.L

    def refused(s, d, c, code=1):
        with api.launch_log() as log:
            rc = L.opk_undistort_frames(ctx.h, ctypes.byref(d) if d is not None else None,
                                        ctypes.byref(s) if s is not None else None,
                                        ctypes.byref(c) if c is not None else None)
        assert rc == code and log == [], (rc, log, L.opk_last_error())

    fs, fd = Frames.bgr(src), Frames.bgr(dst)
    good = lambda: (fs.struct(), fd.struct_out(), cams.struct())
    s, d, c = good()
    assert L.opk_undistort_frames(ctx.h, ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)) == 0
    ctx.sync()
    dst.fill_(POISON)
    refused(None, d, c)
    refused(s, None, c)
    refused(s, d, None)
    # a destination that is not BGR
    yuv = Frames.empty_nv12(n, h + 1, w)
    refused(s, yuv.struct_out(), c)
    # n not a multiple of V; a destination of another count
    s3, d3 = Frames.bgr(src[:3]).struct(), Frames.bgr(dst[:3]).struct_out()
    refused(s3, d3, c)
    refused(s, d3, c)
    # a frame size other than its view's (either view), and a destination of another size
    taller = cameras(rig, w, h + 1)          # (a struct points into its Cameras: keep it alive)
    refused(s, d, taller.struct())
    mixed = api.Cameras([rig[0][0], rig[1][0]], [rig[0][1], rig[1][1]], [(w, h), (w + 2, h)])
    refused(s, d, mixed.struct())
    wider = Frames.bgr(torch.empty((n, h, w + 1, 3), dtype=torch.uint8, device="cuda"))
    refused(s, wider.struct_out(), c)
    # the cameras' own errors
    six = cameras([(rig[0][0], np.zeros(6)), rig[1]], w, h)
    refused(s, d, six.struct())
    tilted = cameras([(rig[0][0], np.zeros(14)), rig[1]], w, h)
    refused(s, d, tilted.struct(), code=4)
    singular = api.Cameras([np.zeros((3, 3))] * 2, [uc.D5_BARREL] * 2, [(w, h)] * 2)
    refused(s, d, singular.struct())
    # descriptor errors of either side: unknown format, negative n, a step shorter than the row, an
    # odd YUV size, a NULL plane
    for side in (0, 1):
        for field, value in (("format", 7), ("n", -1)):
            s, d, c = good()
            setattr((s, d)[side], field, value)
            refused(s, d, c)
        s, d, c = good()
        (s, d)[side].step[0] = w * 3 - 1
        refused(s, d, c)
        s, d, c = good()
        (s, d)[side].plane[0] = None
        refused(s, d, c)
    odd = Frames.empty_nv12(n, h + 1, w).struct()
    odd.height = h
    refused(odd, d, c)
    # overlap: the destination on the source, and destination frames on each other
    s, d, c = good()
    refused(s, Frames.bgr(src).struct_out(), c)
    d.frame_bytes[0] = w * 3 * (h - 1)
    refused(s, d, c)
    ctx.sync()
    assert (dst == POISON).all()


# ---- the stage in the pose pipeline ----------------------------------------------------------------
SIZE = (160, 90)
N, V = 4, 2


class Pipe:
    def __init__(self, ctx):
        self.ctx = ctx
        self.net = Net(ctx, "builtin:BODY_25")
        self.net.set_params(synth.he_weights(body25.layers(), seed=71, out_scale=0.02))
        _, net_sizes = api.scale_and_size(SIZE, (-1, 128))
        W, H = net_sizes[0]
        self.overlay = torch.from_numpy(np.stack(
            [synth.overlay(3, H // 8, W // 8, seed=2600 + k) for k in range(N)])).cuda()
        self.pose = self.extractor()
        self.rig = uc.rig_two(*SIZE)
        self.cams = cameras(self.rig, *SIZE)
        self.frames = torch.from_numpy(uc.frames_bgr(17, N, SIZE[1], SIZE[0])).cuda()
        self.frames2 = torch.from_numpy(uc.frames_bgr(18, N, SIZE[1], SIZE[0])).cuda()

    def extractor(self):
        pose = PoseExtractor(self.ctx, self.net)
        pose.set_input((-1, 128))
        pose.set_overlay(self.overlay)
        return pose

    def close(self):
        self.pose.close()
        self.net.close()


@pytest.fixture(scope="module")
def pipe(ctx):
    p = Pipe(ctx)
    yield p
    p.close()


def results(pose, extra=None, net_input=True):
    """(net_input is the last submit's: left out where a later batch is already in flight)"""
    out = {"net_input": pose.net_input_numpy()} if net_input else {}
    for f in range(N):
        kp, ks = pose.keypoints(f)
        out["kp%d" % f], out["ks%d" % f] = kp, ks
        for p, c in enumerate(pose.candidates(f)):
            out["cand%d_%d" % (f, p)] = c
        if extra:
            for k, v in extra(pose, f).items():
                out["%s%d" % (k, f)] = v
    return out


def same_results(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), k


def staged_and_manual(pipe, frames, extra=None, between=None):
    """(results with the stage on the raw frames, results without it on undistort_frames(frames));
    `between` runs between the two flows (a tracker's reset)."""
    pose, ctx = pipe.pose, pipe.ctx
    pose.set_undistort(pipe.cams)
    try:
        pose.forward_frames(frames)
        staged = results(pose, extra)
        held = pose.undistorted_frames()
        und = held.planes[0].cpu().numpy().reshape(N, SIZE[1], SIZE[0], 3)
    finally:
        pose.set_undistort(None)
    alone = ctx.undistort_frames(frames, pipe.cams)
    assert np.array_equal(und, alone.cpu().numpy())
    if between:
        between()
    pose.forward_frames(alone)
    return staged, results(pose, extra)


def test_pipeline_equals_the_pipeline_on_undistorted_frames(pipe):
    staged, manual = staged_and_manual(pipe, pipe.frames)
    same_results(staged, manual)
    assert sum(staged["kp%d" % f].shape[0] for f in range(N)) >= N   # people in every frame
    # the stage is not a no-op: the raw frames give another net input
    pipe.pose.forward_frames(pipe.frames)
    assert not np.array_equal(pipe.pose.net_input_numpy(), staged["net_input"])
    # the stand-alone call is the restatement
    want = uc.undistort(pipe.frames.cpu().numpy(), pipe.rig)
    assert np.array_equal(pipe.ctx.undistort_frames(pipe.frames, pipe.cams).cpu().numpy(), want)
    # YUV frames in: the stage converts as it reads
    yuv = Frames.from_bgr(pipe.ctx, pipe.frames, "nv12")
    a, b = staged_and_manual(pipe, yuv)
    same_results(a, b)


def test_pipeline_with_views(pipe):
    tri = Triangulator(*tc.plane_rig(V, SIZE), 2)
    pipe.pose.set_views(tri)
    try:
        extra = lambda pose, f: {"xyz": pose.keypoints_3d(f // V)[0]}
        staged, manual = staged_and_manual(pipe, pipe.frames, extra)
        same_results(staged, manual)
        # the rig's checks read the stage's frames: 3 frames are refused by both, before any launch
        pipe.pose.set_undistort(pipe.cams)
        with api.launch_log() as log, pytest.raises(api.OpkError, match="opk error 1"):
            pipe.pose.submit_frames(pipe.frames[:3])
        assert log == [] and pipe.pose.pending() == 0
    finally:
        pipe.pose.set_undistort(None)
        pipe.pose.set_views(None)


def test_pipeline_with_a_tracker(pipe):
    tracker = Tracker(pipe.ctx)
    pipe.pose.attach(tracker=tracker)
    try:
        extra = lambda pose, f: {"ids": pose.person_ids(f)}
        staged, manual = staged_and_manual(pipe, pipe.frames, extra, between=tracker.reset)
        same_results(staged, manual)
        assert sum(staged["ids%d" % f].size for f in range(N)) >= N
    finally:
        pipe.pose.detach_tracker()
        tracker.close()


@pytest.fixture(scope="module")
def whole_body(ctx):
    r = WholeBodyRig(ctx)
    yield r
    r.close()


def test_pipeline_with_face_and_hand_extractors(whole_body):
    """The crops are cut at collect time from what Slot::raw describes.  At 160 x 90 every face
    rectangle is under the reference's 40 px minimum and no crop is ever cut, so this case runs on
    the whole-body tests' rig: two 640 x 360 frames, a 320 x 176 net, two synthetic people per frame
    whose face and hand rectangles are above 44 px.  The keypoints must be non-zero, equal the
    pipeline's on frames undistorted beforehand, and differ from the pipeline's on the raw frames."""
    pose, ctx = whole_body.pose, whole_body.ctx
    w, h = WB_SIZE
    rig = uc.rig_two(w, h)
    cams = cameras(rig, w, h)
    frames = _wb_frames(41)

    def parts():
        out = {}
        for f in range(2):
            out["kp%d" % f] = pose.keypoints(f)[0]
            out["face%d" % f] = pose.face_keypoints(f)
            out["hands%d" % f] = pose.hand_keypoints(f)
            out["face_rects%d" % f] = pose.face_rectangles(f)
        return out

    pose.set_undistort(cams)
    try:
        pose.forward_frames(frames)
        staged = parts()
    finally:
        pose.set_undistort(None)
    pose.forward_frames(ctx.undistort_frames(frames, cams))
    manual = parts()
    pose.forward_frames(frames)
    raw = parts()
    assert staged.keys() == manual.keys()
    for k in staged:
        assert staged[k].shape == manual[k].shape and np.array_equal(staged[k], manual[k]), k
    faces = sum(int(staged["face%d" % f][p].any()) for f in range(2)
                for p in range(staged["face%d" % f].shape[0]))
    hands = sum(int(staged["hands%d" % f][s, p].any()) for f in range(2) for s in range(2)
                for p in range(staged["hands%d" % f].shape[1]))
    print("faces with keypoints %d, hands with keypoints %d" % (faces, hands))
    assert faces >= 1 and hands >= 1
    # on the raw frames the crops are cut from other pixels
    assert any(not np.array_equal(staged["face%d" % f], raw["face%d" % f]) for f in range(2))
    assert any(not np.array_equal(staged["hands%d" % f], raw["hands%d" % f]) for f in range(2))


def test_two_batches_in_flight_use_two_buffers(pipe):
    pose, ctx = pipe.pose, pipe.ctx
    want1 = ctx.undistort_frames(pipe.frames, pipe.cams).cpu().numpy()
    want2 = ctx.undistort_frames(pipe.frames2, pipe.cams).cpu().numpy()
    as_array = lambda fr: fr.planes[0].cpu().numpy().reshape(N, SIZE[1], SIZE[0], 3)
    pose.set_undistort(pipe.cams)
    try:
        pose.forward_frames(pipe.frames)
        solo1 = results(pose, net_input=False)
        pose.forward_frames(pipe.frames2)
        solo2 = results(pose, net_input=False)
        # two in flight: the first batch's results and frames are not touched by the second submit
        pose.submit_frames(pipe.frames)
        pose.submit_frames(pipe.frames2)
        with pytest.raises(api.OpkError, match="opk error 3"):   # attach and clear with batches in flight
            pose.set_undistort(None)
        with pytest.raises(api.OpkError, match="opk error 3"):
            pose.set_undistort(pipe.cams)
        assert pose.collect() == N
        same_results(results(pose, net_input=False), solo1)
        held = pose.undistorted_frames()
        assert np.array_equal(as_array(held), want1)
        assert pose.collect() == N
        same_results(results(pose, net_input=False), solo2)
        assert np.array_equal(as_array(pose.undistorted_frames()), want2)
        # a collected batch's frames survive one further submit
        held2 = pose.undistorted_frames()
        pose.submit_frames(pipe.frames)
        ctx.sync()
        assert np.array_equal(as_array(held2), want2)
        assert pose.collect() == N
        assert np.array_equal(as_array(pose.undistorted_frames()), want1)
        # a batch of another size is refused at submit, before any launch
        with api.launch_log() as log, pytest.raises(api.OpkError, match="opk error 1"):
            pose.submit_frames(torch.zeros((N, SIZE[1] + 2, SIZE[0], 3), dtype=torch.uint8, device="cuda"))
        assert log == [] and pose.pending() == 0
    finally:
        while pose.pending():
            pose.collect()
        pose.set_undistort(None)


def test_cleared_stage_equals_a_fresh_extractor(pipe):
    pose = pipe.pose
    with pytest.raises(api.OpkError, match="opk error 3"):     # no cameras set
        pose.undistorted_frames()
    pose.set_undistort(pipe.cams)
    with pytest.raises(api.OpkError, match="opk error 3"):     # nothing collected with them
        pose.undistorted_frames()
    pose.forward_frames(pipe.frames)
    pose.set_undistort(None)
    with pytest.raises(api.OpkError, match="opk error 3"):
        pose.undistorted_frames()
    pose.forward_frames(pipe.frames)
    used = results(pose)
    fresh = pipe.extractor()
    try:
        fresh.forward_frames(pipe.frames)
        same_results(used, results(fresh))
    finally:
        fresh.close()
