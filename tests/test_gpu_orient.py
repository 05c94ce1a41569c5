"""GPU: opk_orient_frames (kernels/orient.hip) bit for bit against the numpy restatement of the
include/opk.h table (tests/orient_cases.py): all 8 orientations of BGR, NV12 and I420 frames under
both kernel mappings (ORIENT_TILE) and the shipped choice, at sizes of one sample, odd sizes, one
tile and more than one tile on every grid axis, with tight, 4-byte padded and odd row steps, a base
pointer off by one byte and gaps between the frames, the padding and gaps checked untouched; which
kernel a call takes; the conversion property of the text; the errors, none of which launches; and
the stage in the pose pipeline (PoseExtractor.set_orientation) against the same pipeline on frames
oriented by the stand-alone call.  Nothing here reads outside the tree."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd import api, synth
from openpose_amd.api import Frames, Net, PoseExtractor, Tracker, Triangulator
from tests import orient_cases as oc
from tests import triangulate_cases as tc
from tests import undistort_cases as uc

pytestmark = pytest.mark.gpu

# the ORIENT_TILE switch: the dword kernels where the alignment allows them, or the plain one; None:
# unset, the shipped choice
MAPPINGS = (0, 1, None)
POISON = 0xA5
SAMPLE = {"bgr": (3,), "nv12": (1, 2), "i420": (1, 1, 1)}   # sample bytes of each plane's launch


class Block:
    """One plane of n frames on the device: rows of `step` bytes, frames gap_rows rows apart, the
    first byte `offset` bytes into an allocation; filled with `fill` bytes (random if None), then
    with the samples `a` [n, rows, row bytes] if given."""

    def __init__(self, n, rows, row_bytes, step, gap_rows=1, offset=0, fill=None, a=None, seed=1):
        assert step >= row_bytes
        self.n, self.rows, self.row_bytes, self.step, self.offset = n, rows, row_bytes, step, offset
        size = offset + n * (rows + gap_rows) * step
        if fill is None:
            host = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
        else:
            host = np.full(size, fill, np.uint8)
        self.host = host
        if a is not None:
            self.frames(host)[...] = a
        self.flat = torch.from_numpy(host).cuda()
        self.view = self.flat[offset:].view(n, rows + gap_rows, step)[:, :rows, :]
        self.aligned = offset % 4 == 0 and step % 4 == 0 and ((rows + gap_rows) * step) % 4 == 0

    def frames(self, flat):
        """The samples [n, rows, row bytes] inside a host copy of the allocation."""
        return flat[self.offset:].reshape(self.n, -1, self.step)[:, :self.rows, :self.row_bytes]

    def check(self, want):
        """The device bytes: `want` where the samples are, the fill everywhere else."""
        expect = self.host.copy()
        self.frames(expect)[...] = want
        assert np.array_equal(self.flat.cpu().numpy(), expect)


def kernels(fmt, turn, tiled):
    if tiled:
        return ["orient_%s<%d>" % ("turn" if turn else "rows", s) for s in SAMPLE[fmt]]
    return ["orient_plain<%d,%s>" % (s, "turn" if turn else "rows") for s in SAMPLE[fmt]]


def make_frames(fmt, blocks, w):
    views = [b.view for b in blocks]
    return {"bgr": Frames.bgr, "nv12": Frames.nv12, "i420": Frames.i420}[fmt](*views, w)


def plane_shapes(fmt, w, h):
    """(rows, row bytes) of each plane."""
    return {"bgr": [(h, w * 3)], "nv12": [(h, w), (h // 2, w)],
            "i420": [(h, w), (h // 2, w // 2), (h // 2, w // 2)]}[fmt]


def run_mappings(ctx, fmt, planes, w, h, rotate, flip, steps, dst_steps, offset=0, n_gap=1):
    """planes: the source samples per plane [n, rows, row bytes]; steps / dst_steps: a row step per
    plane.  Runs the orientation under every mapping into poisoned destinations and holds samples,
    padding, gaps and the launch log to the restatement."""
    n = planes[0].shape[0]
    src_blocks = [Block(n, a.shape[1], a.shape[2], st, n_gap, offset, a=a, seed=20 + i)
                  for i, (a, st) in enumerate(zip(planes, steps))]
    src = make_frames(fmt, src_blocks, w)
    if fmt == "bgr":
        want = [oc.bgr(planes[0].reshape(n, h, w, 3), rotate, flip)]
        want = [want[0].reshape(n, want[0].shape[1], -1)]
    elif fmt == "nv12":
        want = list(oc.nv12(planes[0], planes[1], rotate, flip))
    else:
        want = list(oc.i420(*planes, rotate, flip))
    ow, oh = oc.size(w, h, rotate)
    turn = oc.normalize(rotate) in (90, 270)
    for switch in MAPPINGS:
        dst_blocks = [Block(n, r, rb, st, n_gap, offset, fill=POISON)
                      for (r, rb), st in zip(plane_shapes(fmt, ow, oh), dst_steps)]
        dst = make_frames(fmt, dst_blocks, ow)
        aligned = all(b.aligned for b in src_blocks + dst_blocks)
        with api.dev_switches(**({} if switch is None else {"ORIENT_TILE": switch})), \
                api.launch_log() as log:
            ctx.orient_frames(src, rotate, flip, out=dst)
        ctx.sync()
        names = [k for _, k in log]
        if switch is None and aligned:   # the shipped choice, per plane (test_which_kernel_runs)
            both = list(zip(kernels(fmt, turn, True), kernels(fmt, turn, False)))
            assert len(names) == len(both) and all(k in pair for k, pair in zip(names, both)), names
        else:
            assert names == kernels(fmt, turn, bool(switch) and aligned), (switch, names)
        for b, wnt in zip(dst_blocks, want):
            b.check(wnt)
    for b in src_blocks:   # the source is only read
        assert np.array_equal(b.flat.cpu().numpy(), b.host)


def pad4(v):
    return (v + 3) // 4 * 4


def odd_step(v):
    """v plus an odd number of bytes, not a multiple of 4."""
    return v + 1 if (v + 1) % 4 else v + 3


# ---- the kernels against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 64), (65, 63), (130, 67)])
def test_bgr(ctx, w, h):
    """n = 3 with a frame gap.  (130, 67): 3 x 2 tiles of the transposing kernel and a partial
    destination dword on every edge; (64, 64): one whole tile; (5, 3), (1, 1): tails only."""
    n = 3
    frames = oc.frames_bgr(100 + w, n, h, w).reshape(n, h, w * 3)
    for rotate, flip in oc.CASES:
        ow, oh = oc.size(w, h, rotate)
        for s, d in ((w * 3, ow * 3), (pad4(w * 3) + 4, pad4(ow * 3)), (odd_step(w * 3), odd_step(ow * 3)),
                     (pad4(w * 3), odd_step(ow * 3))):
            run_mappings(ctx, "bgr", [frames], w, h, rotate, flip, [s], [d])
    # aligned steps, the base pointers one byte off: the byte path
    for rotate, flip in ((90, 0), (180, 0)):
        ow, _ = oc.size(w, h, rotate)
        run_mappings(ctx, "bgr", [frames], w, h, rotate, flip, [pad4(w * 3)], [pad4(ow * 3)], offset=1)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("w,h", [(2, 2), (6, 4), (64, 64), (66, 62), (130, 70)])
def test_yuv(ctx, fmt, w, h):
    n = 2
    y, u, v = oc.yuv_planes(200 + w, n, h, w)
    if fmt == "nv12":
        uv = np.stack([u, v], -1).reshape(n, h // 2, w)
        planes = [y, uv]
    else:
        planes = [y, u, v]
    for rotate, flip in oc.CASES:
        ow, oh = oc.size(w, h, rotate)
        row = lambda ww: [rb for _, rb in plane_shapes(fmt, ww, 2)]
        src_rows, dst_rows = row(w), row(ow)
        # 4-byte padded luma and chroma steps (I420's U and V share theirs)
        run_mappings(ctx, fmt, planes, w, h, rotate, flip, [pad4(r) + 4 for r in src_rows],
                     [pad4(r) + (8 if i else 0) for i, r in enumerate(dst_rows)])
        # chroma steps padded by an odd amount
        run_mappings(ctx, fmt, planes, w, h, rotate, flip,
                     [pad4(r) if i == 0 else odd_step(r) for i, r in enumerate(src_rows)],
                     [pad4(r) if i == 0 else odd_step(r) for i, r in enumerate(dst_rows)])
        # tight
        run_mappings(ctx, fmt, planes, w, h, rotate, flip, src_rows, dst_rows)


SHIPPED_TURN_BGR = "orient_turn<3>"


def test_which_kernel_runs(ctx):
    """An aligned transposing case takes the tile kernel, the same frames from a base one byte off
    the plain one; with the switch unset each family takes what DESIGN.md 4.19 ships."""
    n, w, h = 2, 64, 32
    frames = oc.frames_bgr(7, n, h, w)
    src = Block(n, h, w * 3, w * 3, 0, 0, a=frames.reshape(n, h, w * 3))
    off = Block(n, h, w * 3, w * 3, 0, 1, a=frames.reshape(n, h, w * 3))
    want = oc.bgr(frames, 90, 0)
    with api.dev_switches(ORIENT_TILE=1), api.launch_log() as log:
        a = ctx.orient_frames(Frames.bgr(src.view, w), 90, 0)
        b = ctx.orient_frames(Frames.bgr(off.view, w), 90, 0)
        c = ctx.orient_frames(Frames.bgr(src.view, w), 0, 1)
    assert [k for _, k in log] == ["orient_turn<3>", "orient_plain<3,turn>", "orient_rows<3>"]
    assert isinstance(a, Frames) and a.width == h and a.height == w
    for got in (a, b):
        assert np.array_equal(got.planes[0].cpu().numpy().reshape(n, w, h, 3), want)
    assert np.array_equal(c.planes[0].cpu().numpy().reshape(n, h, w, 3), oc.bgr(frames, 0, 1))
    with api.launch_log() as log:
        t = ctx.orient_frames(torch.from_numpy(frames).cuda(), -270, False)
        ctx.orient_frames(Frames.bgr(off.view, w), 270, 1)
    assert [k for _, k in log] == [SHIPPED_TURN_BGR, "orient_plain<3,turn>"]
    assert isinstance(t, torch.Tensor) and np.array_equal(t.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_conversion_commutes(ctx, fmt):
    """Frames.to_bgr(orient(yuv)) == orient(Frames.to_bgr(yuv)), bit for bit."""
    n, w, h = 2, 66, 38
    bgr = torch.from_numpy(oc.frames_bgr(31, n, h, w)).cuda()
    yuv = Frames.from_bgr(ctx, bgr, fmt)
    as_bgr = yuv.to_bgr(ctx)
    for rotate, flip in oc.CASES:
        a = ctx.orient_frames(yuv, rotate, flip).to_bgr(ctx)
        b = ctx.orient_frames(as_bgr, rotate, flip)
        assert torch.equal(a, b), (rotate, flip)
        assert np.array_equal(b.cpu().numpy(), oc.bgr(as_bgr.cpu().numpy(), rotate, flip))


def test_empty_batch_succeeds_without_a_launch(ctx):
    w, h = 50, 37
    empty = torch.empty((0, h, w, 3), dtype=torch.uint8, device="cuda")
    with api.launch_log() as log:
        out = ctx.orient_frames(empty, 90, True)
    assert out.shape == (0, w, h, 3) and log == []


def test_argument_errors_launch_nothing(ctx):
    w, h, n = 50, 38, 3
    src = torch.from_numpy(oc.frames_bgr(16, n, h, w)).cuda()
    dst = torch.full((n, w, h, 3), POISON, dtype=torch.uint8, device="cuda")
    L = ctx.L

    def refused(s, d, rotate=90, flip=0, code=1):
        with api.launch_log() as log:
            rc = L.opk_orient_frames(ctx.h, ctypes.byref(d) if d is not None else None,
                                     ctypes.byref(s) if s is not None else None, rotate, flip)
        assert rc == code and log == [], (rc, log, L.opk_last_error())

    fs, fd = Frames.bgr(src), Frames.bgr(dst)
    good = lambda: (fs.struct(), fd.struct_out())
    s, d = good()
    assert L.opk_orient_frames(ctx.h, ctypes.byref(d), ctypes.byref(s), 90, 0) == 0
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), oc.bgr(src.cpu().numpy(), 90, 0))
    dst.fill_(POISON)
    refused(None, d)
    refused(s, None)
    # angles and flips
    for rotate in (45, 91, -1):
        refused(s, d, rotate)
        assert ("Rotation angle = %d != {0, 90, 180, 270} degrees." % rotate).encode() in L.opk_last_error()
    refused(s, d, 90, 2)
    refused(s, d, 90, -1)
    # a size other than opk_orient_size's: the source's own at 90, the turned one at 180
    refused(s, Frames.bgr(torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")).struct_out())
    refused(s, d, 180, 0)
    # another format; another n
    yuv = Frames.empty_nv12(n, w, h)
    refused(s, yuv.struct_out())
    refused(yuv.struct(), d)
    refused(s, Frames.bgr(dst[:2]).struct_out())
    refused(Frames.bgr(src[:2]).struct(), d)
    # descriptor errors of either side
    for side in (0, 1):
        for field, value in (("format", 7), ("n", -1)):
            s, d = good()
            setattr((s, d)[side], field, value)
            refused(s, d)
        s, d = good()
        (s, d)[side].step[0] = (w, h)[side] * 3 - 1
        refused(s, d)
        s, d = good()
        (s, d)[side].plane[0] = None
        refused(s, d)
    odd = Frames.empty_nv12(n, h, w).struct()
    odd.width = w - 1
    refused(odd, Frames.empty_nv12(n, w, h).struct_out())
    # a source without area
    s, d = good()
    s.width = 0
    refused(s, d)
    # overlap: in place (a square frame, so the sizes agree), and destination frames on each other
    sq = torch.zeros((n, 8, 8, 3), dtype=torch.uint8, device="cuda")
    refused(Frames.bgr(sq).struct(), Frames.bgr(sq).struct_out())
    refused(Frames.bgr(sq).struct(), Frames.bgr(sq).struct_out(), 180, 1)
    s, d = good()
    d.frame_bytes[0] = h * 3 * (w - 1)
    refused(s, d)
    ctx.sync()
    assert (dst == POISON).all() and not sq.any()


# ---- the stage in the pose pipeline ----------------------------------------------------------------
SIZE = (160, 90)
N, V = 4, 2


def overlay_for(size):
    _, net_sizes = api.scale_and_size(size, (-1, 128))
    W, H = net_sizes[0]
    return torch.from_numpy(np.stack(
        [synth.overlay(3, H // 8, W // 8, seed=2700 + k) for k in range(N)])).cuda()


class Pipe:
    """The synthetic net with people overlaid on its output.  The overlay has the net output's
    shape, which follows the oriented frame size: use(rotate) picks the one that fits."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.net = Net(ctx, "builtin:BODY_25")
        self.net.set_params(synth.he_weights(body25.layers(), seed=71, out_scale=0.02))
        self.overlays = {SIZE: overlay_for(SIZE), SIZE[::-1]: overlay_for(SIZE[::-1])}
        self.pose = self.extractor()
        self.frames = torch.from_numpy(uc.frames_bgr(17, N, SIZE[1], SIZE[0])).cuda()
        self.frames2 = torch.from_numpy(uc.frames_bgr(18, N, SIZE[1], SIZE[0])).cuda()

    def extractor(self, rotate=0):
        pose = PoseExtractor(self.ctx, self.net)
        pose.set_input((-1, 128))
        pose.set_overlay(self.overlays[api.orient_size(SIZE, rotate)])
        return pose

    def use(self, rotate):
        self.pose.set_overlay(self.overlays[api.orient_size(SIZE, rotate)])

    def close(self):
        self.pose.close()
        self.net.close()


@pytest.fixture(scope="module")
def pipe(ctx):
    p = Pipe(ctx)
    yield p
    p.pose.set_orientation(0, False)
    p.close()


def results(pose, extra=None, net_input=True):
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


def planes_numpy(frames):
    return [p.cpu().numpy()[:, :, :rb] for p, (_, rb) in zip(
        frames.planes, plane_shapes({0: "bgr", 1: "nv12", 2: "i420"}[frames.format],
                                    frames.width, frames.height))]


def same_frames(a, b):
    a = a if isinstance(a, Frames) else Frames.bgr(a)
    b = b if isinstance(b, Frames) else Frames.bgr(b)
    assert (a.format, a.n, a.width, a.height) == (b.format, b.n, b.width, b.height)
    for p, q in zip(planes_numpy(a), planes_numpy(b)):
        assert np.array_equal(p, q)


def staged_and_manual(pipe, frames, rotate, flip, extra=None, between=None):
    """(results with the stage on the frames, results without it on orient_frames(frames)); the
    stage's buffer must be the stand-alone call's output."""
    pose, ctx = pipe.pose, pipe.ctx
    pipe.use(rotate)
    pose.set_orientation(rotate, flip)
    try:
        pose.forward_frames(frames)
        staged = results(pose, extra)
        alone = ctx.orient_frames(frames, rotate, flip)
        same_frames(pose.oriented_frames(), alone)
    finally:
        pose.set_orientation(0, False)
    if between:
        between()
    pose.forward_frames(alone)
    return staged, results(pose, extra)


@pytest.mark.parametrize("rotate,flip,fmt", [(90, 0, None), (180, 1, None), (270, 0, "nv12")])
def test_pipeline_equals_the_pipeline_on_oriented_frames(pipe, rotate, flip, fmt):
    frames = pipe.frames if fmt is None else Frames.from_bgr(pipe.ctx, pipe.frames, fmt)
    staged, manual = staged_and_manual(pipe, frames, rotate, flip)
    same_results(staged, manual)
    assert sum(staged["kp%d" % f].shape[0] for f in range(N)) >= N   # people in every frame
    # the stage is not a no-op: the frames as they are give another net input
    pipe.pose.forward_frames(frames)
    other = pipe.pose.net_input_numpy()
    assert other.shape != staged["net_input"].shape or not np.array_equal(other, staged["net_input"])
    # and the stand-alone call is the restatement
    if fmt is None:
        want = oc.bgr(pipe.frames.cpu().numpy(), rotate, flip)
        assert np.array_equal(pipe.ctx.orient_frames(pipe.frames, rotate, flip).cpu().numpy(), want)


def test_pipeline_after_the_undistortion(pipe):
    """Both stages: the oriented buffer is orient(undistort(frames)), the undistorted buffer stays
    unrotated, and the results are those of the pipeline on frames prepared by the two calls."""
    pose, ctx = pipe.pose, pipe.ctx
    rig = uc.rig_two(*SIZE)
    cams = api.Cameras([K for K, _ in rig], [d for _, d in rig], [SIZE] * len(rig))
    und = ctx.undistort_frames(pipe.frames, cams)
    both = ctx.orient_frames(und, 90, 0)
    pipe.use(90)
    pose.set_undistort(cams)
    pose.set_orientation(90, 0)
    try:
        pose.forward_frames(pipe.frames)
        staged = results(pose)
        same_frames(pose.oriented_frames(), both)
        same_frames(pose.undistorted_frames(), und)
        # cameras of the oriented size are refused: they are checked against the source size
        turned = api.Cameras([K for K, _ in rig], [d for _, d in rig], [SIZE[::-1]] * len(rig))
        pose.set_undistort(turned)
        with api.launch_log() as log, pytest.raises(api.OpkError, match="opk error 1"):
            pose.submit_frames(pipe.frames)
        assert log == [] and pose.pending() == 0
    finally:
        pose.set_undistort(None)
        pose.set_orientation(0, False)
    pose.forward_frames(both)
    same_results(staged, results(pose))


def test_pipeline_with_a_tracker(pipe):
    tracker = Tracker(pipe.ctx)
    pipe.pose.attach(tracker=tracker)
    try:
        extra = lambda pose, f: {"ids": pose.person_ids(f)}
        staged, manual = staged_and_manual(pipe, pipe.frames, 90, 0, extra, between=tracker.reset)
        same_results(staged, manual)
        assert sum(staged["ids%d" % f].size for f in range(N)) >= N
    finally:
        pipe.pose.detach_tracker()
        tracker.close()


def test_pipeline_with_views(pipe):
    """A rig of the oriented image sizes; one of the source size at 90 degrees is refused at submit."""
    turned = SIZE[::-1]
    pipe.pose.set_views(Triangulator(*tc.plane_rig(V, turned), 2))
    try:
        extra = lambda pose, f: {"xyz": pose.keypoints_3d(f // V)[0]}
        staged, manual = staged_and_manual(pipe, pipe.frames, 90, 0, extra)
        same_results(staged, manual)
        pipe.pose.set_views(Triangulator(*tc.plane_rig(V, SIZE), 2))
        pipe.pose.set_orientation(90, 0)
        with api.launch_log() as log, pytest.raises(api.OpkError, match="opk error 1"):
            pipe.pose.submit_frames(pipe.frames)
        assert log == [] and pipe.pose.pending() == 0
        # at 180 degrees the source's rig is the oriented one
        pipe.pose.set_orientation(180, 0)
        pipe.use(180)
        pipe.pose.forward_frames(pipe.frames)
    finally:
        pipe.pose.set_orientation(0, False)
        pipe.pose.set_views(None)


def test_two_batches_in_flight_use_two_buffers(pipe):
    pose, ctx = pipe.pose, pipe.ctx
    want1 = ctx.orient_frames(pipe.frames, 90, 0)
    want2 = ctx.orient_frames(pipe.frames2, 90, 0)
    pipe.use(90)
    pose.set_orientation(90, 0)
    try:
        pose.forward_frames(pipe.frames)
        solo1 = results(pose, net_input=False)
        pose.forward_frames(pipe.frames2)
        solo2 = results(pose, net_input=False)
        pose.submit_frames(pipe.frames)
        pose.submit_frames(pipe.frames2)
        with pytest.raises(api.OpkError, match="opk error 3"):   # set and clear with batches in flight
            pose.set_orientation(0, False)
        with pytest.raises(api.OpkError, match="opk error 3"):
            pose.set_orientation(180, True)
        assert pose.collect() == N
        same_results(results(pose, net_input=False), solo1)
        same_frames(pose.oriented_frames(), want1)
        assert pose.collect() == N
        same_results(results(pose, net_input=False), solo2)
        same_frames(pose.oriented_frames(), want2)
        # a collected batch's frames survive one further submit
        held = pose.oriented_frames()
        pose.submit_frames(pipe.frames)
        ctx.sync()
        same_frames(held, want2)
        assert pose.collect() == N
        same_frames(pose.oriented_frames(), want1)
    finally:
        while pose.pending():
            pose.collect()
        pose.set_orientation(0, False)


def test_cleared_stage_equals_a_fresh_extractor(pipe):
    pose = pipe.pose
    pipe.use(0)
    with pytest.raises(api.OpkError, match="opk error 3"):     # no orientation set
        pose.oriented_frames()
    pose.set_orientation(0, True)
    with pytest.raises(api.OpkError, match="opk error 3"):     # nothing collected with it
        pose.oriented_frames()
    pose.forward_frames(pipe.frames)
    pose.oriented_frames()
    pose.set_orientation(360, False)                           # (0, 0): cleared
    with pytest.raises(api.OpkError, match="opk error 3"):
        pose.oriented_frames()
    with api.launch_log() as log:
        pose.forward_frames(pipe.frames)
    assert log and not [k for _, k in log if k.startswith("orient")]
    used = results(pose)
    fresh = pipe.extractor()
    try:
        fresh.forward_frames(pipe.frames)
        same_results(used, results(fresh))
    finally:
        fresh.close()
    with pytest.raises(api.OpkError, match="opk error 1"):
        pose.set_orientation(45, False)
