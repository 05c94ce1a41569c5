"""GPU: NV12 / I420 frames through every frame-taking entry point.

One definition holds everywhere: with YUV frames a function returns, bit for bit, what it returns
on the BGR frames tests/yuv_cases.yuv420_to_bgr (numpy) makes of them.  So every check here runs
the library twice -- on a Frames of the planes and on the numpy-converted BGR tensor -- and
compares all values exactly; the conversion itself is held to numpy over all 2^24 (Y, U, V).
The warp cases read the kernel route they exist for from the launch log before they compare.
"""
import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd import synth
from openpose_amd.api import (CAST_CPU, CAST_CUDA, LAYER_POSE, Frames, Net, PoseExtractor,
                              RenderLayer, launch_log)
from tests import yuv_cases as yc

pytestmark = pytest.mark.gpu

FORMATS = ("nv12", "i420")
# the YUV routes of the frame warp (kernels/yuv.hip) and of the standalone conversion
ROUTES = {"cvmat_to_input_lds<2,a16,yuv>", "cvmat_to_input_lds<2,yuv>",
          "cvmat_to_input_lds<4,a16,yuv>", "cvmat_to_input_lds<4,yuv>", "cvmat_to_input<2,yuv>",
          "cvmat_to_input<4,yuv>", "yuv420_to_bgr<v16>", "yuv420_to_bgr"}


def ran(log, route):
    """tests.kernel_routes.ran for the YUV routes: known, and in the log of this launch."""
    assert route in ROUTES, "unknown route %s" % route
    kernels = [k for _, k in log]
    assert route in kernels, "%s did not run: %s" % (route, kernels)


def _plane(arr, step=None, offset=0, gap=0):
    """arr [n, rows, row bytes] in a device buffer with `step` bytes per row, `gap` bytes between
    frames, starting `offset` bytes into the allocation: a strided view.  Every byte that is not a
    sample holds 0xAA."""
    n, rows, w = arr.shape
    step = step or w
    frame = rows * step + gap
    buf = torch.full((offset + n * frame + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    view = buf[offset:].as_strided((n, rows, w), (frame, step, 1))
    view.copy_(torch.from_numpy(arr))
    assert view.data_ptr() % 16 == offset % 16
    return view


def _frames(fmt, planes, ystep=None, cstep=None, offset=0, gap=0):
    """A Frames of numpy planes (y, u, v) in the layout `fmt`; cstep: the chroma row step."""
    y, u, v = planes
    w = y.shape[2]
    yd = _plane(y, ystep, offset, gap)
    if fmt == "nv12":
        return Frames.nv12(yd, _plane(yc.interleave(u, v), cstep, offset, gap), width=w)
    return Frames.i420(yd, _plane(u, cstep, offset, gap), _plane(v, cstep, offset, 3 * gap), width=w)


def _tight(fmt, planes):
    return _frames(fmt, planes)


def _bgr(planes):
    return torch.from_numpy(yc.yuv420_to_bgr(*planes)).cuda()


# ---- 1. the conversion ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exhaustive():
    planes = yc.exhaustive_planes()
    return planes, _bgr(planes)


@pytest.mark.parametrize("fmt", FORMATS)
def test_conversion_exhaustive(ctx, exhaustive, fmt):
    """Every (Y, U, V) of the 2^24: opk_frames_to_bgr equals numpy."""
    planes, want = exhaustive
    with launch_log() as log:
        got = _tight(fmt, planes).to_bgr(ctx)
    ran(log, "yuv420_to_bgr<v16>")
    ctx.sync()
    assert torch.equal(got, want)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(2, 2), (4, 6), (18, 34)])
def test_conversion_small_shapes(ctx, fmt, h, w):
    """Three frames; row steps that are no multiple of 16, a gap between frames and plane bases
    off 16-byte alignment (the byte route), then 16-byte-friendly ones (the vector route, with a
    2-column tail at 34); the canary bytes of the destination's row padding stay."""
    planes = yc.random_planes(3, h, w, seed=h * w)
    want = yc.yuv420_to_bgr(*planes)
    for aligned in (False, True):
        if aligned:
            ystep = (w + 15) // 16 * 16
            src = _frames(fmt, planes, ystep, ystep if fmt == "nv12" else (w // 2 + 15) // 16 * 16,
                          gap=32)
            dstep = (w * 3 + 15) // 16 * 16 + 16
        else:
            src = _frames(fmt, planes, w + 3, (w if fmt == "nv12" else w // 2) + 5, offset=1, gap=7)
            dstep = w * 3 + 5
        out = torch.full((3, h, dstep), 0x5C, dtype=torch.uint8, device="cuda")
        with launch_log() as log:
            src.to_bgr(ctx, out)
        ran(log, "yuv420_to_bgr<v16>" if aligned else "yuv420_to_bgr")
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:, :, :w * 3].reshape(3, h, w, 3), want)
        assert (got[:, :, w * 3:] == 0x5C).all()


# ---- 2. the frame warp on every route --------------------------------------------------------------
def _size(h, w, scale):
    return int(np.ceil(h * scale)) + 1, int(np.ceil(w * scale)) + 2   # a margin outside the image


def _warp(ctx, frames, n, scale, net_hw, normalize):
    out = torch.full((n, 3) + tuple(net_hw), float("nan"), device="cuda")
    with launch_log() as log:
        ctx.cvmat_to_input(out, frames, scale, normalize)
    assert len(log) == 1
    return out, log


def _check_warp(ctx, fmt, planes, scale, route, **layout):
    n, h, w = planes[0].shape
    net_hw = _size(h, w, scale)
    bgr = _bgr(planes)
    for normalize in (1, 0):
        got, log = _warp(ctx, _frames(fmt, planes, **layout), n, scale, net_hw, normalize)
        ran(log, route)
        want, blog = _warp(ctx, bgr, n, scale, net_hw, normalize)
        assert "yuv" not in blog[0][1]
        ctx.sync()
        assert torch.equal(got, want), (fmt, route, normalize)
    return want


def _steps(fmt, w, aligned):
    """Row steps of the luma and chroma planes: 16-byte friendly, or odd."""
    if aligned:
        return dict(ystep=(w + 15) // 16 * 16,
                    cstep=((w if fmt == "nv12" else w // 2) + 15) // 16 * 16, gap=16)
    return dict(ystep=w + 1, cstep=(w if fmt == "nv12" else w // 2) + 3, offset=1, gap=5)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("aligned", [False, True])
def test_warp_staged_linear(ctx, fmt, aligned):
    """34 x 18 halved: the staged linear routes."""
    planes = yc.random_planes(3, 18, 34, seed=2)
    _check_warp(ctx, fmt, planes, 0.5, "cvmat_to_input_lds<2,a16,yuv>" if aligned
                else "cvmat_to_input_lds<2,yuv>", **_steps(fmt, 34, aligned))


@pytest.mark.parametrize("fmt", FORMATS)
def test_warp_staged_cubic_all_borders(ctx, fmt):
    """6 x 4 enlarged 3 times: the cubic taps leave the image on all four sides, where they must
    contribute BGR 0 -- a border of YUV 0 would be BGR (0, 154, 0) and shows in the green plane."""
    planes = yc.random_planes(2, 4, 6, seed=3)
    _check_warp(ctx, fmt, planes, 3.0, "cvmat_to_input_lds<4,yuv>")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("aligned", [False, True])
def test_warp_staged_cubic_wide(ctx, fmt, aligned):
    """334 x 18 at 1.7 with unaligned steps and bases (byte loads) and at aligned ones (a16: 20
    whole 16-pixel pieces and a 14-pixel tail per row)."""
    planes = yc.random_planes(2, 18, 334, seed=4)
    _check_warp(ctx, fmt, planes, 1.7, "cvmat_to_input_lds<4,a16,yuv>" if aligned
                else "cvmat_to_input_lds<4,yuv>", **_steps(fmt, 334, aligned))


@pytest.mark.parametrize("scale,k", [(0.5, 2), (1.25, 4)])
def test_warp_direct(ctx, scale, k):
    """Frames too wide for the staging gate, 4 rows high: the narrowest even width that takes the
    direct kernel is found from the launch log by bisection (it is the BGR warp's gate), then both
    formats run there and two columns below it (the widest staged frame)."""
    h = 4

    def route(w):
        zeros = (np.zeros((1, h, w), np.uint8), np.zeros((1, h // 2, w // 2), np.uint8),
                 np.zeros((1, h // 2, w // 2), np.uint8))
        _, log = _warp(ctx, _tight("nv12", zeros), 1, scale, _size(h, w, scale), 1)
        return log[0][1]

    lo, hi = 332, 11000 if k == 2 else 5000   # even widths
    assert route(lo).startswith("cvmat_to_input_lds<%d," % k) and route(hi) == "cvmat_to_input<%d,yuv>" % k
    while hi - lo > 2:
        mid = (lo + hi) // 4 * 2
        if route(mid).startswith("cvmat_to_input_lds"):
            lo = mid
        else:
            hi = mid
    for fmt in FORMATS:
        _check_warp(ctx, fmt, yc.random_planes(2, h, hi, seed=hi), scale,
                    "cvmat_to_input<%d,yuv>" % k)
        staged = "cvmat_to_input_lds<%d,%syuv>" % (k, "a16," if lo % 16 == 0 else "")
        _check_warp(ctx, fmt, yc.random_planes(2, h, lo, seed=lo), scale, staged)


def test_bgr_descriptor_with_padded_rows_and_frame_gap(ctx):
    """Frames.bgr of a view with padded rows and frames a gap apart (the descriptor's per-plane
    frame stride) gives what the packed tensor gives, on the BGR route."""
    bgr = np.random.default_rng(9).integers(0, 256, (3, 18, 34, 3), dtype=np.uint8)
    view = _plane(bgr.reshape(3, 18, 34 * 3), step=34 * 3 + 7, offset=1, gap=11)
    net_hw = _size(18, 34, 1.7)
    got, log = _warp(ctx, Frames.bgr(view, width=34), 3, 1.7, net_hw, 1)
    want, wlog = _warp(ctx, torch.from_numpy(bgr).cuda(), 3, 1.7, net_hw, 1)
    assert log[0][1] == wlog[0][1] == "cvmat_to_input_lds<4>"
    ctx.sync()
    assert torch.equal(got, want)


# ---- 3. the pose pipeline ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body_net(ctx):
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=31, out_scale=1.0))
    yield net
    net.close()


def _collected(pose, n):
    return [(pose.num_people(f),) + pose.keypoints(f) for f in range(n)]


@pytest.mark.parametrize("scale_number", [1, 2])
def test_pose_pipeline(ctx, body_net, scale_number):
    """2 frames of 128 x 96 into a 176-high net input (both scales enlarge: cubic): net inputs,
    keypoints and scores from NV12 equal those from the converted BGR frames; one heat element
    and the keypoints drawn on the NV12 frames equal the draw on the BGR frames."""
    planes = yc.random_planes(2, 96, 128, seed=5)
    bgr = _bgr(planes)
    pose = PoseExtractor(ctx, body_net)
    pose.set_input((-1, 176), scale_number=scale_number)
    nv12 = _tight("nv12", planes)
    pose.forward_frames(nv12)
    got_in = [pose.net_input_numpy(i) for i in range(scale_number)]
    got = _collected(pose, 2)
    got_draw = [pose.render_frames(nv12, element=e, cast=CAST_CUDA) for e in (0, 4)]
    pose.forward_frames(bgr)
    want_in = [pose.net_input_numpy(i) for i in range(scale_number)]
    want = _collected(pose, 2)
    want_draw = [pose.render_frames(bgr, element=e, cast=CAST_CUDA) for e in (0, 4)]
    ctx.sync()
    for a, b in zip(got_in, want_in):
        assert a.shape == b.shape and a.shape[2] in (176, 128)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    print("people per frame:", [g[0] for g in got])
    for g, w in zip(got, want):
        assert g[0] == w[0]
        np.testing.assert_array_equal(g[1].view(np.uint32), w[1].view(np.uint32))
        np.testing.assert_array_equal(g[2].view(np.uint32), w[2].view(np.uint32))
    for a, b in zip(got_draw, want_draw):
        assert torch.equal(a, b)
    assert not torch.equal(got_draw[1], bgr)   # the heat element drew something
    pose.close()


# ---- 4. the extractors and the attached whole-body batch --------------------------------------------
@pytest.fixture(scope="module")
def rig(ctx):
    from tests.test_gpu_whole_body import Rig
    r = Rig(ctx)
    yield r
    r.close()


def _wb_planes(seed):
    return yc.random_planes(2, 360, 640, seed=seed)


def test_extractors_on_nv12(ctx, rig):
    """One face and one hand forward on NV12 against BGR, with a frame_of that repeats and
    reorders the source frames: the crops' net inputs and the keypoints are equal."""
    planes = _wb_planes(6)
    nv12, bgr = _tight("nv12", planes), _bgr(planes)
    frame_of = np.array([1, 0, 1], np.int32)
    face_rects = np.array([[100, 60, 120, 120], [300, 150, 90, 90], [-20, 200, 150, 150]], np.float32)
    hand_rects = np.stack([face_rects, face_rects + np.float32([37, -11, 8, 8])], 1)
    for ex, rects in ((rig.face, face_rects), (rig.hand, hand_rects)):
        with launch_log() as log:
            got = ex.forward(nv12, rects, frame_of)
        ran(log, "cvmat_to_input_lds<2,a16,yuv>")
        got_crops = ex.crops()
        want = ex.forward(bgr, rects, frame_of)
        want_crops = ex.crops()
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert len(got_crops) == len(want_crops) >= 3
        for (gm, gx), (wm, wx) in zip(got_crops, want_crops):
            np.testing.assert_array_equal(gm, wm)
            np.testing.assert_array_equal(gx.view(np.uint32), wx.view(np.uint32))
        assert got.any()


def test_whole_body_two_batches_in_flight(ctx, rig):
    """attach(face=, hands=), two batches of different I420 / NV12 frames submitted, then both
    collected: rectangles and keypoints of each equal the BGR run's.  The pipeline must have kept
    its own copy of each descriptor -- the structs the submits passed are gone by then."""
    from tests.test_gpu_whole_body import _same, _stage
    batches = [_wb_planes(7), _wb_planes(8)]
    results = {}
    for kind in ("yuv", "bgr"):
        if kind == "yuv":
            frames = [_tight("i420", batches[0]), _tight("nv12", batches[1])]
        else:
            frames = [_bgr(b) for b in batches]
        for f in frames:
            rig.pose.submit_frames(f)
        out = []
        for _ in frames:
            assert rig.pose.collect() == 2
            out.append(_stage(rig.pose))
        results[kind] = out
    for got, want in zip(results["yuv"], results["bgr"]):
        _same(got, want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g["kp"].view(np.uint32), w["kp"].view(np.uint32))
    faces = sum(int(r["face"].any()) for out in results["yuv"] for r in out)
    assert faces >= 1


# ---- 5. the render ---------------------------------------------------------------------------------
def _pose_layer(n, ow, oh, seed):
    g = np.random.default_rng(seed)
    counts = [2] * n
    kp = np.empty((sum(counts), 25, 3), np.float32)
    kp[..., 0] = g.uniform(0, ow, kp.shape[:2])
    kp[..., 1] = g.uniform(0, oh, kp.shape[:2])
    kp[..., 2] = 1.0
    return RenderLayer(LAYER_POSE, torch.from_numpy(kp).cuda(), counts)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.7])
@pytest.mark.parametrize("h,w", [(18, 34), (96, 128)])
def test_render_frames(ctx, fmt, scale, h, w):
    """render_frames from YUV and from the converted BGR frames: 0 layers and one POSE layer, both
    casts; scale 1 at the same size is the copy route, which becomes a conversion.  Also
    cvmat_to_output, the float image the render starts from."""
    planes = yc.random_planes(2, h, w, seed=h + int(10 * scale))
    src, bgr = _tight(fmt, planes), _bgr(planes)
    out_size = (w, h) if scale == 1.0 else (int(np.ceil(w * scale)), int(np.ceil(h * scale)))
    assert torch.equal(ctx.cvmat_to_output(src, scale, out_size),
                       ctx.cvmat_to_output(bgr, scale, out_size))
    for layers in ([], [_pose_layer(2, out_size[0], out_size[1], seed=w)]):
        for cast in (CAST_CPU, CAST_CUDA):
            got = ctx.render_frames(src, layers, scale, out_size, cast=cast)
            want = ctx.render_frames(bgr, layers, scale, out_size, cast=cast)
            ctx.sync()
            assert got.shape == (2, out_size[1], out_size[0], 3)
            assert torch.equal(got, want), (len(layers), cast)
            if not layers and scale == 1.0:
                assert torch.equal(got, bgr)   # the copy route is the conversion
            if layers:
                assert not torch.equal(got, ctx.render_frames(bgr, [], scale, out_size, cast=cast))
