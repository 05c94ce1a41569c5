"""GPU: drawn frames out as NV12 / I420 -- opk_bgr_to_frames, opk_render_frames_to and
opk_pose_render_frames_to.

One definition holds everywhere: with an NV12 / I420 destination a call writes, bit for bit,
tests/yuv_out_cases.bgr_to_yuv420 (numpy) of the bytes the existing BGR call returns for the same
arguments.  So every render check here runs the library twice -- into a tensor and into a Frames --
and compares all samples exactly; the conversion itself is held to numpy over all 2^24 (B, G, R).
Every destination is a view into a buffer of 0x5C bytes: row padding, the gaps between frames and
the bytes around the planes must keep them.  The store route is read from the launch log.
"""
import numpy as np
import pytest
import torch

from openpose_amd.api import (CAST_CPU, CAST_CUDA, FRAMES_I420, FRAMES_NV12, HEAT_PAFS, HEAT_PART,
                              LAYER_FACE, LAYER_HAND, LAYER_POSE, Frames, RenderHeat, RenderLayer,
                              launch_log)
from tests import yuv_cases as yc
from tests import yuv_out_cases as oc
from tests.test_gpu_output_frames import _dev_layers, _layer_np

pytestmark = pytest.mark.gpu

FORMATS = ("nv12", "i420")
CANARY = 0x5C
# the routes of the standalone conversion (kernels/yuv.hip) and the store routes of the batch
# render (kernels/render.hip): a4 = 4-byte stores from the LDS stage, else byte stores
ROUTES = {"bgr_to_yuv420<v16>", "bgr_to_yuv420", "render_frames<a4>", "render_frames",
          "render_frames<a4,nv12>", "render_frames<nv12>", "render_frames<a4,i420>",
          "render_frames<i420>"}


def ran(log, route):
    """tests.kernel_routes.ran for the routes above: known, and in the log of this launch."""
    assert route in ROUTES, "unknown route %s" % route
    kernels = [k for _, k in log]
    assert route in kernels, "%s did not run: %s" % (route, kernels)


def _ceil16(v):
    return (v + 15) // 16 * 16


class Dest:
    """n frames of w x h to write into, every plane a strided view into its own buffer of canary
    bytes.  aligned: bases, steps and frame strides on 16-byte boundaries (padded all the same);
    else odd steps, bases one byte off and a gap of 7 bytes between frames."""

    def __init__(self, fmt, n, h, w, aligned):
        self.fmt, self.n, self.h, self.w = fmt, n, h, w
        self.bufs, views = [], []
        crow = w if fmt == "nv12" else w // 2
        rows = [(h, w * 3)] if fmt == "bgr" else [(h, w), (h // 2, crow)] + [(h // 2, crow)] * (fmt == "i420")
        for i, (r, row) in enumerate(rows):
            step = _ceil16(row) + 16 if aligned else row + (3 if i == 0 else 5)
            gap, offset = (32, 0) if aligned else (7, 1)
            frame = r * step + gap
            buf = torch.full((offset + n * frame + 16,), CANARY, dtype=torch.uint8, device="cuda")
            views.append(buf[offset:].as_strided((n, r, row), (frame, step, 1)))
            assert views[-1].data_ptr() % 16 == offset
            self.bufs.append(buf)
        if fmt == "bgr":
            self.frames = Frames.bgr(views[0], width=w)
        elif fmt == "nv12":
            self.frames = Frames.nv12(*views, width=w)
        else:
            self.frames = Frames.i420(*views, width=w)

    def check(self, bgr):
        """The samples equal the conversion of `bgr` (uint8 numpy [n, h, w, 3]; BGR: its bytes) and
        every other byte of the buffers is still the canary."""
        if self.fmt == "bgr":
            want = [bgr.reshape(self.n, self.h, self.w * 3)]
        elif self.fmt == "nv12":
            want = list(oc.to_nv12(*oc.bgr_to_yuv420(bgr)))
        else:
            want = list(oc.bgr_to_yuv420(bgr))
        for name, view, w in zip("yuv", self.frames.planes, want):
            np.testing.assert_array_equal(view.cpu().numpy(), w, err_msg="plane " + name)
        for view, buf in zip(self.frames.planes, self.bufs):
            samples = view.clone()
            view.fill_(CANARY)
            assert bool((buf == CANARY).all()), "a byte outside the samples was written"
            view.copy_(samples)


def _source(bgr, aligned):
    """BGR frames as a Frames with padded rows: 16-byte friendly, or odd and one byte off."""
    n, h, w, _ = bgr.shape
    row = w * 3
    step, gap, offset = (_ceil16(row), 32, 0) if aligned else (row + 7, 5, 1)
    frame = h * step + gap
    buf = torch.full((offset + n * frame + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    view = buf[offset:].as_strided((n, h, row), (frame, step, 1))
    view.copy_(torch.from_numpy(bgr.reshape(n, h, row)))
    return Frames.bgr(view, width=w)


# ---- 1. the conversion, exhaustive -----------------------------------------------------------------
@pytest.fixture(scope="module")
def exhaustive():
    """Every (B, G, R) as a block's top-left pixel, on the device, and numpy's planes of it."""
    bgr = oc.exhaustive_bgr()
    parts = [oc.bgr_to_yuv420(bgr[f:f + 8]) for f in range(0, 64, 8)]   # in pieces: less memory
    want = [np.concatenate([p[i] for p in parts]) for i in range(3)]
    return torch.from_numpy(bgr).cuda(), [torch.from_numpy(w).cuda() for w in want]


@pytest.mark.parametrize("fmt", FORMATS)
def test_conversion_exhaustive(ctx, exhaustive, fmt):
    bgr, (y, u, v) = exhaustive
    with launch_log() as log:
        got = Frames.from_bgr(ctx, bgr, fmt)
    ran(log, "bgr_to_yuv420<v16>")
    ctx.sync()
    assert got.format == (FRAMES_NV12 if fmt == "nv12" else FRAMES_I420)
    assert torch.equal(got.planes[0], y)
    if fmt == "nv12":
        assert torch.equal(got.planes[1][:, :, 0::2], u) and torch.equal(got.planes[1][:, :, 1::2], v)
    else:
        assert torch.equal(got.planes[1], u) and torch.equal(got.planes[2], v)


# ---- 2. the conversion, small shapes ----------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h,w", [(2, 2), (4, 6), (8, 32), (18, 34)])
def test_conversion_small_shapes(ctx, fmt, h, w):
    """Three frames; odd steps, bases one byte off and a gap between frames (the byte route), then
    16-byte-friendly ones (the vector route: 32 is two whole pieces, 34 leaves a 2-column tail,
    2 and 6 are all tail); the canaries around the samples stay."""
    bgr = oc.random_bgr(3, h, w, seed=h * w)
    for aligned in (False, True):
        dst = Dest(fmt, 3, h, w, aligned)
        with launch_log() as log:
            out = Frames.from_bgr(ctx, _source(bgr, aligned), None, out=dst.frames)
        assert out is dst.frames
        ran(log, "bgr_to_yuv420<v16>" if aligned else "bgr_to_yuv420")
        ctx.sync()
        dst.check(bgr)
    # a tensor source and fresh frames: the packed layouts
    got = Frames.from_bgr(ctx, torch.from_numpy(bgr).cuda(), fmt)
    y, u, v = oc.bgr_to_yuv420(bgr)
    np.testing.assert_array_equal(got.planes[0].cpu().numpy(), y)
    if fmt == "nv12":
        np.testing.assert_array_equal(got.planes[1].cpu().numpy(), oc.to_nv12(y, u, v)[1])
    else:
        np.testing.assert_array_equal(got.planes[1].cpu().numpy(), u)
        np.testing.assert_array_equal(got.planes[2].cpu().numpy(), v)


# ---- 3. the render ----------------------------------------------------------------------------------
# name -> (source h, w; scale; out w, h): the copy at 2 x 2, at one whole tile, with edge tiles both
# ways (34 = a tile and 2 columns, 10 = a tile and 2 rows; 66 x 18: 3 x 3 tiles, the last 2 wide and
# 2 high), then the linear and the cubic warp to 66 x 18 (the cubic one reaches past the image)
SETUPS = {"2x2": ((2, 2), 1.0, (2, 2)), "8x32": ((8, 32), 1.0, (32, 8)),
          "10x34": ((10, 34), 1.0, (34, 10)), "18x66": ((18, 66), 1.0, (66, 18)),
          "linear": ((36, 132), 0.5, (66, 18)), "cubic": ((10, 34), 1.7, (66, 18))}
BODY_25, CAR_12 = 0, 8


def _crossing_pose(n, ow, oh, seed):
    """Two people per frame with parts all over the frame: their limbs cross every tile border."""
    g = np.random.default_rng(seed)
    kp = np.empty((2 * n, 25, 3), np.float32)
    kp[..., 0] = g.uniform(0, ow, kp.shape[:2])
    kp[..., 1] = g.uniform(0, oh, kp.shape[:2])
    kp[..., 2] = 1.0
    return RenderLayer(LAYER_POSE, torch.from_numpy(kp).cuda(), [2] * n)


@pytest.fixture(scope="module")
def heat_stacks():
    """Heat stacks of 35 channels for 2 frames, made once: 40 x 25 (its window is staged in LDS at
    2.3) and 200 x 130 (at 0.2 no window fits: per-pixel samples)."""
    g = np.random.default_rng(41)
    return {size: torch.from_numpy(g.uniform(-1.2, 1.3, (2, 35, size[1], size[0])).astype(np.float32)).cuda()
            for size in ((40, 25), (200, 130))}


def _cases(n, ow, oh, stacks):
    """(name, layers, keyword arguments) of every render case."""
    three = _dev_layers([_layer_np(LAYER_POSE, (2, 1), ow, oh, 51, googly=True),
                         _layer_np(LAYER_FACE, (1, 2), ow, oh, 52),
                         _layer_np(LAYER_HAND, (2, 2), ow, oh, 53)])
    pose = _crossing_pose(n, ow, oh, seed=ow + oh)
    return [
        ("none", [], dict(cast=CAST_CPU)),
        ("pose", [pose], dict(cast=CAST_CUDA)),
        ("pose+face+hand", three, dict(cast=CAST_CPU)),
        ("heat part", [], dict(cast=CAST_CUDA, heat=RenderHeat(HEAT_PART, stacks[(40, 25)], 2.3, 34))),
        ("heat pafs staged", [pose], dict(cast=CAST_CPU, heat=RenderHeat(
            HEAT_PAFS, stacks[(40, 25)], 2.3, pose_model=CAR_12))),
        ("heat pafs per pixel", [], dict(cast=CAST_CPU, heat=RenderHeat(
            HEAT_PAFS, stacks[(200, 130)], 0.2, pose_model=CAR_12))),
        ("no blend", [pose], dict(cast=CAST_CPU, blend_original=False)),
    ]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("source", ["bgr", "nv12"])
@pytest.mark.parametrize("setup", list(SETUPS))
def test_render_frames_to(ctx, heat_stacks, setup, source, fmt):
    (sh, sw), scale, (ow, oh) = SETUPS[setup]
    n = 2
    if source == "bgr":
        src = torch.from_numpy(oc.random_bgr(n, sh, sw, seed=sh + sw)).cuda()
    else:
        y, u, v = yc.random_planes(n, sh, sw, seed=sh + sw)
        src = Frames.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(yc.interleave(u, v)).cuda())
    drawn = set()
    for name, layers, kw in _cases(n, ow, oh, heat_stacks):
        with launch_log() as log:
            want = ctx.render_frames(src, layers, scale, (ow, oh), **kw)
        ran(log, "render_frames<a4>" if (ow * 3) % 4 == 0 else "render_frames")
        want = want.cpu().numpy()
        drawn.add(want.tobytes())
        for aligned in (False, True):
            dst = Dest(fmt, n, oh, ow, aligned)
            with launch_log() as log:
                out = ctx.render_frames(src, layers, scale, (ow, oh), out=dst.frames, **kw)
            assert out is dst.frames
            ran(log, "render_frames<%s%s>" % ("a4," if aligned else "", fmt))
            ctx.sync()
            dst.check(want)
    # the cases draw different images (at 2 x 2 a layer covers the whole frame: fewer differ)
    assert len(drawn) >= (5 if ow > 2 else 3)
    # out_format allocates packed frames: the same samples
    got = ctx.render_frames(src, [], scale, (ow, oh), out_format=fmt)
    want = ctx.render_frames(src, [], scale, (ow, oh)).cpu().numpy()
    np.testing.assert_array_equal(got.planes[0].cpu().numpy(), oc.bgr_to_yuv420(want)[0])


# ---- 4. the pipeline ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig(ctx):
    from tests.test_gpu_whole_body import Rig
    r = Rig(ctx)
    yield r
    r.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_pose_render_frames_to(ctx, rig, fmt):
    """2 frames of 640 x 360 through the 176-high net with face and hand extractors attached, then
    the collected batch drawn: the keypoints, one heat element, every attached layer (the parts
    call) and a subset of them (put together in Python), at the frames' size and halved."""
    from tests.test_gpu_whole_body import SEED, _frames
    frames = _frames(SEED)
    rig.pose.forward_frames(frames)
    assert sum(rig.pose.num_people(f) for f in range(2)) >= 2
    # the seeded nets' maxima are far below the renderers' default thresholds: draw every keypoint
    # above half the median positive score, so that the face and hand layers put pixels down
    th = {}
    for key, a in (("face_threshold", np.concatenate([rig.pose.face_keypoints(f) for f in range(2)])),
                   ("hand_threshold", np.concatenate([rig.pose.hand_keypoints(f).reshape(-1, 21, 3)
                                                      for f in range(2)]))):
        pos = a[..., 2][a[..., 2] > 0]
        assert pos.size > 0
        th[key] = float(np.median(pos)) / 2
    images = []
    for kw in (dict(), dict(element=4), dict(face=True, hands=True, **th), dict(face=True, **th),
               dict(scale=0.5, out_size=(320, 180), face=True, hands=True, cast=CAST_CUDA, **th)):
        want = rig.pose.render_frames(frames, **kw).cpu().numpy()
        got = rig.pose.render_frames(frames, out_format=fmt, **kw)
        ctx.sync()
        assert (got.n, got.height, got.width) == want.shape[:3]
        y, u, v = oc.bgr_to_yuv420(want)
        np.testing.assert_array_equal(got.planes[0].cpu().numpy(), y, err_msg=str(kw))
        if fmt == "nv12":
            np.testing.assert_array_equal(got.planes[1].cpu().numpy(), oc.to_nv12(y, u, v)[1])
        else:
            np.testing.assert_array_equal(got.planes[1].cpu().numpy(), u)
            np.testing.assert_array_equal(got.planes[2].cpu().numpy(), v)
        images.append(want.tobytes())
    assert len(set(images)) == 5   # each draws something of its own
    # an NV12 source and an NV12 destination: the video loop, no BGR image anywhere
    y, u, v = oc.bgr_to_yuv420(frames.cpu().numpy())
    nv12 = Frames.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(oc.to_nv12(y, u, v)[1]).cuda())
    rig.pose.forward_frames(nv12)
    want = rig.pose.render_frames(nv12).cpu().numpy()
    dst = Dest(fmt, 2, 360, 640, True)
    rig.pose.render_frames(nv12, out=dst.frames)
    ctx.sync()
    dst.check(want)


# ---- 5. no frames, and a BGR destination ---------------------------------------------------------------
def test_no_frames(ctx):
    empty = torch.empty((0, 18, 34, 3), dtype=torch.uint8, device="cuda")
    for fmt in FORMATS:
        with launch_log() as log:
            got = ctx.render_frames(empty, [], out_format=fmt)
            conv = Frames.from_bgr(ctx, empty, fmt)
        assert log == [] and (got.n, got.height, got.width) == (0, 18, 34) and conv.n == 0


@pytest.mark.parametrize("aligned", [False, True])
def test_bgr_frames_as_destination(ctx, aligned):
    """A BGR Frames as `out` -- padded rows, a gap between frames -- takes exactly the bytes of the
    tensor path, on the store route its alignment selects."""
    n, h, w = 3, 18, 34
    src = torch.from_numpy(oc.random_bgr(n, h, w, seed=5)).cuda()
    layers = [_crossing_pose(n, w, h, seed=6)]
    want = ctx.render_frames(src, layers, cast=CAST_CUDA).cpu().numpy()
    dst = Dest("bgr", n, h, w, aligned)
    with launch_log() as log:
        out = ctx.render_frames(src, layers, cast=CAST_CUDA, out=dst.frames)
    assert out is dst.frames
    ran(log, "render_frames<a4>" if aligned else "render_frames")
    ctx.sync()
    dst.check(want)
    assert (want != src.cpu().numpy()).any()
