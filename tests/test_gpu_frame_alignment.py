"""GPU: the alignment predicate of the frame description (host/frames.h), one term at a time.

Five launchers choose between a vectorised and a plain route by frames_aligned(): the frame warp and
frames_to_bgr on their source, bgr_to_frames on both sides, the batch render's BGR store and its
NV12 / I420 stores on their destination.  For each, 2 frames of 32 x 4 pixels -- the smallest width
with a whole 16-pixel piece and a tile-wide 4-byte store -- lie in views sliced out of one buffer:
fully aligned (the vectorised route in the launch log), then with exactly one term of the predicate
broken -- luma base, step or frame stride, a chroma base, the chroma step, a chroma frame stride --
which must take the plain route; the bytes are numpy's either way (tests/yuv_cases, yuv_out_cases,
the oracle's warp) and nothing outside the samples of a destination is written.  The case that
tells the formats apart: chroma planes on 8- but not 16-byte boundaries still take the 16-pixel
pieces with I420 (two 8-byte halves) and not with NV12 (one 16-byte load of pairs).
"""
import numpy as np
import pytest
import torch

import oracle
from openpose_amd.api import Frames, launch_log
from tests import yuv_cases as yc
from tests import yuv_out_cases as oc

pytestmark = pytest.mark.gpu

N, H, W = 2, 4, 32
CANARY = 0x5C
REGION = 1024   # bytes of the buffer each plane has to itself


def _layout(fmt):
    """Every term a multiple of 16: rows padded by 16 bytes, 32 bytes between frames."""
    if fmt == "bgr":
        return dict(base=[0], step=[W * 3 + 16], frame=[H * (W * 3 + 16) + 32])
    crow = W if fmt == "nv12" else W // 2
    planes = 2 if fmt == "nv12" else 3
    return dict(base=[0] * planes, step=[W + 16] + [crow + 16] * (planes - 1),
                frame=[H * (W + 16) + 64] + [H // 2 * (crow + 16) + 32] * (planes - 1))


def _terms(fmt):
    """(name, [(field, plane)]) of every term of the predicate; I420's U and V share one row step."""
    t = [("luma base", [("base", 0)]), ("luma step", [("step", 0)]), ("luma frame", [("frame", 0)])]
    if fmt == "bgr":
        return t
    chroma = (1,) if fmt == "nv12" else (1, 2)
    t += [("chroma base %d" % p, [("base", p)]) for p in chroma]
    t += [("chroma step", [("step", p) for p in chroma])]
    t += [("chroma frame %d" % p, [("frame", p)]) for p in chroma]
    return t


def _cases(fmt, access):
    """(name, layout, vectorised) -- access: 16 for the 16-pixel pieces, 4 for the render's stores."""
    yield "aligned", _layout(fmt), True
    for name, fields in _terms(fmt):
        lay = _layout(fmt)
        chroma = fields[0][1] > 0
        # half the access the term needs: on that boundary and not on the next
        need = 8 if (access == 16 and fmt == "i420" and chroma) else access
        for field, p in fields:
            lay[field][p] += need // 2
        yield name, lay, False
    if access == 16 and fmt != "bgr":
        lay = _layout(fmt)
        for p in range(1, len(lay["base"])):
            for field in ("base", "step", "frame"):
                lay[field][p] += 8
        yield "chroma on 8, not 16", lay, fmt == "i420"


class Views:
    """The planes of N frames of W x H in `fmt`, each a strided view into its own region of one
    buffer of canary bytes."""

    def __init__(self, fmt, lay, planes=None):
        self.fmt = fmt
        crow = W if fmt == "nv12" else W // 2
        shapes = [(H, W * 3)] if fmt == "bgr" else [(H, W)] + [(H // 2, crow)] * (len(lay["base"]) - 1)
        self.buf = torch.full((REGION * len(shapes),), CANARY, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.views = []
        for i, (rows, row) in enumerate(shapes):
            step, frame = lay["step"][i], lay["frame"][i]
            assert step >= row and frame >= rows * step and lay["base"][i] + N * frame <= REGION
            self.views.append(self.buf[i * REGION + lay["base"][i]:].as_strided(
                (N, rows, row), (frame, step, 1)))
        if planes is not None:
            for v, p in zip(self.views, planes):
                v.copy_(torch.from_numpy(np.ascontiguousarray(p)))
        make = {"bgr": Frames.bgr, "nv12": Frames.nv12, "i420": Frames.i420}[fmt]
        self.frames = make(*self.views, width=W)

    def check(self, want):
        """The samples are `want` (a list of numpy planes) and every other byte is the canary."""
        for i, (v, w) in enumerate(zip(self.views, want)):
            np.testing.assert_array_equal(v.cpu().numpy(), w, err_msg="plane %d" % i)
        kept = [v.clone() for v in self.views]
        for v in self.views:
            v.fill_(CANARY)
        assert bool((self.buf == CANARY).all()), "a byte outside the samples was written"
        for v, k in zip(self.views, kept):
            v.copy_(k)


def _ran(log, route):
    assert [k for _, k in log] == [route], (route, log)


@pytest.fixture(scope="module")
def ref():
    """The references, made once: YUV planes and numpy's BGR of them; BGR frames and numpy's planes
    of them; the oracle's half-size net input of both BGR images."""
    y, u, v = yc.random_planes(N, H, W, seed=77)
    yuv_bgr = yc.yuv420_to_bgr(y, u, v)
    bgr = oc.random_bgr(N, H, W, seed=78)
    by, bu, bv = oc.bgr_to_yuv420(bgr)

    def warp(img):
        return np.stack([oracle.cvmat_to_input(img[f], 0.5, W // 2, H // 2) for f in range(N)])
    return dict(yuv={"nv12": [y, yc.interleave(u, v)], "i420": [y, u, v]}, yuv_bgr=yuv_bgr, bgr=bgr,
                bgr_yuv={"nv12": list(oc.to_nv12(by, bu, bv)), "i420": [by, bu, bv]},
                warp_yuv=warp(yuv_bgr), warp_bgr=warp(bgr))


def _source(ref, fmt, lay):
    planes = [ref["bgr"].reshape(N, H, W * 3)] if fmt == "bgr" else ref["yuv"][fmt]
    return Views(fmt, lay, planes).frames


@pytest.mark.parametrize("fmt", ["bgr", "nv12", "i420"])
def test_frame_warp(ctx, ref, fmt):
    tag = "" if fmt == "bgr" else ",yuv"
    for name, lay, vec in _cases(fmt, 16):
        out = torch.full((N, 3, H // 2, W // 2), float("nan"), device="cuda")
        with launch_log() as log:
            ctx.cvmat_to_input(out, _source(ref, fmt, lay), 0.5)
        _ran(log, "cvmat_to_input_lds<2%s%s>" % (",a16" if vec else "", tag))
        np.testing.assert_array_equal(out.cpu().numpy(), ref["warp_bgr" if fmt == "bgr" else "warp_yuv"],
                                      err_msg=name)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_frames_to_bgr(ctx, ref, fmt):
    for name, lay, vec in _cases(fmt, 16):
        out = torch.full((N, H, W * 3 + 16), CANARY, dtype=torch.uint8, device="cuda")
        with launch_log() as log:
            _source(ref, fmt, lay).to_bgr(ctx, out)
        _ran(log, "yuv420_to_bgr<v16>" if vec else "yuv420_to_bgr")
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:, :, :W * 3].reshape(N, H, W, 3), ref["yuv_bgr"], err_msg=name)
        assert (got[:, :, W * 3:] == CANARY).all(), name


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_bgr_to_frames(ctx, ref, fmt):
    """The destination's terms with an aligned source, then the BGR source's with an aligned
    destination."""
    runs = [(name, _layout("bgr"), lay, vec) for name, lay, vec in _cases(fmt, 16)]
    runs += [("source " + name, lay, _layout(fmt), vec) for name, lay, vec in _cases("bgr", 16)][1:]
    for name, src_lay, dst_lay, vec in runs:
        dst = Views(fmt, dst_lay)
        with launch_log() as log:
            Frames.from_bgr(ctx, _source(ref, "bgr", src_lay), None, out=dst.frames)
        _ran(log, "bgr_to_yuv420<v16>" if vec else "bgr_to_yuv420")
        ctx.sync()
        dst.check(ref["bgr_yuv"][fmt])


@pytest.mark.parametrize("fmt", ["bgr", "nv12", "i420"])
def test_render_store(ctx, ref, fmt):
    """No layer, no warp: the drawn frame is the source frame (every byte survives the float image
    and either cast), so the destination holds its bytes or numpy's samples of them."""
    src = torch.from_numpy(ref["bgr"]).cuda()
    want = [ref["bgr"].reshape(N, H, W * 3)] if fmt == "bgr" else ref["bgr_yuv"][fmt]
    tag = "" if fmt == "bgr" else fmt
    for name, lay, vec in _cases(fmt, 4):
        dst = Views(fmt, lay)
        with launch_log() as log:
            ctx.render_frames(src, [], out=dst.frames)
        _ran(log, "render_frames<a4%s>" % ("," + tag if tag else "") if vec
             else "render_frames" + ("<%s>" % tag if tag else ""))
        ctx.sync()
        dst.check(want)
