"""Frames out on the CPU side: the numpy restatement of BGR -> YUV 4:2:0 (tests/yuv_out_cases.py)
against the known answers and the claims of the definition in include/opk.h, the opk_frames_out
struct, and every argument error of opk_bgr_to_frames, opk_render_frames_to and
opk_pose_render_frames_to on a host-only context -- all of them happen before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

from openpose_amd import _lib
from openpose_amd.api import (CAST_CPU, FRAMES_BGR, FRAMES_I420, FRAMES_NV12, Context, Net,
                              PoseExtractor)
from tests import yuv_cases as yc
from tests import yuv_out_cases as oc

OPK_ERR_ARG, OPK_ERR_STATE = 1, 3   # include/opk.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bgr,yuv", oc.KNOWN)
def test_known_answers(bgr, yuv):
    assert tuple(int(c) for c in oc.bgr_to_yuv(*bgr)) == yuv
    b, g, r = bgr   # and in plain Python integers, whose >> is arithmetic too
    assert ((oc.RY * r + oc.GY * g + oc.BY * b + oc.HALF + (16 << 20)) >> 20,
            (oc.RU * r + oc.GU * g + oc.BU * b + oc.HALF + (128 << 20)) >> 20,
            (oc.RV * r + oc.GV * g + oc.BV * b + oc.HALF + (128 << 20)) >> 20) == yuv


@pytest.fixture(scope="module")
def every_colour():
    i = np.arange(1 << 24, dtype=np.uint32)
    return i & 255, (i >> 8) & 255, i >> 16   # b, g, r


def test_every_colour_fits_int32_without_a_clamp(every_colour):
    """Over all 2^24 (B, G, R), in int64: every sum is non-negative and below 2^31, Y lies in
    [16, 235], U and V in [16, 240] with every bound reached -- so int32 is enough and no clamp
    is needed; int32 gives the same values."""
    wide = oc.sums(*every_colour, dtype=np.int64)
    for s in wide:
        assert s.dtype == np.int64 and int(s.min()) >= 0 and int(s.max()) < (1 << 31)
    y, u, v = (s >> 20 for s in wide)
    assert (int(y.min()), int(y.max())) == (16, 235)
    assert (int(u.min()), int(u.max())) == (16, 240)
    assert (int(v.min()), int(v.max())) == (16, 240)
    for a, b in zip(oc.bgr_to_yuv(*every_colour), (y, u, v)):
        np.testing.assert_array_equal(a, b)


def test_known_triples_are_the_input_tests_colours():
    """The blue and green of the header are the triples tests/yuv_cases.KNOWN maps back to pure
    blue and green."""
    back = dict(yc.KNOWN)
    assert back[(41, 240, 110)] == (255, 0, 0) and back[(145, 54, 34)][1] == 255


def test_chroma_depends_on_the_top_left_pixel_only():
    bgr = oc.random_bgr(3, 18, 34, seed=1)
    y, u, v = oc.bgr_to_yuv420(bgr)
    assert y.shape == (3, 18, 34) and u.shape == v.shape == (3, 9, 17) and y.dtype == np.uint8
    other = bgr.copy()
    g = np.random.default_rng(2)
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        other[:, dy::2, dx::2] = g.integers(0, 256, other[:, dy::2, dx::2].shape, dtype=np.uint8)
    y2, u2, v2 = oc.bgr_to_yuv420(other)
    np.testing.assert_array_equal(u, u2)
    np.testing.assert_array_equal(v, v2)
    np.testing.assert_array_equal(y[:, 0::2, 0::2], y2[:, 0::2, 0::2])
    assert not np.array_equal(y, y2)
    # and changing a top-left pixel does change them
    other = bgr.copy()
    other[:, 0::2, 0::2] ^= 0x80
    assert not np.array_equal(oc.bgr_to_yuv420(other)[1], u)
    _, uv = oc.to_nv12(y, u, v)
    np.testing.assert_array_equal(uv[:, :, 0::2], u)
    np.testing.assert_array_equal(uv[:, :, 1::2], v)


def test_exhaustive_frames_hold_every_colour_as_a_top_left_pixel():
    bgr = oc.exhaustive_bgr()
    top = bgr[:, 0::2, 0::2].astype(np.uint32)
    key = top[..., 0] | top[..., 1] << 8 | top[..., 2] << 16
    seen = np.zeros(1 << 24, bool)
    seen[key.ravel()] = True
    assert key.size == 1 << 24 and seen.all()
    for dy, dx in ((0, 1), (1, 0), (1, 1)):   # the other three differ from it in every channel
        assert (bgr[:, dy::2, dx::2] != bgr[:, 0::2, 0::2]).all()


def test_round_trip_of_constant_blocks(every_colour):
    """BGR -> YUV -> BGR (tests/yuv_cases, the input direction) of images whose 2 x 2 blocks are
    constant, so that the subsampling loses nothing: what is left is the rounding of the two 8-bit
    conversions.  Over every colour numpy shows a maximum error of 2 in B, 1 in G and 2 in R."""
    b, g, r = every_colour
    back = yc.yuv_to_bgr(*oc.bgr_to_yuv(b, g, r)).astype(np.int32)
    err = [int(np.abs(back[:, c] - src.astype(np.int32)).max()) for c, src in enumerate((b, g, r))]
    assert err == [2, 1, 2]
    # and through the frame functions, on an image of constant blocks
    blocks = np.random.default_rng(3).integers(0, 256, (2, 9, 17, 3), dtype=np.uint8)
    bgr = blocks.repeat(2, 1).repeat(2, 2)
    again = yc.yuv420_to_bgr(*oc.bgr_to_yuv420(bgr)).astype(np.int32)
    d = np.abs(again - bgr.astype(np.int32)).reshape(-1, 3).max(0)
    assert (d <= [2, 1, 2]).all()


def test_frames_out_struct_matches_header():
    """opk_frames_out: the fields of opk_frames in the same order and sizes, planes writable."""
    text = open(os.path.join(ROOT, "include", "opk.h")).read()
    body = re.search(r"typedef struct opk_frames_out \{(.*?)\} opk_frames_out;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert names == [f[0] for f in _lib.FramesOutStruct._fields_]
    assert names == [f[0] for f in _lib.FramesStruct._fields_]
    assert dict(re.findall(r"(\w+)\[(\d+)\]", body)) == {"plane": "3", "step": "3", "frame_bytes": "3"}
    assert re.search(r"[^t]\s+uint8_t\*\s+plane\[3\]", body), "writable planes"
    assert ctypes.sizeof(_lib.FramesOutStruct) == ctypes.sizeof(_lib.FramesStruct) == 16 + 3 * 24
    for (na, ta), (nb, tb) in zip(_lib.FramesOutStruct._fields_, _lib.FramesStruct._fields_):
        assert getattr(_lib.FramesOutStruct, na).offset == getattr(_lib.FramesStruct, nb).offset


def test_header_states_the_definition():
    text = open(os.path.join(ROOT, "include", "opk.h")).read()
    for c in (oc.RY, oc.GY, oc.BY, -oc.RU, -oc.GU, oc.BU, oc.RV, -oc.GV, -oc.BV):
        assert str(c) in text, c


# ---- the argument errors ---------------------------------------------------------------------------
BASE = 1 << 20   # "device pointers": nothing here reaches the device
W, H = 64, 48


def _fill(s, fmt, n, w, h, planes, step, frame_bytes):
    s.format, s.n, s.width, s.height = fmt, n, w, h
    for i in range(3):
        s.plane[i] = planes[i]
        s.step[i] = step[i]
        s.frame_bytes[i] = frame_bytes[i]
    return s


def _dst(fmt=FRAMES_NV12, n=1, w=W, h=H, planes=(BASE, 2 * BASE, 3 * BASE), step=(0, 0, 0),
         frame_bytes=(0, 0, 0)):
    return _fill(_lib.FramesOutStruct(), fmt, n, w, h, planes, step, frame_bytes)


def _src(fmt=FRAMES_BGR, n=1, w=W, h=H, planes=(8 * BASE, 9 * BASE, 10 * BASE), step=(0, 0, 0),
         frame_bytes=(0, 0, 0)):
    return _fill(_lib.FramesStruct(), fmt, n, w, h, planes, step, frame_bytes)


# (destination, text of the error): the descriptor's own errors, in the style of opk_frames'
BAD_DST = [
    (dict(fmt=3), "unknown frame format"),
    (dict(fmt=-1), "unknown frame format"),
    (dict(n=-1), "negative frame count"),
    (dict(n=2), "frame count differs"),
    (dict(w=W - 1), "even width and height"),
    (dict(h=H - 1), "even width and height"),
    (dict(fmt=FRAMES_I420, w=W - 1), "even width and height"),
    (dict(planes=(0, BASE, BASE)), "NULL plane"),
    (dict(planes=(BASE, 0, BASE)), "NULL plane"),
    (dict(fmt=FRAMES_I420, planes=(BASE, 2 * BASE, 0)), "NULL plane"),
    (dict(step=(W - 1, 0, 0)), "row step shorter than the row"),
    (dict(step=(0, W - 1, 0)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, W // 2 - 1, 0)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, 0, W // 2 - 1)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, W // 2, W // 2 + 16)), "share one row step"),
    # planes that overlap each other: the pair plane inside the luma plane, V on U, the last luma
    # byte; frames of one plane closer than a frame
    (dict(planes=(BASE, BASE + W, 0)), "overlap each other"),
    (dict(planes=(BASE, BASE + W * H - 1, 0)), "overlap each other"),
    (dict(fmt=FRAMES_I420, planes=(BASE, 2 * BASE, 2 * BASE + 5)), "overlap each other"),
]
# ... or the source (BGR at 8 * BASE, W * 3 bytes a row)
BAD_DST_SRC = [
    (dict(planes=(8 * BASE + 100, 2 * BASE, 0)), "overlap the source"),
    (dict(planes=(BASE, 8 * BASE + W * 3 * H - 1, 0)), "overlap the source"),
    (dict(fmt=FRAMES_I420, planes=(BASE, 2 * BASE, 8 * BASE - 1)), "overlap the source"),
]


@pytest.fixture(scope="module")
def host():
    ctx = Context.host_only()
    net = Net(ctx, "builtin:BODY_25")
    pose = PoseExtractor(ctx, net)
    yield ctx, pose
    pose.close()
    net.close()
    ctx.close()


def _calls(host):
    """The three functions as functions of (destination, source), other arguments valid."""
    ctx, pose = host
    L, ref = ctx.L, ctypes.byref
    parts = (ctypes.c_float * 4)(0.4, 0.6, 0.2, 0.6)
    return {
        "opk_bgr_to_frames": lambda d, s: L.opk_bgr_to_frames(ctx.h, ref(d), ref(s)),
        "opk_render_frames_to": lambda d, s: L.opk_render_frames_to(
            ctx.h, ref(d), ref(s), 1.0, None, 0, 1, CAST_CPU, None),
        "opk_pose_render_frames_to": lambda d, s: L.opk_pose_render_frames_to(
            pose.h, ref(d), ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1, CAST_CPU, None),
        "opk_pose_render_frames_to(element)": lambda d, s: L.opk_pose_render_frames_to(
            pose.h, ref(d), ref(s), 1.0, 5, 0.05, 0.6, 0.7, 0, 1, CAST_CPU, None),
        "opk_pose_render_frames_to(parts)": lambda d, s: L.opk_pose_render_frames_to(
            pose.h, ref(d), ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1, CAST_CPU, parts),
    }


NAMES = ["opk_bgr_to_frames", "opk_render_frames_to", "opk_pose_render_frames_to",
         "opk_pose_render_frames_to(element)", "opk_pose_render_frames_to(parts)"]


@pytest.mark.parametrize("name", NAMES)
def test_destination_errors_host_only(host, name):
    call, L = _calls(host)[name], host[0].L
    for kw, msg in BAD_DST + BAD_DST_SRC:
        assert call(_dst(**kw), _src()) == OPK_ERR_ARG, (name, kw)
        assert msg in L.opk_last_error().decode(), (name, kw, L.opk_last_error())
    # a destination frame stride shorter than a frame: its frames overlap each other
    assert call(_dst(n=2, frame_bytes=(W * H - 1, 0, 0)), _src(n=2)) == OPK_ERR_ARG
    assert "overlap each other" in L.opk_last_error().decode()
    # the decoder's surface layout -- Y and UV of a frame adjacent, frames a surface apart -- is fine
    # for the check: the error left is the call's own (no device, or nothing collected)
    surface = W * H * 3 // 2
    d = _dst(n=2, planes=(BASE, BASE + W * H, 0), frame_bytes=(surface, surface, 0))
    rc = call(d, _src(n=2))
    assert rc != 0 and "overlap" not in L.opk_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_source_errors_keep_their_text(host, name):
    """The source descriptor's errors are the `_fmt` calls'."""
    call, L = _calls(host)[name], host[0].L
    for kw, msg in [(dict(fmt=7), "unknown frame format"), (dict(n=-1), "negative frame count"),
                    (dict(step=(W * 3 - 1, 0, 0)), "row step shorter than the row")]:
        assert call(_dst(), _src(**kw)) == OPK_ERR_ARG, (name, kw)
        assert msg in L.opk_last_error().decode(), (name, kw, L.opk_last_error())


def test_bgr_to_frames_own_errors(host):
    ctx, _ = host
    L, call = ctx.L, _calls(host)["opk_bgr_to_frames"]
    assert call(_dst(), _src(fmt=FRAMES_NV12)) == OPK_ERR_ARG
    assert "source frames must be BGR" in L.opk_last_error().decode()
    assert call(_dst(fmt=FRAMES_BGR), _src()) == OPK_ERR_ARG
    assert "nothing to convert" in L.opk_last_error().decode()
    assert call(_dst(w=W + 2), _src()) == OPK_ERR_ARG
    assert "width and height differ" in L.opk_last_error().decode()
    assert L.opk_bgr_to_frames(ctx.h, None, ctypes.byref(_src())) == OPK_ERR_ARG
    assert L.opk_bgr_to_frames(ctx.h, ctypes.byref(_dst()), None) == OPK_ERR_ARG
    assert L.opk_bgr_to_frames(None, ctypes.byref(_dst()), ctypes.byref(_src())) == OPK_ERR_ARG
    # valid arguments reach the device step, which a host-only context refuses
    assert call(_dst(), _src()) == OPK_ERR_STATE and "host-only" in L.opk_last_error().decode()


def test_wrapped_calls_keep_their_errors(host):
    """The errors of the calls being wrapped, with a valid destination: same code, same text."""
    ctx, pose = host
    L, ref = ctx.L, ctypes.byref
    fake = ctypes.c_void_p(BASE)
    d, s = _dst(), _src()

    def both(to, fmt):
        a = to()
        ta = L.opk_last_error().decode()
        b = fmt()
        assert a == b != 0 and ta == L.opk_last_error().decode(), (a, b, ta, L.opk_last_error())
        return a, ta

    # an unknown cast, too many layers, a bad scale, an unknown heat kind
    for n_layers, cast, scale in ((0, 7, 1.0), (4, CAST_CPU, 1.0), (0, CAST_CPU, -1.0)):
        both(lambda: L.opk_render_frames_to(ctx.h, ref(d), ref(s), scale, None, n_layers, 1, cast, None),
             lambda: L.opk_render_frames_fmt(ctx.h, fake, 0, W, H, ref(s), scale, None, n_layers, 1, cast))
    heat = _lib.RenderHeatStruct()
    heat.kind = 9
    rc, text = both(lambda: L.opk_render_frames_to(ctx.h, ref(d), ref(s), 1.0, None, 0, 1, CAST_CPU, ref(heat)),
                    lambda: L.opk_render_frames_heat_fmt(ctx.h, fake, 0, W, H, ref(s), 1.0, None, 0, 1,
                                                         CAST_CPU, ref(heat)))
    assert rc == OPK_ERR_ARG and "unknown heat kind" in text
    # the pose calls: nothing collected is a state error; an element past the model's last an
    # argument error
    rc, text = both(lambda: L.opk_pose_render_frames_to(pose.h, ref(d), ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1,
                                                        CAST_CPU, None),
                    lambda: L.opk_pose_render_frames_fmt(pose.h, fake, 0, W, H, ref(s), 1.0, 0.05, 0.6, 0, 1,
                                                         CAST_CPU))
    assert rc == OPK_ERR_STATE and "no collected batch" in text
    rc, text = both(lambda: L.opk_pose_render_frames_to(pose.h, ref(d), ref(s), 1.0, 9999, 0.05, 0.6, 0.7, 0,
                                                        1, CAST_CPU, None),
                    lambda: L.opk_pose_render_frames_element_fmt(pose.h, fake, 0, W, H, ref(s), 1.0, 9999,
                                                                 0.05, 0.6, 0.7, 0, 1, CAST_CPU))
    assert rc == OPK_ERR_ARG
    parts = (ctypes.c_float * 4)(0.4, 0.6, 0.2, 0.6)
    rc, text = both(lambda: L.opk_pose_render_frames_to(pose.h, ref(d), ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1,
                                                        CAST_CPU, parts),
                    lambda: L.opk_pose_render_frames_parts_fmt(pose.h, fake, 0, W, H, ref(s), 1.0, 0.05, 0.6,
                                                               0, 1, CAST_CPU, 0.4, 0.6, 0.2, 0.6))
    assert rc == OPK_ERR_STATE
    # part layers go with the keypoints
    assert L.opk_pose_render_frames_to(pose.h, ref(d), ref(s), 1.0, 5, 0.05, 0.6, 0.7, 0, 1, CAST_CPU,
                                       parts) == OPK_ERR_ARG
    assert "element 0" in L.opk_last_error().decode()
    # NULL arguments
    assert L.opk_render_frames_to(ctx.h, None, ref(s), 1.0, None, 0, 1, CAST_CPU, None) == OPK_ERR_ARG
    assert L.opk_render_frames_to(ctx.h, ref(d), None, 1.0, None, 0, 1, CAST_CPU, None) == OPK_ERR_ARG
    assert L.opk_pose_render_frames_to(pose.h, None, ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1, CAST_CPU,
                                       None) == OPK_ERR_ARG
    assert L.opk_pose_render_frames_to(None, ref(d), ref(s), 1.0, 0, 0.05, 0.6, 0.7, 0, 1, CAST_CPU,
                                       None) == OPK_ERR_ARG


@pytest.mark.parametrize("fmt", [FRAMES_BGR, FRAMES_NV12, FRAMES_I420])
def test_no_frames_succeed_without_a_device(host, fmt):
    """n == 0: no plane is needed and nothing runs, on a host-only context."""
    ctx, _ = host
    L, ref = ctx.L, ctypes.byref
    d, s = _dst(fmt=fmt, n=0, planes=(0, 0, 0)), _src(n=0, planes=(0, 0, 0))
    assert L.opk_render_frames_to(ctx.h, ref(d), ref(s), 1.0, None, 0, 1, CAST_CPU, None) == 0
    if fmt != FRAMES_BGR:
        assert L.opk_bgr_to_frames(ctx.h, ref(d), ref(s)) == 0
    # a size change is an argument like any other
    d2 = _dst(fmt=fmt, n=0, w=32, h=24, planes=(0, 0, 0))
    assert L.opk_render_frames_to(ctx.h, ref(d2), ref(s), 0.5, None, 0, 1, CAST_CPU, None) == 0
