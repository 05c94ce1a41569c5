"""YUV 4:2:0 frames on the CPU side: the numpy restatement of the conversion (tests/yuv_cases.py)
against the known answers of the definition in include/opk.h, the opk_frames struct, and the
argument checks of every `_fmt` entry point on a host-only context -- all of them happen before any
device work."""
import ctypes
import os
import re

import numpy as np
import pytest

from openpose_amd import _lib
from openpose_amd.api import (CAST_CPU, FACE, FRAMES_BGR, FRAMES_I420, FRAMES_NV12, Context,
                              KeypointExtractor, Net, PoseExtractor)
from tests import yuv_cases as yc

OPK_ERR_ARG = 1   # include/opk.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("yuv,bgr", yc.KNOWN)
def test_known_answers(yuv, bgr):
    assert tuple(int(c) for c in yc.yuv_to_bgr(*yuv)) == bgr


def test_extremes_fit_int32():
    """The largest and smallest sums of the definition, in int64: inside int32."""
    y = np.int64(yc.CY) * (255 - 16) + (1 << 19)
    assert int(y + yc.CUB * 127) == 560969128
    assert int((1 << 19) + yc.CVG * 127 + yc.CUG * 127) > -(1 << 31)
    assert int((1 << 19) + yc.CUB * -128) == -270327040


def test_nv12_and_i420_give_the_same_image():
    y, u, v = yc.random_planes(3, 18, 34, seed=1)
    a = yc.yuv420_to_bgr(y, u, v)
    b = yc.nv12_to_bgr(y, yc.interleave(u, v))
    assert a.shape == (3, 18, 34, 3) and a.dtype == np.uint8
    np.testing.assert_array_equal(a, b)
    # nearest chroma: the four pixels of a block with equal luma are equal
    flat = yc.yuv420_to_bgr(np.full_like(y, 100), u, v)
    np.testing.assert_array_equal(flat[:, 0::2, 0::2], flat[:, 1::2, 1::2])
    np.testing.assert_array_equal(flat[:, 0::2, 1::2], flat[:, 1::2, 0::2])


def test_exhaustive_planes_hold_every_triple():
    y, u, v = yc.exhaustive_planes()
    key = (y.astype(np.uint32) << 16 | u.repeat(2, 1).repeat(2, 2).astype(np.uint32) << 8
           | v.repeat(2, 1).repeat(2, 2))
    seen = np.zeros(1 << 24, bool)
    seen[key.ravel()] = True
    assert key.size == 1 << 24 and seen.all()


def test_frames_struct_matches_header():
    """format, n, width, height, plane, step, frame_bytes -- the field order and array sizes of
    opk_frames in include/opk.h; the format values."""
    text = open(os.path.join(ROOT, "include", "opk.h")).read()
    body = re.search(r"typedef struct opk_frames \{(.*?)\} opk_frames;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*(?=[,;])", body)
    assert names == [f[0] for f in _lib.FramesStruct._fields_]
    sizes = dict(re.findall(r"(\w+)\[(\d+)\]", body))
    assert sizes == {"plane": "3", "step": "3", "frame_bytes": "3"}
    for name, ctype in _lib.FramesStruct._fields_:
        assert ctypes.sizeof(ctype) == (4 if name in ("format", "n", "width", "height") else 24)
    assert ctypes.sizeof(_lib.FramesStruct) == 16 + 3 * 24
    values = dict(re.findall(r"#define (OPK_FRAMES_\w+)\s+(\d+)", text))
    assert values == {"OPK_FRAMES_BGR": str(FRAMES_BGR), "OPK_FRAMES_NV12": str(FRAMES_NV12),
                      "OPK_FRAMES_I420": str(FRAMES_I420)}


FAKE = 64   # a non-NULL "device pointer": nothing here reaches the device


def _desc(fmt=FRAMES_NV12, n=1, w=64, h=48, planes=(FAKE, FAKE, FAKE), step=(0, 0, 0),
          frame_bytes=(0, 0, 0)):
    s = _lib.FramesStruct()
    s.format, s.n, s.width, s.height = fmt, n, w, h
    for i in range(3):
        s.plane[i] = planes[i]
        s.step[i] = step[i]
        s.frame_bytes[i] = frame_bytes[i]
    return s


# (descriptor, text of the error)
BAD = [
    (dict(fmt=3), "unknown frame format"),
    (dict(fmt=-1), "unknown frame format"),
    (dict(n=-1), "negative frame count"),
    (dict(fmt=FRAMES_BGR, n=-1), "negative frame count"),
    (dict(w=63), "even width and height"),
    (dict(h=47), "even width and height"),
    (dict(fmt=FRAMES_I420, w=63), "even width and height"),
    (dict(planes=(0, FAKE, FAKE)), "NULL plane"),
    (dict(planes=(FAKE, 0, FAKE)), "NULL plane"),
    (dict(fmt=FRAMES_I420, planes=(FAKE, FAKE, 0)), "NULL plane"),
    (dict(fmt=FRAMES_I420, planes=(FAKE, 0, FAKE)), "NULL plane"),
    (dict(step=(63, 0, 0)), "row step shorter than the row"),
    (dict(step=(0, 63, 0)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, 31, 0)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, 0, 31)), "row step shorter than the row"),
    (dict(fmt=FRAMES_I420, step=(0, 32, 48)), "share one row step"),
    (dict(fmt=FRAMES_BGR, step=(191, 0, 0)), "row step shorter than the row"),
]


@pytest.fixture(scope="module")
def host():
    ctx = Context.host_only()
    nets = {k: Net(ctx, k) for k in ("builtin:BODY_25", "builtin:FACE")}
    pose = PoseExtractor(ctx, nets["builtin:BODY_25"])
    face = KeypointExtractor(ctx, nets["builtin:FACE"], FACE, (176, 176))
    yield ctx, pose, face
    face.close()
    pose.close()
    for n in nets.values():
        n.close()
    ctx.close()


def _fmt_calls(host):
    """Every `_fmt` entry point as a function of the descriptor, other arguments valid."""
    ctx, pose, face = host
    L, fake = ctx.L, ctypes.c_void_p(FAKE)
    ref = ctypes.byref
    rect = (ctypes.c_float * 4)(10, 10, 50, 50)
    kp = (ctypes.c_float * (70 * 3))()
    return {
        "opk_frames_to_bgr": lambda d: L.opk_frames_to_bgr(ctx.h, fake, 0, ref(d)),
        "opk_cvmat_to_input_fmt": lambda d: L.opk_cvmat_to_input_fmt(ctx.h, fake, ref(d), 1.0, 64, 48, 1),
        "opk_pose_submit_frames_fmt": lambda d: L.opk_pose_submit_frames_fmt(pose.h, ref(d)),
        "opk_pose_forward_frames_fmt": lambda d: L.opk_pose_forward_frames_fmt(pose.h, ref(d)),
        "opk_extractor_forward_fmt": lambda d: L.opk_extractor_forward_fmt(face.h, ref(d), rect, None, 1, kp),
        "opk_cvmat_to_output_fmt": lambda d: L.opk_cvmat_to_output_fmt(ctx.h, fake, ref(d), 1.0, 64, 48),
        "opk_render_frames_fmt": lambda d: L.opk_render_frames_fmt(
            ctx.h, fake, 0, 64, 48, ref(d), 1.0, None, 0, 1, CAST_CPU),
        "opk_render_frames_heat_fmt": lambda d: L.opk_render_frames_heat_fmt(
            ctx.h, fake, 0, 64, 48, ref(d), 1.0, None, 0, 1, CAST_CPU, None),
        "opk_pose_render_frames_fmt": lambda d: L.opk_pose_render_frames_fmt(
            pose.h, fake, 0, 64, 48, ref(d), 1.0, 0.05, 0.6, 0, 1, CAST_CPU),
        "opk_pose_render_frames_parts_fmt": lambda d: L.opk_pose_render_frames_parts_fmt(
            pose.h, fake, 0, 64, 48, ref(d), 1.0, 0.05, 0.6, 0, 1, CAST_CPU, 0.4, 0.6, 0.2, 0.6),
        "opk_pose_render_frames_element_fmt": lambda d: L.opk_pose_render_frames_element_fmt(
            pose.h, fake, 0, 64, 48, ref(d), 1.0, 5, 0.05, 0.6, 0.7, 0, 1, CAST_CPU),
    }


def test_every_fmt_function_is_covered(host):
    fmt = {n for n in _lib.exported_symbols() if n.endswith("_fmt")} | {"opk_frames_to_bgr"}
    assert set(_fmt_calls(host)) == fmt and len(fmt) == 11


@pytest.mark.parametrize("name", ["opk_frames_to_bgr", "opk_cvmat_to_input_fmt",
                                  "opk_pose_submit_frames_fmt", "opk_pose_forward_frames_fmt",
                                  "opk_extractor_forward_fmt", "opk_cvmat_to_output_fmt",
                                  "opk_render_frames_fmt", "opk_render_frames_heat_fmt",
                                  "opk_pose_render_frames_fmt", "opk_pose_render_frames_parts_fmt",
                                  "opk_pose_render_frames_element_fmt"])
def test_fmt_abi_errors_host_only(host, name):
    call = _fmt_calls(host)[name]
    L = host[0].L
    for kw, msg in BAD:
        if name == "opk_frames_to_bgr" and kw.get("fmt") == FRAMES_BGR:
            continue   # refused as a whole: nothing to convert (below)
        assert call(_desc(**kw)) == OPK_ERR_ARG, (name, kw)
        assert msg in L.opk_last_error().decode(), (name, kw, L.opk_last_error())
    if name == "opk_frames_to_bgr":
        assert call(_desc(fmt=FRAMES_BGR)) == OPK_ERR_ARG
        assert "nothing to convert" in L.opk_last_error().decode()


def test_null_descriptor_is_an_argument_error(host):
    ctx, pose, face = host
    L, fake = ctx.L, ctypes.c_void_p(FAKE)
    assert L.opk_frames_to_bgr(ctx.h, fake, 0, None) == OPK_ERR_ARG
    assert L.opk_cvmat_to_input_fmt(ctx.h, fake, None, 1.0, 64, 48, 1) == OPK_ERR_ARG
    assert L.opk_pose_submit_frames_fmt(pose.h, None) == OPK_ERR_ARG
    assert L.opk_render_frames_fmt(ctx.h, fake, 0, 64, 48, None, 1.0, None, 0, 1, CAST_CPU) == OPK_ERR_ARG


@pytest.mark.parametrize("fmt", [FRAMES_BGR, FRAMES_NV12, FRAMES_I420])
def test_no_frames_succeed_without_a_device(host, fmt):
    """n == 0 where the pointer-taking function succeeds on it: no plane is needed, nothing runs."""
    ctx, _, _ = host
    L = ctx.L
    d = _desc(fmt=fmt, n=0, planes=(0, 0, 0))
    ref = ctypes.byref(d)
    assert L.opk_cvmat_to_output(ctx.h, None, None, 0, 64, 48, 0, 1.0, 64, 48) == 0
    assert L.opk_cvmat_to_output_fmt(ctx.h, None, ref, 1.0, 64, 48) == 0
    assert L.opk_render_frames(ctx.h, None, 0, 64, 48, None, 0, 64, 48, 0, 1.0, None, 0, 1, CAST_CPU) == 0
    assert L.opk_render_frames_fmt(ctx.h, None, 0, 64, 48, ref, 1.0, None, 0, 1, CAST_CPU) == 0
    assert L.opk_render_frames_heat_fmt(ctx.h, None, 0, 64, 48, ref, 1.0, None, 0, 1, CAST_CPU, None) == 0
    if fmt != FRAMES_BGR:
        assert L.opk_frames_to_bgr(ctx.h, None, 0, ref) == 0
