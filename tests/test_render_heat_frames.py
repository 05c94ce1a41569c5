"""The heat layer of the batch frame render on the CPU side: opk_render_heat against the header,
opk_render_element against PoseGpuRenderer::renderPose's element mapping restated from the pose
tables, and the argument checks of opk_render_frames_heat / opk_pose_render_frames_element on a
host-only context (every one of them happens before any device work)."""
import ctypes
import json
import os
import re

import pytest

from openpose_amd import _lib
from openpose_amd.api import (CAST_CPU, HEAT_DISTANCE, HEAT_NONE, HEAT_PAF, HEAT_PAFS, HEAT_PART,
                              HEAT_PARTS, render_element)

OPK_ERR_ARG, OPK_ERR_STATE = 1, 3        # include/opk.h
BODY_25, BODY_25D = 0, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_tables.json")))


@pytest.fixture(scope="module")
def host():
    from openpose_amd.api import Context
    ctx = Context.host_only()
    yield ctx
    ctx.close()


def test_render_heat_struct_matches_header():
    text = open(os.path.join(ROOT, "include", "opk.h")).read()
    body = re.search(r"typedef struct opk_render_heat \{(.*?)\} opk_render_heat;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*(?=[,;])", body)
    assert names == [f[0] for f in _lib.RenderHeatStruct._fields_]
    kinds = dict(re.findall(r"#define OPK_HEAT_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in kinds.items()} == dict(
        NONE=HEAT_NONE, PART=HEAT_PART, PARTS=HEAT_PARTS, PAF=HEAT_PAF, PAFS=HEAT_PAFS,
        DISTANCE=HEAT_DISTANCE)


def _last_element(t):
    """getNumberElementsToRender - 1 (poseParametersRender.cpp:98-113)."""
    pb = t["parts"] + int(t["bkg"])
    last = pb + 2 + len(t["pairs"]) // 2
    return last + (2 * (t["parts"] - 1) if t["name"] == "BODY_25D" else 0)


def _restated(t, e):
    """renderPose's mapping (poseGpuRenderer.cpp:102-202) from the pose tables."""
    parts, bkg, pairs = t["parts"], int(t["bkg"]), len(t["pairs"]) // 2
    pb = parts + bkg
    if e == 0:
        return HEAT_NONE, 0
    if e == 1:
        return HEAT_PART, parts if bkg else 0
    if e == 2:
        return HEAT_PARTS, 0
    if e == 3:
        return HEAT_PAFS, pb
    if e <= pb + 2:
        return HEAT_PART, e - 3 - bkg
    if e <= pb + 2 + pairs:
        return HEAT_PAF, pb + t["map_idx"][2 * (e - pb - 3)]
    return HEAT_DISTANCE, pb + 2 * pairs + (e - (pb + 2 + pairs) - 1)


def test_render_element_every_model_and_element():
    assert len(TABLES) == 15
    seen = set()
    for t in TABLES:
        for e in range(_last_element(t) + 1):
            kind, channel = render_element(t["id"], e)
            want = _restated(t, e)
            if want[0] in (HEAT_NONE, HEAT_PARTS):   # no channel of their own
                assert kind == want[0], (t["name"], e)
            else:
                assert (kind, channel) == want, (t["name"], e)
            seen.add(kind)
    assert seen == {HEAT_NONE, HEAT_PART, HEAT_PARTS, HEAT_PAF, HEAT_PAFS, HEAT_DISTANCE}
    # BODY_25: 25 parts + background, 26 pairs
    assert render_element(BODY_25, 1) == (HEAT_PART, 25)
    assert render_element(BODY_25, 4) == (HEAT_PART, 0)
    assert render_element(BODY_25, 28) == (HEAT_PART, 24)
    assert render_element(BODY_25, 29) == (HEAT_PAF, 26 + TABLES[0]["map_idx"][0])
    assert render_element(BODY_25D, 55) == (HEAT_DISTANCE, 78)
    assert render_element(BODY_25D, 102) == (HEAT_DISTANCE, 125)
    # a model without background (BODY_25B): element 1 is channel 0, element 4 part 0
    assert render_element(13, 1) == (HEAT_PART, 0)
    assert render_element(13, 4) == (HEAT_PART, 1)


def test_render_element_errors():
    L = _lib.load()
    k, c = ctypes.c_int(), ctypes.c_int()

    def call(model, e):
        return L.opk_render_element(model, e, ctypes.byref(k), ctypes.byref(c))

    for t in TABLES:
        rc = call(t["id"], _last_element(t) + 1)
        assert rc == OPK_ERR_ARG
        msg = L.opk_last_error().decode()
        if t["name"] == "BODY_25D":
            assert "past the model's last" in msg
        else:
            assert "Neck-part distance channel only for BODY_25D." in msg
    assert call(BODY_25, -1) == OPK_ERR_ARG
    assert call(15, 0) == OPK_ERR_ARG
    assert "Invalid Model." in L.opk_last_error().decode()
    assert L.opk_render_element(BODY_25, 2, None, None) == 0


def _heat(kind=HEAT_PART, channel=0, channels=30, size=(40, 25), alpha=0.7, pose_model=0, scale=2.3,
          ptr=64):
    return _lib.RenderHeatStruct(kind, pose_model, channel, ctypes.c_void_p(ptr), channels, size[0],
                                 size[1], scale, alpha)


def test_render_frames_heat_errors_host_only(host):
    L = host.L
    fake = ctypes.c_void_p(64)

    def frames(heat, n=1, blend=1, layers=None, n_layers=0):
        return L.opk_render_frames_heat(host.h, fake, 0, 64, 48, fake, n, 64, 48, 0, 1.0, layers,
                                        n_layers, blend, CAST_CPU, ctypes.byref(heat))

    cases = [
        (_heat(alpha=1.5), {}, "Alpha must be in the range [0, 1]."),
        (_heat(alpha=-0.1), {}, "Alpha must be in the range [0, 1]."),
        (_heat(HEAT_PARTS, pose_model=15), {}, "Invalid Model."),
        (_heat(HEAT_PAFS, pose_model=-1, channels=200), {}, "Invalid Model."),
        (_heat(HEAT_PAF, pose_model=15), {}, "Invalid Model."),
        (_heat(kind=0), {}, "heat kind"),
        (_heat(kind=6), {}, "heat kind"),
        (_heat(channel=30), {}, "channel outside"),
        (_heat(channel=-1), {}, "channel outside"),
        (_heat(HEAT_DISTANCE, channel=30), {}, "channel outside"),
        (_heat(HEAT_PAF, channel=29), {}, "channel outside"),          # its y channel is 30
        (_heat(HEAT_PARTS, channels=24), {}, "channel outside"),      # BODY_25 draws 25 parts
        (_heat(HEAT_PAFS, channels=77), {}, "channel outside"),       # 26 + 52 channels
        (_heat(size=(0, 25)), {}, "empty heat map"),
        (_heat(ptr=None), {}, "NULL heat"),
        (_heat(), dict(blend=0), "never clear the frame"),
    ]
    for heat, kw, msg in cases:
        assert frames(heat, **kw) == OPK_ERR_ARG, msg
        assert msg in L.opk_last_error().decode(), (msg, L.opk_last_error())
    # the frame render's own checks still hold with a heat layer
    assert L.opk_render_frames_heat(host.h, fake, 0, 0, 48, fake, 1, 64, 48, 0, 1.0, None, 0, 1,
                                    CAST_CPU, ctypes.byref(_heat())) == OPK_ERR_ARG
    assert "Output resolution has 0 area." in L.opk_last_error().decode()
    # valid calls of every kind reach the device work, which a host-only context refuses with a
    # state error: every argument check lies before it
    for heat in (_heat(), _heat(HEAT_PART, channel=29), _heat(HEAT_PARTS, channels=25),
                 _heat(HEAT_PAF, channel=28), _heat(HEAT_PAFS, channels=78),
                 _heat(HEAT_DISTANCE, channel=29, alpha=1.0)):
        assert frames(heat) == OPK_ERR_STATE
        assert "host-only" in L.opk_last_error().decode()
    # without a heat layer it is opk_render_frames
    assert L.opk_render_frames_heat(host.h, fake, 0, 64, 48, fake, 1, 64, 48, 0, 1.0, None, 0, 1,
                                    CAST_CPU, None) == OPK_ERR_STATE


def test_no_frames_is_success_without_device_work(host):
    L = host.L
    fake = ctypes.c_void_p(64)
    for heat in (_heat(), _heat(HEAT_PARTS), _heat(HEAT_PAFS, channels=78), _heat(ptr=None)):
        assert L.opk_render_frames_heat(host.h, fake, 0, 64, 48, fake, 0, 64, 48, 0, 1.0, None, 0,
                                        1, CAST_CPU, ctypes.byref(heat)) == 0
    # the argument errors come first even then
    assert L.opk_render_frames_heat(host.h, fake, 0, 64, 48, fake, 0, 64, 48, 0, 1.0, None, 0, 1,
                                    CAST_CPU, ctypes.byref(_heat(alpha=2.0))) == OPK_ERR_ARG


def test_pose_render_frames_element_needs_a_collected_batch(host):
    from openpose_amd.api import PoseExtractor
    pose = PoseExtractor(host, net=None)
    L = host.L
    fake = ctypes.c_void_p(64)

    def call(element):
        return L.opk_pose_render_frames_element(pose.h, fake, 0, 64, 48, fake, 2, 64, 48, 0, 1.0,
                                                element, 0.05, 0.6, 0.7, 0, 1, CAST_CPU)

    for element in (0, 1, 2, 3, 4, 29):
        assert call(element) == OPK_ERR_STATE, element
        assert "no collected batch" in L.opk_last_error().decode()
    # the element is checked against the pipeline's model (BODY_25) first
    assert call(55) == OPK_ERR_ARG
    assert "Neck-part distance channel only for BODY_25D." in L.opk_last_error().decode()
    pose.close()
