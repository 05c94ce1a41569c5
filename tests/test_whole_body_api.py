"""Argument and state errors of the whole-body entry points on a host-only context: attaching
face / hand extractors to a pose pipeline (opk_pose_attach_extractor) and the lazy heat-map copy
(opk_pose_heatmaps_copy_range).  No device is touched."""
import ctypes

import pytest

from openpose_amd import _lib
from openpose_amd.api import (CONNECT_GPU, FACE, HAND, Context, KeypointExtractor, Net,
                              PoseExtractor)

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 1, 3, 4
CAR_12 = 8


@pytest.fixture()
def host():
    ctx = Context.host_only()
    nets = {k: Net(ctx, k) for k in ("builtin:BODY_25", "builtin:FACE", "builtin:HAND")}
    yield ctx, nets
    for n in nets.values():
        n.close()
    ctx.close()


def _code(exc):
    return int(str(exc.value).split()[2].rstrip(":"))


def test_attach_errors(host):
    ctx, nets = host
    pose = PoseExtractor(ctx, nets["builtin:BODY_25"])
    face = KeypointExtractor(ctx, nets["builtin:FACE"], FACE, (176, 176))
    hand = KeypointExtractor(ctx, nets["builtin:HAND"], HAND, (176, 176))

    other = Context.host_only()
    other_net = Net(other, "builtin:FACE")
    foreign = KeypointExtractor(other, other_net, FACE, (176, 176))
    with pytest.raises(_lib.OpkError, match="share one context") as e:
        pose.attach(face=foreign)
    assert _code(e) == ERR_ARG

    own = KeypointExtractor(ctx, nets["builtin:BODY_25"], FACE, (176, 176))
    with pytest.raises(_lib.OpkError, match="must not be the pose net") as e:
        pose.attach(face=own)
    assert _code(e) == ERR_ARG

    car = PoseExtractor(ctx, None, pose_model=CAR_12, semantics=CONNECT_GPU)
    for kw in ({"face": face}, {"hands": hand}):
        with pytest.raises(_lib.OpkError) as e:
            car.attach(**kw)
        assert _code(e) == ERR_UNSUPPORTED

    # accessors: no such extractor attached, then attached but nothing collected
    for fn in (pose.face_rectangles, pose.face_keypoints, pose.hand_rectangles, pose.hand_keypoints):
        with pytest.raises(_lib.OpkError) as e:
            fn(0)
        assert _code(e) == ERR_STATE
    with pytest.raises(_lib.OpkError) as e:
        pose.read_part_times(FACE)
    assert _code(e) == ERR_STATE

    pose.attach(face=face, hands=hand)
    for fn in (pose.face_rectangles, pose.face_keypoints, pose.hand_rectangles, pose.hand_keypoints):
        with pytest.raises(_lib.OpkError) as e:
            fn(0)
        assert _code(e) == ERR_STATE
    assert pose.read_part_times(HAND) == {"batches": 0, "crops": 0, "host_ms": 0.0, "wait_ms": 0.0}

    face2 = KeypointExtractor(ctx, nets["builtin:FACE"], FACE, (176, 176))
    with pytest.raises(_lib.OpkError, match="already attached") as e:
        pose.attach(face=face2)
    assert _code(e) == ERR_STATE

    # every submit but the raw-frame one is refused, and says why
    L = pose.L
    assert L.opk_pose_submit(pose.h, None, 1, 176, 320, 640, 360) == ERR_STATE
    assert b"needs the frames" in L.opk_last_error()
    assert L.opk_pose_forward(pose.h, None, 1, 176, 320, 640, 360) == ERR_STATE
    assert L.opk_pose_submit_net_output(pose.h, None, 1, 22, 40, 176, 320, 640, 360) == ERR_STATE
    assert b"needs the frames" in L.opk_last_error()
    assert L.opk_pose_forward_multi(pose.h, None, None, 1, 1, 640, 360) == ERR_STATE

    # detached: the refusal is gone (the call now fails on its NULL frames, an argument error)
    pose.detach(FACE)
    assert L.opk_pose_submit(pose.h, None, 1, 176, 320, 640, 360) == ERR_STATE   # hands still on
    pose.detach(HAND)
    rc = L.opk_pose_submit_net_output(pose.h, None, 1, 22, 40, 176, 320, 640, 360)
    assert rc == ERR_ARG and b"needs the frames" not in L.opk_last_error()
    with pytest.raises(_lib.OpkError) as e:
        pose.detach(2)
    assert _code(e) == ERR_ARG

    for o in (face, hand, face2, own, foreign, car, pose):
        o.close()
    other_net.close()
    other.close()


def test_extractor_destroyed_while_attached_is_detached(host):
    ctx, nets = host
    pose = PoseExtractor(ctx, nets["builtin:BODY_25"])
    face = KeypointExtractor(ctx, nets["builtin:FACE"], FACE, (176, 176))
    pose.attach(face=face)
    L = pose.L
    assert L.opk_pose_submit_net_output(pose.h, None, 1, 22, 40, 176, 320, 640, 360) == ERR_STATE
    face.close()   # opk_extractor_destroy: the pipeline drops it
    rc = L.opk_pose_submit_net_output(pose.h, None, 1, 22, 40, 176, 320, 640, 360)
    assert rc == ERR_ARG and b"needs the frames" not in L.opk_last_error()
    with pytest.raises(_lib.OpkError, match="no such extractor") as e:
        pose.read_part_times(FACE)
    assert _code(e) == ERR_STATE
    again = KeypointExtractor(ctx, nets["builtin:FACE"], FACE, (176, 176))
    pose.attach(face=again)   # not "already attached"
    pose.detach(FACE)
    again.close()
    pose.close()


def test_heat_copy_range_argument_errors(host):
    import torch
    ctx, nets = host
    pose = PoseExtractor(ctx, None)
    shape = (ctypes.c_int * 4)()
    L = pose.L

    def call(types, mode, f0, nf, dst_type):
        return L.opk_pose_heatmaps_copy_range(pose.h, types, mode, f0, nf, None, dst_type, shape)

    for mode in (3, 5, 8, 0):   # uint8 (2) is for ScaleMode::UnsignedChar (7) only
        assert call(1, mode, 0, 1, 2) == ERR_ARG
        assert b"UnsignedChar" in L.opk_last_error()
    for types in (0, 8, -1):
        assert call(types, 8, 0, 1, 0) == ERR_ARG
        assert b"types" in L.opk_last_error()
    assert call(7, 8, 0, 1, 3) == ERR_ARG          # unknown destination type
    assert call(7, 9, 0, 1, 0) == ERR_ARG          # unknown ScaleMode
    for f0, nf in ((-1, 1), (0, 0), (0, -2), (-3, -1)):   # a range that no batch holds
        assert call(7, 7, f0, nf, 2) == ERR_ARG
        assert b"frame range" in L.opk_last_error()
    # well-formed, but nothing is collected: a state, as for the lazy map's other readers (the
    # range against a collected batch is checked on the GPU, tests/test_gpu_heat_copy_lazy.py)
    for f0, nf in ((0, 1), (0, -1), (5, 2)):
        assert call(7, 8, f0, nf, 0) == ERR_STATE
        assert b"no collected batch" in L.opk_last_error()
    with pytest.raises(_lib.OpkError, match="frame range"):
        pose.heatmaps_copy_range(7, 8, frames=(-1, 1))
    with pytest.raises(ValueError):
        pose.heatmaps_copy_range(7, 8, dtype=torch.float16)
    pose.close()
