"""GPU: the pointer-taking entry points, called through the C ABI directly.

The Python methods describe every tensor as a Frames and call the `_fmt` forms, so nothing in
openpose_amd/api.py reaches opk_cvmat_to_input, opk_cvmat_to_output, opk_render_frames,
opk_render_frames_heat or the three pointer-taking opk_pose_render_frames* any more.  integration/
and C callers do: each is called once here on 2 frames of 34 x 18 (no multiple of a tile, a piece
or a vector) and must give the bytes of the Python method.  The pose forms draw the collected batch
of a pipeline without a CNN (an injected net output with three people, 96 x 64); with no extractor
attached the parts form draws the keypoints alone.
"""
import ctypes

import numpy as np
import pytest
import torch

from openpose_amd import _lib, synth
from openpose_amd.api import (CAST_CPU, HEAT_PART, LAYER_POSE, PoseExtractor, RenderHeat, RenderLayer,
                              _ptr, check)

pytestmark = pytest.mark.gpu

N, H, W = 2, 18, 34


@pytest.fixture(scope="module")
def frames():
    g = np.random.default_rng(34)
    return torch.from_numpy(g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)).cuda()


def test_cvmat_to_input(ctx, frames):
    want = torch.empty((N, 3, 12, 20), device="cuda")
    ctx.cvmat_to_input(want, frames, 0.55)
    got = torch.full_like(want, float("nan"))
    check(ctx.L.opk_cvmat_to_input(ctx.h, _ptr(got), _ptr(frames), N, W, H, W * 3, 0.55, 20, 12, 1))
    ctx.sync()
    assert torch.equal(got, want)


def test_cvmat_to_output(ctx, frames):
    want = ctx.cvmat_to_output(frames, 1.5, (51, 27))
    got = torch.full_like(want, float("nan"))
    check(ctx.L.opk_cvmat_to_output(ctx.h, _ptr(got), _ptr(frames), N, W, H, W * 3, 1.5, 51, 27))
    ctx.sync()
    assert torch.equal(got, want)


def _pose_layer():
    g = np.random.default_rng(35)
    kp = np.empty((2 * N, 25, 3), np.float32)
    kp[..., 0] = g.uniform(0, W, kp.shape[:2])
    kp[..., 1] = g.uniform(0, H, kp.shape[:2])
    kp[..., 2] = 1.0
    dev = torch.from_numpy(kp).cuda()
    arr = (_lib.RenderLayerStruct * 1)()
    counts = (ctypes.c_int * N)(2, 2)
    arr[0].kind, arr[0].pose_model = LAYER_POSE, 0
    arr[0].keypoints_dev, arr[0].counts_host = _ptr(dev), counts
    arr[0].render_threshold, arr[0].alpha, arr[0].googly_eyes = 0.05, 0.6, 0
    return RenderLayer(LAYER_POSE, dev, [2, 2]), arr, counts


def test_render_frames(ctx, frames):
    layer, arr, _counts = _pose_layer()
    want = ctx.render_frames(frames, [layer])
    assert not torch.equal(want, frames)
    got = torch.zeros_like(want)
    check(ctx.L.opk_render_frames(ctx.h, _ptr(got), W * 3, W, H, _ptr(frames), N, W, H, W * 3, 1.0,
                                  arr, 1, 1, CAST_CPU))
    ctx.sync()
    assert torch.equal(got, want)


def test_render_frames_heat(ctx, frames):
    layer, arr, _counts = _pose_layer()
    g = np.random.default_rng(36)
    stack = torch.from_numpy(g.uniform(-1.0, 1.2, (N, 3, 9, 17)).astype(np.float32)).cuda()
    heat = RenderHeat(HEAT_PART, stack, 2.0, 1)
    want = ctx.render_frames(frames, [layer], heat=heat)
    assert not torch.equal(want, ctx.render_frames(frames, [layer]))
    hs = ctx._heat_struct(heat, N)
    got = torch.zeros_like(want)
    check(ctx.L.opk_render_frames_heat(ctx.h, _ptr(got), W * 3, W, H, _ptr(frames), N, W, H, W * 3,
                                       1.0, arr, 1, 1, CAST_CPU, ctypes.byref(hs)))
    ctx.sync()
    assert torch.equal(got, want)


def test_pose_render_frames(ctx):
    """opk_pose_render_frames, _element and _parts on the frames of the collected batch."""
    pw, ph = 96, 64
    fields = np.stack([synth.overlay(3, 8, 12, seed=1 + f) for f in range(N)]).astype(np.float32)
    pose = PoseExtractor(ctx, None)
    pose.forward_net_output(torch.from_numpy(fields).cuda(), (pw, ph), (pw, ph))
    assert sum(pose.num_people(f) for f in range(N)) >= 2
    g = np.random.default_rng(37)
    img = torch.from_numpy(g.integers(0, 256, (N, ph, pw, 3), dtype=np.uint8)).cuda()
    head = lambda out: (pose.h, _ptr(out), pw * 3, pw, ph, _ptr(img), N, pw, ph, pw * 3, 1.0)
    want = pose.render_frames(img)
    assert not torch.equal(want, img)
    got = torch.zeros_like(want)
    check(pose.L.opk_pose_render_frames(*head(got), 0.05, 0.6, 0, 1, CAST_CPU))
    ctx.sync()
    assert torch.equal(got, want)
    got = torch.zeros_like(want)
    check(pose.L.opk_pose_render_frames_parts(*head(got), 0.05, 0.6, 0, 1, CAST_CPU, 0.4, 0.6, 0.2, 0.6))
    ctx.sync()
    assert torch.equal(got, want)
    want = pose.render_frames(img, element=4)
    assert not torch.equal(want, img) and not torch.equal(want, got)
    got = torch.zeros_like(want)
    check(pose.L.opk_pose_render_frames_element(*head(got), 4, 0.05, 0.6, 0.7, 0, 1, CAST_CPU))
    ctx.sync()
    assert torch.equal(got, want)
    pose.close()
