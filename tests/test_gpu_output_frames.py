"""GPU: the output image stages and the fused batch render (kernels/render.hip).

  1. cvmat_to_output is CvMatToOpOutput's CPU branch bit for bit (oracle.cvmat_to_input with
     normalize 0 is the same cv::warpAffine, in CHW);
  2. output_to_cvmat is the numpy restatement of OpOutputToCvMat's two casts
     (tests/test_output_frames.py);
  3. render_frames is, byte for byte and on every pixel, the unfused chain cvmat_to_output ->
     render_*_keypoints per frame and layer -> output_to_cvmat (both run the same device arithmetic);
  4. render_frames against the CPU oracle chain, on every pixel that no layer's ambiguity mask marks
     (limb-ellipse boundaries, as tests/test_render.py); the marked share is capped at 1 %;
  5. PoseExtractor.render_frames draws the collected batch;
  6. one call over 130 frames (the grid's z dimension, prefix offsets past one wave of frames)."""
import numpy as np
import pytest
import torch

import oracle
from openpose_amd import _lib, synth
from openpose_amd.api import (CAST_CPU, CAST_CUDA, LAYER_FACE, LAYER_HAND, LAYER_POSE,
                              PoseExtractor, RenderLayer)
from tests.test_output_frames import cast_restated, KNOWN
from tests.test_render import people_on

pytestmark = pytest.mark.gpu

PARTS = {LAYER_POSE: 25, LAYER_FACE: 70, LAYER_HAND: 21}
# oracle.render_keypoints arguments of each layer kind (renderPose.cu / renderFace.cu / renderHand.cu)
ORACLE = {LAYER_POSE: dict(table="BODY_25", radius_div=100.0, line_div=120.0),
          LAYER_FACE: dict(table="FACE", radius_div=120.0, line_div=250.0),
          LAYER_HAND: dict(table="HAND", radius_div=100.0, line_div=80.0)}
SPREAD = {LAYER_POSE: 0.15, LAYER_FACE: 0.08, LAYER_HAND: 0.06}


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _layer_np(kind, counts, ow, oh, seed, googly=False):
    """(kind, keypoints [sum(counts), parts, 3] in output pixels, counts, googly)"""
    kp = [people_on(ow, oh, c, PARTS[kind], seed=seed + 17 * f, spread=SPREAD[kind])
          for f, c in enumerate(counts)]
    return kind, np.concatenate(kp).astype(np.float32), list(counts), googly


def _dev_layers(layers):
    out = []
    for kind, kp, counts, googly in layers:
        out.append(RenderLayer(kind, torch.from_numpy(kp).cuda() if len(kp) else None, counts,
                               googly_eyes=googly))
    return out


def _chain(ctx, frames, layers, scale, out_size, blend, cast, out=None):
    """The unfused chain on the device."""
    img = ctx.cvmat_to_output(frames, scale, out_size)
    for f in range(frames.shape[0]):
        for i, l in enumerate(layers):
            c0 = sum(l.counts[:f])
            kp = l.keypoints[c0:c0 + l.counts[f]] if l.counts[f] else None
            if l.kind == LAYER_POSE:
                ctx.render_pose_keypoints(img[f], kp, l.pose_model, threshold=l.threshold,
                                          googly_eyes=l.googly_eyes,
                                          blend_original=blend or i > 0, alpha=l.alpha)
            elif kp is not None and l.kind == LAYER_FACE:
                ctx.render_face_keypoints(img[f], kp, threshold=l.threshold, alpha=l.alpha)
            elif kp is not None:
                ctx.render_hand_keypoints(img[f], kp, threshold=l.threshold, alpha=l.alpha)
    return ctx.output_to_cvmat(img, cast, out=out)


def _oracle_chain(frames, layers, scale, out_size, blend, cast):
    """The CPU chain: (uint8 [n, oh, ow, 3], ambiguous [n, oh, ow])."""
    ow, oh = out_size
    outs, ambs = [], []
    for f in range(frames.shape[0]):
        img = oracle.cvmat_to_input(frames[f], scale, ow, oh, normalize=0).transpose(1, 2, 0)
        img = np.ascontiguousarray(img)
        amb = np.zeros((oh, ow), np.uint8)
        for i, (kind, kp, counts, googly) in enumerate(layers):
            c0 = sum(counts[:f])
            if kind != LAYER_POSE and counts[f] == 0:
                continue   # renderFace / renderHand return at once
            if kind == LAYER_POSE and counts[f] == 0 and (blend or i > 0):
                continue   # renderPose.cu:616
            th = {LAYER_POSE: 0.05, LAYER_FACE: 0.4, LAYER_HAND: 0.2}[kind]
            img, a = oracle.render_keypoints(img, kp[c0:c0 + counts[f]], parts=PARTS[kind],
                                             threshold=th, alpha=0.6, blend=blend or i > 0,
                                             eyes=(15, 16) if googly else (-1, -1), **ORACLE[kind])
            amb |= a
        outs.append(cast_restated(img, cast))
        ambs.append(amb)
    return np.stack(outs), np.stack(ambs)


# ---- 1. cvmat_to_output --------------------------------------------------------------------------
@pytest.mark.parametrize("scale,ow,oh,pad", [(1.0, 97, 61, 0), (1.0, 120, 70, 0), (0.5, 49, 31, 0),
                                             (0.5, 64, 40, 0), (1.7, 165, 104, 0),
                                             (0.5, 49, 31, 5)])
def test_cvmat_to_output_bitexact(ctx, scale, ow, oh, pad):
    n, h, w = 2, 61, 97
    frames = _frames(n, h, w, 3)
    if pad:   # rows of width*3 + 5 bytes
        rows = np.full((n, h, w * 3 + pad), 0xEE, np.uint8)
        rows[:, :, :w * 3] = frames.reshape(n, h, w * 3)
        dev = torch.from_numpy(rows).cuda()
        out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device="cuda")
        _lib.check(ctx.L.opk_cvmat_to_output(ctx.h, out.data_ptr(), dev.data_ptr(), n, w, h,
                                             w * 3 + pad, scale, ow, oh))
    else:
        out = ctx.cvmat_to_output(torch.from_numpy(frames).cuda(), scale, (ow, oh))
    ctx.sync()
    got = out.cpu().numpy()
    for f in range(n):
        want = oracle.cvmat_to_input(frames[f], scale, ow, oh, normalize=0).transpose(1, 2, 0)
        np.testing.assert_array_equal(got[f], want)
    if scale == 1.0 and (ow, oh) == (w, h):
        np.testing.assert_array_equal(got, frames.astype(np.float32))


# ---- 2. output_to_cvmat --------------------------------------------------------------------------
def _cast_inputs():
    rng = np.random.default_rng(5)
    a = rng.uniform(-20, 280, (2, 9, 33, 3)).astype(np.float32)
    flat = a.reshape(-1)
    known = np.float32([v for _, v, _ in KNOWN])
    flat[:len(known)] = known
    halves = np.arange(256, dtype=np.float32) + np.float32(0.5)
    flat[100:100 + 256] = halves
    flat[-256:] = halves      # and in the second image, last rows
    return a


@pytest.mark.parametrize("cast", [CAST_CPU, CAST_CUDA])
@pytest.mark.parametrize("w,pad", [(33, 0), (33, 7), (32, 0), (32, 4), (32, 7)])
def test_output_to_cvmat_matches_restatement(ctx, cast, w, pad):
    """w 33: rows of 99 values, the one-value path; w 32 with 4-byte-aligned rows: four values per
    thread.  Padding bytes keep their 0xA5."""
    a = np.ascontiguousarray(_cast_inputs()[:, :, :w])
    n, h = a.shape[:2]
    dst = torch.full((n, h, w * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.output_to_cvmat(torch.from_numpy(a).cuda(), cast, out=dst)
    ctx.sync()
    got = dst.cpu().numpy()
    np.testing.assert_array_equal(got[:, :, :w * 3].reshape(a.shape), cast_restated(a, cast))
    assert (got[:, :, w * 3:] == 0xA5).all()
    if w == 33 and pad == 0:   # the known answers themselves
        flat = got.reshape(-1)
        for i, (c, _, want) in enumerate(KNOWN):
            if c == cast:
                assert int(flat[i]) == want


# ---- 3. render_frames == the unfused chain, every byte -------------------------------------------
def _case(name):
    """(frame size, out size, scale, layers, blend, cast, dst padding)"""
    P, F, H = LAYER_POSE, LAYER_FACE, LAYER_HAND
    cases = {
        "tile+1": ((33, 9), (33, 9), 1.0, [(P, (1,), 21, False)], True, CAST_CPU, 0),
        "two-rounds": ((161, 67), (161, 67), 1.0, [(P, (7, 0, 2), 33, False)], True, CAST_CPU, 0),
        "clear-cuda": ((161, 67), (161, 67), 1.0, [(P, (7, 0, 2), 33, False)], False, CAST_CUDA, 0),
        "half": ((160, 120), (80, 60), 0.5, [(P, (3, 2), 41, False)], True, CAST_CPU, 0),
        "cubic": ((160, 120), (272, 204), 1.7, [(P, (3, 2), 43, False)], True, CAST_CPU, 0),
        "three-layers": ((200, 150), (200, 150), 1.0,
                         [(P, (3, 1), 51, False), (F, (2, 0), 52, False), (H, (4, 2), 53, False)],
                         True, CAST_CPU, 0),
        "googly": ((161, 67), (161, 67), 1.0, [(P, (7, 0, 2), 33, True)], True, CAST_CUDA, 0),
        "padded": ((161, 67), (161, 67), 1.0, [(P, (7, 0, 2), 33, False)], True, CAST_CPU, 9),
        "no-layers": ((160, 120), (80, 60), 0.5, [], True, CAST_CUDA, 0),
    }
    size, out, scale, ls, blend, cast, pad = cases[name]
    n = len(ls[0][1]) if ls else 2
    layers = [_layer_np(kind, counts, out[0], out[1], seed, googly)
              for kind, counts, seed, googly in ls]
    return _frames(n, size[1], size[0], 7), out, scale, layers, blend, cast, pad


@pytest.mark.parametrize("name", ["tile+1", "two-rounds", "clear-cuda", "half", "cubic",
                                  "three-layers", "googly", "padded", "no-layers"])
def test_render_frames_equals_unfused_chain(ctx, name):
    frames, (ow, oh), scale, layers, blend, cast, pad = _case(name)
    n = frames.shape[0]
    fd = torch.from_numpy(frames).cuda()
    dl = _dev_layers(layers)

    def dst():
        return torch.full((n, oh, ow * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda") if pad else None

    got = ctx.render_frames(fd, dl, scale, (ow, oh), blend_original=blend, cast=cast, out=dst())
    want = _chain(ctx, fd, dl, scale, (ow, oh), blend, cast, out=dst())
    ctx.sync()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    if pad:
        assert (got[:, :, ow * 3:] == 0xA5).all()
        got = got[:, :, :ow * 3].reshape(n, oh, ow, 3)
    plain = ctx.output_to_cvmat(ctx.cvmat_to_output(fd, scale, (ow, oh)), cast).cpu().numpy()
    if layers and blend:
        assert (got != plain).any()          # something was drawn
    if not layers:
        np.testing.assert_array_equal(got, plain)
    if name in ("two-rounds", "padded"):     # nobody in the middle frame: its warp + cast alone
        np.testing.assert_array_equal(got[1], plain[1])
    if name == "clear-cuda":
        assert not got[1].any()


# ---- 4. render_frames against the CPU oracle -----------------------------------------------------
@pytest.mark.parametrize("name", ["two-rounds", "three-layers"])
def test_render_frames_matches_oracle(ctx, name):
    frames, (ow, oh), scale, layers, blend, cast, _ = _case(name)
    want, amb = _oracle_chain(frames, layers, scale, (ow, oh), blend, cast)
    got = ctx.render_frames(torch.from_numpy(frames).cuda(), _dev_layers(layers), scale, (ow, oh),
                            blend_original=blend, cast=cast)
    ctx.sync()
    got = got.cpu().numpy()
    diff = np.any(got != want, axis=3)
    print("%s: %d px, %d ambiguous (%.3f %%), %d of them differ" % (
        name, amb.size, int(amb.sum()), 100.0 * amb.mean(), int((diff & (amb != 0)).sum())))
    bad = diff & (amb == 0)
    assert not bad.any(), "%d unambiguous pixels differ, first %s" % (bad.sum(), np.argwhere(bad)[:5])
    assert amb.mean() <= 0.01


# ---- 5. the pipeline's collected batch -----------------------------------------------------------
def test_pose_render_frames(ctx):
    fields = np.stack([synth.overlay(k + 2, 46, 82, seed=600 + k) for k in range(2)]).astype(np.float32)
    pose = PoseExtractor(ctx, None)
    net_out = torch.from_numpy(fields).cuda()
    pose.forward_net_output(net_out, (656, 368), (1280, 720))
    kps = [pose.keypoints(f)[0] for f in range(2)]
    counts = [len(k) for k in kps]
    assert sum(counts) >= 1
    frames = torch.from_numpy(_frames(2, 720, 1280, 9)).cuda()
    got = pose.render_frames(frames)
    packed = torch.from_numpy(np.concatenate(kps).astype(np.float32)).cuda()
    want = ctx.render_frames(frames, [RenderLayer(LAYER_POSE, packed, counts)])
    ctx.sync()
    assert torch.equal(got, want)
    assert not torch.equal(got, frames)
    three = torch.zeros((3, 720, 1280, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.OpkError, match="opk error 3: .*2 frames, not 3"):
        pose.render_frames(three)
    pose.close()


# ---- 6. a large batch ----------------------------------------------------------------------------
def test_render_frames_130_frames(ctx):
    n, w, h = 130, 64, 48
    frames = torch.from_numpy(_frames(n, h, w, 11)).cuda()
    layers = _dev_layers([_layer_np(LAYER_POSE, (1,) * n, w, h, 71)])
    got = ctx.render_frames(frames, layers)
    want = _chain(ctx, frames, layers, 1.0, (w, h), True, CAST_CPU)
    ctx.sync()
    assert torch.equal(got, want)
    assert not torch.equal(got, frames)
    # every frame has its own person: frame f differs from the undrawn frame f
    changed = (got != frames).reshape(n, -1).any(dim=1)
    assert bool(changed.all())
