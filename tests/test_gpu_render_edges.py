"""GPU: the keypoint renderers (kernels/render.hip: render_prep_kernel, render_keypoints_kernel and the
keypoint layers of render_frames_kernel) on the inputs of tests/render_edge_cases.py -- people off
the frame, straddling crowds, far / coincident / axis-parallel / non-finite geometry, scores on the
threshold, more than 256 hands or faces (the second round of the people compaction, up to the
1024-person limit) and frames smaller than one tile.

  1. the single-frame renderers against the CPU oracle (oracle/render.c, no tiles, no culling, no
     compaction): bit-equal on every pixel the oracle does not mark ambiguous, and on every pixel
     where it marks none;
  2. the fused batch render: byte for byte the unfused chain, and the CPU chain on unambiguous
     pixels;
  3. the people limits on both paths;
  4. tiny frames through the fused path, into padded rows."""
import numpy as np
import pytest
import torch

from openpose_amd import _lib
from openpose_amd.api import CAST_CPU, CAST_CUDA, LAYER_FACE, LAYER_HAND, LAYER_POSE, RenderLayer
from tests import render_edge_cases as rc
from tests.test_gpu_output_frames import _chain, _dev_layers, _frames, _oracle_chain
from tests.test_render import _check_keypoints, people_on

pytestmark = pytest.mark.gpu


def _render(ctx, frame, kind, kp, opts, blend=True):
    """One single-frame render of a case's kind on a copy of frame (numpy in, numpy out)."""
    f = torch.from_numpy(frame).cuda()
    k = torch.from_numpy(kp).cuda()
    if kind == LAYER_POSE:
        ctx.render_pose_keypoints(f, k, 0, threshold=rc.THRESHOLD[kind],
                                  googly_eyes=bool(opts.get("googly")), blend_original=blend,
                                  alpha=rc.ALPHA)
    elif kind == LAYER_FACE:
        ctx.render_face_keypoints(f, k, threshold=rc.THRESHOLD[kind], alpha=rc.ALPHA)
    else:
        ctx.render_hand_keypoints(f, k, threshold=rc.THRESHOLD[kind], alpha=rc.ALPHA)
    ctx.sync()
    return f.cpu().numpy()


# ---- 1. the single-frame path --------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.CASES)
def test_single_frame_matches_oracle(ctx, name):
    _, kind, kp, opts = rc.case(name)
    frame = rc.frame_of(name)
    for blend in (True, False) if kind == LAYER_POSE else (True,):
        want, amb = rc.oracle_render(name, blend)
        got = _render(ctx, frame, kind, kp, opts, blend)
        print("%s, blend %d:" % (name, blend), end=" ")
        _check_keypoints(got, want, amb)
        if name in rc.EXACT:
            assert not amb.any()
            np.testing.assert_array_equal(got, want)
        if name in ("ties-at", "far"):   # nothing above the threshold / nobody near the frame
            np.testing.assert_array_equal(got, frame if blend else np.zeros_like(frame))
        elif blend:
            assert np.any(got != frame)


# ---- 2. the fused batch path ---------------------------------------------------------------------
def _batch(name):
    """(frames uint8 [n, h, w, 3], layers (kind, keypoints, counts, googly), blend, empty frames)"""
    kp = lambda case: rc.case(case)[2]
    if name == "hands-then-crowd":   # 300 hands in frame 0, the straddling crowd in frame 2
        layers = [(LAYER_HAND, kp("hands300"), [300, 0, 0], False),
                  (LAYER_POSE, kp("straddle"), [0, 0, 40], True)]
        return _frames(3, 240, 320, 21), layers, True, [1]
    if name == "pose-edges":         # the frame is cleared: no blending
        layers = [(LAYER_POSE, np.concatenate([kp("nonfinite"), kp("left"), kp("coincident-on"),
                                               kp("coincident-off")]), [40, 1, 2], True)]
        return _frames(3, 240, 320, 22), layers, False, []
    if name == "three-layers":
        layers = [(LAYER_POSE, kp("straddle"), [40], True), (LAYER_FACE, kp("faces300"), [300], False),
                  (LAYER_HAND, kp("hands300"), [300], False)]
        return _frames(1, 240, 320, 23), layers, True, []
    if name == "hands1024":          # the limit, next to a frame with nobody
        w, h = rc.CROWD_SIZE
        return (_frames(2, h, w, 24), [(LAYER_HAND, kp("hands1024"), [0, 1024], False)], True, [0])
    w, h = rc.TINY[name]
    return (_frames(2, h, w, 25), [(LAYER_POSE, kp(name), [2, 0], False)], True, [1])


def _check_batch(ctx, name, cast, pad=0):
    frames, layers, blend, empty = _batch(name)
    n, h, w, _ = frames.shape
    fd = torch.from_numpy(frames).cuda()
    dl = _dev_layers(layers)

    def dst():
        return torch.full((n, h, w * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda") if pad else None

    got = ctx.render_frames(fd, dl, 1.0, (w, h), blend_original=blend, cast=cast, out=dst())
    chain = _chain(ctx, fd, dl, 1.0, (w, h), blend, cast, out=dst())
    plain = ctx.output_to_cvmat(ctx.cvmat_to_output(fd, 1.0, (w, h)), cast)
    ctx.sync()
    got, chain, plain = got.cpu().numpy(), chain.cpu().numpy(), plain.cpu().numpy()
    np.testing.assert_array_equal(got, chain)
    if pad:
        assert (got[:, :, w * 3:] == 0xA5).all()       # the rows' padding keeps its sentinel
        got = got[:, :, :w * 3].reshape(n, h, w, 3)
    want, amb = _oracle_chain(frames, layers, 1.0, (w, h), blend, cast)
    diff = np.any(got != want, axis=3)
    print("%s, cast %d, pad %d: %d px, %d ambiguous (%.3f %%), %d of them differ" % (
        name, cast, pad, amb.size, int(amb.sum()), 100.0 * amb.mean(),
        int((diff & (amb != 0)).sum())))
    bad = diff & (amb == 0)
    assert not bad.any(), "%d unambiguous pixels differ, first %s" % (bad.sum(), np.argwhere(bad)[:5])
    assert amb.mean() <= 0.01
    for f in range(n):
        if f in empty:     # nobody in this frame: its warp + cast alone
            np.testing.assert_array_equal(got[f], plain[f])
        else:
            assert np.any(got[f] != plain[f])
    return got, want, amb


@pytest.mark.parametrize("cast", [CAST_CPU, CAST_CUDA])
def test_batch_hands_then_crowd(ctx, cast):
    _check_batch(ctx, "hands-then-crowd", cast)


def test_batch_pose_edges(ctx):
    got, _, _ = _check_batch(ctx, "pose-edges", CAST_CUDA)
    # `left` on a cleared frame: column 0 only
    assert got[1, :, 0].any() and not got[1, :, 1:].any()


def test_batch_three_layers(ctx):
    _check_batch(ctx, "three-layers", CAST_CPU)


# ---- 3. the limits -------------------------------------------------------------------------------
def test_batch_1024_hands(ctx):
    _check_batch(ctx, "hands1024", CAST_CPU)


def test_people_limits(ctx):
    w, h = rc.CROWD_SIZE
    frame = rc.frame_of("hands1024")
    frames = torch.from_numpy(_frames(1, h, w, 26)).cuda()
    for kind, render in ((LAYER_HAND, ctx.render_hand_keypoints), (LAYER_FACE, ctx.render_face_keypoints)):
        kp = torch.from_numpy(rc.crowd(kind, 1025, 50, 1)[2]).cuda()
        f = torch.from_numpy(frame).cuda()
        with pytest.raises(_lib.OpkError, match="opk error 1: .*at most 1024 people"):
            render(f, kp)
        with pytest.raises(_lib.OpkError, match="opk error 1: .*at most 1024 people"):
            ctx.render_frames(frames, [RenderLayer(kind, kp, [1025])])
        ctx.sync()
        np.testing.assert_array_equal(f.cpu().numpy(), frame)      # refused before any drawing
    kp = torch.from_numpy(people_on(w, h, 128, 25, seed=51)).cuda()
    f = torch.from_numpy(frame).cuda()
    with pytest.raises(_lib.OpkError, match="opk error 1: .*POSE_MAX_PEOPLE = 127"):
        ctx.render_pose_keypoints(f, kp, 0)
    with pytest.raises(_lib.OpkError, match="opk error 1: .*POSE_MAX_PEOPLE = 127"):
        ctx.render_frames(frames, [RenderLayer(LAYER_POSE, kp, [128])])
    ctx.sync()
    np.testing.assert_array_equal(f.cpu().numpy(), frame)


# ---- 4. frames smaller than one tile -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.TINY))
def test_batch_tiny_frames(ctx, name):
    w = rc.TINY[name][0]
    aligned = (-w * 3) % 4 + 4         # rows on 4-byte boundaries: the tile leaves through LDS
    for cast, pad in ((CAST_CPU, 0), (CAST_CPU, aligned), (CAST_CUDA, aligned + 1)):
        got, want, amb = _check_batch(ctx, name, cast, pad)
        assert not amb.any()
        np.testing.assert_array_equal(got, want)
