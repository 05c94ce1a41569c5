"""GPU: the heat layer of the fused batch render (kernels/render.hip, opk_render_frames_heat and
opk_pose_render_frames_element).

Every comparison is byte for byte on every pixel against the chain of the per-frame entry points:
cvmat_to_output -> render_heat_map / render_heat_maps / render_pafs per frame (-> the keypoint
renders per frame) -> output_to_cvmat.  Both run the same device arithmetic, the fused call on heat
values staged in LDS or evaluated per pixel, from a materialised stack or lazily from a net output.

The generic cases use stacks of 35 channels, not 30: no model's PAFs fit 30 (the smallest, CAR_12,
has 12 parts + background + 22 PAF channels = 35), and the all-PAFs kind needs one that does."""
import numpy as np
import pytest
import torch

from openpose_amd import _lib, synth
from openpose_amd.api import (CAST_CPU, CAST_CUDA, HEAT_DISTANCE, HEAT_PAF, HEAT_PAFS, HEAT_PART,
                              HEAT_PARTS, LAYER_FACE, LAYER_HAND, MAPS_CPU, MAPS_CUDA, PoseExtractor,
                              RenderHeat, render_element)
from tests.test_gpu_output_frames import _dev_layers, _frames, _layer_np

pytestmark = pytest.mark.gpu

BODY_25, CAR_12 = 0, 8
CHANNELS = 35
# kind -> (pose model, channel): BODY_25 draws 25 parts (its 18 colors wrap); CAR_12's 11 PAFs are
# channels 13 .. 34; the single channels are the stack's last and an inner one
KINDS = {"part": (HEAT_PART, BODY_25, 34), "parts": (HEAT_PARTS, BODY_25, 0),
         "paf": (HEAT_PAF, BODY_25, 33), "pafs": (HEAT_PAFS, CAR_12, 0),
         "distance": (HEAT_DISTANCE, BODY_25, 7)}
# name -> (frame size, out size, warp scale, heat size, scale_to_keep_ratio, cast, dst padding)
#   overflow: heat 40x25 at 2.3 on 97x61 -- columns >= 93 truncate to x = width and rows >= 59 to
#             y = height (the all-parts flat index steps into the next row / plane); the plain copy;
#             rows of 97 * 3 + 6 = 297 bytes, no multiple of 4 (byte stores)
#   small:    33x9, one tile wide plus one pixel, one row more than a tile; the linear warp
#   perpixel: heat 200x130 at 0.2 -- a tile spans 160x40 heat pixels, no window fits the LDS;
#             the cubic warp
SETUPS = {"overflow": ((97, 61), (97, 61), 1.0, (40, 25), 2.3, CAST_CPU, 6),
          "small": ((66, 18), (33, 9), 0.5, (40, 25), 2.3, CAST_CUDA, 0),
          "perpixel": ((57, 36), (97, 61), 1.7, (200, 130), 0.2, CAST_CPU, 0)}


def _stack(n, size, seed, channels=CHANNELS):
    """n different stacks: values past both ends of [0, 1] (saturation, the color map's clamps) and
    of either sign (PAF directions, |distance|)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.2, 1.3, (n, channels, size[1], size[0])).astype(np.float32)


def _heat_chain(ctx, frames, heat, layers, scale, out_size, cast, out=None):
    """The unfused chain: warp, the heat render of each frame, the keypoint layers, cast."""
    img = ctx.cvmat_to_output(frames, scale, out_size)
    for f in range(frames.shape[0]):
        h = heat.heat[f]
        if heat.kind == HEAT_PART:
            ctx.render_heat_map(img[f], h, heat.scale, heat.channel, heat.alpha)
        elif heat.kind == HEAT_DISTANCE:
            ctx.render_heat_map(img[f], h, heat.scale, heat.channel, heat.alpha, distance=True)
        elif heat.kind == HEAT_PARTS:
            ctx.render_heat_maps(img[f], h, heat.scale, heat.pose_model, heat.alpha)
        elif heat.kind == HEAT_PAF:
            ctx.render_pafs(img[f], h, heat.scale, heat.channel, heat.pose_model, heat.alpha)
        else:
            ctx.render_pafs(img[f], h, heat.scale, None, heat.pose_model, heat.alpha)
    if layers:   # the keypoint chain of tests/test_gpu_output_frames.py on the drawn frames
        from openpose_amd.api import LAYER_POSE
        for f in range(frames.shape[0]):
            for l in layers:
                c0 = sum(l.counts[:f])
                kp = l.keypoints[c0:c0 + l.counts[f]] if l.counts[f] else None
                if l.kind == LAYER_POSE:
                    ctx.render_pose_keypoints(img[f], kp, l.pose_model, threshold=l.threshold,
                                              googly_eyes=l.googly_eyes, blend_original=True,
                                              alpha=l.alpha)
                elif kp is not None and l.kind == LAYER_FACE:
                    ctx.render_face_keypoints(img[f], kp, threshold=l.threshold, alpha=l.alpha)
                elif kp is not None:
                    ctx.render_hand_keypoints(img[f], kp, threshold=l.threshold, alpha=l.alpha)
    return ctx.output_to_cvmat(img, cast, out=out)


def _compare(ctx, frames, heat, layers, scale, out_size, cast, pad=0):
    n = frames.shape[0]
    ow, oh = out_size

    def dst():
        return torch.full((n, oh, ow * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda") if pad else None

    got = ctx.render_frames(frames, layers, scale, out_size, cast=cast, out=dst(), heat=heat)
    want = _heat_chain(ctx, frames, heat, layers, scale, out_size, cast, out=dst())
    ctx.sync()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    if pad:
        assert (got[:, :, ow * 3:] == 0xA5).all()
        got = got[:, :, :ow * 3].reshape(n, oh, ow, 3)
    return got


@pytest.fixture(scope="module")
def stacks():
    """The heat stacks of the generic cases, on the device: made once, never written."""
    return {size: torch.from_numpy(_stack(3, size, 31 + size[0])).cuda()
            for size in {s[3] for s in SETUPS.values()}}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("setup", list(SETUPS))
def test_heat_layer_equals_unfused_chain(ctx, stacks, setup, kind):
    size, out, scale, hsize, ratio, cast, pad = SETUPS[setup]
    k, model, channel = KINDS[kind]
    frames = torch.from_numpy(_frames(3, size[1], size[0], 7)).cuda()
    heat = RenderHeat(k, stacks[hsize], ratio, channel, alpha=0.7, pose_model=model)
    got = _compare(ctx, frames, heat, [], scale, out, cast, pad)
    plain = ctx.output_to_cvmat(ctx.cvmat_to_output(frames, scale, out), cast).cpu().numpy()
    assert (got != plain).any()                 # something was drawn


def test_heat_layer_alpha_one_and_zero(ctx, stacks):
    """alpha 1 replaces the frame (the reference's "no blending"), alpha 0 leaves the warp + cast."""
    size, out, scale, hsize, ratio, cast, _ = SETUPS["overflow"]
    frames = torch.from_numpy(_frames(3, size[1], size[0], 7)).cuda()
    for alpha in (1.0, 0.0):
        got = _compare(ctx, frames, RenderHeat(HEAT_PARTS, stacks[hsize], ratio, alpha=alpha), [],
                       scale, out, cast)
        if alpha == 0.0:
            np.testing.assert_array_equal(got, frames.cpu().numpy())


def test_heat_layer_then_keypoint_layers(ctx, stacks):
    """A face layer and a hand layer drawn after the heat layer."""
    out = (97, 61)
    frames = torch.from_numpy(_frames(3, out[1], out[0], 7)).cuda()
    layers = _dev_layers([_layer_np(LAYER_FACE, (2, 0, 1), out[0], out[1], 52),
                          _layer_np(LAYER_HAND, (1, 2, 0), out[0], out[1], 53)])
    heat = RenderHeat(HEAT_PART, stacks[(40, 25)], 2.3, 3)
    got = _compare(ctx, frames, heat, layers, 1.0, out, CAST_CPU)
    alone = ctx.render_frames(frames, [], heat=heat).cpu().numpy()
    assert (got != alone).any()                 # the keypoints are on top


def test_distance_channel_of_body_25d(ctx):
    """BODY_25D's first and last neck-part distance elements through the generic call: a stack of
    126 channels (26 + 52 + 48), frames of different sign patterns."""
    out, hsize = (97, 61), (24, 15)
    frames = torch.from_numpy(_frames(2, out[1], out[0], 13)).cuda()
    stack = torch.from_numpy(_stack(2, hsize, 77, channels=126)).cuda()
    for element in (55, 102):
        kind, channel = render_element(9, element)
        assert kind == HEAT_DISTANCE
        heat = RenderHeat(kind, stack, 4.0, channel, pose_model=9)
        got = _compare(ctx, frames, heat, [], 1.0, out, CAST_CPU)
        # |value|: not the part render where the interpolated value is negative
        part = ctx.render_frames(frames, [], heat=RenderHeat(HEAT_PART, stack, 4.0, channel))
        assert (got != part.cpu().numpy()).any()


def test_heat_layer_130_frames(ctx):
    """One call over 130 frames: the grid's z dimension, frame f's own planes."""
    n, w, h = 130, 64, 48
    frames = torch.from_numpy(_frames(n, h, w, 11)).cuda()
    stack = torch.from_numpy(_stack(n, (20, 15), 5, channels=4)).cuda()
    for heat in (RenderHeat(HEAT_PART, stack, 3.2, 3), RenderHeat(HEAT_PAF, stack, 3.2, 2)):
        _compare(ctx, frames, heat, [], 1.0, (w, h), CAST_CPU)


# ---- the pipeline's collected batch ---------------------------------------------------------------
PB, PAIRS = 26, 26   # BODY_25: parts + background, pairs
ELEMENTS = [1, 2, 3, 4, PB + 2, PB + 3, PB + 2 + PAIRS]


def _element_chain(ctx, pose, frames, element, scale, out_size, alpha, stack):
    kind, channel = render_element(BODY_25, element)
    ratio = float(np.float32(pose.scale_net_to_output()) * np.float32(scale))
    heat = RenderHeat(kind, stack, ratio, channel, alpha, BODY_25)
    return _heat_chain(ctx, frames, heat, [], scale, out_size, CAST_CPU)


def _injected(ctx, semantics, seed):
    """A BODY_25 pipeline without a CNN: a random net output [2][78][6][10] for a 80x48 net input,
    producer 160x96."""
    pose = PoseExtractor(ctx, None)
    pose.set_map_semantics(semantics)
    rng = np.random.default_rng(seed)
    net_out = torch.from_numpy(rng.uniform(-0.6, 1.1, (2, 78, 6, 10)).astype(np.float32)).cuda()
    pose.forward_net_output(net_out, (80, 48), (160, 96))
    return pose, net_out


@pytest.mark.parametrize("semantics", [MAPS_CPU, MAPS_CUDA])
def test_pose_render_frames_elements(ctx, semantics):
    pose, net_out = _injected(ctx, semantics, 91)
    frames = torch.from_numpy(_frames(2, 96, 160, 9)).cuda()
    # the fused calls first: they read the net output, nothing is materialised for them
    cases = [(e, 1.0, (160, 96), 0.7) for e in ELEMENTS]
    cases.append((PB + 3, 1.5, (240, 144), 0.4))   # scale_input_to_output in the heat scale
    cases.append((4, 1.0, (200, 120), 0.7))        # an output larger than heat x scale
    cases.append((2, 1.0, (200, 120), 0.7))
    got = [pose.render_frames(frames, s, size, element=e, alpha_heatmap=a)
           for e, s, size, a in cases]
    stack = torch.from_numpy(pose.heatmaps_numpy()).cuda()
    assert tuple(stack.shape) == (2, 78, 48, 80)
    for (e, s, size, a), g in zip(cases, got):
        want = _element_chain(ctx, pose, frames, e, s, size, a, stack)
        ctx.sync()
        assert torch.equal(g, want), (e, s, size)
    assert not torch.equal(got[0], got[3])
    # blend_original False: alpha 1, the frame is not cleared
    g = pose.render_frames(frames, element=4, blend_original=False)
    want = _element_chain(ctx, pose, frames, 4, 1.0, (160, 96), 1.0, stack)
    assert torch.equal(g, want)
    # element 0 is the keypoint render
    assert torch.equal(pose.render_frames(frames, element=0), pose.render_frames(frames))
    # state errors: another frame count; a later batch in flight (its heat maps are gone)
    three = torch.zeros((3, 96, 160, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.OpkError, match="opk error 3: .*2 frames, not 3"):
        pose.render_frames(three, element=2)
    pose.submit_net_output(net_out, (80, 48), (160, 96))
    with pytest.raises(_lib.OpkError, match="opk error 3: .*no later batch is in flight"):
        pose.render_frames(frames, element=2)
    pose.collect()
    assert torch.equal(pose.render_frames(frames, element=1, alpha_heatmap=0.7), got[0])
    pose.close()


def test_pose_render_frames_two_scales(ctx):
    """Two merged sources (--scale_number 2): the lazy map averages both net outputs."""
    from oracle import body25
    from openpose_amd.api import Net, scale_and_size
    _, net_sizes = scale_and_size((320, 176), (-1, 176), 1.0, 2, 0.5)
    sizes = [(h, w) for (w, h) in net_sizes]
    assert len(sizes) == 2 and sizes[0] != sizes[1]
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(body25.layers(), seed=3, out_scale=0.02))
    rng = np.random.default_rng(4)
    xs = [torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 3, h, w)).astype(np.float32)).cuda()
          for h, w in sizes]
    ov = np.stack([synth.overlay(2, sizes[0][0] // 8, sizes[0][1] // 8, seed=40 + k)
                   for k in range(2)]).astype(np.float32)
    pose = PoseExtractor(ctx, net)
    ovd = torch.from_numpy(ov).cuda()
    pose.set_overlay(ovd)
    pose.forward_multi(xs, (320, 176))
    frames = torch.from_numpy(_frames(2, 176, 320, 17)).cuda()
    elements = [2, 3, 5, PB + 4]
    got = [pose.render_frames(frames, element=e) for e in elements]
    stack = torch.from_numpy(pose.heatmaps_numpy()).cuda()
    for e, g in zip(elements, got):
        want = _element_chain(ctx, pose, frames, e, 1.0, (320, 176), 0.7, stack)
        ctx.sync()
        assert torch.equal(g, want), e
    pose.close()
    net.close()
