"""Face / hand stages inside the pose pipeline (PoseExtractor.attach, opk_pose_attach_extractor).

Two seeded 640 x 360 frames, a 320 x 176 BODY_25 net (seeded weights of small output scale) with a
synthetic overlay of two people per frame, seeded builtin:FACE / builtin:HAND nets at 176 x 176
crops, hands at two scales, max_batch 4 (the hand stage runs four chunks; with all 4 faces and
8 hands found the crop counts, 4 and 16, are multiples of 4, so the chunks of different sizes are a
case of their own: three hand scales, 24 crops, max_batch 16 -> 16 + 8).  The reference of
every check is the manual flow on the same objects: detect_faces / detect_hands of
pose.keypoints(f), concatenated in frame order, then KeypointExtractor.forward -- the stage must
equal it bit for bit.

Sizes: the synthetic template's face rectangle has side 0.207 x person height (the detector's
terms 2 x 0.10, 3 x 0.06 and 2 x 0.12, averaged), its hand rectangle 0.226 x; at >= 0.6 x 360 px
that is >= 44.6 px and >= 48 px, above the reference's face minimum of 40.  SEED was picked on the
CPU (oracle/extract.py's detectors on the template skeletons scaled to frame pixels: every face
side > 44, every hand side > 44, the people inside the field and more than 12 net-output columns
apart), before any GPU run."""
import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd import api, synth
from openpose_amd.api import (FACE, HAND, LAYER_FACE, LAYER_HAND, LAYER_POSE, PRECISION_SPLIT,
                              KeypointExtractor, Net, PoseExtractor, RenderLayer)
from tests import cpm_graphs, prototxt

pytestmark = pytest.mark.gpu

SEED = 4
SIZE = (640, 360)
CROP = (176, 176)


def _frames(seed, n=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, SIZE[1], SIZE[0], 3), dtype=torch.uint8, generator=g).cuda()


def _overlay(seed, n=2):
    return torch.from_numpy(np.stack([
        synth.render_field(synth.people(2, 22, 40, 2 * seed + f, min_height=0.6, max_height=0.7),
                           22, 40, sigma=1.0, paf_width=1.0) for f in range(n)])).cuda()


class Rig:
    def __init__(self, ctx, split=False):
        self.ctx = ctx
        self.nets = {}
        for name, graph, seed, scale in (
                ("builtin:BODY_25", body25.layers(), 3, 0.02),
                ("builtin:FACE", prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS["builtin:FACE"]())), 5, 0.05),
                ("builtin:HAND", prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS["builtin:HAND"]())), 7, 0.05)):
            net = Net(ctx, name)
            net.set_params(synth.he_weights(graph, seed=seed, out_scale=scale))
            if split:
                net.set_precision(PRECISION_SPLIT)
            self.nets[name] = net
        self.face = KeypointExtractor(ctx, self.nets["builtin:FACE"], FACE, CROP)
        self.hand = KeypointExtractor(ctx, self.nets["builtin:HAND"], HAND, CROP)
        self.hand.set_scales(2, 0.4)
        self.pose = PoseExtractor(ctx, self.nets["builtin:BODY_25"])
        self.pose.set_input((-1, 176))
        self.overlay = _overlay(SEED)
        self.pose.set_overlay(self.overlay)
        self.set_max_batch(4)
        self.pose.attach(face=self.face, hands=self.hand)

    def set_max_batch(self, b):
        self.face.set_max_batch(b)
        self.hand.set_max_batch(b)

    def close(self):
        self.pose.close()
        self.face.close()
        self.hand.close()
        for n in self.nets.values():
            n.close()


def _stage(pose):
    """What the pipeline hands out for the collected batch."""
    out = []
    for f in range(2):
        kp, ks = pose.keypoints(f)
        out.append(dict(kp=kp, ks=ks, face_rects=pose.face_rectangles(f),
                        hand_rects=pose.hand_rectangles(f), face=pose.face_keypoints(f),
                        hands=pose.hand_keypoints(f)))
    return out


def _manual(rig, frames):
    """The hand-glued flow on the same objects, from the collected batch's pose keypoints."""
    kps = [rig.pose.keypoints(f)[0] for f in range(2)]
    counts = [k.shape[0] for k in kps]
    frame_of = np.repeat(np.arange(2, dtype=np.int32), counts)
    face_rects = np.concatenate([api.detect_faces(k) for k in kps])
    hand_rects = np.concatenate([api.detect_hands(k) for k in kps])
    face = rig.face.forward(frames, face_rects, frame_of)
    hands = rig.hand.forward(frames, hand_rects, frame_of)
    out, at = [], 0
    for f in range(2):
        s = slice(at, at + counts[f])
        out.append(dict(face_rects=face_rects[s], hand_rects=hand_rects[s], face=face[s],
                        hands=hands[:, s]))
        at += counts[f]
    return out


def _same(got, want):
    for g, w in zip(got, want):
        for k in ("face_rects", "hand_rects", "face", "hands"):
            assert g[k].shape == w[k].shape, k
            np.testing.assert_array_equal(g[k].view(np.uint32), w[k].view(np.uint32), err_msg=k)


def _non_empty(res):
    faces = sum(int(r["face"][p].any()) for r in res for p in range(r["face"].shape[0]))
    hands = sum(int(r["hands"][h, p].any()) for r in res for h in range(2)
                for p in range(r["hands"].shape[1]))
    print("faces with keypoints %d, hands with keypoints %d" % (faces, hands))
    assert faces >= 3 and hands >= 6


@pytest.fixture(scope="module")
def rig(ctx):
    r = Rig(ctx)
    yield r
    r.close()


@pytest.fixture(scope="module")
def batch(rig):
    """One synchronous run at max_batch 4: (frames, stage results, manual results)."""
    frames = _frames(SEED)
    rig.set_max_batch(4)
    rig.pose.forward_frames(frames)
    got = _stage(rig.pose)
    crops = (rig.face.crops(), rig.hand.crops())
    times = (rig.pose.read_part_times(FACE), rig.pose.read_part_times(HAND))
    want = _manual(rig, frames)
    # the direct call still hands out every crop's input
    assert all(x is not None and x.shape == (3, 176, 176) for _, x in rig.face.crops())
    return frames, got, want, crops, times


def test_stage_equals_manual_flow(rig, batch):
    frames, got, want, crops, times = batch
    _non_empty(got)
    _same(got, want)
    for r in got:
        assert r["face"].shape[1:] == (70, 3) and r["hands"].shape[2:] == (21, 3)
    # chunked staging: the crops' matrices are there, their inputs are not
    nfaces = sum(int(r["face"][p].any()) for r in got for p in range(r["face"].shape[0]))
    assert len(crops[0]) == nfaces
    assert len(crops[1]) >= 12 and len(crops[1]) % 2 == 0     # two scales per hand: > 1 chunk of 4
    for m, x in crops[0] + crops[1]:
        assert m.shape == (2, 3) and x is None
    assert times[0]["batches"] == 1 and times[0]["crops"] == len(crops[0])
    assert times[1]["batches"] == 1 and times[1]["crops"] == len(crops[1])
    assert times[0]["host_ms"] > 0 and times[1]["wait_ms"] > 0


def test_one_chunk_equals_several(rig, batch):
    frames, got, want, _, _ = batch
    rig.set_max_batch(32)
    try:
        rig.pose.forward_frames(frames)
        _same(_stage(rig.pose), got)
    finally:
        rig.set_max_batch(4)


def test_ragged_chunks_equal_manual_flow_and_other_batchings(rig, batch):
    """Chunks of different sizes with non-zero table offsets.  Hands at THREE scales: the scene's
    8 hand rectangles (every one valid at scale 0.8 too: side >= 0.8 x 48 px > 1) give 24 crops,
    which max_batch 16 runs as 16 + 8 -- a smaller power-of-two batch with its own net plan,
    starting at crop 16 of the tap and frame tables -- and max_batch 4 as six chunks of 4.  The 4
    faces at max_batch 3 run as 2 + 2, the second chunk at table offset 2.  Counts known on the
    CPU (oracle detectors on the template skeletons, see the module docstring) and asserted here.
    All batchings and the manual flow (unchunked, 16 + 8) must agree bit for bit."""
    frames = batch[0]
    rig.hand.set_scales(3, 0.4)
    try:
        rig.face.set_max_batch(3)
        rig.hand.set_max_batch(16)
        rig.pose.forward_frames(frames)
        got = _stage(rig.pose)
        ncrops = (len(rig.face.crops()), len(rig.hand.crops()))
        assert ncrops == (4, 24)
        assert all(x is None for _, x in rig.hand.crops())
        _non_empty(got)
        want = _manual(rig, frames)
        assert len(rig.hand.crops()) == 24
        _same(got, want)
        rig.set_max_batch(4)      # 4 and 6 x 4
        rig.pose.forward_frames(frames)
        _same(_stage(rig.pose), got)
        rig.set_max_batch(8)      # 4 and 3 x 8
        rig.pose.forward_frames(frames)
        _same(_stage(rig.pose), got)
    finally:
        rig.hand.set_scales(2, 0.4)
        rig.set_max_batch(4)


def test_pipelined_equals_synchronous(rig, batch):
    frames_a, got_a, _, _, _ = batch
    frames_b = _frames(SEED + 100)
    rig.pose.forward_frames(frames_b)
    got_b = _stage(rig.pose)
    assert any(not np.array_equal(a["face"], b["face"]) for a, b in zip(got_a, got_b))
    rig.pose.submit_frames(frames_a)
    rig.pose.submit_frames(frames_b)
    assert rig.pose.collect() == 2
    pipe_a = _stage(rig.pose)
    assert rig.pose.collect() == 2
    pipe_b = _stage(rig.pose)
    for pipe, sync in ((pipe_a, got_a), (pipe_b, got_b)):
        _same(pipe, sync)
        for p, s in zip(pipe, sync):
            np.testing.assert_array_equal(p["kp"], s["kp"])
            np.testing.assert_array_equal(p["ks"], s["ks"])


def test_render_and_json(rig, batch):
    frames, got, _, _, _ = batch
    rig.pose.forward_frames(frames)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else None
    counts = [r["kp"].shape[0] for r in got]
    face = np.concatenate([r["face"] for r in got])
    # a frame's left hands, then its right hands
    hands = np.concatenate([r["hands"].reshape(-1, 21, 3) for r in got])
    # the seeded nets' maxima are far below the renderers' default thresholds (0.4, 0.2): draw
    # every keypoint above half the median positive score, so that both layers put pixels down
    th = []
    for a in (face, hands):
        pos = a[..., 2][a[..., 2] > 0]
        assert pos.size > 0
        th.append(float(np.median(pos)) / 2)
    out = rig.pose.render_frames(frames, face=True, hands=True, face_threshold=th[0],
                                 hand_threshold=th[1])
    layers = [
        RenderLayer(LAYER_POSE, dev(np.concatenate([r["kp"] for r in got])), counts),
        RenderLayer(LAYER_FACE, dev(face), counts, threshold=th[0]),
        RenderLayer(LAYER_HAND, dev(hands), [2 * c for c in counts], threshold=th[1])]
    want = rig.ctx.render_frames(frames, layers)
    assert torch.equal(out, want)
    pose_only = rig.pose.render_frames(frames)
    assert not torch.equal(out, pose_only)   # the layers draw something
    # scaleInputToOutput 0.5: x and y of all three layers times float(0.5) on the host
    half = np.float32(0.5)

    def scaled(a):
        a = a.copy()
        a[..., :2] *= half
        return dev(a)

    out_h = rig.pose.render_frames(frames, scale=0.5, out_size=(320, 180), face=True, hands=True,
                                   face_threshold=th[0], hand_threshold=th[1])
    layers_h = [
        RenderLayer(LAYER_POSE, scaled(np.concatenate([r["kp"] for r in got])), counts),
        RenderLayer(LAYER_FACE, scaled(face), counts, threshold=th[0]),
        RenderLayer(LAYER_HAND, scaled(hands), [2 * c for c in counts], threshold=th[1])]
    want_h = rig.ctx.render_frames(frames, layers_h, 0.5, (320, 180))
    assert out_h.shape == (2, 180, 320, 3) and torch.equal(out_h, want_h)
    assert not torch.equal(out_h, rig.pose.render_frames(frames, scale=0.5, out_size=(320, 180)))
    # a subset of the attached extractors' layers
    only_face = rig.pose.render_frames(frames, face=True, face_threshold=th[0])
    assert torch.equal(only_face, rig.ctx.render_frames(frames, layers[:2]))
    only_hands = rig.pose.render_frames(frames, hands=True, hand_threshold=th[1])
    assert torch.equal(only_hands, rig.ctx.render_frames(frames, [layers[0], layers[2]]))
    assert not torch.equal(only_face, pose_only) and not torch.equal(only_hands, pose_only)
    assert not torch.equal(only_face, out) and not torch.equal(only_hands, out)
    for f, r in enumerate(got):
        vec = api.datum_keypoint_vector(r["kp"], r["face"], (r["hands"][0], r["hands"][1]))
        assert api.people_json(rig.pose.datum(f)) == api.people_json(vec)
        assert '"face_keypoints_2d":[]' not in api.people_json(vec)


def test_detach_restores_submit(rig, batch):
    frames = batch[0]
    x = torch.zeros((1, 3, 176, 320), device="cuda")
    with pytest.raises(api.OpkError, match="needs the frames"):
        rig.pose.submit(x, SIZE)
    rig.pose.detach(FACE)
    rig.pose.detach(HAND)
    try:
        rig.pose.submit(x, SIZE)
        assert rig.pose.collect() == 1
        with pytest.raises(api.OpkError):
            rig.pose.face_keypoints(0)
    finally:
        rig.pose.attach(face=rig.face, hands=rig.hand)


def test_split_precision_equals_its_manual_flow(ctx):
    r = Rig(ctx, split=True)
    try:
        frames = _frames(SEED)
        r.pose.forward_frames(frames)
        got = _stage(r.pose)
        _non_empty(got)
        _same(got, _manual(r, frames))
    finally:
        r.close()
