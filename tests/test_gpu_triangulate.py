"""GPU: opk_triangulate (kernels/triangulate.hip) bit for bit against opk_triangulate_host and the
numpy restatement (tests/triangulate_cases.py), both lane mappings, at the launch's edges; and the
stage in the pose pipeline (PoseExtractor.set_views) against Triangulator.reconstruct on the
collected keypoints.  Nothing here reads outside the repository's tree."""
import ctypes
import json

import numpy as np
import pytest
import torch

from openpose_amd import api, synth
from openpose_amd.api import Triangulator
from tests import cpm_graphs, prototxt
from tests import triangulate_cases as tc
from tests.test_triangulate import CASES as HOST_CASES
from tests.test_gpu_whole_body import SIZE as FRAME_SIZE
from tests.test_gpu_whole_body import Rig, _frames

pytestmark = pytest.mark.gpu

SIZE = (1280, 720)
MAPPINGS = {"group": 1, "thread": 0}   # the TRI_GROUP switch: 8 lanes per point (shipped), or a thread
NAMES = ("xyz", "status", "errors", "dropped")


def same(got, want):
    for g, w, what in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w, equal_nan=(what == "errors")), what


def all_routes(ctx, P, sizes, kp, present=None, min_views=-1, restate=True):
    """Host route, both kernel mappings and (restate) the restatement: all bit for bit."""
    tri = Triangulator(P, sizes, min_views)
    host = tri.reconstruct(kp, present)
    for name, switch in MAPPINGS.items():
        with api.dev_switches(TRI_GROUP=switch), api.launch_log() as log:
            dev = tri.reconstruct(kp, present, device=ctx)
        assert [k for _, k in log] == ["triangulate<%s>" % name]
        same(dev, host)
    if restate:
        same(host, tc.reconstruct(P, sizes, min_views, kp, present))
    return host


def rig_and_scene(seed, V, steps=1, parts=1, noise=0.0):
    rng = np.random.default_rng(seed)
    P, sizes = tc.ring_rig(rng, V, SIZE)
    kp, _ = tc.scene(rng, P, steps, parts, noise)
    return rng, P, sizes, kp


@pytest.mark.parametrize("V", [2, 3, 4, 7])
@pytest.mark.parametrize("parts", [25, 70, 21])
def test_arrays_equal_host_and_restatement(ctx, V, parts):
    rng, P, sizes, kp = rig_and_scene(100 * V + parts, V, 1, parts, noise=2.0)
    for p in range(0, parts, 3):                       # outliers: the leave-one-out step
        kp[0, p % V, p, 0] += 70
    kp[0, 0, 1::5, 2] = 0.2                            # parts one view does not see
    _, _, errors, dropped = all_routes(ctx, P, sizes, kp)
    assert (errors >= 0).any()
    if V >= 4:
        assert (dropped >= 0).any() and (dropped < 0).any()


@pytest.mark.parametrize("points", [1, 7, 8, 9, 65])
def test_point_counts_around_a_wave(ctx, points):
    _, P, sizes, kp = rig_and_scene(200 + points, 4, 1, points, noise=1.0)
    kp[0, 1, ::2, 1] += 60
    xyz, status, _, dropped = all_routes(ctx, P, sizes, kp)
    assert status[0] == 1 and xyz[0, :, 3].any() and (dropped[0, ::2] == 1).all()


def test_groups_straddle_steps_with_absent_views(ctx):
    rng, P, sizes, kp = rig_and_scene(300, 5, 3, 70, noise=1.5)
    kp[1, 2, ::4, 0] -= 90
    kp[2, :, 10:, 2] = 0.1
    present = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 1, 1], [0, 1, 0, 0, 0]], np.int32)
    _, status, errors, _ = all_routes(ctx, P, sizes, kp, present)
    assert status.tolist() == [1, 1, 0] and (errors[2] == -1).all()


def test_leave_one_out_in_some_lanes_of_a_wave(ctx):
    # V = 7, 8 parts = one wave: every second point has an outlier view, a different one each
    _, P, sizes, kp = rig_and_scene(400, 7, 1, 8, noise=0.3)
    for p in range(0, 8, 2):
        kp[0, p % 7, p, 0] += 120
    _, _, _, dropped = all_routes(ctx, P, sizes, kp)
    assert dropped[0].tolist() == [0, -1, 2, -1, 4, -1, 6, -1]


@pytest.mark.parametrize("name", [c[0] for c in HOST_CASES])
def test_host_cases_on_the_device(ctx, name):
    """Every named case of tests/test_triangulate.py, with its own assertions, on all routes."""
    _, case, args = next(c for c in HOST_CASES if c[0] == name)
    case(lambda *a, **kw: all_routes(ctx, *a, **kw), *args)


def test_two_calls_back_to_back_on_one_stream(ctx):
    _, P, sizes, kp_a = rig_and_scene(600, 4, 2, 25, noise=1.0)
    _, _, _, kp_b = rig_and_scene(601, 4, 3, 21, noise=4.0)
    tri_a = Triangulator(P, sizes)
    tri_b = Triangulator(P[:3], sizes[:3], 2)
    kp_b = np.ascontiguousarray(kp_b[:, :3])
    outs = []
    for tri, kp in ((tri_a, kp_a), (tri_b, kp_b)):     # queued without a sync in between
        steps, _, parts, _ = kp.shape
        d = dict(kp=torch.from_numpy(kp).cuda(),
                 present=torch.ones((steps, tri.views), dtype=torch.int32, device="cuda"),
                 xyz=torch.empty((steps, parts, 4), device="cuda"),
                 status=torch.empty(steps, dtype=torch.int32, device="cuda"),
                 dropped=torch.empty((steps, parts), dtype=torch.int32, device="cuda"))
        outs.append((tri, kp, d))
    for tri, kp, d in outs:
        rig = tri.struct()
        steps, _, parts, _ = kp.shape
        api.check(ctx.L.opk_triangulate(ctx.h, ctypes.byref(rig), steps, parts, api._ptr(d["kp"]),
                                        api._ptr(d["present"]), api._ptr(d["xyz"]),
                                        api._ptr(d["status"]), None, api._ptr(d["dropped"])))
    ctx.sync()
    for tri, kp, d in outs:                            # (errors_dev NULL: the context's scratch)
        xyz, status, _, dropped = tri.reconstruct(kp)
        assert np.array_equal(d["xyz"].cpu().numpy(), xyz)
        assert np.array_equal(d["status"].cpu().numpy(), status)
        assert np.array_equal(d["dropped"].cpu().numpy(), dropped)


# ---- the stage in the pose pipeline -------------------------------------------------------------
N = 8
KIND_NAMES = ("body", "face", "left hand", "right hand")


class ScoringRig(Rig):
    """The whole-body tests' rig with face and hand nets whose keypoints pass the 3-D score
    threshold: their seeded last layer (small random maps, the argmax a seeded position in the
    crop) gets a bias of 0.6, so every score is 0.6 plus the map's maximum."""

    def __init__(self, ctx):
        super().__init__(ctx)
        for name, seed in (("builtin:FACE", 5), ("builtin:HAND", 7)):
            graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[name]()))
            params = synth.he_weights(graph, seed=seed, out_scale=0.05)
            w, b, slope = params["Mconv7_stage6"]
            params["Mconv7_stage6"] = (w, b + np.float32(0.6), slope)
            self.nets[name].set_params(params)


def _step_copies(t, V):
    """Batch of N frames (or overlays) of t [steps...]: every step's entry V times over."""
    return t.repeat_interleave(V, dim=0).contiguous()


@pytest.fixture(scope="module")
def rig(ctx):
    r = ScoringRig(ctx)
    r.scenes = r.overlay                    # the whole-body tests' two synthetic scenes
    r.frames = _frames(31, N)
    r.pose.set_overlay(torch.cat([r.scenes] * (N // 2)).contiguous())
    yield r
    r.close()


def _person0(arrays, parts):
    """[V][parts][3] of person 0 of each view's array (zeros where the view has nobody)."""
    out = np.zeros((len(arrays), parts, 3), np.float32)
    for v, a in enumerate(arrays):
        if a.shape[0]:
            out[v] = a[0]
    return out


@pytest.mark.parametrize("V", [2, 4])
def test_pipeline_equals_reconstruct_on_the_collected_keypoints(rig, V):
    """The views of a time step are copies of one frame and the rig maps one plane to the same
    pixels in every view (tc.plane_rig), so every valid keypoint of person 0 is a consistent 3-D
    point: each of the four kinds must attempt and accept parts, and equal reconstruct() on the
    keypoints the pipeline hands out for the step's frames."""
    pose = rig.pose
    tri = Triangulator(*tc.plane_rig(V, FRAME_SIZE), 2)
    steps = N // V
    frames = _step_copies(rig.frames[:steps], V)
    pose.set_overlay(_step_copies(torch.cat([rig.scenes] * steps)[:steps], V))
    pose.set_views(tri)
    try:
        pose.forward_frames(frames)
        attempted, accepted = [0] * 4, [0] * 4
        for step in range(steps):
            fs = range(step * V, step * V + V)
            body = [pose.keypoints(f)[0] for f in fs]
            assert all(b.shape[0] >= 2 for b in body)     # person 0 is not the only one to pick
            present = np.array([[int(b.shape[0] > 0) for b in body]], np.int32)
            hands = [pose.hand_keypoints(f) for f in fs]
            kinds = ((body, 25), ([pose.face_keypoints(f) for f in fs], 70),
                     ([h[0] for h in hands], 21), ([h[1] for h in hands], 21))
            got = pose.keypoints_3d(step)
            for k, (g, (arrays, parts)) in enumerate(zip(got, kinds)):
                xyz, status, errors, _ = tri.reconstruct(_person0(arrays, parts)[None], present)
                want = xyz if status[0] else np.zeros((0, parts, 4), np.float32)
                assert g.shape == want.shape and np.array_equal(g, want), (step, KIND_NAMES[k])
                attempted[k] += int((errors >= 0).sum())
                accepted[k] += int(xyz[..., 3].sum())
            for f in fs:                            # every frame of the step carries the arrays
                d = pose.datum(f)
                assert [name for _, name in d[5:]] == [
                    "pose_keypoints_3d", "face_keypoints_3d", "hand_left_keypoints_3d",
                    "hand_right_keypoints_3d"]
                for (a, _), g in zip(d[5:], got):
                    assert np.array_equal(a, g)
        print("attempted per kind", attempted, "accepted per kind", accepted)
        for k in range(4):
            assert attempted[k] > 0 and accepted[k] >= 1, (KIND_NAMES[k], attempted, accepted)
        # the steps differ (two scenes, other frames): so do their arrays
        assert not np.array_equal(pose.keypoints_3d(0)[0], pose.keypoints_3d(1)[0])
        # the JSON of a frame cut to one person, as --3d demands (--number_people_max 1)
        d = pose.datum(0)
        one = [(a[:1] if name == "person_id" or name.endswith("_2d") else a, name) for a, name in d]
        people = json.loads(api.people_json(one))["people"]
        assert len(people) == 1 and len(people[0]["pose_keypoints_3d"]) == 4 * 25
        assert len(people[0]["face_keypoints_3d"]) == 4 * 70 * d[6][0].shape[0]
        with pytest.raises(api.OpkError, match="fewer people"):     # two people against one
            api.people_json(d)
    finally:
        pose.set_views(None)
        pose.set_overlay(torch.cat([rig.scenes] * (N // 2)).contiguous())


def test_pipeline_argument_and_state_errors(rig):
    pose, tri = rig.pose, Triangulator(*tc.plane_rig(2, FRAME_SIZE), 2)
    pose.set_views(tri)
    try:
        with pytest.raises(api.OpkError, match="opk error 1"):     # 7 frames, 2 views
            pose.submit_frames(rig.frames[:7])
        assert pose.pending() == 0
        other = Triangulator(tri.P, tri.sizes + 2, 2)                # another frame size
        pose.set_views(other)
        with pytest.raises(api.OpkError, match="opk error 1"):
            pose.submit_frames(rig.frames)
        assert pose.pending() == 0
        pose.set_views(tri)
        with pytest.raises(api.OpkError, match="opk error 3"):     # nothing collected with views
            pose.keypoints_3d(0)
        pose.submit_frames(rig.frames)
        with pytest.raises(api.OpkError, match="opk error 3"):     # a batch in flight
            pose.set_views(None)
        with pytest.raises(api.OpkError, match="opk error 3"):
            pose.set_views(other)
        assert pose.collect() == N
        assert len(pose.keypoints_3d(N // 2 - 1)) == 4
        with pytest.raises(api.OpkError, match="opk error 1"):
            pose.keypoints_3d(N // 2)
    finally:
        if pose.pending():
            pose.collect()
        pose.set_views(None)
    # no views: datum is what it was
    pose.forward_frames(rig.frames)
    d = pose.datum(0)
    assert all(a is None for a, _ in d[5:])
    with pytest.raises(api.OpkError, match="opk error 3"):
        pose.keypoints_3d(0)
