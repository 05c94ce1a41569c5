"""GPU: the small-batch net mode (Net.set_small_batch) on nets with 7x7 layers and a 3-pixel
border -- conv3s_kernel's 7x7 instantiations and its 3x3 tiles at border 3 (launch_conv3s in conv3.hip).

Every case runs the mode off, then on, under LAUNCH_LOG=1; asserts from the log that conv3s_kernel
ran for exactly the convs whose Net.conv_plan says small, on the plan's tile, and that one of them
is a 7x7 conv; and that the blobs and net_output are the same bits as with the mode off.  Where
noted every launch of the mode-on run is also held to the per-launch bound of
tests/launch_check.py (the reference of the same operation fed with the GPU's own input blob).

  1  the miniature CPM nets of test_gpu_net.cpm_stage_graph (both heads) at 1 x 64 x 96, 2 x 64 x 96
     and 1 x 50 x 90, both precisions, per-launch check: 7x7 tiles that straddle a frame, odd
     sizes, 48-wide rows in two strips, the 118-channel concat read as 128, a 96-output layer
     (32-wide tiles only), 3x3 layers at border 3
  2  the same graph at 2 x 128 x 192: the 128 x 64 7x7 tile, rows of 96 in three strips
  3  builtin:FACE at 1 x 368 x 368 (both precisions), builtin:HAND at 2 x 368 x 368 and
     builtin:COCO_18 at 1 x 368 x 656: net_output, the features and a stage concat
  4  KeypointExtractor on FACE (3 rectangles) and HAND (2 scales, 2 rectangles): keypoints and
     scores bit for bit those of the mode off
  5  FACE at 32 x 368 x 368: the launch log does not change
"""
import numpy as np
import pytest
import torch

from openpose_amd import synth
from openpose_amd.api import FACE, HAND, KeypointExtractor, Net
from tests import cpm_graphs, prototxt
from tests.launch_check import check_launches, conv_instantiations, print_rows, random_params
from tests.test_gpu_launch_matrix import every_conv_once, image
from tests.test_gpu_net import cpm_stage_graph
from tests.test_gpu_small_batch import cus, forwarded, readable_blobs

pytestmark = pytest.mark.gpu


def assert_log_matches_plan(net, log, shape, split):
    """conv3s_kernel ran for exactly the convs whose plan says small, on the plan's tile; returns
    {name: kernel size} of those convs."""
    n, _, h, w = shape
    convs = net.convs()
    inst = conv_instantiations(log, [c["name"] for c in convs])
    small = {}
    for i, c in enumerate(convs):
        plan = net.conv_plan(i, n, h, w, cus())
        ks = inst[c["name"]]
        assert len(ks) >= 1, (c["name"], log)
        for k in ks:
            assert k.startswith("conv3s_kernel<") == bool(plan["small"]), (c["name"], k, plan)
            if k.startswith("conv3s_kernel<"):
                assert k.endswith(",split>") == split, (c["name"], k)
                assert k.startswith("conv3s_kernel<%d,%d," % (plan["bm"], plan["bn"])), (c["name"], k, plan)
                assert (",7,7" in k) == (c["kernel_size"] == 7), (c["name"], k)
        if plan["small"]:
            assert ks == net.conv_kernels(i, n, h, w, cus()), (c["name"], ks)
            assert c["kernel_size"] in (3, 7), c
            small[c["name"]] = c["kernel_size"]
    return small


def run_pair(ctx, model, graph, params, x, split, title, check=True, blobs=None):
    """Mode off, then on: the log agrees with the plan, a 7x7 conv ran small, (check) every launch
    of the small run is within its bound, the blobs (all readable ones, or those named) and
    net_output are bit-identical.  Returns ({small conv: kernel size}, {conv: its plan with the mode on})."""
    def read(net):
        if blobs is None:
            return readable_blobs(net, graph)
        return {b: net.blob(b) for b in blobs}

    with forwarded(ctx, model, params, x, split, False) as (net, log_off):
        assert not any(k.startswith("conv3s_kernel") for _, k in log_off), log_off
        assert assert_log_matches_plan(net, log_off, x.shape, split) == {}
        ref = read(net)
        ref_out = net.output_numpy()
    with forwarded(ctx, model, params, x, split, True) as (net, log_on):
        every_conv_once(log_on, graph)
        small = assert_log_matches_plan(net, log_on, x.shape, split)
        assert 7 in small.values(), small
        n, _, h, w = x.shape
        tiles = {c["name"]: net.conv_plan(i, n, h, w, cus()) for i, c in enumerate(net.convs())}
        if check:
            rows = check_launches(net, graph, params, x, sorted({0, x.shape[0] - 1}), split=split,
                                  log=log_on)
            print_rows(rows, title)
        got = read(net)
        got_out = net.output_numpy()
    assert np.abs(ref_out).max() > 0
    np.testing.assert_array_equal(got_out, ref_out, err_msg="net_output")
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert np.abs(ref[name]).max() > 0, name
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    return small, tiles


# ---- 1: the miniature CPM nets, per-launch check ------------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
@pytest.mark.parametrize("shape", [(1, 3, 64, 96), (2, 3, 64, 96), (1, 3, 50, 90)],
                         ids=["1x64x96", "2x64x96", "1x50x90"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "single"])
def test_cpm_stage_graph_small_shapes(ctx, concat, shape, split):
    L = cpm_stage_graph(concat)
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 111)
    x = image(112, shape)
    title = "small batch: CPM stages %dx%dx%d %s" % (shape[0], shape[2], shape[3], "split" if split else "fp16")
    small, tiles = run_pair(ctx, L, graph, params, x, split, title)
    # every 7x7 layer, and every 3x3 layer but the image conv (all far below a tile per CU here)
    want = {l["name"]: l["kernel_size"] for l in graph if l["type"] == "Convolution"
            and l["kernel_size"] in (3, 7) and l["name"] != "c1"}
    assert small == want, (small, want)
    assert sorted(k for k in want.values()) == [3, 3, 3, 3, 7, 7, 7]
    # the 96-output layers: only the 32-wide tile divides the 96-channel packing
    assert tiles["s2c"]["bn"] == 32 and tiles["feat"]["bn"] == 32, tiles


# ---- 2: the larger 7x7 tile -----------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_cpm_stage_graph_larger_tile(ctx, split):
    L = cpm_stage_graph(True)
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 113)
    x = image(114, (2, 3, 128, 192))
    small, tiles = run_pair(ctx, L, graph, params, x, split, "", check=False)
    assert small["s2a"] == 7 and small["s2b"] == 7 and small["s2c"] == 7
    if cus() == 256:   # 2 x 64 x (96 + 6) positions: 102 tiles of 128 by 2 n-blocks of 64
        for name in ("s2a", "s2b"):
            assert (tiles[name]["bm"], tiles[name]["bn"], tiles[name]["workgroups"]) == (128, 64, 204), tiles
    assert any(t["small"] and t["bm"] == 128 for n, t in tiles.items() if small.get(n) == 7), tiles


# ---- 3: the real nets ------------------------------------------------------------------------------

@pytest.mark.parametrize("model,shape,split,blobs", [
    ("builtin:FACE", (1, 3, 368, 368), False, ("conv5_3_CPM", "features_in_stage_3")),
    ("builtin:FACE", (1, 3, 368, 368), True, ("conv5_3_CPM", "features_in_stage_3")),
    ("builtin:HAND", (2, 3, 368, 368), False, ("conv5_3_CPM", "concat_stage3")),
    ("builtin:COCO_18", (1, 3, 368, 656), False, ("conv4_4_CPM", "concat_stage3"))],
    ids=["face-fp16", "face-split", "hand-fp16", "coco-fp16"])
def test_real_nets_bit_identical(ctx, model, shape, split, blobs):
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[model]()))
    params = random_params(graph, 115)
    x = image(116, shape)
    small, _ = run_pair(ctx, model, graph, params, x, split, "", check=False, blobs=blobs)
    k7 = [l["name"] for l in graph if l["type"] == "Convolution" and l["kernel_size"] == 7]
    assert len(k7) == (50 if "COCO" in model else 25)
    assert all(small.get(name) == 7 for name in k7), small
    assert 3 in small.values()


# ---- 4: through KeypointExtractor -----------------------------------------------------------------

def _extractor_net(ctx, name, seed, small):
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[name]()))
    net = Net(ctx, name)
    net.set_params(synth.he_weights(graph, seed=seed, out_scale=0.05))
    net.set_small_batch(small)
    return net


def _frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def test_face_extractor_bit_identical(ctx):
    frames = _frames(2, 360, 480, seed=1).cuda()
    rects = np.array([[100.5, 60.25, 150.0, 150.0], [-30.0, 250.0, 140.0, 140.0],
                      [300.75, 20.5, 97.5, 97.5]], np.float32)
    frame_of = np.array([0, 1, 1], np.int32)
    kp = {}
    for small in (False, True):
        net = _extractor_net(ctx, "builtin:FACE", 3, small)
        try:
            ex = KeypointExtractor(ctx, net, FACE, (368, 368))
            kp[small] = np.array(ex.forward(frames, rects, frame_of))
            assert net.small_batch is small
        finally:
            net.close()
    assert kp[False].shape == (3, 70, 3) and np.abs(kp[False]).max() > 0
    np.testing.assert_array_equal(kp[True], kp[False])


def test_hand_extractor_bit_identical(ctx):
    frames = _frames(1, 300, 400, seed=2).cuda()
    rects = np.array([[[50.5, 40.0, 80.0, 80.0], [250.25, 120.0, 61.0, 61.0]],
                      [[350.0, -20.0, 90.0, 90.0], [0.0, 0.0, 3.0, 3.0]]], np.float32)
    kp = {}
    for small in (False, True):
        net = _extractor_net(ctx, "builtin:HAND", 5, small)
        try:
            ex = KeypointExtractor(ctx, net, HAND, (320, 256))
            ex.set_scales(2, 0.4)
            kp[small] = np.array(ex.forward(frames, rects))
        finally:
            net.close()
    assert kp[False].shape == (2, 2, 21, 3) and np.abs(kp[False]).max() > 0
    np.testing.assert_array_equal(kp[True], kp[False])


# ---- 5: no effect where the chip is already full --------------------------------------------------

def test_full_chip_unchanged(ctx):
    model = "builtin:FACE"
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[model]()))
    params = random_params(graph, 117)
    x = image(118, (32, 3, 368, 368))
    logs = {}
    for small in (False, True):
        with forwarded(ctx, model, params, x, False, small) as (net, log):
            logs[small] = log
    assert not any(k.startswith("conv3s_kernel") for _, k in logs[False])
    assert logs[True] == logs[False]
