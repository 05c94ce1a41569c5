"""GPU: the small-batch net mode (Net.set_small_batch, launch_conv3s in conv3.hip).

With the mode on, 3x3 convs whose conv3_shape tiles give fewer workgroups than the chip has CUs run
on conv3s_kernel's 64 x 32 / 128 x 64 tiles.  Every case first asserts from the launch log that
conv3s_kernel ran exactly where Net.conv_plan says `small` (for every conv), then checks every
launch against the reference of its own input blob (tests/launch_check.py) and that the blobs are
the same bits as with the mode off:

  1  BODY_25 at 1 x 64 x 96, 2 x 64 x 96 and 1 x 50 x 90, both precisions: tiles that straddle a
     frame, odd sizes at every level, cin 180 / 206 padded to 192 / 224 read from concat slices
  2  BODY_25 at 1 x 368 x 656 (the OpenPose frame): net_output, conv4_4_CPM and a stage concat
  3  a wide and short image, 1 x 16 x 1312: conv3s cuts the 1312-column rows into strips
  4  a batch that fills the chip (2 x 256 x 386): the launch log does not change
"""
import contextlib
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import body25
from openpose_amd.api import PRECISION_SPLIT, Net, dev_switches
from tests import prototxt
from tests.launch_check import check_launches, conv_instantiations, print_rows, random_params
from tests.test_gpu_launch_matrix import every_conv_once, image, variants_graph
from tests.test_gpu_net import conv

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def forwarded(ctx, model, params, x, split, small):
    """A net of `model` (a layer list or "builtin:...") after one forward of x under LAUNCH_LOG=1;
    yields (net, launch log) and closes the net."""
    path = None
    if not isinstance(model, str):
        with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
            f.write(prototxt.emit(model))
            path = f.name
    net = None
    try:
        with dev_switches(LAUNCH_LOG=1):
            net = Net(ctx, path or model)
            net.set_params(params)
            if split:
                net.set_precision(PRECISION_SPLIT)
            net.set_small_batch(small)
            assert net.small_batch is bool(small)
            net.forward(torch.from_numpy(x).cuda())
            log = net.launch_log()
        yield net, log
    finally:
        if net is not None:
            net.close()
        if path:
            os.unlink(path)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_log_matches_plan(net, log, shape, split):
    """conv3s_kernel ran for exactly the convs whose plan says small; returns their names."""
    n, _, h, w = shape
    convs = net.convs()
    inst = conv_instantiations(log, [c["name"] for c in convs])
    small = []
    for i, c in enumerate(convs):
        plan = net.conv_plan(i, n, h, w, cus())
        ks = inst[c["name"]]
        assert len(ks) >= 1, (c["name"], log)
        for k in ks:
            assert k.startswith("conv3s_kernel<") == bool(plan["small"]), (c["name"], k, plan)
            if k.startswith("conv3s_kernel<"):
                assert k.endswith(",split>") == split, (c["name"], k)
                assert k.startswith("conv3s_kernel<%d,%d," % (plan["bm"], plan["bn"])), (c["name"], k, plan)
        if plan["small"]:
            assert c["kernel_size"] == 3, c
            small.append(c["name"])
    return small


def readable_blobs(net, graph):
    """{top: values} of every blob of the graph the last forward materialised."""
    out = {}
    for l in graph:
        if l["type"] == "Input":
            continue
        for top in l["top"]:
            if top in out:
                continue
            try:
                out[top] = net.blob(top)
            except Exception as e:   # conv1_1 / conv1_2 / Mconv6: inside a fused kernel
                assert "kept on chip" in str(e), (top, e)
    return out


def run_pair(ctx, model, graph, params, x, split, title, check=True):
    """Mode off, then on: the log agrees with the plan, every launch of the small run is within
    its bound, every readable blob is bit-identical.  Returns (small conv names, on log, off log)."""
    with forwarded(ctx, model, params, x, split, False) as (net, log_off):
        assert not any(k.startswith("conv3s_kernel") for _, k in log_off), log_off
        assert assert_log_matches_plan(net, log_off, x.shape, split) == []
        ref = readable_blobs(net, graph)
        ref_out = net.output_numpy()
    with forwarded(ctx, model, params, x, split, True) as (net, log_on):
        every_conv_once(log_on, graph)
        small = assert_log_matches_plan(net, log_on, x.shape, split)
        if check:
            rows = check_launches(net, graph, params, x, sorted({0, x.shape[0] - 1}), split=split,
                                  log=log_on)
            print_rows(rows, title)
        got = readable_blobs(net, graph)
        got_out = net.output_numpy()
    assert np.abs(ref_out).max() > 0
    np.testing.assert_array_equal(got_out, ref_out, err_msg="net_output")
    assert sorted(got) == sorted(ref)
    for name in ref:
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    return small, log_on, log_off


# ---- 1: BODY_25 at small and odd sizes ----------------------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
@pytest.mark.parametrize("shape", [(1, 3, 64, 96), (2, 3, 64, 96), (1, 3, 50, 90)],
                         ids=["1x64x96", "2x64x96", "1x50x90"])
def test_body25_small_shapes(ctx, shape, split):
    graph = body25.layers()
    params = random_params(graph, 101)
    x = image(102, shape)
    title = "small batch: BODY_25 %dx%dx%d %s" % (shape[0], shape[2], shape[3], "split" if split else "fp16")
    small, log, _ = run_pair(ctx, "builtin:BODY_25", graph, params, x, split, title)
    # every 3x3 conv with a launch of its own (conv1_2: unless inside conv1_fused_kernel) is far
    # below one tile per CU here
    alone = {layer for layer, _ in log}
    own3 = [l["name"] for l in graph if l["type"] == "Convolution" and l["kernel_size"] == 3
            and l["name"] != "conv1_1" and l["name"] in alone]
    assert len(own3) >= 100 and sorted(small) == sorted(own3)
    # the 192- and 224-channel reads of the 180 / 206-channel concat slices
    assert "Mconv1_stage1_L2_0" in small and "Mconv1_stage1_L1_0" in small


# ---- 2: the OpenPose frame ----------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_body25_one_frame_bit_identical(ctx, split):
    graph = body25.layers()
    params = random_params(graph, 103)
    x = image(104, (1, 3, 368, 656))
    names = ("net_output", "conv4_4_CPM", "Mconv3_stage1_L2_concat")
    blobs = {}
    for small in (False, True):
        with forwarded(ctx, "builtin:BODY_25", params, x, split, small) as (net, log):
            picked = assert_log_matches_plan(net, log, x.shape, split)
            blobs[small] = {n: net.blob(n) for n in names}
            blobs[small]["output"] = net.output_numpy()
            if small:
                every_conv_once(log, graph)
                stage = [l["name"] for l in graph if l["type"] == "Convolution" and
                         l["kernel_size"] == 3 and l["name"].startswith("Mconv")]
                assert len(stage) == 90 and set(stage) <= set(picked)
                k = conv_instantiations(log, ["Mconv2_stage1_L2_1"])["Mconv2_stage1_L2_1"]
                assert k == ["conv3s_kernel<64,32,256,9%s>" % (",split" if split else "")], k
            else:
                assert picked == []
    assert np.abs(blobs[False]["conv4_4_CPM"]).max() > 0
    for n in blobs[False]:
        np.testing.assert_array_equal(blobs[True][n], blobs[False][n], err_msg=n)


# ---- 3: wide and short ---------------------------------------------------------------------------

def wide_graph():
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 128, 3, "relu")
    L += conv("c3", "c2", 96, 3, "prelu")
    L.append(dict(name="cat", type="Concat", bottom=["c2", "c3"], top=["cat"]))
    L += conv("c4", "cat", 128, 3, "prelu") + conv("c5", "c4", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c5"], top=["net_output"]))
    return L


@pytest.mark.parametrize("split", [False, True], ids=["fp16", "split"])
def test_wide_and_short(ctx, split):
    L = wide_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 105)
    x = image(106, (1, 3, 16, 1312))
    small, log, _ = run_pair(ctx, L, graph, params, x, split,
                             "small batch: 1x16x1312 %s" % ("split" if split else "fp16"))
    # 1312 columns: 15 strips of 88 under the 256-row halo of the 64 x 32 tile
    assert sorted(small) == ["c2", "c3", "c4"], (small, log)


# ---- 4: no effect where the chip is already full -------------------------------------------------

def test_full_chip_unchanged(ctx):
    L = variants_graph()
    graph = prototxt.parse(prototxt.emit(L))
    params = random_params(graph, 107)
    x = image(108, (2, 3, 256, 386))
    logs = {}
    for small in (False, True):
        with forwarded(ctx, L, params, x, False, small) as (net, log):
            assert assert_log_matches_plan(net, log, x.shape, False) == []
            logs[small] = log
    assert logs[True] == logs[False]
